from mi355x_graph.dataloading import GraphDataLoader  # noqa: F401
from mi355x_graph.sampling import (MultiLayerNeighborSampler, MultiLayerFullNeighborSampler,  # noqa: F401
                                   NodeDataLoader, sample_neighbors)
from mi355x_graph.linkpred import EdgeDataLoader  # noqa: F401
from . import negative_sampler  # noqa: F401
