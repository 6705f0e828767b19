"""dgl.dataloading.negative_sampler: Uniform(k) -- k uniform negative destinations per edge of a batch, drawn where the graph lives."""
from mi355x_graph.linkpred import Uniform  # noqa: F401
