"""dgl.geometry.pytorch: where DGL 0.5 keeps FarthestPointSampler."""
from mi355x_graph.nn import FarthestPointSampler, FixedRadiusNNGraph  # noqa: F401
