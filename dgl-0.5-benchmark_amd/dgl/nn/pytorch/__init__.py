from mi355x_graph.nn import GATConv, SAGEConv, GraphConv, AvgPooling, SumPooling, MaxPooling, Linear, HeteroGraphConv, GINConv, BatchNorm1d, RelGraphConv, DotGatConv, GINEConv, PNAConv  # noqa: F401
from mi355x_graph.nn import GlobalAttentionPooling, Set2Set, WeightAndSum, SortPooling  # noqa: F401
from mi355x_graph.nn import KNNGraph, SegmentedKNNGraph, EdgeConv, FixedRadiusNNGraph, PointNetConv, FeaturePropagation  # noqa: F401
from mi355x_graph.ops import edge_softmax  # noqa: F401
from . import conv, glob, factory  # noqa: F401
