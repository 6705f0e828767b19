from mi355x_graph.nn import GATConv, DotGatConv, GATv2Conv, NNConv, CFConv, GatedGCNConv, GINEConv, PNAConv, SAGEConv, GraphConv, RelGraphConv, TypedRelGraphConv, EdgeConv, PointNetConv  # noqa: F401
