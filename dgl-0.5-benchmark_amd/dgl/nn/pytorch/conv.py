from mi355x_graph.nn import GATConv, DotGatConv, GINEConv, PNAConv, SAGEConv, GraphConv, RelGraphConv, EdgeConv, PointNetConv  # noqa: F401
