from mi355x_graph.nn import GATConv, DotGatConv, GINEConv, SAGEConv, GraphConv, RelGraphConv  # noqa: F401
