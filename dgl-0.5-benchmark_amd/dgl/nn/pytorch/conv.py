from mi355x_graph.nn import GATConv, DotGatConv, SAGEConv, GraphConv, RelGraphConv  # noqa: F401
