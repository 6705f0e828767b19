from mi355x_graph.nn import GATConv, SAGEConv, GraphConv, RelGraphConv  # noqa: F401
