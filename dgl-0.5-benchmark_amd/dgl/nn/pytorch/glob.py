from mi355x_graph.nn import AvgPooling, SumPooling, MaxPooling, GlobalAttentionPooling, Set2Set, WeightAndSum, SortPooling  # noqa: F401
