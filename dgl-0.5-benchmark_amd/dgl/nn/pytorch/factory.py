from mi355x_graph.nn import KNNGraph, SegmentedKNNGraph  # noqa: F401
