"""dgl.geometry: farthest point sampling over batched point clouds (ops.segment_fps, csrc/fps.hip)."""
from mi355x_graph.transform import farthest_point_sampler, fixed_radius_block  # noqa: F401
from mi355x_graph.nn import FarthestPointSampler, FixedRadiusNNGraph  # noqa: F401
from . import pytorch  # noqa: F401
