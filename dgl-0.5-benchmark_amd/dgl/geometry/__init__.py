"""dgl.geometry: farthest point sampling over batched point clouds (ops.segment_fps, csrc/fps.hip), the ball-query block and the
query-set k-NN block with its inverse-distance interpolation (ops.segment_knn_query, csrc/knn.hip)."""
from mi355x_graph.transform import farthest_point_sampler, fixed_radius_block, knn_block, knn_interpolate  # noqa: F401
from mi355x_graph.nn import FarthestPointSampler, FixedRadiusNNGraph  # noqa: F401
from . import pytorch  # noqa: F401
