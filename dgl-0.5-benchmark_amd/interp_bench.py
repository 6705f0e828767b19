"""Query-set k-NN and interpolation benchmark: ops.segment_knn_query (csrc/knn.hip) + the u_mul_e / sum g-SpMM
(dgl.geometry.knn_interpolate) against the padded composition in plain torch they replace, and the pointnet2_seg.py epoch eager and
--hipgraph.

The baseline is written here with plain torch operators and shares nothing with the package:
  search        the padded [B, m, n, D] difference tensor, its squares summed to [B, m, n], torch.topk(k, largest=False), the weights
                (1 / (d + eps)) / sum
  interpolate   ... and the gather of the k neighbours' features ([B, m, k, C]), times the weights, summed over k
Shapes (queries <- references per cloud; for D = 3 the references are the farthest point samples of the queries, as in PointNet++, for
D = 64 the first n of the random queries):
  32x(512<-128) C 256, 32x(1024<-512) C 128    the two feature-propagation levels of pointnet2_seg.py: search + interpolation, k = 3
  16x(4096<-1024), 1x(8192<-1024)               search alone, k = 3
  8x(1024<-512) D 64 k 16                        search alone among feature vectors
  epoch                                          pointnet2_seg.py on 256 clouds, eager and --hipgraph (its own "Training time/epoch")
Timing: HIP events around `--inner` back-to-back calls, `--reps` windows kept after two discarded ones (kernel_bench.time_op); mean, min
and max per call in microseconds; the two forms alternate and the better window mean of two rounds is kept.  Peak memory: the growth of
torch.cuda.max_memory_allocated over one call.  Agreement: the share of queries whose neighbour rows are identical in both forms, and the
largest difference of the interpolated features (fp32 orders near-ties differently in the two forms: printed, not asserted)."""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
import dgl.geometry  # noqa: E402
from fps_bench import line, run_pair  # noqa: E402
from mi355x_graph import ops  # noqa: E402
from mi355x_graph.datasets import shapes_like  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-8

#         name                     clouds queries references D   k   C (0: search alone)
SHAPES = (("32x(512<-128) C256", 32, 512, 128, 3, 3, 256),
          ("32x(1024<-512) C128", 32, 1024, 512, 3, 3, 128),
          ("16x(4096<-1024)", 16, 4096, 1024, 3, 3, 0),
          ("1x(8192<-1024)", 1, 8192, 1024, 3, 3, 0),
          ("8x(1024<-512) D64 k16", 8, 1024, 512, 64, 16, 0))


def torch_search(x, y, k):
    """The baseline: x [B, n, D] references, y [B, m, D] queries -> (global rows [B * m, k], weights [B * m, k])"""
    B, n, _ = x.shape
    diff = y.unsqueeze(2) - x.unsqueeze(1)                                       # [B, m, n, D]
    d, index = (diff * diff).sum(-1).topk(k, dim=2, largest=False)               # [B, m, k]
    inv = 1.0 / (d + EPS)
    weight = inv / inv.sum(-1, keepdim=True)
    return (index + (torch.arange(B, device=x.device) * n).view(B, 1, 1)).view(-1, k), weight.view(-1, k)


def torch_interpolate(x, y, k, feat):
    """... and feat [B * n, C] -> [B * m, C]"""
    index, weight = torch_search(x, y, k)
    return (feat[index] * weight.unsqueeze(-1)).sum(1)                           # the gather is [B * m, k, C]


def main():
    p = argparse.ArgumentParser("query-set k-NN + interpolation: fused kernels vs the padded torch composition; the pointnet2_seg.py epoch")
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--shapes", default="", help="comma-separated subset: shape names, epoch")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    torch.cuda.set_device(dev)
    pick = args.shapes.split(",") if args.shapes else None
    rows = []
    for name, B, m, n, D, k, C in SHAPES:
        if pick and name not in pick:
            continue
        gen = torch.Generator(device=dev).manual_seed(m + D)
        if D == 3:
            y = shapes_like(B, m, seed=3)[0].reshape(B * m, 3).to(dev)
        else:
            y = torch.randn(B * m, D, device=dev, generator=gen)
        q_seglen = torch.full((B,), m, dtype=torch.int64, device=dev)
        r_seglen = torch.full((B,), n, dtype=torch.int64, device=dev)
        if D == 3:
            x = y[ops.segment_fps(q_seglen, y, n, total=B * m, max_len=m).flatten()].contiguous()
        else:
            x = y.view(B, m, D)[:, :n].reshape(B * n, D).contiguous()
        assert ops.segment_knn_query_fused(r_seglen, x, q_seglen, y, k, B * n, B * m)
        x3, y3 = x.view(B, n, D), y.view(B, m, D)
        res = {"shape": name, "clouds": B, "queries": B * m, "references": B * n, "D": D, "k": k, "C": C,
               "baseline_difference_bytes": B * m * n * D * 4}
        with torch.no_grad():
            index = ops.segment_knn_query(r_seglen, x, q_seglen, y, k, ref_total=B * n, query_total=B * m)
            res["same_rows"] = float((index.sort(1).values == torch_search(x3, y3, k)[0].sort(1).values).all(dim=1).float().mean())
            if C:
                feat = torch.randn(B * n, C, device=dev, generator=gen)
                forms = {"fused": lambda: dgl.geometry.knn_interpolate(feat, x, y, [n] * B, [m] * B, k),
                         "baseline": lambda: torch_interpolate(x3, y3, k, feat)}
                res["max_abs_diff"] = float((forms["fused"]() - forms["baseline"]()).abs().max())
            else:
                forms = {"fused": lambda: ops.segment_knn_query(r_seglen, x, q_seglen, y, k, ref_total=B * n, query_total=B * m,
                                                                return_weight=True),
                         "baseline": lambda: torch_search(x3, y3, k)}
            run_pair(res, forms, args.inner, args.reps)
        line(res["shape"], res, "fused", "baseline")
        rows.append(res)
    if not pick or "epoch" in pick:
        res = {"shape": "pointnet2_seg.py epoch", "clouds": 256, "batch": 32, "points": 1024}
        for mode in ("eager", "hipgraph"):
            cmd = [sys.executable, os.path.join(HERE, "pointnet2_seg.py"), "--clouds", "256", "--epochs", "4", "--device", str(args.device)]
            out = subprocess.run(cmd + (["--hipgraph"] if mode == "hipgraph" else []), env=dict(os.environ, PYTHONPATH=HERE),
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
            found = re.search(r"Training time/epoch (\S+)", out.stdout)
            if out.returncode != 0 or not found:
                raise RuntimeError("pointnet2_seg.py %s failed:\n%s" % (mode, out.stdout[-3000:]))
            res[mode + "_epoch_s"] = float(found.group(1))
            res[mode + "_losses"] = [float(v) for v in re.findall(r"epoch \d+ loss (\S+)", out.stdout)]
        print("pointnet2_seg.py epoch (8 steps of 32 x 1024)   eager %.4f s   hipgraph %.4f s   ratio %.2fx"
              % (res["eager_epoch_s"], res["hipgraph_epoch_s"], res["eager_epoch_s"] / res["hipgraph_epoch_s"]), flush=True)
        rows.append(res)
    print(json.dumps({"interp_bench": rows, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
