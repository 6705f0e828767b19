"""Farthest point sampling and ball query benchmark: ops.segment_fps (csrc/fps.hip) and ops.segment_ball_query (csrc/ballquery.hip)
against the plain-torch forms they replace, nn.PointNetConv fused against composed, and the pointnet2.py epoch eager and --hipgraph.

The baselines are written here with plain torch operators and share nothing with the package:
  fps    the padded [B, n, D] loop: per sample a gather of the current points, the distances to them, `minimum` into the running
         distance, `argmax` -- four to five small launches per sample and nothing between them (ragged batches: padding masked with -1)
  ball   torch.cdist of the centres against the padded points (a [B, m, n] tensor), the mask d <= radius, the first K by a sort of the
         masked positions, padded with the first
Shapes:
  32x1024-512, 32x512-128, 16x4096-1024, 1x8192-1024 (D = 3)   the sampling of a PointNet++ level, and one large cloud
  molhiv-256                                                   256 molecule-sized segments (normal(25.5, 12) clipped to [8, 222]), D = 3, 8 samples
  ball 32x1024-512 (r 0.2, K 32) and 32x512-128 (r 0.4, K 64)  the grouping of the two levels, centres from the sampling
  pointnetconv                                                 PointNetConv(0, (64,)) on the first level's block, forward and forward + backward
  epoch                                                        pointnet2.py on 256 clouds, eager and --hipgraph (its own "Training time/epoch")
Timing: HIP events around `--inner` back-to-back calls, `--reps` windows kept after two discarded ones (kernel_bench.time_op); mean, min
and max per call in microseconds; the two forms alternate and the better window mean of two rounds is kept.  Peak memory: the growth of
torch.cuda.max_memory_allocated over one call.  Agreement with the baseline is the share of rows (clouds for fps, queries for ball) whose
results are identical (fp32 orders near-ties differently in the two forms: printed, not asserted)."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
import dgl.geometry  # noqa: E402
from knn_bench import best_of, peak_bytes  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402
from mi355x_graph.datasets import shapes_like  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def fps_shapes():
    rng = np.random.default_rng(5)
    out = [("32x1024-512", np.full(32, 1024, np.int64), 512), ("32x512-128", np.full(32, 512, np.int64), 128),
           ("16x4096-1024", np.full(16, 4096, np.int64), 1024), ("1x8192-1024", np.array([8192], np.int64), 1024)]
    out.append(("molhiv-256", np.clip(np.round(rng.normal(25.5, 12.0, 256)), 8, 222).astype(np.int64), 8))
    return out


def pad(seglen, x, max_len):
    """x [N, D] -> (padded [B, max_len, D], valid [B, max_len], offsets [B])"""
    B, N, D = seglen.shape[0], x.shape[0], x.shape[1]
    offsets = torch.zeros(B + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(seglen, 0, out=offsets[1:])
    seg = torch.repeat_interleave(torch.arange(B, device=x.device), seglen, output_size=N)
    local = torch.arange(N, device=x.device) - offsets[seg]
    padded = x.new_zeros((B * max_len, D)).index_copy(0, seg * max_len + local, x).view(B, max_len, D)
    valid = torch.arange(max_len, device=x.device).view(1, -1) < seglen.view(B, 1)
    return padded, valid, offsets[:-1]


def torch_fps(padded, valid, offsets, npoints):
    """The baseline: global rows [B, npoints], row 0 of every cloud first."""
    B, n, _ = padded.shape
    rows = torch.arange(B, device=padded.device)
    index = torch.empty((B, npoints), dtype=torch.int64, device=padded.device)
    mind = torch.where(valid, padded.new_full((), float("inf")), padded.new_full((), -1.0))
    cur = torch.zeros(B, dtype=torch.int64, device=padded.device)
    for t in range(npoints):
        index[:, t] = cur
        centre = padded[rows, cur]                                               # gather [B, D]
        d = ((padded - centre.unsqueeze(1)) ** 2).sum(-1)
        mind = torch.minimum(mind, d)
        cur = mind.argmax(1)
    return index + offsets.unsqueeze(1)


def torch_ball(padded, centres_local, offsets, radius, K):
    """The baseline: global rows [B * m, K], padded with the first.  centres_local [B, m] rows inside each cloud."""
    B, n, D = padded.shape
    c = padded.gather(1, centres_local.unsqueeze(2).expand(-1, -1, D))
    inside = torch.cdist(c, padded) <= radius                                    # [B, m, n]
    where = torch.where(inside, torch.arange(n, device=padded.device).view(1, 1, n), n)
    first = where.sort(dim=2).values[:, :, :K]
    first = torch.where(first == n, first[:, :, :1], first)
    return (first + offsets.view(B, 1, 1)).view(-1, K)


def line(name, res, a, b):
    f, c = res[a + "_fwd"], res[b + "_fwd"]
    print("%-22s %s %10.1f us [min %.1f max %.1f] peak %8.2f MB   %s %10.1f us [min %.1f max %.1f] peak %8.2f MB   ratio %.2fx%s"
          % (name, a, f[0] * 1e6, f[1] * 1e6, f[2] * 1e6, res[a + "_peak_bytes"] / 1e6, b, c[0] * 1e6, c[1] * 1e6, c[2] * 1e6,
             res[b + "_peak_bytes"] / 1e6, c[0] / f[0], "   same rows %.4f" % res["same_rows"] if "same_rows" in res else ""), flush=True)


def run_pair(res, forms, inner, reps):
    for form, fn in forms.items():
        res[form + "_peak_bytes"] = peak_bytes(fn)
    res.update({form + "_fwd": t for form, t in best_of(forms, inner, reps).items()})


def main():
    p = argparse.ArgumentParser("farthest point sampling and ball query: fused kernels vs plain torch; PointNetConv; the pointnet2.py epoch")
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--shapes", default="", help="comma-separated subset: fps shape names, ball, pointnetconv, epoch")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    torch.cuda.set_device(dev)
    pick = args.shapes.split(",") if args.shapes else None
    rows = []
    for name, lens, m in fps_shapes():
        if pick and name not in pick:
            continue
        S, N, max_len = len(lens), int(lens.sum()), int(lens.max())
        seglen = torch.from_numpy(lens).to(dev)
        if S == 256:
            x = torch.randn(N, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(S))
        else:
            x = shapes_like(S, max_len, seed=3)[0].reshape(N, 3).to(dev)
        assert ops.segment_fps_fused(seglen, x, m, total=N, max_len=max_len)
        padded, valid, offsets = pad(seglen, x, max_len)
        forms = {"fused": lambda: ops.segment_fps(seglen, x, m, total=N, max_len=max_len),
                 "baseline": lambda: torch_fps(padded, valid, offsets, m)}
        with torch.no_grad():
            res = {"shape": "fps " + name, "segments": S, "rows": N, "D": 3, "npoints": m,
                   "same_rows": float((forms["fused"]() == forms["baseline"]()).all(dim=1).float().mean())}
            run_pair(res, forms, args.inner, args.reps)
        line(res["shape"], res, "fused", "baseline")
        rows.append(res)
    if not pick or "ball" in pick:
        for B, n, m, radius, K in ((32, 1024, 512, 0.2, 32), (32, 512, 128, 0.4, 64)):
            x = shapes_like(B, n, seed=3)[0].reshape(B * n, 3).to(dev)
            seglen = torch.full((B,), n, dtype=torch.int64, device=dev)
            centers = ops.segment_fps(seglen, x, m, total=B * n, max_len=n).flatten()
            local = (centers.view(B, m) - torch.arange(B, device=dev).unsqueeze(1) * n)
            padded, offsets = x.view(B, n, 3), torch.arange(B, device=dev) * n
            assert ops.segment_ball_query_fused(seglen, x, centers, radius, K)
            forms = {"fused": lambda: ops.segment_ball_query(seglen, x, centers, radius, K, total=B * n)[0],
                     "baseline": lambda: torch_ball(padded, local, offsets, radius, K)}
            with torch.no_grad():
                count = ops.segment_ball_query(seglen, x, centers, radius, K, total=B * n)[1].float()
                res = {"shape": "ball %dx%d-%d r%.1f K%d" % (B, n, m, radius, K), "queries": B * m, "rows": B * n, "K": K, "radius": radius,
                       "mean_count": float(count.mean()), "full_share": float((count == K).float().mean()),
                       "baseline_distance_bytes": B * m * n * 4,
                       "same_rows": float((forms["fused"]() == forms["baseline"]()).all(dim=1).float().mean())}
                run_pair(res, forms, args.inner, args.reps)
            line(res["shape"], res, "fused", "baseline")
            rows.append(res)
    if not pick or "pointnetconv" in pick:
        B, n, m, radius, K, width = 32, 1024, 512, 0.2, 32, 64
        x = shapes_like(B, n, seed=3)[0].reshape(B * n, 3).to(dev)
        seglen = torch.full((B,), n, dtype=torch.int64, device=dev)
        centers = ops.segment_fps(seglen, x, m, total=B * n, max_len=n).flatten()
        block = dgl.geometry.fixed_radius_block(x, centers, radius, K, [n] * B)
        conv = dgl.nn.PointNetConv(0, (width,)).to(dev)
        up = torch.randn(B * m, width, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

        def form(fused, backward):
            def run():
                config.POINTNETCONV_FUSED = fused
                if not backward:
                    with torch.no_grad():
                        return conv(block)
                conv.zero_grad(set_to_none=True)
                out = conv(block)
                out.backward(up)
                return out
            return run

        for leg, backward in (("fwd", False), ("fwd_bwd", True)):
            res = {"shape": "pointnetconv " + leg, "rows": B * n, "centres": B * m, "K": K, "width": width}
            run_pair(res, {"fused": form(True, backward), "composed": form(False, backward)}, args.inner, args.reps)
            line(res["shape"], res, "fused", "composed")
            rows.append(res)
        config.POINTNETCONV_FUSED = True
    if not pick or "epoch" in pick:
        res = {"shape": "pointnet2.py epoch", "clouds": 256, "batch": 32, "points": 1024}
        for mode in ("eager", "hipgraph"):
            cmd = [sys.executable, os.path.join(HERE, "pointnet2.py"), "--clouds", "256", "--epochs", "4", "--device", str(args.device)]
            out = subprocess.run(cmd + (["--hipgraph"] if mode == "hipgraph" else []), env=dict(os.environ, PYTHONPATH=HERE),
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
            found = re.search(r"Training time/epoch (\S+)", out.stdout)
            if out.returncode != 0 or not found:
                raise RuntimeError("pointnet2.py %s failed:\n%s" % (mode, out.stdout[-3000:]))
            res[mode + "_epoch_s"] = float(found.group(1))
            res[mode + "_losses"] = [float(v) for v in re.findall(r"epoch \d+ loss (\S+)", out.stdout)]
        print("pointnet2.py epoch (8 steps of 32 x 1024)   eager %.4f s   hipgraph %.4f s   ratio %.2fx"
              % (res["eager_epoch_s"], res["hipgraph_epoch_s"], res["eager_epoch_s"] / res["hipgraph_epoch_s"]), flush=True)
        rows.append(res)
    print(json.dumps({"fps_bench": rows, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
