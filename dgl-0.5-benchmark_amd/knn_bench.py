"""Segment k-NN benchmark: ops.segment_knn (csrc/knn.hip) against the padded cdist + topk form it replaces, and nn.EdgeConv fused
against composed.

The baseline is written here with plain torch operators and shares nothing with the package: scatter the points into a [B, max_len, D]
tensor, torch.cdist of it with itself (a [B, max_len, max_len] distance tensor), padding columns set to +inf, topk(k, largest=False),
local indices shifted to global rows.  (cdist takes the expansion form above 25 rows; that is what a user of plain torch gets.)
Shapes:
  clouds-D{3,64,128}   32 clouds of 1024 points, k = 20 and 40: a DGCNN batch, the graph of every layer
  molhiv-256           256 molecule-sized segments (normal(25.5, 12) clipped to [2, 222]), D = 64, k = 2 (every segment has k rows)
  one-16384            one segment of 16 384 points, D = 3, k = 20
  edgeconv             nn.EdgeConv(64, 64) on the k = 20 graph of 32 x 1024 points, forward and forward + backward, config.EDGECONV_FUSED
                       on and off
Timing: HIP events around `--inner` back-to-back calls, `--reps` windows kept after two discarded ones (kernel_bench.time_op); mean, min
and max per call in microseconds; the two forms alternate and the better window mean of two rounds is kept.  Peak memory: the growth of
torch.cuda.max_memory_allocated over one call.  The neighbour SETS of both forms are compared before timing (fp32 cdist orders near-ties
differently: the share of rows whose sets agree is printed, not asserted)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402


def shapes():
    rng = np.random.default_rng(5)
    out = [("clouds-D%d" % D, np.full(32, 1024, np.int64), D, k) for D in (3, 64, 128) for k in (20, 40)]
    out.append(("molhiv-256", np.clip(np.round(rng.normal(25.5, 12.0, 256)), 2, 222).astype(np.int64), 64, 2))
    out.append(("one-16384", np.array([16384], np.int64), 3, 20))
    return out


def cdist_topk(seglen, x, k, max_len):
    """The baseline: global neighbour rows [N, k] (-1 past a short segment's end).  max_len is a host number known from batching."""
    B, N, D = seglen.shape[0], x.shape[0], x.shape[1]
    offsets = torch.zeros(B + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(seglen, 0, out=offsets[1:])
    seg = torch.repeat_interleave(torch.arange(B, device=x.device), seglen, output_size=N)
    local = torch.arange(N, device=x.device) - offsets[seg]
    padded = x.new_zeros((B * max_len, D)).index_copy(0, seg * max_len + local, x).view(B, max_len, D)
    d = torch.cdist(padded, padded)                                              # [B, max_len, max_len]
    d = d.masked_fill(torch.arange(max_len, device=x.device).view(1, 1, -1) >= seglen.view(B, 1, 1), float("inf"))
    val, idx = d.topk(min(k, max_len), dim=2, largest=False)                     # [B, max_len, k]
    idx = torch.where(torch.isinf(val), idx.new_full((), -1), idx + offsets[:-1].view(B, 1, 1))
    return idx.view(B * max_len, -1)[seg * max_len + local]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def best_of(forms, inner, reps, rounds=2):
    def many(fn):
        def run():
            for _ in range(inner):
                fn()
        return run

    res = {}
    for _ in range(rounds):                                                      # alternate the forms: other work shares the machine
        for form, fn in forms.items():
            t = [v / inner for v in time_op(many(fn), reps + N_COLD)]
            if form not in res or t[0] < res[form][0]:
                res[form] = t
    return res


def main():
    p = argparse.ArgumentParser("segment k-NN: fused kernel vs padded cdist + topk; EdgeConv fused vs composed")
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--shapes", default="", help="comma-separated subset of the shape names (edgeconv is one)")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    torch.cuda.set_device(dev)
    pick = args.shapes.split(",") if args.shapes else None
    rows = []
    for name, lens, D, k in shapes():
        if pick and name not in pick:
            continue
        S, N, max_len = len(lens), int(lens.sum()), int(lens.max())
        seglen = torch.from_numpy(lens).to(dev)
        x = torch.randn(N, D, device=dev, generator=torch.Generator(device=dev).manual_seed(S + D))
        assert ops.segment_knn_fused(seglen, x, k)
        forms = {"fused": lambda: ops.segment_knn(seglen, x, k, total=N), "baseline": lambda: cdist_topk(seglen, x, k, max_len)}
        with torch.no_grad():
            got, want = forms["fused"]().sort(dim=1).values, forms["baseline"]().sort(dim=1).values
            agree = float((got == want).all(dim=1).float().mean())
            res = {"shape": name, "segments": S, "rows": N, "D": D, "k": k, "same_neighbour_sets": agree,
                   "baseline_distance_bytes": S * max_len * max_len * 4}
            for form, fn in forms.items():
                res[form + "_peak_bytes"] = peak_bytes(fn)
            res.update({form + "_fwd": t for form, t in best_of(forms, args.inner, args.reps).items()})
        f, c = res["fused_fwd"], res["baseline_fwd"]
        print("%-12s D %-3d k %-2d fused %9.1f us [min %.1f max %.1f] peak %7.2f MB   baseline %9.1f us [min %.1f max %.1f] peak %7.2f MB   "
              "ratio %.2fx   same sets %.4f" % (name, D, k, f[0] * 1e6, f[1] * 1e6, f[2] * 1e6, res["fused_peak_bytes"] / 1e6, c[0] * 1e6,
                                              c[1] * 1e6, c[2] * 1e6, res["baseline_peak_bytes"] / 1e6, c[0] / f[0], agree), flush=True)
        rows.append(res)
    if not pick or "edgeconv" in pick:
        B, n, D, k = 32, 1024, 64, 20
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(B * n, D, device=dev, generator=gen).requires_grad_(True)
        up = torch.randn(B * n, D, device=dev, generator=gen)
        g = dgl.knn_graph(x.detach().view(B, n, D), k)
        conv = dgl.nn.EdgeConv(D, D).to(dev)

        def form(fused, backward):
            def run():
                config.EDGECONV_FUSED = fused
                if not backward:
                    with torch.no_grad():
                        return conv(g, x)
                x.grad = None
                conv.zero_grad(set_to_none=True)
                out = conv(g, x)
                out.backward(up)
                return out
            return run

        res = {"shape": "edgeconv", "rows": B * n, "D": D, "k": k}
        for leg, backward in (("fwd", False), ("fwd_bwd", True)):
            forms = {"fused": form(True, backward), "composed": form(False, backward)}
            for name, fn in forms.items():
                res["%s_%s_peak_bytes" % (name, leg)] = peak_bytes(fn)
            for name, t in best_of(forms, args.inner, args.reps).items():
                res["%s_%s" % (name, leg)] = t
            f, c = res["fused_" + leg], res["composed_" + leg]
            print("edgeconv %-7s fused %9.1f us [min %.1f max %.1f] peak %7.2f MB   composed %9.1f us [min %.1f max %.1f] peak %7.2f MB   ratio %.2fx"
                  % (leg, f[0] * 1e6, f[1] * 1e6, f[2] * 1e6, res["fused_%s_peak_bytes" % leg] / 1e6, c[0] * 1e6, c[1] * 1e6, c[2] * 1e6,
                     res["composed_%s_peak_bytes" % leg] / 1e6, c[0] / f[0]), flush=True)
        config.EDGECONV_FUSED = True
        rows.append(res)
    print(json.dumps({"knn_bench": rows, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
