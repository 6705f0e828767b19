"""Segment top-k benchmark: ops.segment_topk (csrc/segtopk.hip) against the pad-and-argsort form it replaces.

The baseline is written here with plain torch operators and shares nothing with the package: scatter the rows into a [B, max_len, D]
tensor filled with -inf (descending), argsort along the rows of every graph, keep k, gather, zero the padding -- what dgl.topk_nodes does
through pad_packed_tensor.  Both forms start from the device tensor of segment lengths and build their own offsets on every call.
Shapes (D = 64 everywhere, k in {8, 30, 64, 200}, rows ordered by the last column and every column on its own):
  molhiv-64 / -256 / -2048   batches of that many molecule-sized segments (normal(25.5, 12) clipped to [2, 222]: datasets.molhiv_like)
  ppa-32                     32 segments of about 243 rows (the shape of an ogbg-ppa batch)
  skewed                     255 molecule-sized segments and one of 200 000 rows: the baseline pads every segment to the longest one and
                             is not run when its padded tensor exceeds --max-padded-gb (the size is reported)
Timing: HIP events around `--inner` back-to-back calls, `--reps` windows kept after two discarded ones (kernel_bench.time_op); mean, min
and max per call in microseconds; the two forms alternate.  Device launches per call are counted once per form with torch.profiler (not
timed).  Both forms are checked against each other before they are timed (ties may order differently in the baseline: random keys)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import ops  # noqa: E402

D = 64
KS = (8, 30, 64, 200)


def shapes():
    rng = np.random.default_rng(5)

    def molecules(n):
        return np.clip(np.round(rng.normal(25.5, 12.0, n)), 2, 222).astype(np.int64)

    out = [("molhiv-%d" % n, molecules(n)) for n in (64, 256, 2048)]
    out.append(("ppa-32", np.clip(np.round(rng.normal(243.0, 40.0, 32)), 50, 300).astype(np.int64)))
    out.append(("skewed", np.concatenate([molecules(128), [200000], molecules(127)])))
    return out


def pad_argsort(seglen, feat, k, sortby, max_len):
    """The baseline: (values [B, k, D], index).  max_len is a host number known from batching, as in DGL."""
    B, N, width = seglen.shape[0], feat.shape[0], feat.shape[1]
    max_len = max(max_len, k)
    offsets = torch.zeros(B + 1, dtype=torch.int64, device=feat.device)
    torch.cumsum(seglen, 0, out=offsets[1:])
    seg = torch.repeat_interleave(torch.arange(B, device=feat.device), seglen, output_size=N)
    where = torch.arange(N, device=feat.device) - offsets[seg] + seg * max_len
    padded = feat.new_full((B * max_len, width), -float("inf"))
    padded = padded.index_copy(0, where, feat).view(B, max_len, width)
    if sortby is None:
        order = padded.argsort(dim=1, descending=True)[:, :k]
        values = padded.gather(1, order)
        live = order < seglen.view(B, 1, 1)
    else:
        order = padded[:, :, sortby].argsort(dim=1, descending=True)[:, :k]
        values = padded.gather(1, order.unsqueeze(-1).expand(B, k, width))
        live = order < seglen.view(B, 1)
    zero = values.new_zeros(())
    return torch.where(live if sortby is None else live.unsqueeze(-1), values, zero), torch.where(live, order, order.new_full((), -1))


def count_launches(fn):
    """device kernels and copies of one call, or None where the profiler is not usable"""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def main():
    p = argparse.ArgumentParser("segment top-k: fused kernel vs pad-and-argsort")
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--max-padded-gb", type=float, default=2.0)
    p.add_argument("--shapes", default="", help="comma-separated subset of the shape names")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    rows = []
    for name, lens in shapes():
        if args.shapes and name not in args.shapes.split(","):
            continue
        S, N, max_len = len(lens), int(lens.sum()), int(lens.max())
        seglen = torch.from_numpy(lens).to(dev)
        gen = torch.Generator(device=dev).manual_seed(S)
        feat = torch.randn(N, D, device=dev, generator=gen).requires_grad_(True)
        for k in KS:
            up = torch.randn(S, k, D, device=dev, generator=gen)
            padded_bytes = S * max(max_len, k) * D * 4
            for mode, sortby in (("rows", D - 1), ("columns", None)):
                forms = {"fused": lambda: ops.segment_topk(seglen, feat, k, sortby=sortby, total=N)}
                assert ops.segment_topk_fused(seglen, feat, k, sortby=sortby)
                if padded_bytes <= args.max_padded_gb * 2 ** 30:
                    forms["baseline"] = lambda: pad_argsort(seglen, feat, k, sortby, max_len)

                def fwd_bwd(fn):
                    def run():
                        feat.grad = None
                        fn()[0].backward(up)
                    return run

                def many(fn):
                    def run():
                        for _ in range(args.inner):
                            fn()
                    return run

                res = {"shape": name, "segments": S, "rows": N, "D": D, "k": k, "mode": mode, "baseline_padded_bytes": padded_bytes}
                if "baseline" in forms:
                    got, want = forms["fused"](), forms["baseline"]()
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "fused and baseline disagree"
                for form, fn in forms.items():
                    with torch.no_grad():
                        res[form + "_fwd_launches"] = count_launches(fn)
                    res[form + "_fwd_bwd_launches"] = count_launches(fwd_bwd(fn))
                for _ in range(2):                                      # alternate the forms: other work shares the machine
                    for form, fn in forms.items():
                        with torch.no_grad():
                            t = [v / args.inner for v in time_op(many(fn), args.reps + N_COLD)]
                        tb = [v / args.inner for v in time_op(many(fwd_bwd(fn)), args.reps + N_COLD)]
                        if form + "_fwd" not in res or t[0] < res[form + "_fwd"][0]:
                            res[form + "_fwd"] = t
                        if form + "_fwd_bwd" not in res or tb[0] < res[form + "_fwd_bwd"][0]:
                            res[form + "_fwd_bwd"] = tb
                for leg in ("fwd", "fwd_bwd"):
                    f = res["fused_" + leg]
                    line = "%-11s k %-3d %-7s %-7s fused %9.1f us [min %.1f max %.1f] launches %s" % (
                        name, k, mode, leg, f[0] * 1e6, f[1] * 1e6, f[2] * 1e6, res["fused_%s_launches" % leg])
                    if "baseline" in forms:
                        c = res["baseline_" + leg]
                        line += "   baseline %9.1f us [min %.1f max %.1f] launches %s   ratio %.2fx" % (
                            c[0] * 1e6, c[1] * 1e6, c[2] * 1e6, res["baseline_%s_launches" % leg], c[0] / f[0])
                    else:
                        line += "   baseline not run: padded tensor %.1f GB" % (padded_bytes / 1e9)
                    print(line + "   padded %.1f MB" % (padded_bytes / 1e6), flush=True)
                rows.append(res)
    print(json.dumps({"topk_bench": rows, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
