"""Typed linear layer benchmark: ops.segment_mm (csrc/segmm.hip) against the two compositions a user would write.

Forward and forward + backward (d a and d b) of out[p] = a[p] x b[seg(p)] for
  R = 1 / 8 / 64 / 133 weight matrices, n = 1 M and 6 M rows, equal and Zipf-skewed (length ~ 1 / rank) segment lengths,
  (K, M) = (16, 16), (64, 64), (128, 64)
as
  fused   ops.segment_mm: one launch each for out, d a, two for d b, whatever R
  loop    one torch.matmul per segment over row slices (host offsets known: no read-back inside the timed window)
  bmm     torch.bmm of the rows against an [n, K, M] gather of the weights; not run where that gather alone exceeds --bmm-gb
  rows    R = 1 only, forward: mgx_rows_gemm on the same shape (the one-weight kernel of csrc/rowsgemm.hip, unchanged by this file's kernels)
then --item-rows: the fused forward with config.SEGMENT_MM_ITEM_ROWS set to each value given, and --layer: one training step
(forward, loss, backward) of nn.TypedRelGraphConv on a synthetic graph of 133 relations, fused against composed.
Timing: HIP events around --inner back-to-back calls, --reps windows kept after two discarded ones, every form warmed first, all forms
in one process; mean / min / max per call in microseconds.  bytes = (n K + n M + R K M) * 4, the operands a forward must move once,
over the fused forward's time as a rate.  The forms are compared with each other before they are timed."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import config, nn as mnn, ops, sparse  # noqa: E402
import mi355x_graph as mg  # noqa: E402


def lengths(n, R, skew):
    if not skew:
        lens = torch.full((R,), n // R, dtype=torch.int64)
    else:
        w = 1.0 / torch.arange(1, R + 1, dtype=torch.float64)
        lens = (w / w.sum() * n).long()
    lens[0] += n - int(lens.sum())
    return lens


def timed(fn, args):
    def window():
        for _ in range(args.inner):
            fn()
    return [round(v / args.inner * 1e6, 1) for v in time_op(window, args.reps + N_COLD)]


def bench_shape(args, dev, n, R, skew, K, M):
    gen = torch.Generator(device=dev).manual_seed(n + R + K)
    a = torch.randn(n, K, device=dev, generator=gen).requires_grad_(True)
    b = torch.randn(R, K, M, device=dev, generator=gen).requires_grad_(True)
    up = torch.randn(n, M, device=dev, generator=gen)
    lens = lengths(n, R, skew)
    seglen, ends = lens.to(dev), [0] + torch.cumsum(lens, 0).tolist()
    types = torch.repeat_interleave(torch.arange(R, device=dev), seglen)
    assert ops.segment_mm_fused(a, b, seglen, total=n)
    forms = {"fused": lambda: ops.segment_mm(a, b, seglen, total=n),
             "loop": lambda: torch.cat([torch.matmul(a[s:e], b[r]) for r, (s, e) in enumerate(zip(ends[:-1], ends[1:])) if e > s], 0)}
    if n * K * M * 4 <= args.bmm_gb * 2 ** 30:
        forms["bmm"] = lambda: torch.bmm(a.unsqueeze(1), b[types]).squeeze(1)
    res = {"n": n, "R": R, "skew": skew, "K": K, "M": M}
    want = forms["loop"]().detach()
    for name, fn in forms.items():
        assert torch.allclose(fn().detach(), want, rtol=1e-4, atol=1e-3 * K ** 0.5), name

        def step(fn=fn):
            a.grad = b.grad = None
            fn().backward(up)
        with torch.no_grad():
            res[name + "_fwd_us"] = timed(fn, args)
        res[name + "_fwd_bwd_us"] = timed(step, args)
    if R == 1:
        be = sparse.backend_for(a)
        with torch.no_grad():
            if be.rows_gemm(a.detach(), b.detach()[0]) is not None:
                res["rows_fwd_us"] = timed(lambda: be.rows_gemm(a.detach(), b.detach()[0]), args)
    res["fused_fwd_TBps"] = round((n * K + n * M + R * K * M) * 4 / res["fused_fwd_us"][0] / 1e6, 2)
    return res


def bench_item_rows(args, dev):
    out, default = [], config.SEGMENT_MM_ITEM_ROWS
    for n, R, skew, K, M in ((1000000, 133, True, 64, 64), (1000000, 8, False, 64, 64), (6000000, 133, False, 64, 64), (1000000, 133, True, 16, 16),
                             (1000000, 133, True, 128, 64)):
        a, b = torch.randn(n, K, device=dev), torch.randn(R, K, M, device=dev)
        seglen = lengths(n, R, skew).to(dev)
        res = {"n": n, "R": R, "skew": skew, "K": K, "M": M}
        for rounds in range(2):  # alternating: every value twice, the smaller mean kept
            for rows in args.item_rows:
                config.SEGMENT_MM_ITEM_ROWS = rows
                t = timed(lambda: ops.segment_mm(a, b, seglen, total=n), args)
                key = "item_rows_%d_us" % rows
                res[key] = t if key not in res or t[0] < res[key][0] else res[key]
        out.append(res)
    config.SEGMENT_MM_ITEM_ROWS = default
    return out


def bench_layer(args, dev):
    N, E, R, D = 200000, 2000000, 133, 64
    gen = torch.Generator().manual_seed(1)
    src, dst = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    etypes = torch.multinomial(1.0 / torch.arange(1, R + 1, dtype=torch.float64), E, replacement=True, generator=gen).to(dev)
    g = mg.graph((src, dst), num_nodes=N).int().to(dev)
    feat, norm = torch.randn(N, D, generator=gen).to(dev), torch.rand(E, 1, generator=gen).to(dev)
    layer = mnn.TypedRelGraphConv(D, D, R, activation=torch.relu).to(dev)
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        layer(g, feat, etypes, norm=norm).square().mean().backward()
        opt.step()

    res = {"nodes": N, "edges": E, "R": R, "D": D}
    for form, flag in (("fused", True), ("composed", False), ("fused", True), ("composed", False)):
        config.SEGMENT_MM = flag
        t = timed(step, args)
        key = form + "_step_us"
        res[key] = t if key not in res or t[0] < res[key][0] else res[key]
    config.SEGMENT_MM = True
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+", default=[1000000, 6000000])
    p.add_argument("--R", type=int, nargs="+", default=[1, 8, 64, 133])
    p.add_argument("--shapes", type=int, nargs="+", default=[16, 16, 64, 64, 128, 64], help="K M pairs")
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--bmm-gb", type=float, default=8.0)
    p.add_argument("--item-rows", type=int, nargs="*", default=[])
    p.add_argument("--layer", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segmm_bench.py needs the GPU: a host timing says nothing about these kernels")
    dev = torch.device("cuda:0")
    results = {"shapes": [], "item_rows": [], "layer": None}
    time_op(lambda: torch.randn(1 << 20, device=dev).sum(), 3)  # the process's first measurement is discarded whole
    if args.item_rows:
        results["item_rows"] = bench_item_rows(args, dev)
        for r in results["item_rows"]:
            print(json.dumps(r), flush=True)
    for n in args.rows:
        for R in args.R:
            for skew in ((False,) if R == 1 else (False, True)):
                for K, M in zip(args.shapes[::2], args.shapes[1::2]):
                    results["shapes"].append(bench_shape(args, dev, n, R, skew, K, M))
                    print(json.dumps(results["shapes"][-1]), flush=True)
    if args.layer:
        results["layer"] = bench_layer(args, dev)
        print(json.dumps(results["layer"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
