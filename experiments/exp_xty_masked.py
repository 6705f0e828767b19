"""Layer-1 weight + bias gradient at the benchmark's N: relu_dropout_bwd + xty(colsum=True) (the parent's six launches) against
xty_masked (two launches), interleaved rounds in one process.  docs/LOG_xty_masked.md section 2; listing in profiles/xty_masked_kernel_level.txt.

    python experiments/exp_xty_masked.py [--n 2449029] [--rounds 5] [--reps 10]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-0.5-benchmark_amd"))
from mi355x_graph import sparse  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def line(name, ts):
    print("%-46s median %.3f  min %.3f  max %.3f ms  (%d calls)" % (name, statistics.median(ts), min(ts), max(ts), len(ts)))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2449029)
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = sparse.backend_for(torch.zeros(1, device=dev))
    gen = torch.Generator(device=dev).manual_seed(1)
    n, K = args.n, args.K
    _, mask = be.relu_dropout_fwd(torch.randn(n, 64, device=dev, generator=gen), 0.5, 11, 5)
    dy = torch.randn(n, 64, device=dev, generator=gen)
    b = torch.randn(n, K, device=dev, generator=gen)

    def parent():
        return be.xty(be.relu_dropout_bwd(dy, mask, 0.5), b, colsum=True)

    def elementwise():
        return be.relu_dropout_bwd(dy, mask, 0.5)

    dz = be.relu_dropout_bwd(dy, mask, 0.5)

    def xty_only():
        return be.xty(dz, b, colsum=True)

    def child():
        return be.xty_masked(dy, mask, 0.5, b)

    want, got = parent(), child()
    assert got is not None, "no masked kernel for K = %d" % K
    print("n = %d, K = %d; bitwise equal: out %s, colsum %s" % (n, K, torch.equal(want[0], got[0]), torch.equal(want[1], got[1])))
    for fn in (parent, elementwise, xty_only, child):
        timed(fn, 3)
    t = {"parent": [], "elementwise": [], "xty": [], "child": []}
    for r in range(args.rounds):
        t["parent"] += timed(parent, args.reps)
        t["child"] += timed(child, args.reps)
        t["elementwise"] += timed(elementwise, args.reps)
        t["xty"] += timed(xty_only, args.reps)
    p = line("relu_dropout_bwd + xty(colsum) (parent)", t["parent"])
    e = line("  relu_dropout_bwd alone", t["elementwise"])
    line("  xty(colsum) alone", t["xty"])
    c = line("xty_masked (child)", t["child"])
    print("gain %.3f ms; the elementwise pass alone %.3f ms; criterion (gain >= elementwise): %s" % (p - c, e, p - c >= e))
    gb = (n * 64 * 4 + n * 16 + n * K * 4) / 1e9
    print("child: %.2f GB of operands -> %.2f TB/s; %.1f TFLOP/s of fp32 MFMA (2 n 64 (K + 1))" % (gb, gb / c, 2 * n * 64 * (K + 1) / c / 1e9))


if __name__ == "__main__":
    main()
