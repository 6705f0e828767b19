"""Attention readout benchmark: the fused pair of csrc/segattn.hip against the composition it replaces.

ops.segment_attention in gate mode (GlobalAttentionPooling) and in query mode (Set2Set), forward and forward + backward, with
config.SEGMENT_ATTENTION_FUSED on (one launch each way) and off (segment max -> gather -> exp -> segment sum -> gather -> multiply ->
segment sum through segment_reduce and row gathers: the operators that existed before), on
  molhiv   256 graphs drawn by the package's small-graph generator (datasets.molhiv_like), D = 256: the batch of graph_classification.py
  long     8 segments of 4096 rows, D = 64: few, long segments -- one wave walks a segment, so this is the kernels' weak side
Timing: HIP events around `--inner` back-to-back calls (one call is tens of microseconds: a window of one would time the event pair), `--reps`
windows kept after two discarded ones (kernel_bench.time_op drops its first two); mean, min and max per call, all in microseconds.
Both forms are checked against each other before they are timed."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402


def shapes(dev):
    from mi355x_graph.datasets import molhiv_like
    data = molhiv_like(256, seed=5)
    lens = torch.tensor([data[i][0].number_of_nodes() for i in range(256)], dtype=torch.int64)
    return [("molhiv", lens.to(dev), 256), ("long", torch.full((8,), 4096, dtype=torch.int64, device=dev), 64)]


def main():
    p = argparse.ArgumentParser("attention readout: fused pair vs composition")
    p.add_argument("--reps", type=int, default=12)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--device", type=int, default=0)
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    rows = []
    for name, seglen, D in shapes(dev):
        S, N = int(seglen.shape[0]), int(seglen.sum())
        gen = torch.Generator(device=dev).manual_seed(D)
        feat = torch.randn(N, 1, D, device=dev, generator=gen).requires_grad_(True)
        up = torch.randn(S, 1, D, device=dev, generator=gen)
        for mode in ("gate", "query"):
            if mode == "gate":
                other = torch.randn(N, 1, device=dev, generator=gen).requires_grad_(True)
                kw = {"logits": other}
            else:
                other = (torch.randn(S, 1, D, device=dev, generator=gen) / D ** 0.5).requires_grad_(True)
                kw = {"query": other}

            def fwd():
                return ops.segment_attention(seglen, feat, total=N, **kw)

            def fwd_bwd():
                feat.grad = other.grad = None
                fwd().backward(up)

            def many(fn):
                def run():
                    for _ in range(args.inner):
                        fn()
                return run

            res = {"shape": name, "segments": S, "rows": N, "D": D, "mode": mode}
            outs = {}
            for form, flag in (("fused", True), ("composed", False)):
                config.SEGMENT_ATTENTION_FUSED = flag
                assert ops.segment_attention_fused(seglen, feat, **kw) == flag
                fwd_bwd()
                outs[form] = (fwd().detach(), feat.grad.clone(), other.grad.clone())
            for a, b in zip(outs["fused"], outs["composed"]):
                err = float((a - b).abs().max() / b.abs().max())
                assert err < 1e-4, "fused and composed disagree: %g" % err
            for _ in range(2):                                      # alternate the two forms: other work shares the machine
                for form, flag in (("fused", True), ("composed", False)):
                    config.SEGMENT_ATTENTION_FUSED = flag
                    with torch.no_grad():
                        t = [v / args.inner for v in time_op(many(fwd), args.reps + N_COLD)]
                    tb = [v / args.inner for v in time_op(many(fwd_bwd), args.reps + N_COLD)]
                    if form + "_fwd" not in res or t[0] < res[form + "_fwd"][0]:
                        res[form + "_fwd"] = t
                    if form + "_fwd_bwd" not in res or tb[0] < res[form + "_fwd_bwd"][0]:
                        res[form + "_fwd_bwd"] = tb
            config.SEGMENT_ATTENTION_FUSED = True
            for leg in ("fwd", "fwd_bwd"):
                f, c = res["fused_" + leg], res["composed_" + leg]
                print("%-7s %-5s %-8s fused %8.1f us [min %.1f max %.1f]   composed %8.1f us [min %.1f max %.1f]   ratio %.2fx" % (
                    name, mode, leg, f[0] * 1e6, f[1] * 1e6, f[2] * 1e6, c[0] * 1e6, c[1] * 1e6, c[2] * 1e6, c[0] / f[0]))
            rows.append(res)
    print(json.dumps({"readout_bench": rows, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
