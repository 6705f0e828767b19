"""Multi-aggregator message benchmark: the fused walks of csrc/multiagg.hip against the composition they replace.

ops.multi_aggregate(g, x, aggregators, w) forward + backward (d x, and d w with w), with config.MULTI_AGG_FUSED on (one launch each way,
nothing of size E written but d w) and off (one g-SpMM per aggregate -- two for std -- through the operators that existed before, over
the [E, D] messages gsddmm(copy_lhs) + w when w is given), on
  molhiv-64 / -256 / -2048   batches of 64, 256 and 2048 graphs of the package's small-graph generator (datasets.molhiv_like)
  ppa-32                     32 graphs of 240 nodes and 2 300 random edges each (the shape of an ogbg-ppa batch)
for D = 64 and 256, with and without w, the four PNA aggregates (mean, max, min, std) and ("max",) alone, then ("sum",), ("mean",) and
("min",) alone at the first width without w; then one training step of
graph_classification.py's --model pna (emb_dim 64, 3 layers, a molhiv batch of 256 graphs) with the switch on and off.
Timing: HIP events around `--inner` back-to-back calls (one call is tens of microseconds: a window of one would time the event pair),
`--reps` windows kept after two discarded ones, every form warmed by `--inner` calls first and the process's first measurement
discarded whole, the two forms alternating in one process; mean, min and max per call in microseconds.
Also per form the peak allocation of one forward + backward above its inputs, and for the fused kernels the algorithmic bytes
  forward   E D 4 (x rows) [+ E D 4 (w)] read + N A D 4 written [+ 2 N D 4 stats, 2 N D 4 args] + 8 E + 4 N of ids
  backward  E D 4 per gathered destination row (A; B with var / std; g and arg per max / min) [+ E D 4 (w) read, E D 4 (d w) written]
            + N D 4 (x) + N D 4 (d x) + ids
over the time of the pair, as a rate in TB/s.  These are the bytes the walks REQUEST: gathered rows repeat (a source row is read once per
out-edge) and mostly hit the L2, so the rate is not an HBM rate and can exceed the 8 TB/s HBM peak; it is a whole-call figure that
includes autograd's N-sized launches.
Both forms are checked against each other before they are timed."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from gine_bench import shapes  # noqa: E402
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402

PNA4 = ("mean", "max", "min", "std")


def many(fn, inner):
    def run():
        for _ in range(inner):
            fn()
    return run


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def alternate(fn, args, res, key):
    """time fn() with the switch on and off, twice each, alternating; keep the window set with the smaller mean per form"""
    for _ in range(2):
        for form, flag in (("fused", True), ("composed", False)):
            config.MULTI_AGG_FUSED = flag
            t = [v / args.inner for v in time_op(many(fn, args.inner), args.reps + N_COLD)]
            if form + key not in res or t[0] < res[form + key][0]:
                res[form + key] = t
    config.MULTI_AGG_FUSED = True


def bench_op(args, dev, name, g, D, with_w, aggs, quiet=False):
    N, E, A = g.number_of_nodes(), g.number_of_edges(), len(aggs)
    gen = torch.Generator(device=dev).manual_seed(N + D)
    x = torch.randn(N, D, device=dev, generator=gen).requires_grad_(True)
    w = torch.randn(E, D, device=dev, generator=gen).requires_grad_(True) if with_w else None
    up = torch.randn(N, A, D, device=dev, generator=gen)

    def fwd_bwd():
        x.grad = None
        if w is not None:
            w.grad = None
        ops.multi_aggregate(g, x, aggs, w=w).backward(up)

    res = {"shape": name, "nodes": N, "edges": E, "D": D, "w": with_w, "aggregators": "+".join(aggs)}
    outs = {}
    for form, flag in (("fused", True), ("composed", False)):
        config.MULTI_AGG_FUSED = flag
        assert ops.multi_aggregate_fused(g, x, aggs, w) == flag, (name, D, with_w, aggs)
        fwd_bwd()
        outs[form] = [ops.multi_aggregate(g, x, aggs, w=w).detach(), x.grad.clone()] + ([w.grad.clone()] if with_w else [])
        res[form + "_peak_bytes"] = peak(fwd_bwd)
    for a, b in zip(outs["fused"], outs["composed"]):
        err = float((a - b).abs().max() / b.abs().max())
        assert err < 1e-3, "fused and composed disagree: %g" % err
    for flag in (True, False):                      # every form of every shape is warm before its first timed window
        config.MULTI_AGG_FUSED = flag
        many(fwd_bwd, args.inner)()
    alternate(fwd_bwd, args, res, "_fwd_bwd")
    if quiet:
        return res
    sq, mm = ("std" in aggs or "var" in aggs), ("max" in aggs or "min" in aggs)
    ids = 8 * E + 4 * N
    fwd_b = E * D * 4 * (2 if with_w else 1) + N * A * D * 4 + (2 * N * D * 4 if sq else 0) + (2 * N * D * 4 if mm else 0) + ids
    rows_gathered = 1 + (1 if sq else 0) + 2 * sum(1 for a in ("max", "min") if a in aggs)
    bwd_b = E * D * 4 * (rows_gathered + (2 if with_w else 0)) + 2 * N * D * 4 + ids
    res["fwd_bytes"], res["bwd_bytes"] = fwd_b, bwd_b
    f_, c_ = res["fused_fwd_bwd"], res["composed_fwd_bwd"]
    res["pair_requested_TBps"] = (fwd_b + bwd_b) / f_[0] / 1e12
    print("%-11s N %6d E %6d D %3d w %-5s %-16s fused %8.1f us [min %.1f max %.1f]   composed %8.1f us [min %.1f max %.1f]   ratio %.2fx   "
          "peak %.2f / %.2f MB   fused pair requests %.1f MB -> %.2f TB/s"
          % (name, N, E, D, with_w, res["aggregators"], f_[0] * 1e6, f_[1] * 1e6, f_[2] * 1e6, c_[0] * 1e6, c_[1] * 1e6, c_[2] * 1e6,
             c_[0] / f_[0], res["fused_peak_bytes"] / 1e6, res["composed_peak_bytes"] / 1e6, (fwd_b + bwd_b) / 1e6,
             res["pair_requested_TBps"]))
    return res


def bench_model(args, dev):
    import graph_classification as gc
    from mi355x_graph.datasets import molhiv_like
    from dgl.dataloading import GraphDataLoader
    data = molhiv_like(256, seed=5)
    bg, labels = next(iter(GraphDataLoader(data, batch_size=256, shuffle=False)))
    g = bg.to(dev).int().formats("coo")
    labels = labels.to(dev).float().view(-1)
    torch.manual_seed(0)
    model = gc.PNA(64, 1, 3, 0.0, delta=gc.pna_delta(data)).to(dev)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        out = model(g, g.ndata["feat"], g.edata["feat"])
        F.binary_cross_entropy_with_logits(out.float().view(-1), labels).backward()
        opt.step()

    res = {"shape": "molhiv-256 --model pna, emb_dim 64, 3 layers", "nodes": g.number_of_nodes(), "edges": g.number_of_edges()}
    for form, flag in (("fused", True), ("composed", False)):
        config.MULTI_AGG_FUSED = flag
        step()
        res[form + "_peak_bytes"] = peak(step)
    alternate(step, args, res, "_step")
    f_, c_ = res["fused_step"], res["composed_step"]
    print("model step  %s: fused %8.1f us [min %.1f max %.1f]   composed %8.1f us [min %.1f max %.1f]   ratio %.2fx   peak %.2f / %.2f MB"
          % (res["shape"], f_[0] * 1e6, f_[1] * 1e6, f_[2] * 1e6, c_[0] * 1e6, c_[1] * 1e6, c_[2] * 1e6, c_[0] / f_[0],
             res["fused_peak_bytes"] / 1e6, res["composed_peak_bytes"] / 1e6))
    return res


def main():
    p = argparse.ArgumentParser("sum / mean / var / std / max / min of the same messages: fused walks vs composition")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--dims", type=int, nargs="+", default=[64, 256])
    p.add_argument("--no-model", action="store_true")
    args = p.parse_args()
    config.MULTI_AGG_SINGLE_MIN_EDGES, config.MULTI_AGG_SINGLE_SUM_FUSED = 0, True   # time the kernels everywhere: config.py's gates come from this table
    if not torch.cuda.is_available():
        raise SystemExit("pna_bench.py times device kernels: no GPU is visible")
    dev = torch.device("cuda:%d" % args.device)
    rows = []
    graphs = [(name, graph.to(dev).int()) for name, graph in shapes()]
    bench_op(args, dev, graphs[0][0], graphs[0][1], args.dims[0], False, PNA4, quiet=True)   # the process's first windows: discarded
    for name, g in graphs:
        for D in args.dims:
            for with_w in (False, True):
                for aggs in (PNA4, ("max",)):
                    rows.append(bench_op(args, dev, name, g, D, with_w, aggs))
    for name, g in graphs:                          # the other plain aggregates alone, the corner of config.MULTI_AGG_SINGLE_MIN_EDGES
        for aggs in (("sum",), ("mean",), ("min",)):
            rows.append(bench_op(args, dev, name, g, args.dims[0], False, aggs))
    model = None if args.no_model else bench_model(args, dev)
    print(json.dumps({"pna_bench": rows, "model_step": model, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
