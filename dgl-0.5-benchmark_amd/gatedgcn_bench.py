"""Edge-gated aggregation benchmark: the fused walks of csrc/edgegate.hip against the composition they replace.

ops.edge_gated_sum(g, b, s, d, c) forward and forward + backward (all four gradients, from d h and d e_hat), with
config.EDGE_GATED_FUSED on (one walk forward, two backward; of size E only e_hat and d c are written) and off (u_add_v -> add -> sigmoid
-> u_mul_e/sum, copy_e/sum -> divide through the operators that existed before), on
  molhiv-64 / -256 / -2048   batches of the package's small-graph generator (gine_bench.shapes)
  ppa-32                     32 graphs of 240 nodes and 2 300 random edges each
  random-1M                  one graph of 100 000 nodes and 1 000 000 random edges
at F = 64 / 128 / 256 (--dims), and one training step (forward, backward, SGD update) of four nn.GatedGCNConv layers of width --hidden on
the molhiv batches.
Timing as gine_bench.py: HIP events around `--inner` back-to-back calls, `--reps` windows kept after two discarded ones, the two forms
alternating in one process, the better of two rounds; mean, min and max per call in microseconds.  Also per form: kernel launches per
call (torch.profiler; --no-launch-count skips it) and the peak allocation of one call above its operands.  For the fused kernels the
achieved bytes/s against the algorithmic bytes
  forward   (2 E + 5 N) F 4 (c read, e_hat written; s, b, d read, h, den written) + 8 E + 4 N of ids
as a share of the 8 TB/s peak (a whole-call figure: event time, not kernel time).  Both forms are checked against each other first."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
from gine_bench import shapes, count_launches  # noqa: E402
from kernel_bench import time_op, N_COLD, HBM_PEAK  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402
from mi355x_graph.nn import GatedGCNConv  # noqa: E402


def all_shapes():
    rng = np.random.default_rng(11)
    n, m = 100000, 1000000
    big = dgl.graph((torch.from_numpy(rng.integers(0, n, m)), torch.from_numpy(rng.integers(0, n, m))), num_nodes=n)
    return shapes() + [("random-1M", big)]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def both_forms(args, res, legs):
    """legs: {name: (fn, no_grad)}; times every leg in both forms, alternating, and keeps the better round of two"""
    def many(fn):
        def run():
            for _ in range(args.inner):
                fn()
        return run
    for _ in range(2):                                          # alternate the two forms: other work shares the machine
        for form, flag in (("fused", True), ("composed", False)):
            config.EDGE_GATED_FUSED = flag
            for leg, (fn, no_grad) in legs.items():
                with torch.set_grad_enabled(not no_grad):
                    t = [v / args.inner for v in time_op(many(fn), args.reps + N_COLD)]
                key = "%s_%s" % (form, leg)
                if key not in res or t[0] < res[key][0]:
                    res[key] = t
    config.EDGE_GATED_FUSED = True


def report(name, res, legs):
    for leg in legs:
        f_, c_ = res["fused_" + leg], res["composed_" + leg]
        print("%-11s N %6d E %7d F %3d %-8s fused %9.1f us [min %.1f max %.1f]   composed %9.1f us [min %.1f max %.1f]   ratio %.2fx   "
              "launches %s / %s   peak %.2f / %.2f MB" % (
                  name, res["nodes"], res["edges"], res["F"], leg, f_[0] * 1e6, f_[1] * 1e6, f_[2] * 1e6, c_[0] * 1e6, c_[1] * 1e6,
                  c_[2] * 1e6, c_[0] / f_[0], res.get("fused_%s_launches" % leg), res.get("composed_%s_launches" % leg),
                  res.get("fused_%s_peak_bytes" % leg, 0) / 1e6, res.get("composed_%s_peak_bytes" % leg, 0) / 1e6))


def bench_operator(args, name, g, F_, dev):
    N, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator(device=dev).manual_seed(N + F_)
    b, s, d = (torch.randn(N, F_, device=dev, generator=gen).requires_grad_(True) for _ in range(3))
    c = torch.randn(E, F_, device=dev, generator=gen).requires_grad_(True)
    xs = (b, s, d, c)
    up_h, up_e = torch.randn(N, F_, device=dev, generator=gen), torch.randn(E, F_, device=dev, generator=gen)

    def fwd():
        return ops.edge_gated_sum(g, b, s, d, c)

    def fwd_bwd():
        for x in xs:
            x.grad = None
        h, e = fwd()
        torch.autograd.backward((h, e), (up_h, up_e))

    res = {"shape": name, "nodes": N, "edges": E, "F": F_}
    outs = {}
    for form, flag in (("fused", True), ("composed", False)):
        config.EDGE_GATED_FUSED = flag
        assert ops.edge_gated_sum_fused(g, *xs) == flag
        fwd_bwd()
        outs[form] = [t.detach() for t in fwd()] + [x.grad.clone() for x in xs]
        with torch.no_grad():
            res[form + "_fwd_peak_bytes"] = peak(fwd)
        res[form + "_fwd_bwd_peak_bytes"] = peak(fwd_bwd)
        if not args.no_launch_count:
            with torch.no_grad():
                res[form + "_fwd_launches"] = count_launches(fwd)
            res[form + "_fwd_bwd_launches"] = count_launches(fwd_bwd)
    for a, b_ in zip(outs["fused"], outs["composed"]):
        err = float((a - b_).abs().max() / b_.abs().max())
        assert err < 1e-4, "fused and composed disagree: %g" % err
    legs = {"fwd": (fwd, True), "fwd_bwd": (fwd_bwd, False)}
    both_forms(args, res, legs)
    res["fwd_bytes"] = (2 * E + 5 * N) * F_ * 4 + 8 * E + 4 * N
    res["fwd_share_of_peak"] = res["fwd_bytes"] / res["fused_fwd"][0] / HBM_PEAK
    report(name, res, legs)
    print("%-11s F %3d fused forward: %.1f MB -> %.2f TB/s (%.1f %% of 8 TB/s, whole call)" % (
        name, F_, res["fwd_bytes"] / 1e6, res["fwd_bytes"] / res["fused_fwd"][0] / 1e12, 100 * res["fwd_share_of_peak"]))
    return res


def bench_model(args, name, g, dev):
    """one training step of four GatedGCNConv layers of width --hidden"""
    N, E, F_ = g.number_of_nodes(), g.number_of_edges(), args.hidden
    torch.manual_seed(N)
    layers = torch.nn.ModuleList([GatedGCNConv(F_, F_, F_) for _ in range(4)]).to(dev)
    opt = torch.optim.SGD(layers.parameters(), lr=1e-3)
    feat, efeat = torch.randn(N, F_, device=dev), torch.randn(E, F_, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        h, e = feat, efeat
        for layer in layers:
            h, e = layer(g, h, e)
        (h * h).mean().backward()
        opt.step()

    res = {"shape": name + " 4 layers", "nodes": N, "edges": E, "F": F_}
    for form, flag in (("fused", True), ("composed", False)):
        config.EDGE_GATED_FUSED = flag
        step()
        res[form + "_step_peak_bytes"] = peak(step)
    legs = {"step": (step, False)}
    both_forms(args, res, legs)
    report(name + "-x4", res, legs)
    return res


def main():
    p = argparse.ArgumentParser("edge-gated aggregation: fused walks vs composition")
    p.add_argument("--reps", type=int, default=12)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--dims", type=int, nargs="+", default=[64, 128, 256])
    p.add_argument("--hidden", type=int, default=128)
    p.add_argument("--no-launch-count", action="store_true")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    rows, steps = [], []
    for name, graph in all_shapes():
        g = graph.to(dev).int()
        for F_ in args.dims:
            rows.append(bench_operator(args, name, g, F_, dev))
        if name.startswith("molhiv"):
            steps.append(bench_model(args, name, g, dev))
    print(json.dumps({"gatedgcn_bench": rows, "gatedgcn_steps": steps, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
