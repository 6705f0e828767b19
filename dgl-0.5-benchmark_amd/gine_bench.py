"""relu(x_u + w_e) message benchmark: the fused walks of csrc/gine.hip against the composition they replace.

ops.gine_sum(g, x, w, scale) forward and forward + backward (d x and d w), with config.GINE_FUSED on (one launch each way, nothing of
size E written but d w) and off (gather -> add -> relu -> mul -> copy_e/sum through the operators that existed before: what
graph_classification.py runs without --fused-message), on
  molhiv-64 / -256 / -2048   batches of 64, 256 and 2048 graphs of the package's small-graph generator (datasets.molhiv_like), D = 256
  ppa-32                     32 graphs of 240 nodes and 2 300 random edges each (the shape of an ogbg-ppa batch), D = 256
Timing: HIP events around `--inner` back-to-back calls (one call is tens of microseconds: a window of one would time the event pair),
`--reps` windows kept after two discarded ones (kernel_bench.time_op drops its first two), the two forms alternating in one process; mean,
min and max per call in microseconds.  Also per form: kernel launches per call (torch.profiler's device kernel events; --no-launch-count
skips it) and the peak allocation of one call above its inputs.  For the fused kernels the achieved bytes/s against the algorithmic bytes
  forward   (E + N) D 4 read + N D 4 written + ids (8 E + 4 N + 4 E of scales);   backward   + N D 4 (d out) read, + E D 4 (d w) written
as a share of the 8 TB/s peak.  Both forms are checked against each other before they are timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
from kernel_bench import time_op, N_COLD, HBM_PEAK  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402


def shapes():
    from mi355x_graph.datasets import molhiv_like
    from dgl.dataloading import GraphDataLoader
    out = []
    for b in (64, 256, 2048):
        bg, _ = next(iter(GraphDataLoader(molhiv_like(b, seed=5), batch_size=b, shuffle=False)))
        out.append(("molhiv-%d" % b, bg))
    rng = np.random.default_rng(7)
    n, m, graphs = 240, 2300, 32
    src = np.concatenate([rng.integers(0, n, m) + i * n for i in range(graphs)])
    dst = np.concatenate([rng.integers(0, n, m) + i * n for i in range(graphs)])
    out.append(("ppa-32", dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n * graphs)))
    return out


def count_launches(fn):
    """device kernels one call of fn() launches, or None when the profiler gives no device events"""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower()
                and "memset" not in ev.name.lower())
        return n or None
    except Exception as exc:  # noqa: BLE001 -- a build without device tracing: the table says so
        print("launch count unavailable: %s" % (exc,))
        return None


def main():
    p = argparse.ArgumentParser("relu(x_u + w_e) messages: fused walks vs composition")
    p.add_argument("--reps", type=int, default=12)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--dim", type=int, default=256)
    p.add_argument("--no-launch-count", action="store_true")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    D = args.dim
    rows = []
    for name, graph in shapes():
        g = graph.to(dev).int()
        N, E = g.number_of_nodes(), g.number_of_edges()
        gen = torch.Generator(device=dev).manual_seed(N)
        x = torch.randn(N, D, device=dev, generator=gen).requires_grad_(True)
        w = torch.randn(E, D, device=dev, generator=gen).requires_grad_(True)
        scale = torch.rand(E, device=dev, generator=gen) + 0.1
        up = torch.randn(N, D, device=dev, generator=gen)

        def fwd():
            return ops.gine_sum(g, x, w, scale)

        def fwd_bwd():
            x.grad = w.grad = None
            fwd().backward(up)

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        def peak(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base

        res = {"shape": name, "nodes": N, "edges": E, "D": D}
        outs = {}
        for form, flag in (("fused", True), ("composed", False)):
            config.GINE_FUSED = flag
            assert ops.gine_sum_fused(g, x, w, scale) == flag
            fwd_bwd()
            outs[form] = (fwd().detach(), x.grad.clone(), w.grad.clone())
            x.grad = w.grad = None
            with torch.no_grad():
                res[form + "_fwd_peak_bytes"] = peak(fwd)
            res[form + "_fwd_bwd_peak_bytes"] = peak(fwd_bwd)
            if not args.no_launch_count:
                with torch.no_grad():
                    res[form + "_fwd_launches"] = count_launches(fwd)
                res[form + "_fwd_bwd_launches"] = count_launches(fwd_bwd)
        for a, b in zip(outs["fused"], outs["composed"]):
            err = float((a - b).abs().max() / b.abs().max())
            assert err < 1e-4, "fused and composed disagree: %g" % err
        for _ in range(2):                                      # alternate the two forms: other work shares the machine
            for form, flag in (("fused", True), ("composed", False)):
                config.GINE_FUSED = flag
                with torch.no_grad():
                    t = [v / args.inner for v in time_op(many(fwd), args.reps + N_COLD)]
                tb = [v / args.inner for v in time_op(many(fwd_bwd), args.reps + N_COLD)]
                if form + "_fwd" not in res or t[0] < res[form + "_fwd"][0]:
                    res[form + "_fwd"] = t
                if form + "_fwd_bwd" not in res or tb[0] < res[form + "_fwd_bwd"][0]:
                    res[form + "_fwd_bwd"] = tb
        config.GINE_FUSED = True
        ids = 8 * E + 4 * N + 4 * E
        res["fwd_bytes"] = (E + N) * D * 4 + N * D * 4 + ids
        res["bwd_bytes"] = (E + N) * D * 4 + N * D * 4 + N * D * 4 + E * D * 4 + ids
        f, fb = res["fused_fwd"][0], res["fused_fwd_bwd"][0]
        res["fwd_share_of_peak"] = res["fwd_bytes"] / f / HBM_PEAK
        res["bwd_share_of_peak"] = res["bwd_bytes"] / max(fb - f, 1e-9) / HBM_PEAK   # backward alone: the pair minus the forward (with autograd's own launches)
        for leg in ("fwd", "fwd_bwd"):
            f_, c_ = res["fused_" + leg], res["composed_" + leg]
            print("%-11s N %6d E %6d %-8s fused %8.1f us [min %.1f max %.1f]   composed %8.1f us [min %.1f max %.1f]   ratio %.2fx   "
                  "launches %s / %s   peak %.2f / %.2f MB" % (
                      name, N, E, leg, f_[0] * 1e6, f_[1] * 1e6, f_[2] * 1e6, c_[0] * 1e6, c_[1] * 1e6, c_[2] * 1e6, c_[0] / f_[0],
                      res.get("fused_%s_launches" % leg), res.get("composed_%s_launches" % leg),
                      res["fused_%s_peak_bytes" % leg] / 1e6, res["composed_%s_peak_bytes" % leg] / 1e6))
        print("%-11s fused kernels: forward %.1f MB -> %.2f TB/s (%.1f %% of 8 TB/s); backward %.1f MB -> %.2f TB/s (%.1f %%)" % (
            name, res["fwd_bytes"] / 1e6, res["fwd_bytes"] / f / 1e12, 100 * res["fwd_share_of_peak"],
            res["bwd_bytes"] / 1e6, res["bwd_bytes"] / max(fb - f, 1e-9) / 1e12, 100 * res["bwd_share_of_peak"]))
        rows.append(res)
    print(json.dumps({"gine_bench": rows, "inner": args.inner, "reps": args.reps}))


if __name__ == "__main__":
    main()
