"""Continuous-filter convolution benchmark: ops.edge_filter_sum fused (csrc/cfconv.hip) against the composition it replaces.

Forward, and forward + backward (d x, d w1, d b1, d w2, d b2), at F = 64 and 128, K = 50, edge features as a tensor and as distances
expanded in the kernel (rbf), on
  mols     256 complete graphs of 18 atoms (78 336 edges)
  clouds   32 clouds of 1024 points, transform.fixed_radius_block with 32 neighbours of every point (1 048 576 edges)
  random   one graph of 32 768 nodes and 1 000 000 random edges
as
  fused     config.CFCONV_FUSED = True: no E-sized tensor forward, three transient [E, F] ones in backward
  composed  config.CFCONV_FUSED = False: expansion -> Linear, ssp, Linear, ssp over edges -> u_mul_e/sum
--sweep times the fused forms of `random` at F = 64 for config.CFCONV_ITEM_EDGES in 64, 128, 256, 512, 1024.
Timing: HIP events around every call after --warmup discarded ones, the two forms alternating call by call; median / min / max of --reps
calls in microseconds; peak memory above what is allocated before the call.  Both forms are compared before they are timed.  The script
only reports."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from gatv2_bench import peak_mib  # noqa: E402
from mi355x_graph import config, ops, transform  # noqa: E402
import mi355x_graph as mg  # noqa: E402

K = 50


def graphs(dev):
    gen = torch.Generator().manual_seed(0)
    a, b = torch.meshgrid(torch.arange(18), torch.arange(18), indexing="ij")
    keep, first = a != b, (18 * torch.arange(256)).view(-1, 1)
    yield "mols", mg.graph(((a[keep] + first).flatten(), (b[keep] + first).flatten()), num_nodes=256 * 18).int().formats(["csr", "csc"]).to(dev)
    pos = torch.rand(32 * 1024, 3, generator=gen).to(dev)
    yield "clouds", transform.fixed_radius_block(pos, torch.arange(32 * 1024, device=dev), 0.2, 32, [1024] * 32)
    src, dst = (torch.randint(0, 32768, (1_000_000,), generator=gen) for _ in range(2))
    yield "random", mg.graph((src, dst), num_nodes=32768).int().formats(["csr", "csc"]).to(dev)


def op_forms(g, F, mode):
    dev, n_src, n_dst, E = g.device, g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    torch.manual_seed(F)
    l1, l2 = torch.nn.Linear(K, F).to(dev), torch.nn.Linear(F, F).to(dev)
    gen = torch.Generator(device=dev).manual_seed(F + E)
    x = torch.randn(n_src, F, device=dev, generator=gen).requires_grad_(True)
    up = torch.randn(n_dst, F, device=dev, generator=gen)
    rbf = (torch.arange(K, device=dev) * (5.0 / K), K / 5.0) if mode == "rbf" else None
    ef = 5 * torch.rand(E, device=dev, generator=gen) if rbf else torch.randn(E, K, device=dev, generator=gen)
    leaves = (x, l1.weight, l1.bias, l2.weight, l2.bias)

    def call():
        return ops.edge_filter_sum(g, x, ef, l1.weight, l1.bias, l2.weight, l2.bias, rbf)

    def fwd():
        with torch.no_grad():
            return call()

    def fwd_bwd():
        return torch.autograd.grad((call() * up).sum(), leaves)

    assert ops.edge_filter_sum_fused(g, x, ef, l1.weight, l1.bias, l2.weight, l2.bias, rbf)
    got = [fwd()] + list(fwd_bwd())
    config.CFCONV_FUSED = False
    want = [fwd()] + list(fwd_bwd())
    config.CFCONV_FUSED = True
    worst = max(float((a - c).abs().max() / c.abs().max()) for a, c in zip(got, want))
    return {"fwd": fwd, "fwd_bwd": fwd_bwd}, {"src": n_src, "dst": n_dst, "edges": E, "F": F, "K": K, "mode": mode, "max_rel_diff": worst}


def timed_pair(fn, args):
    """fn with the kernels on and off, call by call in turn -> {form: median / min / max in us}"""
    out = {True: [], False: []}
    for i in range(args.warmup + args.reps):
        for fused in (True, False):
            config.CFCONV_FUSED = fused
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= args.warmup:
                out[fused].append(start.elapsed_time(end) * 1e3)
    config.CFCONV_FUSED = True
    res = {}
    for fused, name in ((True, "fused"), (False, "composed")):
        t = sorted(out[fused])
        res[name] = {"median_us": round(t[len(t) // 2], 1), "min_us": round(t[0], 1), "max_us": round(t[-1], 1)}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    recs = []
    for name, g in graphs(dev):
        if args.sweep:
            if name != "random":
                continue
            for item in (64, 128, 256, 512, 1024):
                config.CFCONV_ITEM_EDGES = item
                forms, extra = op_forms(g, 64, "rbf")
                recs.append(dict(extra, shape=name, item_edges=item, **{k: timed_pair(fn, args)["fused"] for k, fn in forms.items()}))
                print(json.dumps(recs[-1]), flush=True)
            continue
        for F in (64, 128):
            for mode in ("tensor", "rbf"):
                forms, extra = op_forms(g, F, mode)
                rec = dict(extra, shape=name)
                for what, fn in forms.items():
                    rec[what] = timed_pair(fn, args)
                    for fused, form in ((True, "fused"), (False, "composed")):
                        config.CFCONV_FUSED = fused
                        rec[what][form]["peak_mib"] = peak_mib(fn)
                    config.CFCONV_FUSED = True
                recs.append(rec)
                print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
