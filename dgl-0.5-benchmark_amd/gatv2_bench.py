"""GATv2 attention benchmark: ops.gatv2_attention fused (csrc/gatv2.hip) against the composition it replaces.

Forward, and forward + backward (d feat_src, d feat_dst, d attn), of the block between a GATv2Conv's projections and its result on
  cora and arxiv stand-ins with (H, F) = (8, 8) and (8, 16), reddit-small with (8, 16) and (1, 64), a molhiv batch of 2048 graphs with (8, 16)
(self-loops added, as the models do) as
  fused     three walks and no E-sized tensor
  composed  config.GATV2_FUSED = False: u_add_v -> leaky_relu -> (. * attn).sum(-1) -> edge_softmax -> u_mul_e/sum, which keeps
            [E, H, F] tensors forward and backward; where ONE such tensor exceeds --composed-gb the composition is not run and the line
            says "composition does not fit" with the bytes it would have needed
Timing: HIP events around --inner back-to-back calls, --reps windows kept after the discarded ones, every form warmed first, both forms
of a shape in one process and compared with each other before they are timed; mean / min / max per call in microseconds; peak memory above
what is allocated before the call.  The script only reports."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402
from mi355x_graph.datasets import SHAPES, synthetic_edges  # noqa: E402
import mi355x_graph as mg  # noqa: E402


def node_graph(name, dev):
    sp = SHAPES[name]
    src, dst = synthetic_edges(sp["n"], sp["m"], sp["max_deg"], seed=sp["seed"], symmetric=sp["symmetric"])
    return mg.graph((src, dst), num_nodes=sp["n"]).add_self_loop().int().formats(["csr", "csc"]).to(dev)


def molhiv_batch(graphs, dev):
    """`graphs` molecule-sized graphs (6..45 nodes, a ring plus a few chords, both directions) as one block-diagonal graph"""
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(6, 46, (graphs,), generator=gen)
    first = torch.cumsum(lens, 0) - lens
    seg = torch.repeat_interleave(torch.arange(graphs), lens)
    pos = torch.arange(int(lens.sum())) - first[seg]
    ring = first[seg] + (pos + 1) % lens[seg]
    hop = first[seg] + (pos + torch.randint(2, 6, pos.shape, generator=gen)) % lens[seg]
    keep = torch.rand(pos.shape, generator=gen) < 0.15
    a = torch.cat([torch.arange(pos.shape[0]), torch.arange(pos.shape[0])[keep]])
    b = torch.cat([ring, hop[keep]])
    return mg.graph((torch.cat([a, b]), torch.cat([b, a])), num_nodes=int(lens.sum())).add_self_loop().int().formats(["csr", "csc"]).to(dev)


def timed(fn, args):
    def window():
        for _ in range(args.inner):
            fn()
    return [round(v / args.inner * 1e6, 1) for v in time_op(window, args.reps + N_COLD)]


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench_shape(args, name, g, H, F):
    dev = g.device
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator(device=dev).manual_seed(n + H + F)
    fs, fd = (torch.randn(n, H, F, device=dev, generator=gen).requires_grad_(True) for _ in range(2))
    attn = torch.randn(1, H, F, device=dev, generator=gen).requires_grad_(True)
    up = torch.randn(n, H, F, device=dev, generator=gen)
    assert ops.gatv2_attention_fused(g, fs, fd, attn)
    call = lambda: ops.gatv2_attention(g, fs, fd, attn)  # noqa: E731

    def composed():
        config.GATV2_FUSED = False
        try:
            return call()
        finally:
            config.GATV2_FUSED = True

    res = {"graph": name, "nodes": n, "edges": E, "H": H, "F": F, "EHF_MiB": round(E * H * F * 4 / 2 ** 20, 1)}
    forms = {"fused": call}
    if E * H * F * 4 <= args.composed_gb * 2 ** 30:
        forms["composed"] = composed
    else:
        res["composed"] = "composition does not fit: one [E, H, F] tensor is %.1f GB" % (E * H * F * 4 / 1e9)
    want = None
    for form, fn in forms.items():
        def fwd(fn=fn):
            with torch.no_grad():
                fn()

        def step(fn=fn):
            fs.grad = fd.grad = attn.grad = None
            fn().backward(up)
        out = fn().detach()
        want = out if want is None else want
        assert torch.allclose(out, want, rtol=1e-4, atol=1e-4), form
        res[form + "_fwd_peak_MiB"], res[form + "_fwd_bwd_peak_MiB"] = peak_mib(fwd), peak_mib(step)
        res[form + "_fwd_us"], res[form + "_fwd_bwd_us"] = timed(fwd, args), timed(step, args)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--composed-gb", type=float, default=16.0, help="composed form: not run where ONE [E, H, F] tensor exceeds this")
    p.add_argument("--only", default=None, help="comma-separated graph names (cora, arxiv, reddit-small, molhiv-2048)")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gatv2_bench.py needs the GPU: a host timing says nothing about these kernels")
    dev = torch.device("cuda:0")
    shapes = [("cora", ((8, 8), (8, 16))), ("arxiv", ((8, 8), (8, 16))), ("reddit-small", ((8, 16), (1, 64))), ("molhiv-2048", ((8, 16),))]
    results = []
    time_op(lambda: torch.randn(1 << 20, device=dev).sum(), 3)  # the process's first measurement is discarded whole
    for name, layouts in shapes:
        if args.only and name not in args.only.split(","):
            continue
        g = molhiv_batch(2048, dev) if name == "molhiv-2048" else node_graph(name, dev)
        for H, F in layouts:
            results.append(bench_shape(args, name, g, H, F))
            print(json.dumps(results[-1]), flush=True)
        del g
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
