"""Segment multi-head attention benchmark: ops.segment_mha (csrc/segmha.hip) against the two forms a user could write today.

Forward + backward (d q, d k, d v) of self-attention inside every graph of a batch, for (H, F) = (4, 16), (4, 64), (8, 32), on
  molhiv-shaped batches of 64 / 256 / 2048 graphs (about 25 nodes each), a ppa-shaped batch (32 graphs of about 243 nodes),
  32 clouds x 1024 points, one segment of 16 384 rows
as
  fused   ops.segment_mha: two launches forward (item scan, kernel), five backward, no padded and no [n, n] tensor
  padded  the operator's own composition (config.SEGMENT_MHA_FUSED = False): [S, max_len, H, F] operands, a key mask, torch.softmax;
          its peak memory above the operands is reported beside the fused form's
  dot     ops.dot_attention over the explicit block-complete graph of sum n_g^2 edges (built outside the timed window; not run above
          --max-edges)
then the PMA cross form (k = 1 and k = 4 query rows per graph against the graph's nodes), fused against padded, and with --epoch one
`graph_classification.py --readout settrans` run eager and one with --hipgraph, each in a child process (their own epoch times).
Timing: HIP events around --inner back-to-back calls, --reps windows kept after the discarded ones, every form warmed first, all forms of
a shape in one process; mean / min / max per call in microseconds.  The forms are compared with each other before they are timed.  The
script only reports."""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from kernel_bench import time_op, N_COLD  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402
import mi355x_graph as mg  # noqa: E402


def batches():
    gen = torch.Generator().manual_seed(0)
    mol = lambda b: torch.randint(6, 46, (b,), generator=gen)  # noqa: E731  (molhiv: 25.5 nodes on average)
    return [("molhiv-64", mol(64)), ("molhiv-256", mol(256)), ("molhiv-2048", mol(2048)),
            ("ppa-32", torch.randint(120, 367, (32,), generator=gen)), ("clouds-32x1024", torch.full((32,), 1024)),
            ("one-16384", torch.full((1,), 16384))]


GRAPHS = {}


def timed(fn, args):
    def window():
        for _ in range(args.inner):
            fn()
    return [round(v / args.inner * 1e6, 1) for v in time_op(window, args.reps + N_COLD)]


def block_complete(lens, dev):
    """the graph in which every node has an in-edge from every node of its segment"""
    ends = torch.cumsum(lens, 0)
    seg = torch.repeat_interleave(torch.arange(lens.shape[0]), lens)
    dst = torch.repeat_interleave(torch.arange(int(ends[-1])), lens[seg])
    first = torch.repeat_interleave((ends - lens)[seg], lens[seg])
    src = torch.arange(dst.shape[0]) - torch.repeat_interleave(torch.cumsum(lens[seg], 0) - lens[seg], lens[seg]) + first
    return mg.graph((src, dst), num_nodes=int(ends[-1])).int().to(dev)


def measure(forms, tensors, up, args, res):
    """forward + backward time of every form, its peak memory above what is allocated before the call; the forms agree first"""
    want = None
    for name, fn in forms.items():
        def step(fn=fn):
            for t in tensors:
                t.grad = None
            fn().backward(up)
        out = fn().detach()
        want = out if want is None else want
        assert torch.allclose(out, want, rtol=1e-4, atol=1e-4), name
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        res[name + "_peak_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        res[name + "_fwd_bwd_us"] = timed(step, args)


def bench_shape(args, dev, name, lens, H, F, k_rows=None):
    n, S = int(lens.sum()), lens.shape[0]
    gen = torch.Generator(device=dev).manual_seed(n + H + F)
    nq = n if k_rows is None else S * k_rows
    q = torch.randn(nq, H, F, device=dev, generator=gen).requires_grad_(True)
    k, v = (torch.randn(n, H, F, device=dev, generator=gen).requires_grad_(True) for _ in range(2))
    up = torch.randn(nq, H, F, device=dev, generator=gen)
    kv_len = lens.to(dev)
    q_len = kv_len if k_rows is None else torch.full((S,), k_rows, device=dev)
    call = lambda: ops.segment_mha(q, k, v, q_len, None if k_rows is None else kv_len, q_total=nq, kv_total=n)  # noqa: E731
    assert ops.segment_mha_fused(q, k, v, q_len, None if k_rows is None else kv_len, q_total=nq, kv_total=n)

    def padded():
        config.SEGMENT_MHA_FUSED = False
        try:
            return call()
        finally:
            config.SEGMENT_MHA_FUSED = True

    forms = {"fused": call}
    if S * int(lens.max()) ** 2 * H * 4 <= args.padded_gb * 2 ** 30:
        forms["padded"] = padded
    edges = int((lens * lens).sum())
    if k_rows is None and edges <= args.max_edges:
        g = GRAPHS[name] = GRAPHS[name] if name in GRAPHS else block_complete(lens, dev)  # (one build per batch)
        if ops.dot_attention_fused(g, q, k, v):
            forms["dot"] = lambda: ops.dot_attention(g, q, k, v)
    res = {"batch": name, "segments": S, "rows": n, "H": H, "F": F, "edges": edges}
    if k_rows is not None:
        res["k"] = k_rows
    measure(forms, (q, k, v), up, args, res)
    return res


def epoch_times(flags):
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "graph_classification.py"), "--readout", "settrans",
           "--epochs", "3"] + flags
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    return {"command": " ".join(cmd[1:]), "lines": [l for l in out.stdout.splitlines() if l.startswith(("epoch", "Training", "hipgraph"))],
            "returncode": out.returncode}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--max-edges", type=int, default=40000000, help="dot form: the block-complete graph is not built above this")
    p.add_argument("--padded-gb", type=float, default=8.0, help="padded form: not run where its [S, H, L, L] weights alone exceed this")
    p.add_argument("--epoch", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("setattn_bench.py needs the GPU: a host timing says nothing about these kernels")
    dev = torch.device("cuda:0")
    results = {"self": [], "pma": [], "epoch": []}
    time_op(lambda: torch.randn(1 << 20, device=dev).sum(), 3)  # the process's first measurement is discarded whole
    for name, lens in batches():
        for H, F in ((4, 16), (4, 64), (8, 32)):
            results["self"].append(bench_shape(args, dev, name, lens, H, F))
            print(json.dumps(results["self"][-1]), flush=True)
    for name, lens in batches()[:4]:
        for k_rows in (1, 4):
            results["pma"].append(bench_shape(args, dev, name, lens, 4, 16, k_rows))
            print(json.dumps(results["pma"][-1]), flush=True)
    if args.epoch:
        for flags in ([], ["--hipgraph"]):
            results["epoch"].append(epoch_times(flags))
            print(json.dumps(results["epoch"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
