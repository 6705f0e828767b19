"""Edge-conditioned convolution benchmark: ops.edge_bilinear fused (csrc/nnconv.hip) against the composition it replaces.

Forward, and forward + backward (d x, d h, d weight, d bias), of NNConv's message passing with the edge network's last linear layer on
  qm9      128 complete graphs of 9 .. 29 nodes, I = O = 64, DH = 128
  molhiv   bond-graph batches of 256 and 2048 molecules at the same widths
  small    the 256-molecule batch at I = 16, O = 32, DH = 16
  mpnn     one training step of graph_classification.MPNN (width 64, 3 steps) on the 256-molecule batch
as
  fused     config.NNCONV_FUSED = True: no [E, I*O] tensor
  composed  config.NNCONV_FUSED = False: gather -> h @ weight -> bmm -> copy_e/sum, an [E, I*O] tensor forward, kept for backward
--sweep times the fused forms of qm9 for config.NNCONV_ITEM_EDGES in 64, 128, 192, 256.
Timing: HIP events around every call after --warmup discarded ones; median / min / max of --reps calls in microseconds; peak memory
above what is allocated before the call.  Both forms run in one process and are compared before they are timed.  The script only reports."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from gatv2_bench import molhiv_batch, peak_mib  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402
import mi355x_graph as mg  # noqa: E402


def qm9_batch(graphs, dev):
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(9, 30, (graphs,), generator=gen)
    first = torch.cumsum(lens, 0) - lens
    src, dst = [], []
    for n, f in zip(lens.tolist(), first.tolist()):
        a, b = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
        keep = a != b
        src.append(a[keep] + f)
        dst.append(b[keep] + f)
    return mg.graph((torch.cat(src), torch.cat(dst)), num_nodes=int(lens.sum())).int().formats(["csr", "csc"]).to(dev)


def timed(fn, args):
    out = []
    for i in range(args.warmup + args.reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        if i >= args.warmup:
            out.append(start.elapsed_time(end) * 1e3)
    out.sort()
    return {"median_us": round(out[len(out) // 2], 1), "min_us": round(out[0], 1), "max_us": round(out[-1], 1)}


def both(args, name, forms, extra):
    rec = dict(extra, shape=name)
    for form, fused in (("fused", True), ("composed", False)):
        config.NNCONV_FUSED = fused
        for what, fn in forms.items():
            rec["%s_%s" % (form, what)] = dict(timed(fn, args), peak_mib=peak_mib(fn))
    config.NNCONV_FUSED = True
    print(json.dumps(rec), flush=True)
    return rec


def op_forms(g, I, O, DH):
    dev, n, E = g.device, g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator(device=dev).manual_seed(I + O + DH)
    x, h, w, b = (torch.randn(*s, device=dev, generator=gen).requires_grad_(True) for s in ((n, I), (E, DH), (DH, I, O), (I, O)))
    with torch.no_grad():
        w.mul_(1.0 / (DH * I) ** 0.5)
    up = torch.randn(n, O, device=dev, generator=gen)

    def fwd():
        with torch.no_grad():
            return ops.edge_bilinear(g, x, h, w, b)

    def fwd_bwd():
        return torch.autograd.grad((ops.edge_bilinear(g, x, h, w, b) * up).sum(), (x, h, w, b))

    assert ops.edge_bilinear_fused(g, x, h, w, b)
    got = [fwd()] + list(fwd_bwd())
    config.NNCONV_FUSED = False
    want = [fwd()] + list(fwd_bwd())
    config.NNCONV_FUSED = True
    worst = max(float((a - c).abs().max() / c.abs().max()) for a, c in zip(got, want))
    return {"fwd": fwd, "fwd_bwd": fwd_bwd}, {"nodes": n, "edges": E, "I": I, "O": O, "DH": DH, "max_rel_diff": worst}


def mpnn_forms(g, dev):
    import graph_classification as gc
    torch.manual_seed(0)
    model = gc.MPNN(64, 1).to(dev).train()
    n, E = g.number_of_nodes(), g.number_of_edges()
    atom, bond = torch.randint(0, 2, (n, 9), device=dev), torch.randint(0, 2, (E, 3), device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        model(g, atom, bond).sum().backward()

    return {"step": step}, {"nodes": n, "edges": E}


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
    qm9 = qm9_batch(128, dev)
    if args.sweep:
        for item in (64, 128, 192, 256):
            config.NNCONV_ITEM_EDGES = item
            forms, extra = op_forms(qm9, 64, 64, 128)
            rec = dict(extra, shape="qm9", item_edges=item, **{k: timed(fn, args) for k, fn in forms.items()})
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    else:
        m256, m2048 = molhiv_batch(256, dev), molhiv_batch(2048, dev)
        for name, g, (I, O, DH) in (("qm9", qm9, (64, 64, 128)), ("molhiv256", m256, (64, 64, 128)), ("molhiv2048", m2048, (64, 64, 128)),
                                    ("small", m256, (16, 32, 16))):
            recs.append(both(args, name, *op_forms(g, I, O, DH)))
        recs.append(both(args, "mpnn", *mpnn_forms(m256, dev)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
