"""Edge-MLP benchmark: ops.edge_mlp_reduce fused (csrc/edgemlp.hip) against the composition it replaces.

Shapes (widths H0 - hidden.. - H_L of the operator, i.e. without PointNetConv's first Linear, which runs over the nodes in both forms):
  level1  the first set-abstraction level of pointnet2.py: 32 clouds x 512 balls of 32 points, 524 288 edges, 64-64-128
  level2  its second level: 32 clouds x 128 balls of 64 points, 262 144 edges, 128-128-256 (two slabs of the output columns)
  mols    256 complete graphs of 18 nodes (a molhiv-sized batch, 78 336 edges), 64-64-64
  random  32 768 nodes, 1 000 000 random edges, one layer 64-128 (a two-layer PointNetConv)
Each is timed forward (no_grad) and forward + backward (all gradients), reduce = max:
  fused     config.EDGE_MLP_FUSED = True (and config.EDGE_MLP_GRAD_MAX_EDGES lifted): no E-sized tensor forward, transient [E, H] ones in backward
  composed  config.EDGE_MLP_FUSED = False: u_sub_v -> relu -> (Linear, relu) over edges -> copy_e / max
--sweep times the fused forms of level1 and level2 for config.EDGE_MLP_ITEM_EDGES in 64 .. 1024; --epoch the pointnet2.py epoch (eager,
its default sizes) with the switch on and off.

Timing: HIP events around every call after --warmup discarded ones, the two forms alternating call by call; median / min / max of --reps
calls in microseconds; peak memory above what is allocated before the call.  Both forms are compared before they are timed.  The script
only reports."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from gatv2_bench import peak_mib  # noqa: E402
from mi355x_graph import config, ops, transform  # noqa: E402
import mi355x_graph as mg  # noqa: E402


def graphs(dev):
    gen = torch.Generator().manual_seed(0)
    for name, per, balls, radius, k, widths in (("level1", 1024, 512, 0.2, 32, (64, 64, 128)), ("level2", 512, 128, 0.4, 64, (128, 128, 256))):
        pos = torch.rand(32 * per, 3, generator=gen).to(dev)
        centers = (per * torch.arange(32).view(-1, 1) + torch.arange(balls).view(1, -1)).flatten().to(dev)
        yield name, transform.fixed_radius_block(pos, centers, radius, k, [per] * 32), widths
    a, b = torch.meshgrid(torch.arange(18), torch.arange(18), indexing="ij")
    keep, first = a != b, (18 * torch.arange(256)).view(-1, 1)
    yield "mols", mg.graph(((a[keep] + first).flatten(), (b[keep] + first).flatten()), num_nodes=256 * 18).int().formats(["csr", "csc"]).to(dev), (64, 64, 64)
    src, dst = (torch.randint(0, 32768, (1_000_000,), generator=gen) for _ in range(2))
    yield "random", mg.graph((src, dst), num_nodes=32768).int().formats(["csr", "csc"]).to(dev), (64, 128)


def op_forms(g, widths):
    dev, n_src, n_dst, E = g.device, g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    torch.manual_seed(sum(widths))
    layers = [torch.nn.Linear(i, o).to(dev) for i, o in zip(widths[:-1], widths[1:])]
    gen = torch.Generator(device=dev).manual_seed(E)
    u = torch.randn(n_src, widths[0], device=dev, generator=gen).requires_grad_(True)
    v = torch.randn(n_dst, widths[0], device=dev, generator=gen).requires_grad_(True)
    up = torch.randn(n_dst, widths[-1], device=dev, generator=gen)
    ws, bs = [l.weight for l in layers], [l.bias for l in layers]

    def call():
        return ops.edge_mlp_reduce(g, u, v, ws, bs, "max")

    def fwd():
        with torch.no_grad():
            return call()

    def fwd_bwd():
        return torch.autograd.grad((call() * up).sum(), [u, v] + ws + bs)

    assert ops.edge_mlp_reduce_fused(g, u, v, ws, bs, "max")
    got = [fwd()] + list(fwd_bwd())
    config.EDGE_MLP_FUSED = False
    want = [fwd()] + list(fwd_bwd())
    config.EDGE_MLP_FUSED = True
    worst = max(float((a - c).abs().max() / c.abs().max()) for a, c in zip(got, want))
    return {"fwd": fwd, "fwd_bwd": fwd_bwd}, {"src": n_src, "dst": n_dst, "edges": E, "widths": list(widths), "max_rel_diff": worst}


def timed_pair(fn, args):
    """fn with the kernels on and off, call by call in turn -> {form: median / min / max in us}"""
    out = {True: [], False: []}
    for i in range(args.warmup + args.reps):
        for fused in (True, False):
            config.EDGE_MLP_FUSED = fused
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= args.warmup:
                out[fused].append(start.elapsed_time(end) * 1e3)
    config.EDGE_MLP_FUSED = True
    res = {}
    for fused, name in ((True, "fused"), (False, "composed")):
        t = sorted(out[fused])
        res[name] = {"median_us": round(t[len(t) // 2], 1), "min_us": round(t[0], 1), "max_us": round(t[-1], 1)}
    return res


def epoch_seconds(dev, epochs):
    """the eager pointnet2.py epoch (default sizes) with the switch on and off: the mean of the epochs after the first"""
    import pointnet2
    from mi355x_graph.datasets import POINT_SHAPES, shapes_like
    xyz, label = shapes_like(1024, 1024)
    res = {}
    for fused, name in ((True, "fused"), (False, "composed")):
        config.EDGE_MLP_FUSED = fused
        torch.manual_seed(0)
        model = pointnet2.PointNet2(len(POINT_SHAPES)).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.001)
        dur, losses = [], []
        for epoch in range(1, epochs + 1):
            t0 = time.time()
            losses.append(round(pointnet2.train_epoch(model, dev, xyz, label, 32, opt, epoch), 4))
            torch.cuda.synchronize()
            dur.append(time.time() - t0)
        res[name] = {"epoch_s": round(sum(dur[1:]) / len(dur[1:]), 4), "losses": losses}
    config.EDGE_MLP_FUSED = True
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--epoch", type=int, default=0, help="epochs of pointnet2.py per form (the first is not counted); 0: skip")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    config.EDGE_MLP_GRAD_MAX_EDGES = 2 ** 31  # the kernels at every size, also where the operator would not choose them
    recs = []
    for name, g, widths in graphs(dev):
        if args.sweep:
            if not name.startswith("level"):
                continue
            for item in (64, 128, 256, 512, 1024):
                config.EDGE_MLP_ITEM_EDGES = item
                forms, extra = op_forms(g, widths)
                recs.append(dict(extra, shape=name, item_edges=item, **{k: timed_pair(fn, args)["fused"] for k, fn in forms.items()}))
                print(json.dumps(recs[-1]), flush=True)
            continue
        forms, extra = op_forms(g, widths)
        rec = dict(extra, shape=name)
        for what, fn in forms.items():
            rec[what] = timed_pair(fn, args)
            for fused, form in ((True, "fused"), (False, "composed")):
                config.EDGE_MLP_FUSED = fused
                rec[what][form]["peak_mib"] = peak_mib(fn)
            config.EDGE_MLP_FUSED = True
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.epoch > 1:
        recs.append(dict(shape="pointnet2.py epoch", **epoch_seconds(dev, args.epoch)))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
