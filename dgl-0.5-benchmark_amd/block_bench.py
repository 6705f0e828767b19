"""Block and subgraph construction benchmark: the relabelling kernels of csrc/relabel.hip against the torch composition they replace.

Every row times ONE function with its config attribute on (the kernels) and off (the composition: the code as it was before the kernels
existed), at
  to_block   reddit NS-SAGE shapes: the frontier of 1 000 seeds at fan-out 25, then that block's sources at fan-out 10 (the two calls of
             a sampling_sage.py step), and a products-sized frontier (2.4 M nodes, 100 000 seeds at fan-out 10)
  sample_blocks([10, 25])   the sampler and both blocks, as the data loader calls it (and sample_neighbors alone at both fan-outs:
             the part of a sampled step that has one form only)
  node_subgraph   a batch of 32 out of 15 000 clusters of the products-shaped stand-in (planted communities), in-CSR present
  epoch      sampling_sage.py's training loop on the reddit stand-in (`--epochs` timed epochs after one warm-up epoch)
Timing (experiments/exp_sampler.py --modes): 3 warm-up calls, then 10 calls each between two device synchronisations; the median, the
fastest and the slowest, in milliseconds.  The two forms alternate, twice, and the better median of a form is kept (other work shares
the machine).  Both forms are checked against each other before they are timed.  --scale shrinks the graphs (a quick look)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from mi355x_graph import config, sampling  # noqa: E402
from mi355x_graph.datasets import NodeData, SHAPES, synthetic_edges  # noqa: E402
from mi355x_graph.sampling import NID, EID  # noqa: E402


def med(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(ts), min(ts), max(ts)]


def ab(name, attr, fn, same, rows, **meta):
    """Time fn() with config.<attr> on and off; `same(a, b)` compares the two results first."""
    out = {}
    for flag in (True, False):
        setattr(config, attr, flag)
        out[flag] = fn()
    same(out[True], out[False])
    res = dict(row=name, **meta)
    for _ in range(2):
        for form, flag in (("device", True), ("torch", False)):
            setattr(config, attr, flag)
            t = med(fn)
            if form not in res or t[0] < res[form][0]:
                res[form] = t
    setattr(config, attr, True)
    d, t = res["device"], res["torch"]
    print("%-34s device %9.3f ms [min %.3f max %.3f]   torch %9.3f ms [min %.3f max %.3f]   ratio %.2fx" % (
        name, d[0], d[1], d[2], t[0], t[1], t[2], t[0] / d[0]), flush=True)
    rows.append(res)


def same_block(a, b):
    assert torch.equal(a.srcdata[NID], b.srcdata[NID]) and torch.equal(a.dstdata[NID], b.dstdata[NID])
    assert torch.equal(a.edges()[0], b.edges()[0]) and torch.equal(a.edges()[1], b.edges()[1])
    assert torch.equal(a._index._csc.indptr, b._index._csc.indptr) and torch.equal(a._index._csc.indices, b._index._csc.indices)


def same_blocks(a, b):
    for x, y in zip(a, b):
        same_block(x, y)


def same_subgraph(a, b):
    assert torch.equal(a.edges()[0], b.edges()[0]) and torch.equal(a.edges()[1], b.edges()[1])
    assert torch.equal(a.ndata[NID], b.ndata[NID]) and torch.equal(a.edata[EID], b.edata[EID])


def epoch_times(g, feats, labels, num_classes, train_nid, epochs, dev):
    import torch.nn as nn
    import torch.nn.functional as F
    from sampling_sage import SAGE
    torch.manual_seed(0)
    sampler = dgl.dataloading.MultiLayerNeighborSampler([10, 25])
    loader = dgl.dataloading.NodeDataLoader(g, train_nid, sampler, batch_size=1000, shuffle=True, drop_last=False)
    model = SAGE(feats.shape[1], 16, num_classes, 2, F.relu, 0.5).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.003)
    loss_fcn = nn.CrossEntropyLoss()
    times = []
    for epoch in range(epochs + 1):
        torch.cuda.synchronize()
        tic = time.perf_counter()
        for input_nodes, seeds, blocks in loader:
            loss = loss_fcn(model(blocks, feats[input_nodes]), labels[seeds])
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        if epoch:
            times.append(time.perf_counter() - tic)
    return times


def main():
    p = argparse.ArgumentParser("sampled blocks and induced subgraphs: device kernels vs torch composition")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--epochs", type=int, default=3)
    p.add_argument("--skip", default="", help="comma-separated: reddit, products, epoch")
    args = p.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    dev = torch.device("cuda:%d" % args.device)
    rows = []

    if "reddit" not in skip:
        data = NodeData("reddit", device=dev, scale=args.scale)
        g = dgl.add_self_loop(data.graph).int()
        g.create_formats_()
        n = g.number_of_nodes()
        gen = torch.Generator().manual_seed(0)
        train_nid = torch.nonzero(torch.rand(n, generator=gen) < 0.66).flatten()
        seeds = train_nid[torch.randperm(train_nid.shape[0], generator=gen)[:1000]].to(dev)
        f25 = sampling.sample_neighbors(g, seeds, 25, generator=torch.Generator().manual_seed(1))
        b25 = sampling.to_block(f25, seeds, num_nodes=n, idtype=g.idtype, dst_sorted=True, max_in_degree=25)
        seeds10 = b25.srcdata[NID]
        f10 = sampling.sample_neighbors(g, seeds10, 10, generator=torch.Generator().manual_seed(2))
        for name, fr, sd, fan in (("to_block reddit fan-out 25", f25, seeds, 25), ("to_block reddit fan-out 10", f10, seeds10, 10)):
            ab(name, "DEVICE_BLOCKS", lambda: sampling.to_block(fr, sd, num_nodes=n, idtype=g.idtype, dst_sorted=True, max_in_degree=fan),
               same_block, rows, num_nodes=n, num_dst=int(sd.shape[0]), nnz=int(fr[0].shape[0]))
        for name, sd, fan in (("sample_neighbors reddit fan-out 25", seeds, 25), ("sample_neighbors reddit fan-out 10", seeds10, 10)):
            t = med(lambda: sampling.sample_neighbors(g, sd, fan))  # the other half of a sampled step: no switch, one form
            print("%-34s        %9.3f ms [min %.3f max %.3f]" % (name, t[0], t[1], t[2]), flush=True)
            rows.append({"row": name, "num_seeds": int(sd.shape[0]), "device": t})
        sampler = sampling.MultiLayerNeighborSampler([10, 25])
        ab("sample_blocks([10, 25]) reddit", "DEVICE_BLOCKS",
           lambda: sampler.sample_blocks(g, seeds, generator=torch.Generator().manual_seed(3)), same_blocks, rows, num_nodes=n, seeds=1000)
        if "epoch" not in skip:
            res = {"row": "sampling_sage epoch reddit", "epochs": args.epochs}
            for form, flag in (("device", True), ("torch", False), ("device", True), ("torch", False)):
                config.DEVICE_BLOCKS = flag
                res.setdefault(form, []).extend(epoch_times(g, data.features, data.labels, data.num_classes, train_nid, args.epochs, dev))
            config.DEVICE_BLOCKS = True
            for form in ("device", "torch"):
                ts = res[form]
                res[form] = [statistics.median(ts), min(ts), max(ts)]
            print("%-34s device %9.4f s [min %.4f max %.4f]   torch %9.4f s [min %.4f max %.4f]   ratio %.2fx" % (
                res["row"], *res["device"], *res["torch"], res["torch"][0] / res["device"][0]), flush=True)
            rows.append(res)
        del data, g, f25, f10, b25

    if "products" not in skip:
        spec = SHAPES["products"]
        n, m = max(16, int(spec["n"] * args.scale)), max(16, int(spec["m"] * args.scale))
        gen = torch.Generator().manual_seed(4)
        seeds = torch.randperm(n, generator=gen)[:max(1, int(100_000 * args.scale))].to(dev)
        dst = torch.repeat_interleave(seeds, 10)
        src = torch.randint(0, n, (dst.shape[0],), generator=gen).to(dev)
        ab("to_block products frontier", "DEVICE_BLOCKS",
           lambda: sampling.to_block((src, dst), seeds, num_nodes=n, idtype=torch.int32, dst_sorted=True, max_in_degree=10),
           same_block, rows, num_nodes=n, num_dst=int(seeds.shape[0]), nnz=int(src.shape[0]))
        parts = max(32, int(15_000 * args.scale))
        s, d, comm = synthetic_edges(n, m, min(spec["max_deg"], n - 1), spec["seed"], dev, symmetric=True, avg_comm=max(1, n // parts),
                                     return_communities=True)
        g = dgl.graph((s, d), num_nodes=n).int()
        del s, d
        g._index.csc()
        pick = torch.randperm(int(comm.max()) + 1, generator=gen)[:32].to(dev)
        nodes = torch.nonzero(torch.isin(comm, pick)).flatten()
        ab("node_subgraph products 32 clusters", "DEVICE_SUBGRAPH", lambda: g.subgraph(nodes), same_subgraph, rows, num_nodes=n,
           parent_edges=g.number_of_edges(), selected=int(nodes.shape[0]), kept_edges=int(g.subgraph(nodes).number_of_edges()))

    print(json.dumps({"block_bench": rows, "scale": args.scale}))


if __name__ == "__main__":
    main()
