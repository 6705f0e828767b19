"""Link-prediction minibatch benchmark: the kernels of csrc/edgefind.hip and the edge-batch half of csrc/relabel.hip against the torch
compositions of the same semantics (config.DEVICE_LINKPRED on / off; the lookup's composition is the parent commit's
DGLGraph.has_edges_between).

On the reddit-shaped and the products-shaped stand-ins (both bidirected: the reverse of edge e is (e + E / 2) % E), every row times ONE
function in both forms:
  has_edges_between   4 096 and 65 536 queries, half of them edges of the graph
  edge_ids            4 096 edges of the graph
  negatives           Uniform(k) for a batch of edges, without rejection and with exclude_existing (in-CSR and out-CSR scans)
  frontier exclusion  the fan-out-25 frontier of a batch's endpoints without the batch's edges and their reverses
  compaction          the endpoints of a batch and its negatives -> ascending distinct nodes + positions
  loader epoch        `--batches` batches of an EdgeDataLoader (fan-outs 10, 25; k negatives; exclude="reverse_id"), iteration only
Timing is block_bench.py's: 3 warm-up calls, then 10 calls each between two device synchronisations; median, fastest, slowest in
milliseconds; the two forms alternate, twice, and the better median of a form is kept.  Both forms are compared (torch.equal) before they
are timed.  --scale shrinks the graphs (a quick look)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
from block_bench import ab  # noqa: E402
from mi355x_graph import config, linkpred, sampling  # noqa: E402
from mi355x_graph.datasets import NodeData  # noqa: E402
from mi355x_graph.sampling import NID, EID  # noqa: E402


def same_tensors(a, b):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def batch_ids(batch):
    input_nodes, pair, neg, blocks = batch
    out = [input_nodes, pair.ndata[NID], pair.edata[EID], *pair.edges(), *neg.edges()]
    for b in blocks:
        out += [b.srcdata[NID], b.edata[EID], *b.edges()]
    return out


def loader_epoch(g, eids, reverse, k, batch_size, seed):
    loader = dgl.dataloading.EdgeDataLoader(g, eids, dgl.dataloading.MultiLayerNeighborSampler([10, 25]), batch_size=batch_size,
                                            shuffle=True, exclude="reverse_id", reverse_eids=reverse,
                                            negative_sampler=dgl.dataloading.negative_sampler.Uniform(k),
                                            generator=torch.Generator().manual_seed(seed))
    last = None
    for batch in loader:
        last = batch
    return batch_ids(last)


def epoch_row(name, g, eids, reverse, k, batch_size, rows, reps):
    """One loader epoch per call, the forms alternating; the last batch of both forms is compared first."""
    res = {"row": name, "batches": -(-int(eids.shape[0]) // batch_size), "batch_size": batch_size, "k": k}
    out = {}
    for flag in (True, False):
        config.DEVICE_LINKPRED = flag
        out[flag] = loader_epoch(g, eids, reverse, k, batch_size, 0)  # also the warm-up of this form
    same_tensors(out[True], out[False])
    ts = {"device": [], "torch": []}
    for r in range(reps):
        for form, flag in (("device", True), ("torch", False)):
            config.DEVICE_LINKPRED = flag
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loader_epoch(g, eids, reverse, k, batch_size, r + 1)
            torch.cuda.synchronize()
            ts[form].append(time.perf_counter() - t0)
    config.DEVICE_LINKPRED = True
    for form in ts:
        res[form] = [statistics.median(ts[form]), min(ts[form]), max(ts[form])]
    print("%-34s device %9.4f s [min %.4f max %.4f]   torch %9.4f s [min %.4f max %.4f]   ratio %.2fx" % (
        name, *res["device"], *res["torch"], res["torch"][0] / res["device"][0]), flush=True)
    rows.append(res)


def bench_graph(name, dev, scale, k, batch_size, batches, reps, rows):
    data = NodeData(name, device=dev, scale=scale)
    g = data.graph.int()
    g.create_formats_()
    n, E = g.number_of_nodes(), g.number_of_edges()
    reverse = (torch.arange(E, device=dev) + E // 2) % E
    gen = torch.Generator().manual_seed(0)
    meta = dict(graph=name, num_nodes=n, num_edges=E)
    A = "DEVICE_LINKPRED"

    for nq in (4096, 65536):
        e = torch.randint(0, E, (nq // 2,), generator=gen).to(dev)
        u, v = g.find_edges(e)
        u = torch.cat([u.long(), torch.randint(0, n, (nq - nq // 2,), generator=gen).to(dev)])
        v = torch.cat([v.long(), torch.randint(0, n, (nq - nq // 2,), generator=gen).to(dev)])
        ab("has_edges_between %s %dk" % (name, nq // 1024), A, lambda: g.has_edges_between(u, v), same_tensors, rows, queries=nq, **meta)
    e = torch.randint(0, E, (4096,), generator=gen).to(dev)
    u, v = g.find_edges(e)
    ab("edge_ids %s 4k" % name, A, lambda: g.edge_ids(u, v), same_tensors, rows, queries=4096, **meta)

    batch = torch.randint(0, E // 2, (batch_size,), generator=gen).to(dev)
    pos_src = g.find_edges(batch)[0].long()
    for label, flags, form in (("plain", 0, None), ("exclude_existing in-CSR", 1, "in"), ("exclude_existing out-CSR", 1, "out")):
        ab("negatives %s %s" % (name, label), A, lambda: linkpred.negative_destinations(g._index, pos_src, k, flags, 16, 12345, form=form)[0],
           same_tensors, rows, positives=batch_size, k=k, **meta)

    bu, bv = g.find_edges(batch)
    ids = torch.cat([bu.long(), bv.long(), pos_src.repeat_interleave(k), linkpred.negative_destinations(g._index, pos_src, k, 0, 16, 1)[0]])
    ab("compact_nodes %s" % name, A, lambda: linkpred.compact_nodes(n, ids, g.idtype), same_tensors, rows, ids=int(ids.shape[0]), **meta)

    seeds = linkpred.compact_nodes(n, ids, g.idtype)[0]
    frontier, counts = sampling._sample_frontier(g, seeds, 25, generator=torch.Generator().manual_seed(1), want_counts=True)
    excl = torch.sort(torch.cat([batch, reverse[batch]]))[0]
    ab("frontier exclusion %s" % name, A, lambda: sampling.exclude_frontier_edges(frontier, counts, seeds, excl), same_tensors, rows,
       seeds=int(seeds.shape[0]), frontier_edges=int(frontier[0].shape[0]), excluded_ids=int(excl.shape[0]), **meta)

    eids = torch.randperm(E // 2, generator=gen)[:batch_size * batches]
    epoch_row("EdgeDataLoader epoch %s" % name, g, eids, reverse, k, batch_size, rows, reps)


def main():
    p = argparse.ArgumentParser("link-prediction minibatches: device kernels vs torch composition")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--graphs", default="reddit,products")
    p.add_argument("--num-negs", type=int, default=5)
    p.add_argument("--batch-size", type=int, default=4096)
    p.add_argument("--batches", type=int, default=32, help="batches of the timed loader epoch")
    p.add_argument("--epoch-reps", type=int, default=3)
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    rows = []
    for name in filter(None, args.graphs.split(",")):
        bench_graph(name, dev, args.scale, args.num_negs, args.batch_size, args.batches, args.epoch_reps, rows)
    print(json.dumps({"linkpred_bench": rows, "scale": args.scale}))


if __name__ == "__main__":
    main()
