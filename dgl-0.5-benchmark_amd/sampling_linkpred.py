"""Neighbor-sampling link prediction: a 2-layer GraphSAGE over dgl.dataloading.EdgeDataLoader.

The second task family of end_to_end/sampling/ (link-prediction/): a batch of EDGES, k uniform negatives per edge, the batch's own edges
and their reverses kept out of the sampled neighbourhoods, a dot-product score on the model's output and the logsigmoid loss of
cluster_gcn_dgl.py:133-144.  The graph, the features, the edge batches, the negatives and the blocks all stay on the GPU.  Dataset: the
seeded citation-shaped synthetic stand-in (directed citations made bidirected, so the reverse of edge e is e +- E / 2); it follows
MGX_DATASET_SCALE.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
import dgl.function as fn  # noqa: E402
from sampling_sage import SAGE  # noqa: E402


def citation_graph(device, scale=1.0):
    """(bidirected graph, features, reverse_eids): edge e and edge (e + E / 2) % E are each other's reverse."""
    from mi355x_graph.datasets import NodeData
    data = NodeData("citation", device=device, scale=scale)
    s, d = data.graph.edges()
    g = dgl.graph((torch.cat([s, d]), torch.cat([d, s])), num_nodes=data.num_nodes).int()
    g.create_formats_()
    E = g.number_of_edges()
    return g, data.features, (torch.arange(E, device=device) + E // 2) % E


def edge_scores(graph, h):
    with graph.local_scope():
        graph.ndata["h"] = h
        graph.apply_edges(fn.u_dot_v("h", "h", "score"))
        return graph.edata["score"]


def link_loss(pair_graph, neg_graph, h):
    """cluster_gcn_dgl.py:133-144: -mean logsigmoid(score+) - mean logsigmoid(-score-)."""
    pos_loss = -F.logsigmoid(edge_scores(pair_graph, h)).mean()
    neg_loss = -F.logsigmoid(-edge_scores(neg_graph, h)).mean()
    return pos_loss + neg_loss


def make_loader(g, eids, reverse_eids, fanouts, batch_size, k, exclude="reverse_id", exclude_existing=False, generator=None):
    sampler = dgl.dataloading.MultiLayerNeighborSampler(fanouts)
    negatives = dgl.dataloading.negative_sampler.Uniform(k, exclude_existing=exclude_existing)
    return dgl.dataloading.EdgeDataLoader(g, eids, sampler, batch_size=batch_size, shuffle=True, drop_last=False, exclude=exclude,
                                          reverse_eids=reverse_eids if exclude == "reverse_id" else None, negative_sampler=negatives,
                                          generator=generator)


def train_step(model, opt, feats, batch):
    input_nodes, pair_graph, neg_graph, blocks = batch
    h = model(blocks, feats[input_nodes])
    loss = link_loss(pair_graph, neg_graph, h)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def main():
    p = argparse.ArgumentParser("neighbor-sampling link prediction on the MI355X message-passing backend")
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--num-epochs", type=int, default=3)
    p.add_argument("--num-hidden", type=int, default=64)
    p.add_argument("--fan-out", default="10,25")
    p.add_argument("--batch-size", type=int, default=4096)
    p.add_argument("--num-negs", type=int, default=1, help="k: negative destinations per positive edge")
    p.add_argument("--num-train-edges", type=int, default=1 << 20, help="edges of the training set (a seeded sample of the citations)")
    p.add_argument("--exclude", default="reverse_id", choices=["none", "self", "reverse_id"])
    p.add_argument("--exclude-existing", action="store_true", help="reject negatives that are edges of the graph")
    p.add_argument("--lr", type=float, default=0.003)
    p.add_argument("--dropout", type=float, default=0.0)
    args = p.parse_args()
    device = torch.device("cuda:%d" % args.gpu)
    g, feats, reverse_eids = citation_graph(device)
    E = g.number_of_edges()
    gen = torch.Generator().manual_seed(0)
    train_eids = torch.randperm(E // 2, generator=gen)[:min(args.num_train_edges, E // 2)]
    loader = make_loader(g, train_eids, reverse_eids, [int(f) for f in args.fan_out.split(",")], args.batch_size, args.num_negs,
                         None if args.exclude == "none" else args.exclude, args.exclude_existing, generator=gen)
    model = SAGE(feats.shape[1], args.num_hidden, args.num_hidden, 2, F.relu, args.dropout).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    times = []
    for epoch in range(args.num_epochs):
        tic = time.time()
        seen = 0
        for batch in loader:
            loss = train_step(model, opt, feats, batch)
            seen += batch[1].number_of_edges()
        torch.cuda.synchronize()
        toc = time.time()
        print("Epoch {:03d} | Loss {:.4f} | Epoch Time(s): {:.4f} | {:.0f} edges/s".format(epoch, loss.item(), toc - tic, seen / (toc - tic)))
        if epoch >= 1:
            times.append(toc - tic)
    if times:
        print("Training time/epoch {:.5f}".format(sum(times) / len(times)))


if __name__ == "__main__":
    main()
