"""DGCNN-style point-cloud classifier (Wang et al., Dynamic Graph CNN for Learning on Point Clouds) on the MI355X backend.

Four dgl.nn.EdgeConv layers 3 -> 64 -> 64 -> 128 -> 256; the k-NN graph is REBUILT from every layer's input, in feature space
(dgl.knn_graph: csrc/knn.hip, whose output is the in-CSR), so graph construction is on the hot path of every step.  Readout: the
per-cloud maximum of the last layer (max_nodes), then an MLP.  The data is the seeded synthetic stand-in mi355x_graph.datasets.shapes_like
(eight noisy parametric shapes).

    PYTHONPATH=dgl-0.5-benchmark_amd python dgl-0.5-benchmark_amd/point_cloud.py --points 1024 --batch 32 --k 20 [--hipgraph]
"""
import argparse
import os
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

import dgl
from dgl.nn import EdgeConv
from mi355x_graph.datasets import POINT_SHAPES, shapes_like
from mi355x_graph.utils import GraphedStep

WIDTHS = (3, 64, 64, 128, 256)


class DGCNN(nn.Module):
    def __init__(self, k, num_classes, widths=WIDTHS, hidden=256, dropout=0.5):
        super(DGCNN, self).__init__()
        self.k = k
        self.convs = nn.ModuleList([EdgeConv(a, b) for a, b in zip(widths[:-1], widths[1:])])
        self.head = nn.Sequential(nn.Linear(widths[-1], hidden), nn.LeakyReLU(0.2), nn.Dropout(dropout), nn.Linear(hidden, num_classes))

    def forward(self, xyz):
        """xyz [B, n, 3] -> logits [B, classes]"""
        B, n = int(xyz.shape[0]), int(xyz.shape[1])
        h = xyz.reshape(B * n, -1)
        for conv in self.convs:
            g = dgl.knn_graph(h.view(B, n, -1), self.k)  # every cloud on its own; no gradient flows through the selection
            h = F.leaky_relu(conv(g, h), 0.2)
        g.set_batch_num_nodes(torch.full((B,), n, dtype=torch.int64, device=h.device))  # the last graph doubles as the batch of B clouds
        g.ndata["h"] = h
        return self.head(dgl.max_nodes(g, "h"))


def batches(xyz, label, batch, device, shuffle_seed=None):
    """whole batches only: every step has one shape"""
    order = torch.arange(xyz.shape[0])
    if shuffle_seed is not None:
        order = torch.randperm(xyz.shape[0], generator=torch.Generator().manual_seed(shuffle_seed))
    for i in range(0, xyz.shape[0] - batch + 1, batch):
        pick = order[i:i + batch]
        yield xyz[pick].to(device), label[pick].to(device)


def train_epoch(model, device, xyz, label, batch, optimizer, shuffle_seed=None):
    model.train()
    total, steps = 0.0, 0
    for x, y in batches(xyz, label, batch, device, shuffle_seed):
        optimizer.zero_grad()
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        optimizer.step()
        total, steps = total + float(loss.detach()), steps + 1
    return total / max(steps, 1)


def train_epoch_graphed(model, device, xyz, label, batch, optimizer, state, shuffle_seed=None):
    """the same epoch with ONE captured step (utils.GraphedStep) replayed on static input buffers"""
    model.train()
    total, steps = 0.0, 0
    for x, y in batches(xyz, label, batch, device, shuffle_seed):
        if "step" not in state:
            state["x"], state["y"] = x.clone(), y.clone()
            state["step"] = GraphedStep(lambda: F.cross_entropy(model(state["x"]), state["y"]), optimizer)
        state["x"].copy_(x)
        state["y"].copy_(y)
        total, steps = total + float(state["step"]().detach()), steps + 1
        state["replayed"] = state.get("replayed", 0) + 1
    return total / max(steps, 1)


def make_parser():
    p = argparse.ArgumentParser("DGCNN-style point-cloud classifier on the MI355X message-passing backend")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--points", type=int, default=1024)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--k", type=int, default=20)
    p.add_argument("--clouds", type=int, default=1024, help="clouds in the synthetic training set")
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--no-shuffle", action="store_true")
    p.add_argument("--hipgraph", action="store_true", help="capture one training step in a HIP graph and replay it (GraphedStep)")
    return p


def main():
    args = make_parser().parse_args()
    torch.set_num_threads(max(1, min(int(os.environ.get("MGX_HOST_THREADS", "4")), os.cpu_count() or 1)))
    device = torch.device("cuda:%d" % args.device)
    xyz, label = shapes_like(args.clouds, args.points)
    torch.manual_seed(0)
    model = DGCNN(args.k, len(POINT_SHAPES), dropout=args.dropout).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, capturable=args.hipgraph)
    state, dur = {}, []
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        seed = None if args.no_shuffle else epoch
        if args.hipgraph:
            loss = train_epoch_graphed(model, device, xyz, label, args.batch, opt, state, seed)
        else:
            loss = train_epoch(model, device, xyz, label, args.batch, opt, seed)
        torch.cuda.synchronize()
        if epoch >= 2:
            dur.append(time.time() - t0)
        print("epoch %d loss %.4f time %.3f" % (epoch, loss, time.time() - t0))
    if args.hipgraph:
        print("hipgraph: %d steps replayed" % state.get("replayed", 0))
    if dur:
        print("Training time/epoch {:.4f}".format(sum(dur) / len(dur)))


if __name__ == "__main__":
    main()
