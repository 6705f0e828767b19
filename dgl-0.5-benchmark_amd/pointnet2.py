"""PointNet++-style point-cloud classifier (Qi et al., PointNet++: Deep Hierarchical Feature Learning on Point Sets in a Metric Space,
single-scale grouping) on the MI355X backend.

Two set-abstraction levels, 1024 -> 512 centres (radius 0.2, 32 neighbours) -> 128 centres (radius 0.4, 64 neighbours).  Each level is
farthest point sampling (ops.segment_fps: csrc/fps.hip, the whole chain of a cloud in one workgroup), the ball query as a block
(dgl.geometry.fixed_radius_block: csrc/ballquery.hip, whose padded output is the in-CSR) and dgl.nn.PointNetConv; then the per-cloud
maximum and an MLP.  Sampling and grouping are on the hot path of every step, read nothing back to the host and write nothing of
[B, n, n] elements, so a step can be captured in a HIP graph.  The data is the seeded synthetic stand-in
mi355x_graph.datasets.shapes_like (eight noisy parametric shapes).

    PYTHONPATH=dgl-0.5-benchmark_amd python dgl-0.5-benchmark_amd/pointnet2.py --points 1024 --batch 32 [--hipgraph]
"""
import argparse
import os
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

import dgl
import dgl.geometry
from dgl.nn import PointNetConv
from mi355x_graph.datasets import POINT_SHAPES, shapes_like
from mi355x_graph.utils import GraphedStep
from point_cloud import batches

NPOINTS, RADII, NEIGHBORS = (512, 128), (0.2, 0.4), (32, 64)
WIDTHS = ((64, 64, 128), (128, 128, 256))


class PointNet2(nn.Module):
    def __init__(self, num_classes, npoints=NPOINTS, radii=RADII, neighbors=NEIGHBORS, widths=WIDTHS, hidden=256, dropout=0.5):
        super(PointNet2, self).__init__()
        self.npoints, self.radii, self.neighbors = tuple(npoints), tuple(radii), tuple(neighbors)
        feats = [0] + [w[-1] for w in widths[:-1]]
        self.convs = nn.ModuleList([PointNetConv(f, w) for f, w in zip(feats, widths)])
        self.head = nn.Sequential(nn.Linear(widths[-1][-1], hidden), nn.ReLU(), nn.Dropout(dropout), nn.Linear(hidden, num_classes))

    def forward(self, xyz):
        """xyz [B, n, 3] -> logits [B, classes]"""
        B, n = int(xyz.shape[0]), int(xyz.shape[1])
        pos, h = xyz.reshape(B * n, -1), None
        for conv, m, radius, k in zip(self.convs, self.npoints, self.radii, self.neighbors):
            seglen = torch.full((B,), n, dtype=torch.int64, device=pos.device)  # filled in on the device
            centers = dgl.ops.segment_fps(seglen, pos, m, total=B * n, max_len=n).flatten()   # row 0 of every cloud starts: a step is reproducible
            block = dgl.geometry.fixed_radius_block(pos, centers, radius, k, [n] * B)
            h = conv(block, h)
            pos, n = block.dstdata["pos"], m
        return self.head(h.view(B, n, -1).max(1).values)


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
    p = argparse.ArgumentParser("PointNet++-style point-cloud classifier on the MI355X message-passing backend")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--points", type=int, default=1024)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--npoints", type=int, nargs=2, default=list(NPOINTS), help="centres of the two set-abstraction levels")
    p.add_argument("--radius", type=float, nargs=2, default=list(RADII))
    p.add_argument("--neighbors", type=int, nargs=2, default=list(NEIGHBORS), help="points kept per ball, at most")
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
    model = PointNet2(len(POINT_SHAPES), args.npoints, args.radius, args.neighbors, dropout=args.dropout).to(device)
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
