"""PointNet++-style per-point segmentation (Qi et al., PointNet++: Deep Hierarchical Feature Learning on Point Sets in a Metric Space,
single-scale grouping) on the MI355X backend: the encoder of pointnet2.py and the decoder that file lacks.

Down: the two set-abstraction levels of pointnet2.PointNet2, 1024 -> 512 -> 128 centres (ops.segment_fps, the ball-query block,
dgl.nn.PointNetConv), the positions and features of every level kept.  Up: two dgl.nn.FeaturePropagation levels, 128 -> 512 -> 1024:
every finer point takes the features of its 3 nearest coarser points of its own cloud with normalised inverse squared-distance weights
(ops.segment_knn_query: csrc/knn.hip, whose index is the in-CSR of the u_mul_e / sum g-SpMM), concatenates its own features (its
coordinates at the input level) and applies a unit MLP; then a per-point head and per-point cross-entropy.  Nothing on the way reads
back to the host or writes [B, m, n] elements, so a step can be captured in a HIP graph.  The data is the seeded synthetic stand-in
mi355x_graph.datasets.shape_scenes_like (three shapes per cloud, a point's label is its shape).

    PYTHONPATH=dgl-0.5-benchmark_amd python dgl-0.5-benchmark_amd/pointnet2_seg.py --points 1024 --batch 32 [--hipgraph]
"""
import argparse
import os
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

import dgl
import dgl.geometry
from dgl.nn import FeaturePropagation, PointNetConv
from mi355x_graph.datasets import POINT_SHAPES, shape_scenes_like
from mi355x_graph.utils import GraphedStep
from point_cloud import batches
from pointnet2 import NEIGHBORS, NPOINTS, RADII, WIDTHS

UP_WIDTHS = ((256, 128), (128, 128))   # 128 -> 512 centres, 512 centres -> the input points


class PointNet2Seg(nn.Module):
    def __init__(self, num_classes, npoints=NPOINTS, radii=RADII, neighbors=NEIGHBORS, widths=WIDTHS, up_widths=UP_WIDTHS, hidden=128,
                 dropout=0.5, k=3):
        super(PointNet2Seg, self).__init__()
        self.npoints, self.radii, self.neighbors = tuple(npoints), tuple(radii), tuple(neighbors)
        feats = [0] + [w[-1] for w in widths[:-1]]
        self.convs = nn.ModuleList([PointNetConv(f, w) for f, w in zip(feats, widths)])
        skips = [3] + [w[-1] for w in widths[:-1]]          # the input level's own features are its coordinates
        ups, carried = [], widths[-1][-1]
        for skip, w in zip(reversed(skips), up_widths):
            ups.append(FeaturePropagation(carried, skip, w, k=k))
            carried = w[-1]
        self.ups = nn.ModuleList(ups)
        self.head = nn.Sequential(nn.Linear(carried, hidden), nn.ReLU(), nn.Dropout(dropout), nn.Linear(hidden, num_classes))

    def forward(self, xyz):
        """xyz [B, n, 3] -> logits [B * n, classes]"""
        B, n = int(xyz.shape[0]), int(xyz.shape[1])
        pos, h = xyz.reshape(B * n, -1), None
        levels = [(pos, pos, n)]                              # (positions, own features, points per cloud) of every level
        for conv, m, radius, k in zip(self.convs, self.npoints, self.radii, self.neighbors):
            seglen = torch.full((B,), n, dtype=torch.int64, device=pos.device)  # filled in on the device
            centers = dgl.ops.segment_fps(seglen, pos, m, total=B * n, max_len=n).flatten()   # row 0 of every cloud starts: a step is reproducible
            block = dgl.geometry.fixed_radius_block(pos, centers, radius, k, [n] * B)
            h = conv(block, h)
            pos, n = block.dstdata["pos"], m
            levels.append((pos, h, n))
        for up, (fine_pos, fine_h, fine_n) in zip(self.ups, reversed(levels[:-1])):
            h = up(h, pos, fine_pos, [n] * B, [fine_n] * B, fine_h)
            pos, n = fine_pos, fine_n
        return self.head(h)


def train_epoch(model, device, xyz, label, batch, optimizer, shuffle_seed=None):
    model.train()
    total, steps = 0.0, 0
    for x, y in batches(xyz, label, batch, device, shuffle_seed):
        optimizer.zero_grad()
        loss = F.cross_entropy(model(x), y.reshape(-1))
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
            state["step"] = GraphedStep(lambda: F.cross_entropy(model(state["x"]), state["y"].reshape(-1)), optimizer)
        state["x"].copy_(x)
        state["y"].copy_(y)
        total, steps = total + float(state["step"]().detach()), steps + 1
        state["replayed"] = state.get("replayed", 0) + 1
    return total / max(steps, 1)


def make_parser():
    p = argparse.ArgumentParser("PointNet++-style per-point segmentation on the MI355X message-passing backend")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--points", type=int, default=1024)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--npoints", type=int, nargs=2, default=list(NPOINTS), help="centres of the two set-abstraction levels")
    p.add_argument("--radius", type=float, nargs=2, default=list(RADII))
    p.add_argument("--neighbors", type=int, nargs=2, default=list(NEIGHBORS), help="points kept per ball, at most")
    p.add_argument("--k", type=int, default=3, help="coarser points a finer point interpolates from")
    p.add_argument("--clouds", type=int, default=512, help="clouds in the synthetic training set")
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
    xyz, label = shape_scenes_like(args.clouds, args.points)
    torch.manual_seed(0)
    model = PointNet2Seg(len(POINT_SHAPES), args.npoints, args.radius, args.neighbors, dropout=args.dropout, k=args.k).to(device)
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
