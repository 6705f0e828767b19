"""Batched small-graph classification: this backend's launcher for
end_to_end/full_graph/graph_classification/main_dgl_molhiv_gcn.py (BASELINE config 5).

The model restates the script's GCN-with-bond-encoder: per layer `in_degrees()`, a Python UDF message
`norm * relu(src.x + edge.w)` reduced with the builtin fn.sum (main_dgl_molhiv_gcn.py:37-52), AvgPooling
readout (:75,93), batches built by GraphDataLoader/dgl.batch and moved with
`.to(device).int().formats('coo')` (:101).  The UDF path here = two per-edge gathers (g-SDDMM copy
kernels), the UDF in PyTorch, then a copy_e/sum g-SpMM; the readout is mgx_segment_reduce.
The dataset is the seeded molhiv-shaped synthetic stand-in (mi355x_graph.datasets.molhiv_like).
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402
import dgl.function as fn  # noqa: E402
from dgl.dataloading import GraphDataLoader  # noqa: E402


class CategoricalEncoder(nn.Module):
    """Sum of one embedding table per integer feature column (the role of OGB's AtomEncoder/BondEncoder)."""

    def __init__(self, emb_dim, num_columns, cardinality=16):
        super(CategoricalEncoder, self).__init__()
        self.tables = nn.ModuleList([nn.Embedding(cardinality, emb_dim) for _ in range(num_columns)])
        for t in self.tables:
            nn.init.xavier_uniform_(t.weight.data)

    def forward(self, x):
        # sum_i table_i[x[:, i]] as ONE product of the concatenated one-hot codes with the stacked tables: the same sum,
        # one GEMM each way instead of num_columns lookups + adds -- and safe to capture in a HIP graph: the sort-based
        # backward of torch.embedding reads a segment count back to the host (thrust::unique_by_key_copy), which under
        # capture bakes whatever that memory held into the following launches (the replay then faulted inside
        # rocprim::partition_kernel; bisected in round 2).
        card = self.tables[0].num_embeddings
        codes = F.one_hot(x, card).to(self.tables[0].weight.dtype).flatten(1)       # [rows, columns * cardinality]
        return codes @ torch.cat([t.weight for t in self.tables], dim=0)


class GCNConv(nn.Module):
    """fused=True (--fused-message): the message-and-sum of the UDF below as ONE operator, dgl.ops.gine_sum -- the same values with
    no [E, D] tensor written (csrc/gine.hip); `norm` is then formed once per batch by GCN.forward and handed in."""

    def __init__(self, in_feats, out_feats, bond_columns=3, fused=False):
        super(GCNConv, self).__init__()
        self.fused = fused
        self.fc = nn.Linear(in_feats, out_feats, bias=False)
        self.root_emb = nn.Embedding(1, in_feats)
        self.bond_encoder = CategoricalEncoder(in_feats, bond_columns)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.fc.weight, gain=nn.init.calculate_gain("relu"))
        self.root_emb.reset_parameters()

    def forward(self, graph, feat, bond, norm=None):
        graph = graph.local_var()
        x = self.fc(feat)
        deg = graph.in_degrees().float().unsqueeze(1) + 1
        if self.fused:
            h = dgl.ops.gine_sum(graph, x, self.bond_encoder(bond), scale=norm)
            return h + F.relu(x + self.root_emb.weight) * 1. / deg
        graph.ndata["c"] = deg.pow(-0.5)
        graph.ndata["x"] = x
        graph.edata["w"] = self.bond_encoder(bond)
        graph.update_all(self.message, fn.sum("m", "h"))
        return graph.ndata["h"] + F.relu(x + self.root_emb.weight) * 1. / deg

    def message(self, edges):
        norm = edges.src["c"] * edges.dst["c"]
        return {"m": norm * F.relu(edges.src["x"] + edges.data["w"])}


def make_readout(kind, emb_dim, sortpool_k=30):
    """(readout module, width of its output) for --readout: `mean` is the reference's AvgPooling (main_dgl_molhiv_gcn.py:75); `attention`
    is dgl.nn.GlobalAttentionPooling with a Linear(emb_dim, 1) gate; `set2set` is dgl.nn.Set2Set(emb_dim, 3 iterations, 1 LSTM layer),
    whose output is twice as wide.  Both attention readouts run ops.segment_attention (csrc/segattn.hip): one launch each way.
    `sortpool` is dgl.nn.SortPooling(sortpool_k): the k nodes with the largest last (sorted) feature, flattened to k * emb_dim columns
    (ops.segment_topk, csrc/segtopk.hip); its output shape is static, so the padded batches of --hipgraph capture it as it is."""
    if kind == "mean":
        return dgl.nn.AvgPooling(), emb_dim
    if kind == "attention":
        return dgl.nn.GlobalAttentionPooling(nn.Linear(emb_dim, 1)), emb_dim
    if kind == "set2set":
        return dgl.nn.Set2Set(emb_dim, n_iters=3, n_layers=1), 2 * emb_dim
    if kind == "sortpool":
        return dgl.nn.SortPooling(sortpool_k), sortpool_k * emb_dim
    raise ValueError("unknown readout %r" % (kind,))


class GCN(nn.Module):
    def __init__(self, emb_dim, num_classes, num_layers, dropout, atom_columns=9, bond_columns=3, readout="mean", fused=False, sortpool_k=30):
        super(GCN, self).__init__()
        self.fused = fused
        self.atom_encoder = CategoricalEncoder(emb_dim, atom_columns)
        self.layers = nn.ModuleList([GCNConv(emb_dim, emb_dim, bond_columns, fused=fused) for _ in range(num_layers)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(emb_dim) for _ in range(num_layers - 1)])
        self.dropout = nn.Dropout(p=dropout)
        self.readout, width = make_readout(readout, emb_dim, sortpool_k)
        self.graph_pred_fc = nn.Linear(width, num_classes, bias=False)

    def edge_norm(self, g):
        """[E] c[src] * c[dst], c = (in_degree + 1) ** -0.5: the `norm` of GCNConv.message, the same for every layer of a batch"""
        c = (g.in_degrees().float() + 1).pow(-0.5)
        src, dst = g.edges()
        return c[src.long()] * c[dst.long()]

    def forward(self, g, atom, bond):
        x = self.atom_encoder(atom)
        extra = (self.edge_norm(g),) if self.fused else ()
        for i, layer in enumerate(self.layers[:-1]):
            x = self.dropout(F.relu(self.bns[i](layer(g, x, bond, *extra))))
        x = self.layers[-1](g, x, bond, *extra)
        return self.graph_pred_fc(self.readout(g, x))


class GIN(nn.Module):
    """5-layer GIN (BASELINE.json config 5 as worded): h <- MLP((1 + eps) h + sum_{u->v} h_u) with dgl.nn.GINConv, i.e. one
    copy_u/sum g-SpMM per layer on the batched graph; atom encoder, BatchNorm / relu / dropout and the mean readout as in
    the GCN above.  Bond features are not used (plain GIN)."""

    def __init__(self, emb_dim, num_classes, num_layers, dropout, atom_columns=9, readout="mean", sortpool_k=30):
        super(GIN, self).__init__()
        from dgl.nn.pytorch import GINConv
        self.atom_encoder = CategoricalEncoder(emb_dim, atom_columns)
        mlp = lambda: nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.BatchNorm1d(2 * emb_dim), nn.ReLU(),
                                    nn.Linear(2 * emb_dim, emb_dim))
        self.layers = nn.ModuleList([GINConv(mlp(), "sum", learn_eps=True) for _ in range(num_layers)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(emb_dim) for _ in range(num_layers - 1)])
        self.dropout = nn.Dropout(p=dropout)
        self.readout, width = make_readout(readout, emb_dim, sortpool_k)
        self.graph_pred_fc = nn.Linear(width, num_classes, bias=False)

    def forward(self, g, atom, bond=None):
        x = self.atom_encoder(atom)
        for i, layer in enumerate(self.layers[:-1]):
            x = self.dropout(F.relu(self.bns[i](layer(g, x))))
        x = self.layers[-1](g, x)
        return self.graph_pred_fc(self.readout(g, x))


class PNA(nn.Module):
    """Principal Neighbourhood Aggregation on the molhiv-shaped batches: dgl.nn.PNAConv layers (mean / max / min / std of one message
    per bond, identity / amplification / attenuation scalers, bond features of width `edge_dim` through edge_feat_size, 4 towers when
    emb_dim allows), whose aggregation is ONE dgl.ops.multi_aggregate call per layer (csrc/multiagg.hip); atom encoder and readout as
    in the GCN above.  `delta` is the training set's mean of log(in_degree + 1) (pna_delta)."""

    AGGREGATORS = ("mean", "max", "min", "std")
    SCALERS = ("identity", "amplification", "attenuation")

    def __init__(self, emb_dim, num_classes, num_layers, dropout, delta=1.0, atom_columns=9, bond_columns=3, readout="mean", sortpool_k=30,
                 edge_dim=16):
        super(PNA, self).__init__()
        from dgl.nn.pytorch import PNAConv
        towers = 4 if emb_dim % 16 == 0 else 1
        self.atom_encoder = CategoricalEncoder(emb_dim, atom_columns)
        self.bond_encoder = CategoricalEncoder(edge_dim, bond_columns)
        self.layers = nn.ModuleList([PNAConv(emb_dim, emb_dim, self.AGGREGATORS, self.SCALERS, delta, dropout=dropout, num_towers=towers,
                                             edge_feat_size=edge_dim) for _ in range(num_layers)])
        self.readout, width = make_readout(readout, emb_dim, sortpool_k)
        self.graph_pred_fc = nn.Linear(width, num_classes, bias=False)

    def forward(self, g, atom, bond):
        x = self.atom_encoder(atom)
        e = self.bond_encoder(bond)
        for layer in self.layers:
            x = layer(g, x, e)
        return self.graph_pred_fc(self.readout(g, x))


def pna_delta(data, batch_size=1024):
    """PNA's degree normaliser: the mean of log(in_degree + 1) over the nodes of the training graphs, read from their batches"""
    total, count = 0.0, 0
    for bg, _ in GraphDataLoader(data, batch_size=batch_size, shuffle=False):
        deg = bg.in_degrees().double()
        total += float(torch.log(deg + 1).sum())
        count += int(deg.shape[0])
    return total / max(count, 1)


class MaskedBatchNorm1d(nn.BatchNorm1d):
    """nn.BatchNorm1d whose training-mode statistics span only the rows flagged in `mask` ([N, 1] bool, `count` = their
    number as a 0-dim device tensor): batches padded to a bucket size keep the statistics, outputs, gradients and running
    estimates of the unpadded batch.  Same parameters / buffers / state_dict as nn.BatchNorm1d; without a mask it IS it."""

    _mask = None
    _count = None

    def set_valid(self, mask, count):
        self._mask, self._count = mask, count

    def forward(self, x):
        if self._mask is None or not self.training:
            return super(MaskedBatchNorm1d, self).forward(x)
        m, n = self._mask, self._count  # m: [N, 1] bool; masked rows may hold anything (where, not multiply: inf * 0 = nan)
        zero = x.new_zeros(())
        mean = torch.where(m, x, zero).sum(0) / n
        xc = x - mean
        var = torch.where(m, xc * xc, zero).sum(0) / n
        y = xc * torch.rsqrt(var + self.eps)
        if self.affine:
            y = y * self.weight + self.bias
        # masked (ghost) rows restart from zero after every normalisation.  They are scaled by the REAL rows' statistics, so
        # a near-constant real column (variance ~ 0) multiplies a ghost value by up to 1/sqrt(eps) = 316 per layer; left
        # alone that overflowed after a few layers (GIN, 5 layers x 2 BatchNorms) and 0 * inf in the next weight-gradient
        # GEMM made every parameter NaN, although ghost rows carry a zero output gradient.
        y = torch.where(m, y, zero)
        if self.track_running_stats:
            with torch.no_grad():
                self.num_batches_tracked += 1
                mom = self.momentum if self.momentum is not None else 0.1
                self.running_mean.mul_(1 - mom).add_(mean.detach() * mom)
                self.running_var.mul_(1 - mom).add_(var.detach() * (n / (n - 1).clamp(min=1.0)) * mom)
        return y


def convert_masked_batchnorm(module):
    """Every nn.BatchNorm1d under `module` -> MaskedBatchNorm1d with the same state."""
    out = module
    if isinstance(module, nn.BatchNorm1d) and not isinstance(module, MaskedBatchNorm1d):
        out = MaskedBatchNorm1d(module.num_features, module.eps, module.momentum, module.affine, module.track_running_stats)
        out.load_state_dict(module.state_dict())
        out.to(module.weight.device if module.affine else "cpu")
        out.train(module.training)
    for name, child in module.named_children():
        out.add_module(name, convert_masked_batchnorm(child))
    return out


class GraphedBatchTrainer(object):
    """The batched small-graph loop (main_dgl_molhiv_gcn.py:95-115) with the launch latency taken out: a training step on
    256 molecules is ~300 kernels of a few microseconds each, and eager mode spends ~11 ms of host time launching ~1.5 ms
    of device work.  Every batch -- the last, smaller one of an epoch too -- is padded to ONE static shape (ghost nodes
    at the end, ghost edges spread round-robin over the ghost nodes so that no ghost row becomes a hub, empty ghost
    graphs up to the batch size, one extra ghost "graph" holding the ghost
    nodes in the readout), and the whole step (device CSR build, forward, masked loss,
    backward, Adam) is captured once in a HIP graph and replayed.  Ghost rows never reach a real graph's output, the
    loss or a parameter gradient (their output gradient is zero); BatchNorm statistics are masked to the real rows
    (MaskedBatchNorm1d); the loss is the mean over the real graphs.  A batch larger than the static shape (4.5 sigma above
    the mean batch: ~1 in 300,000) is trained as two half batches.
    One captured graph, no eager steps in between: replaying an older capture after a later, larger one faulted on
    ROCm 7.2 in this loop (bisected in round 2), so there is a single static shape rather than buckets."""

    def __init__(self, model, optimizer, loss_fn, device, batch_size, n_pad, e_pad):
        if not isinstance(loss_fn, nn.BCEWithLogitsLoss) or loss_fn.reduction != "mean":
            raise ValueError("GraphedBatchTrainer masks a mean-reduced BCEWithLogitsLoss (main_dgl_molhiv_gcn.py:160)")
        self.model, self.opt, self.device = model, optimizer, device
        self.B, self.n_pad, self.e_pad = batch_size, int(n_pad), int(e_pad)
        self.graph = None
        self.stats = {"replayed": 0, "split": 0}
        self.bns = [m for m in model.modules() if isinstance(m, MaskedBatchNorm1d)]

    @staticmethod
    def static_shape(dataset, batch_size, sigmas=4.5, edge_slack=1.03):
        """(n_pad, e_pad) covering a random batch of `batch_size` graphs with `sigmas` to spare."""
        import math
        nn_ = torch.tensor([g.number_of_nodes() for g, _ in (dataset[i] for i in range(len(dataset)))], dtype=torch.float64)
        ne_ = torch.tensor([g.number_of_edges() for g, _ in (dataset[i] for i in range(len(dataset)))], dtype=torch.float64)
        n = batch_size * float(nn_.mean()) + sigmas * math.sqrt(batch_size) * float(nn_.std())
        e = batch_size * float(ne_.mean()) + sigmas * math.sqrt(batch_size) * float(ne_.std())
        return (int(n) // 256 + 1) * 256, (int(e * edge_slack) // 256 + 1) * 256

    def fits(self, bg):
        return bg.number_of_nodes() + 2 <= self.n_pad and bg.number_of_edges() <= self.e_pad  # two ghost nodes at least

    def _pad(self, bg, labels, into=None):
        """Host tensors of the padded batch (ghost nodes / edges / graphs appended), written IN PLACE into `into` (a set of static-shape
        buffers: the pinned staging set of step()) or into new tensors.  A dozen slice assignments: no concatenation, no second copy."""
        n, e, b = bg.number_of_nodes(), bg.number_of_edges(), int(labels.shape[0])
        n_pad, e_pad, B = self.n_pad, self.e_pad, self.B
        src, dst = bg.edges()
        atom, bond = bg.ndata["feat"], bg.edata["feat"]
        if into is None:
            into = {"src": torch.empty(e_pad, dtype=torch.int32), "dst": torch.empty(e_pad, dtype=torch.int32),
                    "atom": atom.new_empty((n_pad,) + tuple(atom.shape[1:])), "bond": bond.new_empty((e_pad,) + tuple(bond.shape[1:])),
                    "bnn": torch.empty(B + 1, dtype=torch.int64), "labels": torch.empty(B), "gmask": torch.empty(B),
                    "gcount": torch.empty(()), "mask": torch.empty((n_pad, 1), dtype=torch.bool), "count": torch.empty(())}
        if getattr(self, "_ramp", None) is None:
            self._ramp = torch.arange(e_pad + 1, dtype=torch.int32)
        # ghost edges run round-robin over the ghost nodes (i -> i + 1): ghost rows keep the degree of ordinary nodes, so
        # their values stay in the range of real rows under a sum aggregator (one ghost hub overflowed GIN's to inf)
        ghosts, ge = n_pad - n, e_pad - e
        into["src"][:e].copy_(src)
        into["dst"][:e].copy_(dst)
        if ge:
            torch.remainder(self._ramp[:ge], ghosts, out=into["src"][e:])
            torch.remainder(self._ramp[1:ge + 1], ghosts, out=into["dst"][e:])
            into["src"][e:].add_(n)
            into["dst"][e:].add_(n)
        into["atom"][:n].copy_(atom)
        into["atom"][n:].zero_()
        into["bond"][:e].copy_(bond)
        into["bond"][e:].zero_()
        bnn = into["bnn"]
        bnn[:b].copy_(bg.batch_num_nodes())
        bnn[b:B].zero_()
        bnn[B] = ghosts
        into["labels"][:b].copy_(labels.view(-1))
        into["labels"][b:].zero_()
        into["gmask"][:b].fill_(1.0)
        into["gmask"][b:].zero_()
        into["gcount"].fill_(float(b))
        into["mask"][:n].fill_(True)
        into["mask"][n:].fill_(False)
        into["count"].fill_(float(n))
        return into

    def _forward_loss(self, buf):
        from mi355x_graph.graph import DGLGraph, GraphIndex
        g = DGLGraph(GraphIndex(self.n_pad, self.n_pad, coo=(buf["src"], buf["dst"])))
        g._batch_num_nodes = buf["bnn"]
        g._batch_num_edges = None
        for view in (g._index.csc(), g._index.csr()):  # built on the device inside the step; small graphs run without a schedule
            view._plan = None                            # (building one reads a maximum degree back: a host sync)
            view.short_hint = True                       # molecules + round-robin ghost edges: short rows, one item per lane group
        for bn in self.bns:
            bn.set_valid(buf["mask"], buf["count"])
        out = self.model(g, buf["atom"], buf["bond"])
        per_graph = F.binary_cross_entropy_with_logits(out[:self.B].float().view(-1), buf["labels"], reduction="none")
        return (per_graph * buf["gmask"]).sum() / buf["gcount"]

    def _capture(self, pad):
        self.buf = buf = {k: v.to(self.device) for k, v in pad.items()}
        # warm-up steps outside the capture (allocator, GEMM heuristics, lazily created optimizer state); the training
        # state they change -- parameters, BatchNorm buffers, Adam moments and step counts -- is put back afterwards, in
        # place (the captured graph holds these tensors' addresses), so the capture does not alter the optimisation trajectory
        params, buffers = list(self.model.parameters()), list(self.model.buffers())
        snap_p = [t.detach().clone() for t in params]
        snap_b = [t.detach().clone() for t in buffers]
        snap_o = {id(p): {k: v.detach().clone() for k, v in self.opt.state[p].items() if torch.is_tensor(v)}
                  for p in params if p in self.opt.state}
        # Warm-up and capture run on ONE side stream.  Autograd remembers the stream a parameter's gradient accumulator
        # first ran on; capturing on a different stream makes every accumulation a cross-stream fork / join inside the
        # graph, and such a forked graph gave NaNs after a hipDeviceSynchronize between replays on ROCm 7.2 (GIN, 5
        # layers; bisected in round 2).  Same stream -> a linear graph.
        side = self.side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        from mi355x_graph import ops as _ops
        with torch.cuda.stream(side), _ops.warming_up_for_capture():  # the forms operators take under capture, here too
            for _ in range(2):
                self.opt.zero_grad(set_to_none=True)
                self._forward_loss(buf).backward()
                self.opt.step()
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():
            for t, v in zip(params, snap_p):
                t.copy_(v)
            for t, v in zip(buffers, snap_b):
                t.copy_(v)
            for p_ in params:
                for k, v in self.opt.state.get(p_, {}).items():
                    if torch.is_tensor(v):
                        old = snap_o.get(id(p_), {}).get(k)
                        v.copy_(old) if old is not None else v.zero_()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        self.opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(self.graph, stream=side):
            self.loss = self._forward_loss(buf)
            self.loss.backward()
            self.opt.step()

    def step(self, bg, labels):
        """One training step on a collated (host) batch; returns the loss as a 0-dim device tensor."""
        if not self.fits(bg) or labels.shape[0] > self.B:
            from mi355x_graph.transform import batch as batch_graphs, unbatch
            parts = unbatch(bg)
            if len(parts) < 2:
                raise ValueError("a single graph with %d nodes exceeds the static shape" % bg.number_of_nodes())
            self.stats["split"] += 1
            h = len(parts) // 2
            self.step(batch_graphs(parts[:h]), labels[:h])
            return self.step(batch_graphs(parts[h:]), labels[h:])
        pad = None
        if self.graph is None:
            pad = self._pad(bg, labels)
            self._capture(pad)
            self.done = torch.cuda.Event()
            # pinned staging, two sets in ping-pong: the copies below are then real stream commands (a copy from pageable
            # memory is carried out by the HOST once the stream has drained what was submitted before it -- which is not
            # the same thing as "the previous replay has finished" for a graph launch)
            self.stage = [{k: torch.empty_like(v, device="cpu").pin_memory() for k, v in pad.items()} for _ in range(2)]
            self.staged = [torch.cuda.Event(), torch.cuda.Event()]
            self.turn = 0
        # ONE stream orders everything (round 3): the static inputs are copied and the graph is replayed on
        # the stream it was captured on, so a replay's kernels, the next step's input copies and the next replay follow each other
        # in stream order -- no host-side wait for the previous replay, and a device-wide synchronize() anywhere is harmless.
        i = self.turn
        self.turn ^= 1
        self.staged[i].synchronize()  # the copies that last read this staging set (two steps ago) are done
        if pad is None:
            self._pad(bg, labels, into=self.stage[i])  # straight into the pinned set: host work that overlaps with the previous replay
        else:
            for k, v in pad.items():
                self.stage[i][k].copy_(v)
        with torch.cuda.stream(self.side):
            for k in self.buf:
                self.buf[k].copy_(self.stage[i][k], non_blocking=True)
            self.staged[i].record()
            self.graph.replay()
            self.done.record()
        self.stats["replayed"] += 1
        return self.loss

    def loss_value(self):
        """The last step's loss on the host (waits for that replay: it ran on the capture stream, not the current one)."""
        self.done.synchronize()
        return float(self.loss.detach())


def train_epoch_graphed(trainer, loader):
    trainer.model.train()
    loss = None
    for batched_graph, labels in loader:
        loss = trainer.step(batched_graph, labels)
    return trainer.loss_value()


def train_epoch(model, device, loader, optimizer, loss_fn):
    model.train()
    loss = None
    for batched_graph, labels in loader:
        batched_graph = batched_graph.to(device).int().formats("coo")  # main_dgl_molhiv_gcn.py:101
        labels = labels.to(device)
        optimizer.zero_grad()
        out = model(batched_graph, batched_graph.ndata["feat"], batched_graph.edata["feat"])
        loss = loss_fn(out.float().view(-1), labels.float().view(-1))
        loss.backward()
        optimizer.step()
    return loss.item()


def make_parser():
    p = argparse.ArgumentParser("molhiv-shaped GCN on the MI355X message-passing backend")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--num_layers", type=int, default=5)
    p.add_argument("--emb_dim", type=int, default=256)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--num_graphs", type=int, default=32901)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--num_workers", type=int, default=0)
    p.add_argument("--hipgraph", action="store_true",
                   help="pad every batch to one static shape and replay one captured HIP graph (GraphedBatchTrainer)")
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--model", default="gcn", choices=["gcn", "gin", "pna"],
                   help="gcn: the reference's main_dgl_molhiv_gcn.py model; gin: BASELINE.json's wording of config 5; pna: Principal "
                        "Neighbourhood Aggregation (dgl.nn.PNAConv with bond features; eager only)")
    p.add_argument("--readout", default="mean", choices=["mean", "attention", "set2set", "sortpool"],
                   help="mean: the reference's AvgPooling; attention: GlobalAttentionPooling; set2set: Set2Set (3 iterations); "
                        "sortpool: SortPooling (--sortpool-k nodes per graph)")
    p.add_argument("--sortpool-k", type=int, default=30, help="--readout sortpool: nodes kept per graph")
    p.add_argument("--fused-message", action="store_true",
                   help="gcn: run every layer's norm * relu(x_u + w_e) message and its sum as ONE operator (dgl.ops.gine_sum) instead "
                        "of the UDF's gathers, add / relu / mul and copy_e/sum g-SpMM")
    return p


def main():
    parser = make_parser()
    args = parser.parse_args()
    if args.model == "pna" and args.hipgraph:
        # the captured step pads every batch with dummy nodes and edges; PNAConv owns its batch norms and its 1 / sqrt(nodes of the graph)
        # factor, which would count the padding -- the capture machinery is not bent for it
        parser.error("--model pna runs eager only: --hipgraph pads batches, and the padding would enter PNAConv's batch norms and graph sizes")
    # batching is a handful of tiny CPU tensor ops per step: with torch's default of one thread per visible core (128 on
    # the GPU box, 16 usable) every one of them fans out and an iteration's host work takes 17 ms instead of 0.1 ms
    torch.set_num_threads(max(1, min(int(os.environ.get("MGX_HOST_THREADS", "4")), os.cpu_count() or 1)))
    from mi355x_graph.datasets import molhiv_like
    device = torch.device("cuda:%d" % args.device)
    data = molhiv_like(args.num_graphs)
    loader = GraphDataLoader(data, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers)
    torch.manual_seed(0)
    extra = {"fused": True} if args.fused_message and args.model == "gcn" else {}
    if args.model == "pna":
        extra = {"delta": pna_delta(data)}
    model = {"gcn": GCN, "gin": GIN, "pna": PNA}[args.model](args.emb_dim, 1, args.num_layers, args.dropout, readout=args.readout,
                                                             sortpool_k=args.sortpool_k, **extra).to(device)
    loss_fn = nn.BCEWithLogitsLoss()
    trainer = None
    if args.hipgraph:
        model = convert_masked_batchnorm(model)
        opt = torch.optim.Adam(model.parameters(), lr=0.001, capturable=True)
        n_pad, e_pad = GraphedBatchTrainer.static_shape(data, args.batch_size)
        trainer = GraphedBatchTrainer(model, opt, loss_fn, device, args.batch_size, n_pad, e_pad)
        print("hipgraph: static batch shape %d nodes, %d edges, %d graphs" % (n_pad, e_pad, args.batch_size))
    else:
        opt = torch.optim.Adam(model.parameters(), lr=0.001)
    dur = []
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        if trainer is not None:
            loss = train_epoch_graphed(trainer, loader)
            # loss_value() waited for the epoch's last replay (the event covers the Adam update).  Round 2 avoided a device-wide
            # synchronize here (later replays of the 5-layer GIN turned NaN); with copies and replays ordered on one stream
            # (GraphedBatchTrainer.step) it is harmless -- tests/test_graphed_batches.py soaks 300 replays with one every 10.
            torch.cuda.synchronize()
        else:
            loss = train_epoch(model, device, loader, opt, loss_fn)
            torch.cuda.synchronize()
        if epoch >= 2:
            dur.append(time.time() - t0)
        print("epoch %d loss %.4f time %.3f" % (epoch, loss, time.time() - t0))
    if trainer is not None:
        print("hipgraph: %d steps replayed, %d oversize batches split" % (trainer.stats["replayed"], trainer.stats["split"]))
    if dur:
        print("Training time/epoch {:.4f}".format(sum(dur) / len(dur)))


if __name__ == "__main__":
    main()
