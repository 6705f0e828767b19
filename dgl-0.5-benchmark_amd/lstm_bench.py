"""LSTM aggregator benchmark: ops.lstm_aggregate fused (csrc/lstm_agg.hip) against the composition it replaces.

Forward + backward (d x, d w_ih, d w_hh, both bias gradients) at D = H = 16, 32 and 64 on
  reddit_f25  a sampled block, 11 000 destinations x 25 in-edges out of 150 000 sources (the first layer of a 1 000-seed batch, fanouts 25, 10)
  reddit_f10  the second block of that batch: 1 000 destinations x 10 in-edges out of 11 000 sources
  arxiv       a full graph of 169 343 nodes and about 1.17 M edges, power-law in-degrees up to 13 155
  molhiv256   bond graphs of 256 molecules (in-degrees 3 .. 5)
  hub         20 000 nodes with power-law in-degrees around 8 and one row of 20 000 in-edges
and one training step (forward, backward, SGD) of SAGEConv(64, 64, "lstm") on reddit_f25, as
  fused     config.LSTM_AGG_FUSED = True: one dense projection per source node, one launch each way for every row's recurrence
  composed  config.LSTM_AGG_FUSED = False: the rows bucketed by in-degree, one LSTM call per bucket on a gathered [B, deg, D] mailbox
Timing: HIP events around every call, after --warmup discarded ones; median / min / max in microseconds of up to --reps calls, fewer
(at least 3) where one call takes so long that --budget seconds would be passed; peak memory above what is allocated before the call.
Both forms run in one process and their results are compared before they are timed.  The script only reports."""
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


def sampled_block(n_dst, fanout, n_src, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    dst = torch.repeat_interleave(torch.arange(n_dst), fanout)
    return mg.create_block((torch.randint(0, n_src, dst.shape, generator=gen), dst), n_src, n_dst, idtype=torch.int32, device=dev)


def power_law_graph(n, edges, longest, dev, seed, hub=None):
    """in-degrees ~ u^-0.9 scaled to about `edges` in all and cut at `longest`; `hub`: the length of one more row"""
    gen = torch.Generator().manual_seed(seed)
    raw = torch.rand(n, generator=gen).clamp(min=1e-6) ** -0.9
    deg = (raw * (edges / float(raw.clamp(max=longest * raw.mean() * n / edges).sum()))).long().clamp(max=longest)
    if hub is not None:
        deg[n // 2] = hub
    dst = torch.repeat_interleave(torch.arange(n), deg)
    return mg.graph((torch.randint(0, n, dst.shape, generator=gen), dst), num_nodes=n).int().formats(["csr", "csc"]).to(dev)


def timed(fn, args):
    out, reps, warmup = [], args.reps, args.warmup
    while len(out) < reps:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        if warmup > 0:  # discarded; a call of a second or more is warm after one
            warmup = 0 if ms >= 1e3 else warmup - 1
            reps = min(args.reps, max(3, int(args.budget * 1e3 / max(ms, 1e-3))))
        else:
            out.append(ms * 1e3)
    out.sort()
    return {"median_us": round(out[len(out) // 2], 1), "min_us": round(out[0], 1), "max_us": round(out[-1], 1), "calls": len(out)}


def both(args, name, fn, extra):
    rec = dict(extra, shape=name)
    for form, fused in (("fused", True), ("composed", False)):
        config.LSTM_AGG_FUSED = fused
        rec[form] = dict(timed(fn, args), peak_mib=peak_mib(fn))
    config.LSTM_AGG_FUSED = True
    rec["speedup"] = round(rec["composed"]["median_us"] / rec["fused"]["median_us"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def op_form(g, H):
    dev, n_src, n_dst = g.device, g.number_of_src_nodes(), g.number_of_dst_nodes()
    torch.manual_seed(H)
    lstm = torch.nn.LSTM(H, H, batch_first=True).to(dev)
    params = tuple(lstm.parameters())
    gen = torch.Generator(device=dev).manual_seed(H)
    x = torch.randn(n_src, H, device=dev, generator=gen).requires_grad_(True)
    up = torch.randn(n_dst, H, device=dev, generator=gen)

    def fwd_bwd():
        return torch.autograd.grad((ops.lstm_aggregate(g, x, *params) * up).sum(), (x,) + params)

    assert ops.lstm_aggregate_fused(g, x, *params)
    got = fwd_bwd()
    config.LSTM_AGG_FUSED = False
    want = fwd_bwd()
    config.LSTM_AGG_FUSED = True
    worst = max(float((a - c).abs().max() / c.abs().max()) for a, c in zip(got, want))
    return fwd_bwd, {"dst": n_dst, "src": n_src, "edges": g.number_of_edges(), "steps": int(g.in_degrees().max()), "H": H, "max_rel_diff": worst}


def layer_form(g, dev):
    torch.manual_seed(0)
    conv = dgl.nn.SAGEConv(64, 64, "lstm").to(dev)
    opt = torch.optim.SGD(conv.parameters(), lr=0.01)
    x = torch.randn(g.number_of_src_nodes(), 64, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        conv(g, x).sum().backward()
        opt.step()

    return step, {"dst": g.number_of_dst_nodes(), "src": g.number_of_src_nodes(), "edges": g.number_of_edges()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--budget", type=float, default=6.0, help="seconds of timed calls per form and shape")
    p.add_argument("--shapes", default="reddit_f25,reddit_f10,arxiv,molhiv256,hub,sage")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    builders = {"reddit_f25": lambda: sampled_block(11000, 25, 150000, dev, 1), "reddit_f10": lambda: sampled_block(1000, 10, 11000, dev, 2),
                "arxiv": lambda: power_law_graph(169343, 1166243, 13155, dev, 3), "molhiv256": lambda: molhiv_batch(256, dev),
                "hub": lambda: power_law_graph(20000, 160000, 2000, dev, 4, hub=20000)}
    recs = []
    for name in args.shapes.split(","):
        if name == "sage":
            recs.append(both(args, "sage_step_reddit_f25", *layer_form(builders["reddit_f25"](), dev)))
            continue
        g = builders[name]()
        for H in (16, 32, 64):
            recs.append(both(args, name, *op_form(g, H)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
