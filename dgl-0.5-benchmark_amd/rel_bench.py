"""Multi-relation g-SpMM benchmark: the per-relation loop of the reference's relational layer against the one-pass kernels.

On the proteins-shaped stand-in of mi355x_graph.datasets (N 132,534, E 79.1 M, R 8) and for D in {1, 32, 64}:
  (a) loop     R x dgl.ops.gspmm(g, 'mul', 'mean', x, w[:, r:r+1]) with the [E, 1] column views the reference layer passes
               (main_dgl_proteins_rgcn_for.py:50-53, 159-161) -- the path the package took before csrc/spmm_rel.hip;
  (b) fused    ops.rel_gspmm forward (permuted weights cached, as in training);
  (c) both, forward + backward (gradient with respect to x);
  (d) one training step of full_graph.RGCN against the same model built from per-relation loop layers.
Timing follows kernel_bench.time_op (HIP events, 10 repetitions, the first 2 discarded).  GB/s is against the algorithmic bytes
nnz * (idx + 4 R) + N_src * 4 D + N_dst * 4 R D (the reverse walk: the same with the roles of x and out exchanged).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
import dgl.ops  # noqa: E402
import full_graph  # noqa: E402
from kernel_bench import time_op, spread  # noqa: E402
from mi355x_graph import ops  # noqa: E402


def rel_bytes(n_src, n_dst, nnz, R, D, idx_bytes=4):
    return nnz * (idx_bytes + 4 * R) + n_src * 4 * D + n_dst * 4 * R * D


class LoopRelGraphConv(torch.nn.Module):
    """nn.RelGraphConv's parameters with the aggregation as the reference layer issues it: one u_mul_e / mean g-SpMM and one matmul per
    relation, the products stacked and summed."""

    def __init__(self, in_feats, out_feats, num_relations, activation=None, dropout=0.):
        super(LoopRelGraphConv, self).__init__()
        self._rel_fcs = torch.nn.ParameterList([torch.nn.Parameter(torch.empty(in_feats, out_feats)) for _ in range(num_relations)])
        self._skip = torch.nn.Linear(in_feats, out_feats, bias=True)
        self._activation, self._dropout = activation, torch.nn.Dropout(dropout)

    def forward(self, g, x, edge_weights):
        outs = [torch.matmul(dgl.ops.gspmm(g, "mul", "mean", x, w), fc) for w, fc in zip(edge_weights, self._rel_fcs)]
        h = torch.stack(outs, 0).sum(0) + self._skip(x)
        if self._activation:
            h = self._activation(h)
        return self._dropout(h)


def main():
    p = argparse.ArgumentParser("multi-relation g-SpMM: per-relation loop vs one pass")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--widths", type=int, nargs="+", default=[1, 32, 64])
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--no-step", action="store_true", help="skip leg (d), the training steps")
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    data, g, node_feats, edge_weights, model, opt = full_graph.build_rgcn(dev, args.scale)
    n, nnz, R = g.number_of_nodes(), g.number_of_edges(), len(edge_weights)
    w = data.edge_feat
    print("proteins stand-in: N %d  E %d  R %d  (scale %g)" % (n, nnz, R, args.scale))
    rows = []
    for D in args.widths:
        gen = torch.Generator(device=dev).manual_seed(D)
        x = torch.rand(n, D, device=dev, generator=gen).requires_grad_(True)
        up = torch.rand(n, R, D, device=dev, generator=gen)

        def loop_fwd():
            return torch.stack([dgl.ops.gspmm(g, "mul", "mean", x, wr) for wr in edge_weights], 1)

        def fused_fwd():
            return ops.rel_gspmm(g, x, w, "mean")

        def fwd_bwd(fn):
            def run():
                x.grad = None
                fn().backward(up)
            return run

        assert ops.rel_gspmm_fused(g, x, w), "the one-pass kernels do not cover D = %d" % D
        with torch.no_grad():
            a, b = loop_fwd(), fused_fwd()
            err = float((a - b).abs().max() / a.abs().max())
        assert err < 1e-4, "loop and fused disagree: %g" % err
        res = {"D": D, "R": R, "nnz": nnz, "max_rel_diff": err}
        with torch.no_grad():
            res["loop_fwd"] = time_op(loop_fwd, args.reps)
            res["fused_fwd"] = time_op(fused_fwd, args.reps)
        res["loop_fwd_bwd"] = time_op(fwd_bwd(loop_fwd), args.reps)
        res["fused_fwd_bwd"] = time_op(fwd_bwd(fused_fwd), args.reps)
        gb = rel_bytes(n, n, nnz, R, D) / 1e9
        print("D %3d  forward      loop %9.3f ms%s\n                    fused %9.3f ms%s   ratio %.2fx   %.0f GB/s (algorithmic %.2f GB)" % (
            D, res["loop_fwd"][0] * 1e3, spread(*res["loop_fwd"]), res["fused_fwd"][0] * 1e3, spread(*res["fused_fwd"]),
            res["loop_fwd"][0] / res["fused_fwd"][0], gb / res["fused_fwd"][0], gb))
        print("       fwd + bwd    loop %9.3f ms%s\n                    fused %9.3f ms%s   ratio %.2fx   %.0f GB/s (both walks)" % (
            res["loop_fwd_bwd"][0] * 1e3, spread(*res["loop_fwd_bwd"]), res["fused_fwd_bwd"][0] * 1e3, spread(*res["fused_fwd_bwd"]),
            res["loop_fwd_bwd"][0] / res["fused_fwd_bwd"][0], 2 * gb / res["fused_fwd_bwd"][0]))
        rows.append({k: (list(v) if isinstance(v, tuple) else v) for k, v in res.items()})
        del x, up
    step = None
    if not args.no_step:
        torch.manual_seed(0)
        loop_model = full_graph.RGCN(3, 1, 32, data.num_tasks, R, layer=LoopRelGraphConv).to(dev)
        loop_model.load_state_dict(model.state_dict())
        loop_opt = torch.optim.Adam(loop_model.parameters(), lr=0.01)
        t_loop = time_op(lambda: full_graph.rgcn_train_step(loop_model, g, node_feats, edge_weights, data.y_true, data.train_idx, loop_opt),
                         args.reps)
        t_fused = time_op(lambda: full_graph.rgcn_train_step(model, g, node_feats, edge_weights, data.y_true, data.train_idx, opt), args.reps)
        print("RGCN step (3 layers, hidden 32)   loop %9.3f ms%s\n                                  fused %9.3f ms%s   ratio %.2fx" % (
            t_loop[0] * 1e3, spread(*t_loop), t_fused[0] * 1e3, spread(*t_fused), t_loop[0] / t_fused[0]))
        step = {"loop": list(t_loop), "fused": list(t_fused)}
    print(json.dumps({"rel_bench": rows, "rgcn_step": step, "N": n, "E": nnz, "R": R}))


if __name__ == "__main__":
    main()
