"""The last SAGE layer's dense work on the loss rows: what ran over all N rows against what runs over the R loss rows, call by
call, in one process on the benchmark's graph (N = 2,449,029, R = 8 % of the nodes from a mask).  Median and range of 12
synchronised calls after 3 warm-up calls.  docs/LOG_head_rows.md has the figures."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dgl-0.5-benchmark_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import dgl  # noqa: E402
from mi355x_graph import ops, sparse  # noqa: E402
from mi355x_graph.datasets import SHAPES, synthetic_edges  # noqa: E402

dev = torch.device("cuda:0")
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0


def timed(fn, reps=12):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


spec = SHAPES["products"]
n, m = int(spec["n"] * scale), int(spec["m"] * scale)
src, dst = synthetic_edges(n, m, min(spec["max_deg"], n - 1), spec["seed"], dev, symmetric=spec["symmetric"])
g = dgl.graph((src, dst), num_nodes=n).int().formats(["csr", "csc"]).to(dev)
del src, dst
gen = torch.Generator(device="cpu").manual_seed(spec["seed"] + 100)
torch.rand(n, spec["feat"], generator=gen)
torch.randint(0, spec["classes"], (n,), generator=gen)
rows = torch.nonzero(torch.rand(n, generator=gen) < 0.08).flatten().to(dev)
R = int(rows.shape[0])
print("N = %d, E = %d, R = %d" % (n, g.number_of_edges(), R))

be = sparse.backend_for(torch.zeros(1, device=dev))
dgen = torch.Generator(device=dev).manual_seed(0)
cat = torch.randn(n, 128, device=dev, generator=dgen)
w = torch.randn(47, 128, device=dev, generator=dgen) * 0.1   # [W_self | W_neigh]
bias = torch.randn(47, device=dev, generator=dgen)
dyr = torch.randn(R, 47, device=dev, generator=dgen)
csr, inv = g._index.csr(), g._index.csc().inv_degrees()
inv_r = inv.index_select(0, rows)
total = {"all rows": 0.0, "loss rows": 0.0, "(other)": 0.0}


def report(side, what, t):
    total[side] += t[0]
    print("%-10s %-86s %.4f ms  (%.4f .. %.4f)" % (side, what, t[0], t[1], t[2]))


# 1. forward projection (+ the selection of the loss rows)
report("all rows", "forward: F.linear [N,128] x [128,47] + index_select of the loss rows", timed(lambda: F.linear(cat, w, bias).index_select(0, rows)))
report("loss rows", "forward: rows_gemm(rows=) [R,128] x [128,47]", timed(lambda: be.rows_gemm(cat, w, b_transposed=True, bias=bias, rows=rows)))


# 2. the output gradient and its input gradient
def dgrad_all():
    dy = torch.zeros(n, 47, device=dev)
    dy.index_copy_(0, rows, dyr)
    return dy, be.rows_gemm(dy, w, row_scale=inv, scale_from=64, split_col=64)


def dgrad_rows():
    dn = torch.zeros(n, 64, device=dev)
    return be.rows_gemm(dyr, w, row_scale=inv_r, scale_from=64, split_col=64, scatter_rows=rows, out2=dn)


report("all rows", "dgrad: zero fill [N,47] + index_copy + rows_gemm [N,47] -> two [N,64]", timed(dgrad_all))
report("loss rows", "dgrad: zero fill [N,64] + rows_gemm(scatter_rows=) [R,47] -> [R,64], [N,64]", timed(dgrad_rows))

# 3. weight and bias gradient
dy_all, (dh_all, dn_all) = dgrad_all()
d_self, dn_rows = dgrad_rows()
report("all rows", "wgrad: xty_colsum [N,47]^T [N,128]", timed(lambda: be.xty(dy_all, cat, colsum=True)))
pos = ops._row_pos(rows, n)
report("loss rows", "wgrad: xty_pos [R,47] at its N places ^T [N,128], the all-rows summation order", timed(lambda: be.xty_pos(dyr, pos, cat, colsum=True)))
report("(other)", "wgrad: xty_colsum(rows=) [R,47]^T [R of N,128], its own summation order (not used by the layer)", timed(lambda: be.xty(dyr, cat, colsum=True, rows=rows)))
assert all(torch.equal(x_, y_) for x_, y_ in zip(be.xty_pos(dyr, pos, cat, colsum=True), be.xty(dy_all, cat, colsum=True)))
assert torch.equal(dn_all, dn_rows) and torch.equal(dh_all.index_select(0, rows), d_self)


# 4. the backward aggregation
def agg_rows():
    dh = torch.zeros(n, 64, device=dev).index_copy_(0, rows, d_self)
    return be.spmm_copy_u_strided(csr, "sum", dn_rows, dh, accumulate=True)


def agg_plain():
    dh = torch.empty(n, 64, device=dev)
    be.spmm_copy_u_strided(csr, "sum", dn_rows, dh)
    return dh.index_add_(0, rows, d_self)


report("all rows", "backward aggregation accumulating into d self [N,64]", timed(lambda: be.spmm_copy_u_strided(csr, "sum", dn_all, dh_all, accumulate=True)))
report("loss rows", "zero fill [N,64] + index_copy of d self + the same accumulating aggregation", timed(agg_rows))
report("(other)", "backward aggregation plain + index_add of d self on R rows: other bits (not used by the layer)", timed(agg_plain))
print("sum: all rows %.4f ms, loss rows %.4f ms, difference %.4f ms" % (total["all rows"], total["loss rows"], total["all rows"] - total["loss rows"]))
