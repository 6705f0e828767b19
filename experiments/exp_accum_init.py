"""The backward of the last SAGE layer on the loss rows (ops.SageMeanCatHeadFn), from the output gradient dyr [R, 47] to d h [N, 64]:
the sequence it ran -- two zero fills of [N, 64], the scatter GEMM, index_copy_ of d self, the accumulating aggregation -- against the
one it runs under config.SAGE_HEAD_INIT -- the scatter GEMM into a matrix kept zero elsewhere, the aggregation started from the
compact d self (mgx_spmm_copy_u_strided_init) -- and the aggregations alone, in one process on the benchmark's graph
(N = 2,449,029, R = 8 % of the nodes from a mask).  12 interleaved rounds after 3 warm-up rounds: one synchronised call of every
variant per round, so a drift of the clock meets all of them alike.  docs/LOG_accum_init.md has the figures."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dgl-0.5-benchmark_amd"))
import torch  # noqa: E402
import dgl  # noqa: E402
from mi355x_graph import ops, sparse  # noqa: E402
from mi355x_graph.datasets import SHAPES, synthetic_edges  # noqa: E402

dev = torch.device("cuda:0")
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
ROUNDS = 12

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
w = torch.randn(47, 128, device=dev, generator=dgen) * 0.1   # [W_self | W_neigh]
dyr = torch.randn(R, 47, device=dev, generator=dgen)
csr, inv = g._index.csr(), g._index.csc().inv_degrees()
inv_r = inv.index_select(0, rows)
pos = ops._row_pos(rows, n)
kept = torch.zeros(n, 64, device=dev)   # the matrix kept between steps: zero outside `rows`


def parent_sequence():
    dn = torch.zeros(n, 64, device=dev)
    d_self, dn = be.rows_gemm(dyr, w, row_scale=inv_r, scale_from=64, split_col=64, scatter_rows=rows, out2=dn)
    dh = torch.zeros_like(dn).index_copy_(0, rows, d_self)
    return be.spmm_copy_u_strided(csr, "sum", dn, dh, accumulate=True)


def new_sequence():
    d_self, dn = be.rows_gemm(dyr, w, row_scale=inv_r, scale_from=64, split_col=64, scatter_rows=rows, out2=kept)
    return be.spmm_copy_u_strided_init(csr, "sum", dn, d_self, pos, torch.empty_like(dn))


d_self0, dn0 = be.rows_gemm(dyr, w, row_scale=inv_r, scale_from=64, split_col=64, scatter_rows=rows, out2=torch.zeros(n, 64, device=dev))
dh_acc = torch.zeros(n, 64, device=dev).index_copy_(0, rows, d_self0)
dh_new = torch.empty(n, 64, device=dev)
variants = [
    ("parent: zero fill x 2 + scatter GEMM + index_copy_ + accumulating aggregation", parent_sequence),
    ("new:    scatter GEMM into the kept matrix + aggregation started from the compact d self", new_sequence),
    ("        accumulating aggregation alone (into a prepared d h: values grow, time does not)", lambda: be.spmm_copy_u_strided(csr, "sum", dn0, dh_acc, accumulate=True)),
    ("        aggregation started from the compact d self alone", lambda: be.spmm_copy_u_strided_init(csr, "sum", dn0, d_self0, pos, dh_new)),
    ("        plain aggregation alone (no initial value: other bits, not used)", lambda: be.spmm_copy_u_strided(csr, "sum", dn0, dh_new)),
    ("        zero fill of one [N, 64]", lambda: torch.zeros(n, 64, device=dev)),
]
assert torch.equal(parent_sequence().view(torch.int32), new_sequence().view(torch.int32)), "the two sequences differ"
times = [[] for _ in variants]
for rnd in range(3 + ROUNDS):
    for i, (_, fn) in enumerate(variants):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rnd >= 3:
            times[i].append(a.elapsed_time(b))
med = []
for (name, _), ts in zip(variants, times):
    s = sorted(ts)
    med.append(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))
    print("%-92s median %.4f ms  (min %.4f, max %.4f)" % (name, med[-1], s[0], s[-1]))
print("new sequence faster than the parent's in %d of %d rounds" % (sum(1 for p_, c_ in zip(times[0], times[1]) if c_ < p_), ROUNDS))
print("modelled gain per epoch (difference of the two sequences' medians): %.4f ms" % (med[0] - med[1]))
