"""The reversed aggregation of the last SAGE layer (ops.SageMeanCatHeadFn) over d neigh / deg -- an [N, 64] matrix that is dense on the
loss rows (8 % of the nodes) and zero elsewhere -- on the benchmark's graph, one process:
  a) mgx_spmm_copy_u_strided_init on the dense rows (two lines per edge);
  b) the existing slot entry, mgx_spmm_copy_u_slots accumulating into a prepared matrix: a pessimistic stand-in (other bits, no initial
     value, every flagged row read where it is needed);
  c) mgx_rows_slots_pack_rows of the step's rows + mgx_spmm_copy_u_slots_init (what the layer runs under config.SAGE_HEAD_SLOTS);
  d) mgx_spmm_copy_u_slots_init alone.
ROUNDS rounds of CALLS synchronised calls per variant, the variants interleaved inside a round, after one warm-up round; per variant the
median of the round medians (min .. max of them).  argv[1]: scale of the graph (the sweep that sets the path's edge threshold).
docs/LOG_head_slots.md has the figures."""
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
ROUNDS, CALLS = 5, 10

spec = SHAPES["products"]
n, m = int(spec["n"] * scale), int(spec["m"] * scale)
src, dst = synthetic_edges(n, m, min(spec["max_deg"], n - 1), spec["seed"], dev, symmetric=spec["symmetric"])
g = dgl.graph((src, dst), num_nodes=n).int().formats(["csr", "csc"]).to(dev)
del src, dst
gen = torch.Generator(device="cpu").manual_seed(spec["seed"] + 100)
rows = torch.nonzero(torch.rand(n, generator=gen) < 0.08).flatten().to(dev)
R = int(rows.shape[0])
print("scale %g: N = %d, E = %d, R = %d" % (scale, n, g.number_of_edges(), R))

be = sparse.backend_for(torch.zeros(1, device=dev))
dgen = torch.Generator(device=dev).manual_seed(0)
csr = g._index.csr()
pos = ops._row_pos(rows, n)
d_self = torch.randn(R, 64, device=dev, generator=dgen)
dn = torch.zeros(n, 64, device=dev)
dn[rows] = torch.randn(R, 64, device=dev, generator=dgen)
slots, overflow = be.rows_slots_pack(dn)
print("flagged slots: %d of %d rows" % (int(overflow), n))
out_a, out_b, out_c = torch.empty(n, 64, device=dev), torch.zeros(n, 64, device=dev), torch.empty(n, 64, device=dev)


def new_call():
    be.rows_slots_pack_rows(dn, rows, slots)
    return be.spmm_copy_u_slots_init(csr, "sum", dn, slots, d_self, pos, out_c)


variants = [
    ("a) dense rows: spmm_copy_u_strided_init", lambda: be.spmm_copy_u_strided_init(csr, "sum", dn, d_self, pos, out_a)),
    ("b) stand-in: spmm_copy_u_strided(accumulate, slots)", lambda: be.spmm_copy_u_strided(csr, "sum", dn, out_b, accumulate=True, slots=slots)),
    ("c) pack of the step's rows + spmm_copy_u_slots_init", new_call),
    ("d) spmm_copy_u_slots_init alone", lambda: be.spmm_copy_u_slots_init(csr, "sum", dn, slots, d_self, pos, out_c)),
]
assert variants[0][1]() is out_a and new_call() is out_c
assert torch.equal(out_a.view(torch.int32), out_c.view(torch.int32)), "the slot call's bits are not the dense call's"
meds = [[] for _ in variants]
for rnd in range(1 + ROUNDS):
    ts = [[] for _ in variants]
    for _ in range(CALLS):
        for i, (_, fn) in enumerate(variants):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b))
    if rnd >= 1:
        for i, t in enumerate(ts):
            s = sorted(t)
            meds[i].append(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))
res = []
for (name, _), ms in zip(variants, meds):
    s = sorted(ms)
    res.append((s[len(s) // 2], s[0], s[-1]))
    print("%-56s median of round medians %.4f ms  (%.4f .. %.4f)" % (name, s[len(s) // 2], s[0], s[-1]))
spread = res[0][2] - res[0][1]
print("spread of a): %.4f ms; gain of c) over a): %.4f ms = %.1f x the spread (the path is the default from 3 x on)"
      % (spread, res[0][0] - res[2][0], (res[0][0] - res[2][0]) / max(spread, 1e-9)))
