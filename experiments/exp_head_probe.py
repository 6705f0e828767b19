"""The reversed aggregation of the last SAGE layer (ops.SageMeanCatHeadFn) over d neigh / deg -- [N, 64], dense on the loss rows (8 % of
the nodes), zero elsewhere -- on the benchmark's graph: mgx_spmm_copy_u_slots_init of THIS build against the same entry of other builds
of the library loaded into the same process (argv: SCALE name=path/to/libmi355x_graph.so ...; the parent commit's build is the
yardstick), and against this build's dense call.  All builds get the same CSR, plan, operands and output buffer; the outputs are compared
bit for bit before anything is timed.  ROUNDS rounds of CALLS synchronised calls per variant, the variants interleaved inside a round,
after one warm-up round; per variant the median of the round medians (min .. max of them).  The call is the short-item launch (dense
rows, lane group per item), the long-item launch and the hub fix-up; the parts are told apart by kernel name in a kernel trace of the
benchmark (profiles/head_probe_trace.txt).  `MGX_EXP_ONCE=1`: one call of this build's entry and nothing else -- the child process of a
counter pass.  docs/LOG_head_probe.md has the figures."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dgl-0.5-benchmark_amd"))
import torch  # noqa: E402
import dgl  # noqa: E402
from mi355x_graph import _lib, ops, sparse  # noqa: E402
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
out_dense, out = torch.empty(n, 64, device=dev), torch.empty(n, 64, device=dev)

own = _lib.lib()


def load(path):
    handle = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


def slots_call(handle):
    def call():
        _lib._lib = handle
        try:
            return be.spmm_copy_u_slots_init(csr, "sum", dn, slots, d_self, pos, out)
        finally:
            _lib._lib = own
    return call


if os.environ.get("MGX_EXP_ONCE"):
    slots_call(own)()
    torch.cuda.synchronize()
    sys.exit(0)

variants = [("dense rows: spmm_copy_u_strided_init (this build)", lambda: be.spmm_copy_u_strided_init(csr, "sum", dn, d_self, pos, out_dense))]
for arg in sys.argv[2:]:
    name, path = arg.split("=", 1)
    variants.append(("spmm_copy_u_slots_init, build '%s'" % name, slots_call(load(path))))
variants.append(("spmm_copy_u_slots_init, this build", slots_call(own)))
assert variants[0][1]() is out_dense
for name, fn in variants[1:]:
    out.fill_(float("nan"))
    assert fn() is out
    assert torch.equal(out_dense.view(torch.int32), out.view(torch.int32)), "%s: not the dense call's bits" % name
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
if len(variants) >= 3:   # the first other build is the yardstick
    spread = res[1][2] - res[1][1]
    gain = res[1][0] - res[-1][0]
    print("yardstick spread %.4f ms; gain of this build %.4f ms = %.1f x the spread; ranges %s"
          % (spread, gain, gain / max(spread, 1e-9), "disjoint" if res[-1][2] < res[1][1] else "OVERLAP"))
