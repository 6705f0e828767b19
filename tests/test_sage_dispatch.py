"""Which autograd node each SAGE entry point of mi355x_graph.ops applies -- or that it declines (None) -- over a table of operands: one
property changed at a time from a base case every fused form takes (a square int32 ring graph of 65536 nodes, [N, 64] float32 features
that take no gradient, a 64-wide output with a bias, a matching CatBuffer, an aligned destination).  The table pins the dispatch: a
change to an eligibility clause shows up here as a changed name, not as a slower or differently rounded epoch."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dgl-0.5-benchmark_amd")
sys.path.insert(0, PKG)
import mi355x_graph as mg  # noqa: E402
from mi355x_graph import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ENTRY_POINTS = ("sage_mean_layer", "sage_mean_layer_act", "sage_project_first", "sage_static_input_project", "sage_mean_layer_rows")

BASE = dict(n=65536, idtype=torch.int32, block=False, dtype=torch.float32, three_d=False, grad_enabled=True, h_grad=False,
            bias="yes", d_in=64, d_out=64, cat="match", out="aligned", env={})

# 65535: one row short of ops._ROWS_GEMM_MIN; 260: wider than HipBackend.COLUMN_SUM_MAX (256); 602 -> 16: the reddit layer that
# sage_project_first's rule takes
CASES = {
    "base": {},
    "n65535": dict(n=65535),
    "n65535_h_grad": dict(n=65535, h_grad=True),
    "int64": dict(idtype=torch.int64),
    "block": dict(block=True),
    "float64": dict(dtype=torch.float64),
    "three_d": dict(three_d=True),
    "no_grad": dict(grad_enabled=False),
    "h_grad": dict(h_grad=True),
    "bias_none": dict(bias="none"),
    "bias_wide": dict(d_out=260),
    "bias_none_wide": dict(d_out=260, bias="none"),
    "in64_out16": dict(d_out=16),
    "in64_out16_h_grad": dict(d_out=16, h_grad=True),
    "in64_out47": dict(d_out=47),
    "in602_out16": dict(d_in=602, d_out=16),
    "in602_out16_h_grad": dict(d_in=602, d_out=16, h_grad=True),
    "in602_out47": dict(d_in=602, d_out=47),
    "in602_out64": dict(d_in=602, d_out=64),
    "in602_out64_h_grad": dict(d_in=602, d_out=64, h_grad=True),
    "cat_none": dict(cat="none"),
    "cat_wrong_k": dict(cat="wrong"),
    "out_none": dict(out="none"),
    "out_offset": dict(out="offset"),
    "sparse_last": dict(env={"MGX_SAGE_SPARSE_LAST": "1"}),
    "sparse_last_block": dict(block=True, env={"MGX_SAGE_SPARSE_LAST": "1"}),
    "head_rows_off": dict(env={"MGX_SAGE_HEAD_ROWS": "0"}),
    "l1_project_first": dict(env={"MGX_SAGE_L1_PROJECT_FIRST": "1"}),
    "l1_project_first_out16": dict(d_out=16, env={"MGX_SAGE_L1_PROJECT_FIRST": "1"}),
    "l1_project_first_out16_h_grad": dict(d_out=16, h_grad=True, env={"MGX_SAGE_L1_PROJECT_FIRST": "1"}),
    "l1_project_first_out16_block": dict(d_out=16, block=True, env={"MGX_SAGE_L1_PROJECT_FIRST": "1"}),
}

# Recorded by running _dispatch() over CASES at the commit before the eligibility clause was shared, and read against the
# predicates there; in ENTRY_POINTS' order.  (L = SageMeanLayerFn, C = SageMeanCatFn, P = SageMeanProjectFirstFn,
# S = SageMeanStaticInputProjectFn, H = SageMeanCatHeadFn, R = SageMeanCatRowsFn; the names asserted carry autograd's "Backward".)
EXPECTED = {
    'base': ('C', 'C', None, None, 'H'),
    'n65535': ('C', None, None, None, None),
    'n65535_h_grad': ('C', None, None, None, None),
    'int64': (None, None, None, None, None),
    'block': (None, None, None, None, None),
    'float64': (None, None, None, None, None),
    'three_d': (None, None, None, None, None),
    'no_grad': (None, None, None, None, None),
    'h_grad': ('C', 'C', None, None, 'H'),
    'bias_none': ('C', 'C', None, None, 'H'),
    'bias_wide': (None, None, None, None, None),
    'bias_none_wide': ('C', None, None, None, None),
    'in64_out16': ('C', None, 'P', None, 'H'),
    'in64_out16_h_grad': ('C', None, 'P', None, 'H'),
    'in64_out47': ('C', None, None, None, 'H'),
    'in602_out16': ('L', None, 'P', None, None),
    'in602_out16_h_grad': ('L', None, 'P', None, None),
    'in602_out47': ('L', None, None, None, None),
    'in602_out64': ('L', None, 'P', None, None),
    'in602_out64_h_grad': ('L', None, 'P', None, None),
    'cat_none': ('L', None, None, None, None),
    'cat_wrong_k': ('L', None, None, None, None),
    'out_none': ('C', 'C', None, None, 'H'),
    'out_offset': ('C', None, None, None, 'H'),
    'sparse_last': ('C', 'C', None, None, 'R'),
    'sparse_last_block': (None, None, None, None, 'R'),
    'head_rows_off': ('C', 'C', None, None, None),
    'l1_project_first': ('C', 'C', None, None, 'H'),
    'l1_project_first_out16': ('C', None, 'P', 'S', 'H'),
    'l1_project_first_out16_h_grad': ('C', None, 'P', None, 'H'),
    'l1_project_first_out16_block': (None, None, None, None, None),
}

_NAMES = {"L": "SageMeanLayerFnBackward", "C": "SageMeanCatFnBackward", "P": "SageMeanProjectFirstFnBackward",
          "S": "SageMeanStaticInputProjectFnBackward", "H": "SageMeanCatHeadFnBackward", "R": "SageMeanCatRowsFnBackward", None: None}


@functools.lru_cache(maxsize=None)
def _ring(n, idtype, block):
    """node v has the in-edges v - 2, v - 1, v + 1, v + 2 (mod n): 4-regular, square"""
    v = torch.arange(n, dtype=torch.int64, device=DEV)
    src = torch.cat([(v + d) % n for d in (-2, -1, 1, 2)])
    dst = v.repeat(4)
    if block:
        return mg.create_block((src, dst), n, n, idtype=idtype, device=DEV)
    g = mg.graph((src, dst), num_nodes=n, device=DEV)
    return g.int() if idtype == torch.int32 else g.long()


def _dispatch(case):
    """The name of y.grad_fn (the tag of ops._structural_zeros is an attribute of y itself) or None, per entry point."""
    c = dict(BASE, **case)
    n, d_in, d_out = c["n"], c["d_in"], c["d_out"]
    g = _ring(n, c["idtype"], c["block"])
    h = torch.rand(n, d_in, device=DEV).to(c["dtype"])
    if c["three_d"]:
        h = h.view(n, 1, d_in)
    h.requires_grad_(c["h_grad"])
    w_self = torch.rand(d_out, d_in, device=DEV).requires_grad_(True)
    w_neigh = torch.rand(d_out, d_in, device=DEV).requires_grad_(True)
    bias = None if c["bias"] == "none" else torch.rand(d_out, device=DEV).requires_grad_(True)
    cat = None if c["cat"] == "none" else ops.CatBuffer(n, 32 if c["cat"] == "wrong" else d_in, DEV)
    flat = torch.empty(n * d_out + 4, device=DEV)
    out = {"none": None, "aligned": flat[:n * d_out].view(n, d_out), "offset": flat[1:1 + n * d_out].view(n, d_out)}[c["out"]]
    assert out is None or out.data_ptr() % 16 == (4 if c["out"] == "offset" else 0)
    rows = torch.arange(0, n, 7, dtype=torch.int64, device=DEV)
    calls = {
        "sage_mean_layer": lambda: ops.sage_mean_layer(g, h, w_self, w_neigh, bias, cat),
        "sage_mean_layer_act": lambda: ops.sage_mean_layer_act(g, h, w_self, w_neigh, bias, cat, 0.5, out),
        "sage_project_first": lambda: ops.sage_project_first(g, h, w_self, w_neigh, bias),
        "sage_static_input_project": lambda: ops.sage_static_input_project(g, h, w_self, w_neigh, bias, cat),
        "sage_mean_layer_rows": lambda: ops.sage_mean_layer_rows(g, h, w_self, w_neigh, bias, cat, rows),
    }
    saved_env = {k: os.environ.get(k) for k in c["env"]}
    stream_position = ops.ReluDropout._calls
    os.environ.update(c["env"])
    try:
        with torch.set_grad_enabled(c["grad_enabled"]):
            got = []
            for name in ENTRY_POINTS:
                y = calls[name]()
                got.append(None if y is None else type(y.grad_fn).__name__)
    finally:
        ops.ReluDropout._calls = stream_position
        for k, v in saved_env.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    torch.cuda.synchronize()
    return tuple(got)


def test_the_table_covers_every_case():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_entry_points_apply_the_recorded_node(case):
    want = tuple(_NAMES[k] for k in EXPECTED[case])
    got = _dispatch(CASES[case])
    assert got == want, dict(zip(ENTRY_POINTS, zip(got, want)))
