"""Values and gradients of gspmm / gsddmm / edge_softmax over the whole matrix of ops, operand targets, broadcast shapes and
requires_grad patterns, against an fp64 restatement with fp64 autograd (ops.GSpMM.backward / ops.GSDDMM.backward: SURVEY Appendix A).

Reference: the gathered formulation in plain torch on the host, on the fp32 inputs cast to double -- gather every operand by its target,
right-align the feature dimensions, apply the op, index_add over dst (mean: / max(deg, 1)); gradients by autograd with one random fp64
upstream weight per case.  Nothing of it goes through mi355x_graph.

Bound, per element:  |got - ref| <= (T + 8) * 2^-23 * A
  A: the same expression with every term replaced by its absolute value (for a gradient: the sum of the absolute per-edge contributions)
  T: the largest number of terms summed into any element of that tensor: the maximum degree on the side summed over, times the number
     of broadcast positions that _reduce_grad folds, times the dot length (forward of `dot`)
which is the fp32 summation bound plus a constant for the roundings of the element-wise ops, the mean scale and the fp32 copy of the
upstream weight.  Where nothing contributes (A == 0: isolated nodes) the bound asks for exactly 0.  edge_softmax takes the same
bound with T = the longest normalised row and A from the softmax Jacobian with absolute terms, a (|w| + sum a |w|).

Every test loops its shapes and requires_grad patterns, collects every failing case and asserts once; its last output line
("broadcast-grad <graph/route>: N cases, max err/bound R") is what a run reports."""
import zlib

import numpy as np
import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import ops, sparse
from conftest import random_graph

DEV = "cuda:0"
EPS = 2.0 ** -23

# feature shapes (lhs, rhs) after the row dimension; () is a 1-D operand (result squeezed, except for dot)
PAIRS = [((5,), (5,)), ((2, 4), (2, 1)), ((2, 1), (2, 4)), ((4,), (2, 4)), ((2, 4), (4,)), ((1,), (6,)), ((6,), (1,)), ((3, 1), (1, 4)),
         ((), ()), ((2, 64), (2, 1))]
# dot: the broadcast is planned on shape[:-1], so the rank-mismatched pairs of PAIRS are head-wise there (a NULL table); the last two
# pairs need a real offset table over the output positions, the first on the lhs ([0, 1, 0, 1, 0, 1]), the second on the rhs
DOT_TABLE_PAIRS = [((2, 4), (3, 2, 4)), ((3, 1, 4), (1, 2, 4))]
DOT_PAIRS = [((5,), (5,)), ((4,), (2, 4)), ((2, 4), (4,)), ((), ()), ((2, 8), (8,))] + DOT_TABLE_PAIRS
TABLE_PAIRS = [((4,), (2, 4)), ((2, 4), (4,)), ((3, 1), (1, 4))]  # rank mismatch / a non-NULL offset table
PATTERNS = {"both": (True, True), "left": (True, False), "right": (False, True)}
SDDMM_OPS = ["add", "sub", "mul", "div", "dot", "copy_lhs", "copy_rhs"]
SPMM_OPS = ["add", "sub", "mul", "div", "copy_lhs", "copy_rhs"]
TARGET_PAIRS = [(a, b) for a in "uev" for b in "uev"]


# ----------------------------------------------------------------------------- graphs
class HostGraph(object):
    def __init__(self, name, src, dst, n_src, n_dst):
        self.name, self.np_src, self.np_dst, self.n_src, self.n_dst = name, src, dst, n_src, n_dst
        self.src, self.dst = torch.from_numpy(src).long(), torch.from_numpy(dst).long()
        self.E = int(src.shape[0])
        self.in_deg = torch.bincount(self.dst, minlength=n_dst)
        self.out_deg = torch.bincount(self.src, minlength=n_src)
        self.rows = {"u": n_src, "v": n_dst, "e": self.E}
        self.max_deg = {"u": int(self.out_deg.max()), "v": int(self.in_deg.max()), "e": 1}
        self.live = {"u": self.out_deg > 0, "v": self.in_deg > 0, "e": torch.ones(self.E, dtype=torch.bool)}

    def gather(self, x, target):
        return x[self.src] if target == "u" else (x[self.dst] if target == "v" else x)


def _small():
    """tests/test_gine.py::small_graph: 37 x 29, 300 edges from an unsorted COO, isolated destinations, duplicates, self pairs"""
    src, dst = random_graph(37, 29, 300, seed=3)
    src[:2], dst[:2] = (4, 9), (4, 9)
    return HostGraph("small", src, dst, 37, 29)


def _square():
    src, dst = random_graph(40, 40, 400, seed=5)
    src[:3], dst[:3] = (0, 7, 39), (0, 7, 39)  # self loops
    return HostGraph("square", src, dst, 40, 40)


def _hubby():
    """tests/test_gine.py::hubby_graph(200, 200, 8000, seed=17, hub_deg=3000): one hub destination (11), one hub source (7),
    destinations 0..4 without in-edges"""
    n, hub_deg = 200, 3000
    src, dst = random_graph(n, n, 8000, seed=17)
    rng = np.random.default_rng(17)
    keep = dst >= 5
    src, dst = src[keep], dst[keep]
    hs = rng.integers(0, n, hub_deg)
    src = np.concatenate([src, hs, np.full(hub_deg, 7)])
    dst = np.concatenate([dst, np.full(hub_deg, 11), rng.integers(5, n, hub_deg)])
    return HostGraph("hubby", src.astype(np.int64), dst.astype(np.int64), n, n)


_HOST = {}


def host_graph(name):
    if name not in _HOST:
        _HOST[name] = {"small": _small, "square": _square, "hubby": _hubby}[name]()
    return _HOST[name]


class View(object):
    """A graph as the operators get it: `g` on a device, and `eperm` when its edges are renumbered (GraphIndex.canonical():
    eperm[new edge id] = old edge id) -- edge operands go in, and edge results come back, in that order."""

    def __init__(self, host, g, dev, eperm=None):
        self.host, self.g, self.dev, self.eperm = host, g, dev, eperm

    def put(self, x, target):
        if target == "e" and self.eperm is not None:
            x = x[self.eperm]
        return x.to(self.dev, copy=True)  # always a new tensor: the reference's own stay as they are

    def expect(self, ref, target):
        return ref[self.eperm] if (target == "e" and self.eperm is not None) else ref


# variant -> (host graph, how it is built, MGX_TORCH_OPS or None = default route, full matrix?)
VARIANTS = {
    "small": ("small", "int32", None, True),
    "coo": ("small", "coo", None, True),
    "csr_csc": ("small", "csr_csc", None, True),
    "ctypes": ("small", "int32", "0", False),
    "torch_ops": ("small", "int32", "1", False),
    "int64": ("small", "int64", None, False),
    "square": ("square", "int32", None, False),
    "canonical": ("square", "canonical", None, False),
    "hubby": ("hubby", "int32", None, False),
}
CPU_VARIANTS = ["small", "int64", "square", "canonical", "hubby"]
GPU_VARIANTS = ["coo", "csr_csc", "ctypes", "torch_ops", "square", "canonical", "int64", "hubby"]
_VIEWS = {}


def _build(host, dev, idtype=torch.int32):
    s, d = torch.from_numpy(host.np_src), torch.from_numpy(host.np_dst)
    if host.name == "square":
        g = mg.graph((s, d), num_nodes=host.n_src)
        return (g.int() if idtype == torch.int32 else g.long()).to(dev)
    return mg.create_block((s, d), host.n_src, host.n_dst, idtype=idtype, device=dev)


def view_of(variant, dev):
    key = (variant, dev)
    if key not in _VIEWS:
        name, how, _, _ = VARIANTS[variant]
        host = host_graph(name)
        g = _build(host, dev, torch.int64 if how == "int64" else torch.int32)
        eperm = None
        if how == "coo":
            g = g.formats(["coo"])
        elif how == "csr_csc":
            g = g.formats(["csr", "csc"])
        elif how == "canonical":
            g, perm = g._index.canonical()
            assert perm is not None, "the square graph's edge list is already in in-CSR order: nothing is renumbered"
            eperm = perm.cpu().long()
        _VIEWS[key] = View(host, g, dev, eperm)
    return _VIEWS[key]


@pytest.fixture()
def cpu_on():
    was = mg.enable_cpu_backend(True)
    try:
        yield
    finally:
        mg.enable_cpu_backend(was)


def _route(monkeypatch, variant):
    env = VARIANTS[variant][2]
    if env is None:
        monkeypatch.delenv("MGX_TORCH_OPS", raising=False)
    else:
        monkeypatch.setenv("MGX_TORCH_OPS", env)


# ----------------------------------------------------------------------------- the fp64 restatement
def _feat(x):
    return x.unsqueeze(-1) if x.dim() == 1 else x


def _ralign(x, nd):
    """size-1 dimensions after dimension 0 until x has nd feature dimensions"""
    return x.reshape((x.shape[0],) + (1,) * (nd - (x.dim() - 1)) + tuple(x.shape[1:]))


def _expr(op, l, r):
    if op == "add":
        return l + r
    if op == "sub":
        return l - r
    if op == "mul":
        return l * r
    if op == "div":
        return l / r
    if op == "dot":
        return (l * r).sum(-1, keepdim=True)
    return l if op == "copy_lhs" else r


def _messages(host, op, lt, rt, l, r):
    le, re = host.gather(_feat(l), lt), host.gather(_feat(r), rt)
    nd = max(le.dim(), re.dim()) - 1
    return _expr(op, _ralign(le, nd), _ralign(re, nd))


def _arg_extreme(host, m, reduce):
    """edge id of the extreme message of every (destination, feature position); asserts, from the reference alone, that no live row
    has a tie"""
    arg = torch.zeros((host.n_dst,) + tuple(m.shape[1:]), dtype=torch.long)
    for v in range(host.n_dst):
        e = (host.dst == v).nonzero().flatten()
        if e.numel():
            mv = m[e]
            i = (mv.argmax(0) if reduce == "max" else mv.argmin(0)).unsqueeze(0)
            assert bool(((mv == mv.gather(0, i)).sum(0) == 1).all()), "tie in the reference's row %d" % v
            arg[v] = e[i[0]]
    return arg


def _evaluate(host, kind, op, aux, l, r, w, squeeze, arg=None):
    """(out, d l, d r) of sum(out * w) in fp64; kind "sddmm": aux = (lhs target, rhs target); kind "spmm": aux = reduce"""
    l, r = l.clone().requires_grad_(True), r.clone().requires_grad_(True)
    if kind == "sddmm":
        out = _messages(host, op, aux[0], aux[1], l, r)
    else:
        m = _messages(host, op, "u", "e", l, r)
        if aux in ("sum", "mean"):
            out = torch.zeros((host.n_dst,) + tuple(m.shape[1:]), dtype=m.dtype).index_add(0, host.dst, m)
            if aux == "mean":
                out = out / _ralign(host.in_deg.clamp(min=1).to(m.dtype).unsqueeze(-1), m.dim() - 1)
        else:
            out = m.gather(0, arg) * _ralign(host.live["v"].to(m.dtype).unsqueeze(-1), m.dim() - 1)
    if squeeze:
        out = out.squeeze(-1)
    if w is None:
        return out.detach(), None, None
    (out * w).sum().backward()
    return out.detach(), l.grad, r.grad


def _prod(shape):
    return int(np.prod(shape)) if len(shape) else 1


def _randn(shape, gen, dtype=torch.float32):
    """N(0, 1); the rare exact 0 of the generator is replaced, so that "A > 0 wherever an edge contributes" holds for every draw"""
    x = torch.randn(shape, generator=gen, dtype=dtype)
    return torch.where(x == 0, torch.full_like(x, 0.5), x)


class Ref(object):
    pass


_REFS = {}


def reference(host, kind, op, aux, lshape, rshape):
    """Inputs (fp32), upstream weight (fp64), fp64 values and gradients, their magnitudes A and term counts T.  Computed once per case
    and shared by every route, graph format and requires_grad pattern."""
    key = (host.name, kind, op, aux, lshape, rshape)
    if key in _REFS:
        return _REFS[key]
    lt, rt = aux if kind == "sddmm" else ("u", "e")
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    ref = Ref()
    ref.l = _randn((host.rows[lt],) + lshape, gen)
    ref.r = _randn((host.rows[rt],) + rshape, gen)
    if op == "div":
        ref.r = ref.r.abs() + 0.5
    l64, r64 = ref.l.double(), ref.r.double()
    used = [s for s, unused in ((lshape, "copy_rhs"), (rshape, "copy_lhs")) if op != unused]
    squeeze = all(s == () for s in used) and op != "dot"
    arg = None
    if kind == "spmm" and aux in ("max", "min"):
        arg = _arg_extreme(host, _messages(host, op, "u", "e", l64, r64), aux)
    out, _, _ = _evaluate(host, kind, op, aux, l64, r64, None, squeeze, arg)
    ref.w = _randn(out.shape, gen, torch.float64)
    ref.out, ref.gl, ref.gr = _evaluate(host, kind, op, aux, l64, r64, ref.w, squeeze, arg)
    mag_op = "add" if op == "sub" else op
    ref.A_out, A_gl, A_gr = _evaluate(host, kind, mag_op, aux, l64.abs(), r64.abs(), ref.w.abs(), squeeze, arg)
    ref.A_gl = None if A_gl is None else A_gl.abs()  # (div: every contribution to d r is negative; the sum of their sizes)
    ref.A_gr = None if A_gr is None else A_gr.abs()
    # term counts
    fl, fr = (lshape or (1,)), (rshape or (1,))
    full = fl if op == "copy_lhs" else (fr if op == "copy_rhs" else tuple(torch.broadcast_shapes(fl, fr)))
    summed = {"sum": host.max_deg["v"], "mean": host.max_deg["v"]}.get(aux, 1) if kind == "spmm" else 1
    ref.T_out = summed * (full[-1] if op == "dot" else 1)
    ref.T_gl = host.max_deg[lt] * (_prod(full) // _prod(fl))
    ref.T_gr = host.max_deg[rt] * (_prod(full) // _prod(fr))
    # a case whose reference is all zero would pass whatever the kernels do
    out_live = host.live["v"] if kind == "spmm" else host.live["e"]
    assert bool((ref.A_out[out_live] > 0).all()) and bool((ref.A_out[~out_live] == 0).all()), key
    for A, t in ((ref.A_gl, lt), (ref.A_gr, rt)):
        if A is not None and arg is not None:  # max / min: only the selected edges carry a gradient, one per live output element
            assert int((A > 0).sum()) >= int(host.live["v"].sum()) and bool((A[~host.live[t]] == 0).all()), key
        elif A is not None:
            assert bool((A[host.live[t]] > 0).all()) and bool((A[~host.live[t]] == 0).all()), key
    _REFS[key] = ref
    return ref


# ----------------------------------------------------------------------------- comparison
class Tally(object):
    def __init__(self, label):
        self.label, self.cases, self.ratio, self.fails = label, 0, 0.0, []

    def check(self, tag, got, ref, A, T):
        if got is None:
            self.fails.append("%s: None" % tag)
            return
        got = got.detach().cpu().double()
        if tuple(got.shape) != tuple(ref.shape):
            self.fails.append("%s: shape %s, expected %s" % (tag, tuple(got.shape), tuple(ref.shape)))
            return
        bound = (T + 8) * EPS * A
        err = (got - ref).abs()
        ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, 0.0, float("inf")).double())
        worst = float(ratio.max()) if ratio.numel() else 0.0
        worst = float("inf") if worst != worst else worst
        self.ratio = max(self.ratio, worst)
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = int(ratio.flatten().nan_to_num(nan=float("inf")).argmax())
            self.fails.append("%s: %d of %d elements over the bound (T = %d), worst err/bound %.3g: got %.9g, ref %.9g"
                              % (tag, int(bad.sum()), bad.numel(), T, worst, float(got.flatten()[i]), float(ref.flatten()[i])))

    def done(self):
        print("broadcast-grad %s: %d cases, max err/bound %.3f" % (self.label, self.cases, self.ratio))
        assert not self.fails, "%d failures\n%s" % (len(self.fails), "\n".join(self.fails))


def _run_case(tally, view, kind, op, aux, lshape, rshape, pattern):
    host = view.host
    lt, rt = aux if kind == "sddmm" else ("u", "e")
    ref = reference(host, kind, op, aux, lshape, rshape)
    tag = "%s %s %s %s x %s, grad %s" % (kind, op, aux if kind == "spmm" else lt + rt, lshape, rshape, pattern)
    tally.cases += 1
    req_l, req_r = PATTERNS[pattern]
    l = view.put(ref.l, lt).requires_grad_(req_l)
    r = view.put(ref.r, rt).requires_grad_(req_r)
    try:
        if kind == "sddmm":
            out = ops.gsddmm(view.g, op, l, r, lt, rt)
        else:
            out = ops.gspmm(view.g, op, aux, l, r)
        tally.check(tag + ": out", out, view.expect(ref.out, "e" if kind == "sddmm" else "v"), view.expect(ref.A_out, "e" if kind == "sddmm" else "v"),
                    ref.T_out)
        flows = (req_l and ref.gl is not None) or (req_r and ref.gr is not None)
        if out.requires_grad != flows:
            tally.fails.append("%s: out.requires_grad is %s" % (tag, out.requires_grad))
        if out.requires_grad:
            out.backward(view.put(ref.w.float(), "e" if kind == "sddmm" else "v"))
    except Exception as err:  # noqa: BLE001 -- reported with the case it belongs to
        tally.fails.append("%s: %s: %s" % (tag, type(err).__name__, str(err).split("\n")[0]))
        return not str(view.dev).startswith("cuda")  # after an error from the device nothing more is launched
    for name, x, req, g, A, T, t in (("d lhs", l, req_l, ref.gl, ref.A_gl, ref.T_gl, lt), ("d rhs", r, req_r, ref.gr, ref.A_gr, ref.T_gr, rt)):
        if req and g is not None:
            tally.check("%s: %s" % (tag, name), x.grad, view.expect(g, t), view.expect(A, t), T)
        elif x.grad is not None:
            tally.fails.append("%s: %s is set for an operand that %s" % (tag, name, "asked for none" if not req else "is not used"))
    return True


def _shape_pairs(op, full):
    pairs = DOT_PAIRS if op == "dot" else (PAIRS if full else TABLE_PAIRS)
    if op == "copy_lhs":  # one operand: each of its shapes once
        seen = sorted(set(p[0] for p in pairs), key=repr)
        return [(s, s) for s in seen]
    if op == "copy_rhs":
        seen = sorted(set(p[1] for p in pairs), key=repr)
        return [(s, s) for s in seen]
    return pairs


def _run_matrix(view, variant, kind, op, aux):
    """The full matrix (every shape pair, every requires_grad pattern) or the reduced one (the rank-mismatch / table pairs and the dot
    pairs; right only and both)."""
    full = VARIANTS[variant][3]
    tally = Tally("%s %s" % (variant, "cpu" if view.dev == "cpu" else "gpu"))
    for lshape, rshape in _shape_pairs(op, full):
        for pattern in (("both", "left", "right") if full else ("right", "both")):
            if not _run_case(tally, view, kind, op, aux, lshape, rshape, pattern):
                tally.done()
    tally.done()


def _softmax_reference(host, norm_by, shape):
    key = (host.name, "softmax", norm_by, shape)
    if key in _REFS:
        return _REFS[key]
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    seg = host.dst if norm_by == "dst" else host.src
    n = host.n_dst if norm_by == "dst" else host.n_src
    ref = Ref()
    ref.z = _randn((host.E,) + shape, gen)
    ref.w = _randn((host.E,) + shape, gen, torch.float64)
    z = ref.z.double().requires_grad_(True)
    top = torch.full((n,) + shape, -float("inf"), dtype=torch.float64).scatter_reduce(
        0, seg.view((-1,) + (1,) * len(shape)).expand_as(z), z.detach(), "amax", include_self=True)
    ex = torch.exp(z - top[seg])
    a = ex / torch.zeros((n,) + shape, dtype=torch.float64).index_add(0, seg, ex)[seg]
    (a * ref.w).sum().backward()
    ref.out, ref.gz = a.detach(), z.grad
    ref.A_out = ref.out  # every term of a softmax is positive
    aw = ref.out * ref.w.abs()
    ref.A_gz = ref.out * (ref.w.abs() + torch.zeros((n,) + shape, dtype=torch.float64).index_add(0, seg, aw)[seg])
    ref.T = int(torch.bincount(seg, minlength=n).max())
    assert bool((ref.A_out > 0).all()) and bool((ref.A_gz > 0).all())
    _REFS[key] = ref
    return ref


def _run_softmax(view, variant, norm_by):
    tally = Tally("%s %s" % (variant, "cpu" if view.dev == "cpu" else "gpu"))
    for shape in ((3,), (2, 1)):
        ref = _softmax_reference(view.host, norm_by, shape)
        for req in (True, False):
            tag = "edge_softmax %s %s, grad %s" % (norm_by, shape, req)
            tally.cases += 1
            z = view.put(ref.z, "e").requires_grad_(req)
            out = ops.edge_softmax(view.g, z, norm_by=norm_by)
            tally.check(tag + ": out", out, view.expect(ref.out, "e"), view.expect(ref.A_out, "e"), ref.T)
            if req:
                out.backward(view.put(ref.w.float(), "e"))
                tally.check(tag + ": d logits", z.grad, view.expect(ref.gz, "e"), view.expect(ref.A_gz, "e"), ref.T)
            elif out.requires_grad or z.grad is not None:
                tally.fails.append("%s: a gradient for logits that asked for none" % tag)
    tally.done()


def test_table_pairs_take_an_offset_table():
    """what the names promise: every TABLE_PAIRS / DOT_TABLE_PAIRS case hands the kernels a non-NULL table, on the side stated above"""
    for lshape, rshape in TABLE_PAIRS:
        _, lt, rt = sparse._bcast_plan(lshape, rshape)
        assert lt is not None or rt is not None, (lshape, rshape)
    sides = []
    for lshape, rshape in DOT_TABLE_PAIRS:
        out, lt, rt = sparse._bcast_plan(lshape[:-1], rshape[:-1])
        sides.append((lt is not None, rt is not None))
        for t in (lt, rt):
            assert t is None or (len(t) == _prod(out) and sorted(set(t.tolist())) != list(range(len(t)))), (lshape, rshape)
    assert sides == [(True, False), (False, True)]
    assert sparse._bcast_plan((2,), (3, 2))[1].tolist() == [0, 1, 0, 1, 0, 1]


# ----------------------------------------------------------------------------- CPU backend (runs anywhere)
@pytest.mark.parametrize("variant", CPU_VARIANTS)
@pytest.mark.parametrize("lt,rt", TARGET_PAIRS)
@pytest.mark.parametrize("op", SDDMM_OPS)
def test_gsddmm_cpu(cpu_on, monkeypatch, op, lt, rt, variant):
    _route(monkeypatch, variant)
    _run_matrix(view_of(variant, "cpu"), variant, "sddmm", op, (lt, rt))


@pytest.mark.parametrize("variant", CPU_VARIANTS)
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("op", SPMM_OPS)
def test_gspmm_cpu(cpu_on, monkeypatch, op, reduce, variant):
    _route(monkeypatch, variant)
    _run_matrix(view_of(variant, "cpu"), variant, "spmm", op, reduce)


def _run_max_min(view, variant, op, reduce):
    """the broadcast `gather` of the max / min backward branch (ties: tests/test_value_edges.py)"""
    tally = Tally("%s %s" % (variant, "cpu" if view.dev == "cpu" else "gpu"))
    for lshape, rshape in (((2, 1), (2, 4)), ((4,), (2, 4))):
        for pattern in ("both", "left", "right"):
            if not _run_case(tally, view, "spmm", op, reduce, lshape, rshape, pattern):
                tally.done()
    tally.done()


@pytest.mark.parametrize("variant", ["small", "int64", "canonical"])
@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("op", ["add", "mul"])
def test_gspmm_max_min_cpu(cpu_on, monkeypatch, op, reduce, variant):
    _route(monkeypatch, variant)
    _run_max_min(view_of(variant, "cpu"), variant, op, reduce)


@pytest.mark.parametrize("variant", ["small", "int64"])
@pytest.mark.parametrize("norm_by", ["dst", "src"])
def test_edge_softmax_cpu(cpu_on, monkeypatch, norm_by, variant):
    _route(monkeypatch, variant)
    _run_softmax(view_of(variant, "cpu"), variant, norm_by)


# ----------------------------------------------------------------------------- HIP
@pytest.mark.gpu
@pytest.mark.parametrize("variant", GPU_VARIANTS)
@pytest.mark.parametrize("lt,rt", TARGET_PAIRS)
@pytest.mark.parametrize("op", SDDMM_OPS)
def test_gsddmm_gpu(monkeypatch, op, lt, rt, variant):
    _route(monkeypatch, variant)
    _run_matrix(view_of(variant, DEV), variant, "sddmm", op, (lt, rt))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", GPU_VARIANTS)
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("op", SPMM_OPS)
def test_gspmm_gpu(monkeypatch, op, reduce, variant):
    _route(monkeypatch, variant)
    _run_matrix(view_of(variant, DEV), variant, "spmm", op, reduce)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["coo", "ctypes", "torch_ops", "int64", "canonical"])
@pytest.mark.parametrize("reduce", ["max", "min"])
@pytest.mark.parametrize("op", ["add", "mul"])
def test_gspmm_max_min_gpu(monkeypatch, op, reduce, variant):
    _route(monkeypatch, variant)
    _run_max_min(view_of(variant, DEV), variant, op, reduce)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["coo", "ctypes", "torch_ops", "int64"])
@pytest.mark.parametrize("norm_by", ["dst", "src"])
def test_edge_softmax_gpu(monkeypatch, norm_by, variant):
    _route(monkeypatch, variant)
    _run_softmax(view_of(variant, DEV), variant, norm_by)
