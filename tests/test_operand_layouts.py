"""Layout matrix: every operator with ONE float operand at a time -- and the upstream gradient alone -- handed over as something other
than a fresh dense tensor (tests/layouts.py: offset4, colblock, colblock_off, alt_rows, transposed, expanded), the other operands dense.

For every cell of the matrix:
  (a) no exception: an operand torch accepts is an operand the operator accepts;
  (b) the outputs and every input gradient are those of the all-dense call:
        exact operators (sums, max / min, copies: `exact=True` below) are fed small signed integers (dyadic fractions where a mean is
        taken over a power-of-two row); every sum is then exact in fp32 in ANY order, so another kernel for another alignment must still
        give the same bits: torch.equal.  The precondition -- the number of terms of the longest sum times the product of the operands'
        largest magnitudes stays below 2^24 (exact_ladder.LIMIT) -- is asserted from the inputs alone;
        relu_dropout: torch.manual_seed and the stream position are reset before each call, the mask is a function of the position in
        the stream, so the dense and the layout call agree bit for bit;
        softmax / statistics operators (`exact=False`): the layout call against the fp64 restatement their own test file holds, at that
        file's own bound (imported, not repeated); edge_softmax, gat_attention, gat_fused and BatchNorm1d have no importable
        restatement: fp64 torch autograd of the definition at the bound of their test in tests/test_gpu_parity.py / test_gat_fused.py;
  (c) every operand's backing buffer -- the operand and the NaN guard elements around it -- holds the bits it held before the call;
  (d) every gradient has its operand's shape.

The matrix is data: CASES (operator, shapes, float slots) and EXCLUDED ((case, slot, layout) -> reason); TABLE is their difference and
test_every_slot_meets_every_layout_or_is_excluded holds them to each other.  Graph operators run on int32 and int64 graphs, the segment
operators once more with `seglen` as every other element of a longer tensor.  The same table runs on the OpenMP CPU backend (no marker;
the layout handling of ops.py is shared) and on the device (-m gpu); operators without a CPU form (relu_dropout, gat_fused,
sage_mean_layer) are device-only.  The tall-input kernels (mgx_xty behind linear / linear_sum, the column kernels behind bias_add and
BatchNorm1d: 65536 rows and up) get the colblock and offset4 columns of the matrix once more at n = 65537."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mi355x_graph as mg
import mi355x_graph.nn  # noqa: F401
from mi355x_graph import config, ops, sparse

import exact_ladder as xl
import layouts
import test_dot_attention as t_dot
import test_multi_aggregate as t_multi
import test_readout as t_readout

DEV = "cuda:0"
HUB = int(config.HUB_SPLIT)
SEG_LENS = (3, 0, 4, 1)
SEG_ROWS = sum(SEG_LENS)
TALL_N, TALL_K, TALL_M = 65537, 12, 8
# Where an upstream gradient with equal rows (`expanded`: what `.sum().backward()` delivers) makes a gradient CANCEL -- softmax weights
# sum to 1, so a (d a - sum a d a) is zero; a normalised column sums to zero, so d weight and d x of BatchNorm1d are zero -- the reference
# gradient is 1e-16 of rounding in fp64 and a bound "1e-4 of the reference gradient's largest element" has no scale.  Those cells
# (`cancels`) keep the bound and take the scale from the same case's gradient under its ordinary upstream gradient, whose first row the
# expanded one repeats: the terms that cancel are of that size.
assert TALL_N > max(ops._ROWS_GEMM_MIN, sparse.HipBackend.XTY_MIN_ROWS)


# ----------------------------------------------------------------------------- graphs
def _graph(lens, n_src, seed, hub_source_edges=50):
    """(src, dst, n_src, n_dst): destination v has lens[v] in-edges in a shuffled edge order (edge ids are not CSR positions), sources
    random with duplicates, source 3 gathered by `hub_source_edges` edges, the last two sources by nobody."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    dst = np.repeat(np.arange(lens.shape[0], dtype=np.int64), lens)
    src = rng.integers(0, n_src - 2, dst.shape[0]).astype(np.int64)
    src[rng.choice(dst.shape[0], hub_source_edges, replace=False)] = 3
    perm = rng.permutation(dst.shape[0])
    return src[perm], dst[perm], n_src, int(lens.shape[0])


# bipartite, 40 destinations and 60 sources: an empty row, short rows, rows around and above the hub split (their fix-up writes run)
BLOCK = _graph([0, 1, 2, 3, 5, 17, 64, 65, HUB - 1, HUB, HUB + 1, 2 * HUB + 1] + [1, 2, 3, 4] * 7, 60, seed=7)
# square, 48 nodes, every in-degree a power of two: a mean of integers is a dyadic fraction, so sage_mean_layer stays exact
SQUARE = _graph([0, 1, 2, 4, 8, 16, 64, HUB, 2 * HUB] + [1, 2, 4] * 13, 48, seed=8)
assert BLOCK[3] == 40 and SQUARE[3] == SQUARE[2] == 48


@functools.lru_cache(maxsize=None)
def graph_on(which, idtype, dev):
    src, dst, n_src, n_dst = BLOCK if which == "block" else SQUARE
    if n_src == n_dst:
        g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n_src)
        return (g.int() if idtype == torch.int32 else g.long()).to(dev)
    return mg.create_block((torch.from_numpy(src), torch.from_numpy(dst)), n_src, n_dst, idtype=idtype, device=dev)


# ----------------------------------------------------------------------------- the cases
def ints(seed, *shape, bound=3):
    return torch.from_numpy(xl.ints(np.random.default_rng(seed), shape, bound))


def normal(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def case(name, slots, call, ups, exact=True, nograd=(), weights=(), ref=None, graph=None, terms=1, backends=("cpu", "gpu"),
         idtypes=None, seeded=False, cancels=False):
    """slots: {name: dense fp32 value} in call order; call(g, t) -> the outputs, the first len(ups) of them differentiable; ups: their
    upstream gradients; nograd: slots that take no gradient; weights: the per-edge scale / weight slots whose rows may be equal
    (`expanded`); ref(values, ups, g) -> check(outs, grads, on_gpu, scales) for the exact=False cases; terms: the longest sum;
    cancels: an upstream gradient with equal rows makes a gradient of this case cancel to zero (see above)."""
    if idtypes is None:
        idtypes = (torch.int32, torch.int64) if graph else (None,)
    return types.SimpleNamespace(name=name, slots=slots, call=call, ups=list(ups), exact=exact, nograd=tuple(nograd), weights=tuple(weights),
                                 ref=ref, graph=graph, terms=terms, backends=backends, idtypes=idtypes, seeded=seeded, cancels=cancels)


def _softmax_by(z, idx, n):
    """fp64 softmax of z [E, ...] over the entries that share idx (the maximum is a constant shift: no gradient through it)"""
    with torch.no_grad():
        m = torch.full((n,) + tuple(z.shape[1:]), -float("inf"), dtype=z.dtype).index_reduce_(0, idx, z, "amax", include_self=True)
    e = torch.exp(z - m[idx])
    s = torch.zeros((n,) + tuple(z.shape[1:]), dtype=z.dtype).index_add(0, idx, e)
    return e / s[idx]


def _autograd_ref(fn, values, ups, scale_of=None):
    """(outs, {slot: grad}, row scales | None) of fn(**fp64 leaves) by plain torch autograd"""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in values.items()}
    outs = fn(**leaves)
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    grads = torch.autograd.grad(outs, list(leaves.values()), [u.double() for u in ups], allow_unused=True)
    scales = None if scale_of is None else scale_of(**{k: v.detach() for k, v in leaves.items()})
    return [o.detach() for o in outs], dict(zip(leaves, grads)), scales


def _close(got, want):
    """the bound the restating test files hold their CPU compositions to"""
    return torch.allclose(got.detach().cpu().double(), want, rtol=1e-5, atol=1e-6)


def _rel(a, b):
    """tests/test_gpu_parity.rel"""
    return float(((a.detach().cpu().double() - b).abs() / (b.abs() + 1e-5)).max()) if b.numel() else 0.0


def _maxerr(a, b):
    return float((a.detach().cpu().double() - b).abs().max()) if b.numel() else 0.0


def build_cases():
    c = []
    src, dst, n_src, n_dst = BLOCK
    E = int(src.shape[0])
    tsrc, tdst = torch.from_numpy(src), torch.from_numpy(dst)
    deg_in, deg_out = int(np.bincount(dst).max()), int(np.bincount(src).max())
    longest = max(deg_in, deg_out)

    # ---- gspmm
    for D in (4, 8, 64, 7):
        c.append(case("gspmm copy_u sum D=%d" % D, {"x": ints(10 + D, n_src, D)}, lambda g, t: [ops.gspmm(g, "copy_lhs", "sum", t["x"], None)],
                      [ints(20 + D, n_dst, D)], graph="block", terms=longest))
    for D in (8, 7):
        c.append(case("gspmm copy_u mean D=%d" % D, {"x": ints(30 + D, n_src, D)}, lambda g, t: [ops.gspmm(g, "copy_lhs", "mean", t["x"], None)],
                      [ints(40 + D, n_dst, D)], graph="block", terms=longest))
        c.append(case("gspmm copy_u max D=%d" % D, {"x": ints(50 + D, n_src, D)}, lambda g, t: [ops.gspmm(g, "copy_lhs", "max", t["x"], None)],
                      [ints(60 + D, n_dst, D)], graph="block", terms=longest))
        c.append(case("gspmm u_add_e sum D=%d" % D, {"x": ints(70 + D, n_src, D), "e": ints(80 + D, E, D)},
                      lambda g, t: [ops.gspmm(g, "add", "sum", t["x"], t["e"])], [ints(90 + D, n_dst, D)], graph="block", terms=2 * longest))
        c.append(case("gspmm copy_e sum D=%d" % D, {"e": ints(100 + D, E, D)}, lambda g, t: [ops.gspmm(g, "copy_rhs", "sum", None, t["e"])],
                      [ints(110 + D, n_dst, D)], graph="block", terms=longest))
    for H, Fd in ((1, 4), (2, 4)):
        c.append(case("gspmm u_mul_e sum [E,H,1] H=%d F=%d" % (H, Fd), {"x": ints(120 + H, n_src, H, Fd), "w": ints(130 + H, E, H, 1)},
                      lambda g, t: [ops.gspmm(g, "mul", "sum", t["x"], t["w"])], [ints(140 + H, n_dst, H, Fd)], weights=("w",), graph="block",
                      terms=longest * Fd))
    c.append(case("gspmm u_mul_e sum [E,H,F] H=2 F=4", {"x": ints(150, n_src, 2, 4), "w": ints(151, E, 2, 4)},
                  lambda g, t: [ops.gspmm(g, "mul", "sum", t["x"], t["w"])], [ints(152, n_dst, 2, 4)], weights=("w",), graph="block", terms=longest))

    # ---- gsddmm
    for D in (8, 7):
        c.append(case("gsddmm u_add_v D=%d" % D, {"u": ints(160 + D, n_src, D), "v": ints(170 + D, n_dst, D)},
                      lambda g, t: [ops.gsddmm(g, "add", t["u"], t["v"], "u", "v")], [ints(180 + D, E, D)], graph="block", terms=longest))
    c.append(case("gsddmm u_mul_e D=8", {"u": ints(190, n_src, 8), "e": ints(191, E, 8)},
                  lambda g, t: [ops.gsddmm(g, "mul", t["u"], t["e"], "u", "e")], [ints(192, E, 8)], graph="block", terms=longest))
    for H, Fd in ((2, 4), (1, 7)):
        c.append(case("gsddmm u_dot_v H=%d F=%d" % (H, Fd), {"u": ints(200 + Fd, n_src, H, Fd), "v": ints(210 + Fd, n_dst, H, Fd)},
                      lambda g, t: [ops.gsddmm(g, "dot", t["u"], t["v"], "u", "v")], [ints(220 + Fd, E, H, 1)], graph="block", terms=longest * Fd))

    # ---- softmax over the in-edges (no importable restatement: fp64 autograd of the definition, the bounds of tests/test_gpu_parity.py)
    def edge_softmax_ref(values, ups, g):
        outs, grads, _ = _autograd_ref(lambda z: _softmax_by(z, tdst, n_dst), values, ups)

        def check(got, got_grads, on_gpu, scales=None):
            assert _rel(got[0], outs[0]) < 1e-4                                    # test_edge_softmax_fwd_bwd
            assert _maxerr(got_grads["z"], grads["z"]) < 1e-5
        return check
    c.append(case("edge_softmax H=2", {"z": normal(230, E, 2, scale=4.0)}, lambda g, t: [ops.edge_softmax(g, t["z"])], [normal(231, E, 2)],
                  exact=False, ref=edge_softmax_ref, graph="block"))   # (an absolute gradient bound: no scale to lose)

    def gat_attention_ref(values, ups, g):
        def fn(el, er):
            return _softmax_by(F.leaky_relu(el[tsrc] + er[tdst], 0.2), tdst, n_dst)
        outs, grads, _ = _autograd_ref(fn, values, ups)
        top = {k: float(v.abs().max()) for k, v in grads.items()}

        def check(got, got_grads, on_gpu, scales=None):
            assert _rel(got[0], outs[0]) < 1e-4                                    # test_fused_gat_attention_matches_composition
            for k in ("el", "er"):
                assert _maxerr(got_grads[k], grads[k]) < 1e-4 * max((scales or top)[k], 1e-12), k
        check.top = top
        return check
    c.append(case("gat_attention H=2", {"el": normal(240, n_src, 2, 1, scale=2.0), "er": normal(241, n_dst, 2, 1, scale=2.0)},
                  lambda g, t: [ops.gat_attention(g, t["el"], t["er"], 0.2)], [normal(242, E, 2, 1)], exact=False, ref=gat_attention_ref, graph="block", cancels=True))

    def gat_fused_ref(values, ups, g):
        def fn(feat, el, er):
            a = _softmax_by(F.leaky_relu(el[tsrc] + er[tdst], 0.2), tdst, n_dst)
            return torch.zeros((n_dst,) + tuple(feat.shape[1:]), dtype=feat.dtype).index_add(0, tdst, a * feat[tsrc])

        def scale_of(feat, el, er):
            return [fn(feat.abs(), el, er)]
        outs, grads, row_scale = _autograd_ref(fn, values, ups, scale_of)

        def check(got, got_grads, on_gpu, scales=None):
            err = (got[0].detach().cpu().double() - outs[0]).abs()                 # tests/test_gat_fused.py: 1e-4 of sum_e a |feat|
            assert not (err > 1e-4 * row_scale[0] + 1e-30).any(), float((err / (row_scale[0] + 1e-30)).max())
            for k in ("feat", "el", "er"):
                assert _maxerr(got_grads[k], grads[k]) < 1e-4 * max(float(grads[k].abs().max()), 1e-6), k
        return check
    for H, Fd in ((1, 4), (2, 4)):
        c.append(case("gat_fused H=%d F=%d" % (H, Fd),
                      {"feat": normal(250 + H, n_src, H, Fd), "el": normal(252 + H, n_src, H, 1, scale=2.0), "er": normal(254 + H, n_dst, H, 1, scale=2.0)},
                      lambda g, t: [ops.gat_fused(g, t["feat"], t["el"], t["er"], 0.2, 0.0, True)], [normal(256 + H, n_dst, H, Fd)],
                      exact=False, ref=gat_fused_ref, graph="block", backends=("gpu",),
                      idtypes=(torch.int32,)))   # mgx_gat_fused_* take 32-bit indices only (HipBackend.gat_fused_supported): no int64 form to run

    # ---- dot_attention: the restatement and the two bounds of tests/test_dot_attention.py
    def dot_ref(shared):
        def ref(values, ups, g):
            q, k = values["q"], values["kv" if shared else "k"]
            r = t_dot.Restated(src, dst, n_src, n_dst, q, k, k if shared else values["v"], 4 ** -0.5, ups[0])
            want = types.SimpleNamespace(out=r.out, row_scale=r.row_scale, dq=r.dq, dk=r.dk, dv=r.dv, dkv=r.dk + r.dv)
            names = ("q", "kv") if shared else ("q", "k", "v")

            def check(got, got_grads, on_gpu, scales=None):
                if on_gpu:
                    t_dot.check_forward(got[0], want)
                    t_dot.check_grads([got_grads[n] for n in names], want, ["d" + n for n in names])
                else:
                    assert _close(got[0], want.out)
                    for n in names:
                        assert _close(got_grads[n], getattr(want, "d" + n)), n
            return check
        return ref
    c.append(case("dot_attention H=2 F=4", {"q": normal(260, n_dst, 2, 4), "k": normal(261, n_src, 2, 4), "v": normal(262, n_src, 2, 4)},
                  lambda g, t: [ops.dot_attention(g, t["q"], t["k"], t["v"])], [normal(263, n_dst, 2, 4)], exact=False, ref=dot_ref(False), graph="block"))
    c.append(case("dot_attention k is v H=2 F=4", {"q": normal(264, n_dst, 2, 4), "kv": normal(265, n_src, 2, 4)},
                  lambda g, t: [ops.dot_attention(g, t["q"], t["kv"], t["kv"])], [normal(266, n_dst, 2, 4)], exact=False, ref=dot_ref(True), graph="block"))

    # ---- fused messages
    for D in (8, 64):
        c.append(case("gine_sum D=%d" % D, {"x": ints(270 + D, n_src, D), "w": ints(280 + D, E, D), "scale": ints(290 + D, E)},
                      lambda g, t: [ops.gine_sum(g, t["x"], t["w"], t["scale"])], [ints(300 + D, n_dst, D)], nograd=("scale",),
                      weights=("w", "scale"), graph="block", terms=2 * longest))
    c.append(case("multi_aggregate sum max min D=8", {"x": ints(310, n_src, 8), "w": ints(311, E, 8)},
                  lambda g, t: [ops.multi_aggregate(g, t["x"], ("sum", "max", "min"), w=t["w"])], [ints(312, n_dst, 3, 8)], weights=("w",),
                  graph="block", terms=2 * longest))

    STATS = ("mean", "var", "std")

    def multi_ref(values, ups, g):
        r = t_multi.Restated(src, dst, n_src, n_dst, values["x"], values["w"], np.arange(E))   # (the rank orders ties of max / min only)
        up = {n: ups[0][:, i, :].double().numpy() for i, n in enumerate(STATS)}
        assert not any(up[n][r.ill].any() for n in ("var", "std"))                 # (multi_up below: zeroed from the reference alone)
        want = r.grads(up)

        def check(got, got_grads, on_gpu, scales=None):
            t_multi.check_forward(got[0], STATS, r, "layouts")
            t_multi.check_grads(got_grads["x"], got_grads["w"], want, "layouts")
        return check
    mx, mw = normal(320, n_src, 8), normal(321, E, 8)
    ill = t_multi.Restated(src, dst, n_src, n_dst, mx, mw, np.arange(E)).ill       # where msq - mean^2 cancels: no var / std gradient there
    multi_up = normal(322, n_dst, 3, 8)
    multi_up[:, 1][torch.from_numpy(ill)] = 0.0
    multi_up[:, 2][torch.from_numpy(ill)] = 0.0
    c.append(case("multi_aggregate mean var std D=8", {"x": mx, "w": mw}, lambda g, t: [ops.multi_aggregate(g, t["x"], STATS, w=t["w"], eps=t_multi.EPS)],
                  [multi_up], exact=False, ref=multi_ref, graph="block"))
    c.append(case("rel_gspmm sum D=8 R=2", {"x": ints(330, n_src, 8), "w": ints(331, E, 2)},
                  lambda g, t: [ops.rel_gspmm(g, t["x"], t["w"], "sum", cache=False)], [ints(332, n_dst, 2, 8)], nograd=("w",), weights=("w",),
                  graph="block", terms=longest))

    # ---- dense-side operators
    n = 40
    c.append(case("head_dot one vector H=2 F=4", {"feat": ints(340, n, 2, 4), "attn_a": ints(341, 1, 2, 4)},
                  lambda g, t: [ops.head_dot(t["feat"], t["attn_a"])], [ints(342, n, 2)], weights=("attn_a",), terms=n))
    for H, Fd in ((2, 4), (1, 7)):
        c.append(case("head_dot two vectors H=%d F=%d" % (H, Fd),
                      {"feat": ints(350 + Fd, n, H, Fd), "attn_a": ints(351 + Fd, 1, H, Fd), "attn_b": ints(352 + Fd, 1, H, Fd)},
                      lambda g, t: list(ops.head_dot(t["feat"], t["attn_a"], t["attn_b"])), [ints(353 + Fd, n, H), ints(354 + Fd, n, H)],
                      weights=("attn_a", "attn_b"), terms=2 * n))   # (a [1, H, F] vector is one row: `expanded` is formed, and is the dense tensor)
    c.append(case("bias_add C=8", {"x": ints(360, n, 8), "bias": ints(361, 8)}, lambda g, t: [ops.bias_add(t["x"], t["bias"])], [ints(362, n, 8)], terms=n))
    c.append(case("relu_dropout C=8", {"x": normal(370, n, 8)}, lambda g, t: [ops.relu_dropout(t["x"], 0.5, True)], [normal(371, n, 8)],
                  backends=("gpu",), seeded=True))
    c.append(case("linear K=12 M=8", {"x": ints(380, n, 12), "weight": ints(381, 8, 12), "bias": ints(382, 8)},
                  lambda g, t: [ops.linear(t["x"], t["weight"], t["bias"])], [ints(383, n, 8)], terms=n))
    c.append(case("linear_sum K=12 M=8", {"x1": ints(390, n, 12), "weight1": ints(391, 8, 12), "x2": ints(392, n, 12), "weight2": ints(393, 8, 12),
                                           "bias": ints(394, 8)},
                  lambda g, t: [ops.linear_sum(t["x1"], t["weight1"], t["x2"], t["weight2"], t["bias"])], [ints(395, n, 8)], terms=2 * n))
    c.append(batch_norm_case("BatchNorm1d C=8", n, 8, 400))

    # ---- segment operators
    seglen = torch.tensor(SEG_LENS)
    for D in (8, 7):
        for red in ("sum", "mean", "max"):
            c.append(case("segment_reduce %s D=%d" % (red, D), {"value": ints(410 + D, SEG_ROWS, D)},
                          (lambda red: lambda s, t: [ops.segment_reduce(s, t["value"], red, total=SEG_ROWS)])(red),
                          [ints(420 + D, len(SEG_LENS), D)], graph="segments", terms=max(SEG_LENS), idtypes=(None,)))

    def seg_softmax_ref(values, ups, g):
        want, want_dx = t_readout.restated_softmax(SEG_LENS, values["value"], ups[0])
        top = {"value": float(want_dx.abs().max())}

        def check(got, got_grads, on_gpu, scales=None):
            if on_gpu:                                                              # test_segment_softmax_on_the_device
                err = (got[0].detach().cpu().double() - want).abs()
                assert not (err > t_readout.RTOL * want + 1e-30).any(), float((err / want).max())
                assert _maxerr(got_grads["value"], want_dx) <= t_readout.RTOL * (scales or top)["value"]
            else:                                                                   # test_segment_softmax_matches_the_restatement
                assert _close(got[0], want) and _close(got_grads["value"], want_dx)
        check.top = top
        return check
    c.append(case("segment_softmax D=4", {"value": normal(430, SEG_ROWS, 4, scale=3.0)}, lambda s, t: [ops.segment_softmax(s, t["value"], total=SEG_ROWS)],
                  [normal(431, SEG_ROWS, 4)], exact=False, ref=seg_softmax_ref, graph="segments", idtypes=(None,), cancels=True))

    def seg_attention_ref(mode):
        def ref(values, ups, g):
            r = t_readout.Restated(SEG_LENS, values["feat"], values.get("logits"), values.get("query"), 0.37 if mode == "query" else 1.0, ups[0])
            names = {"feat": "d_feat", "logits": "d_logits", "query": "d_query"}

            def check(got, got_grads, on_gpu, scales=None):
                if on_gpu:
                    t_readout.check_forward(got[0], r)
                    t_readout.check_grads({names[k]: v for k, v in got_grads.items()}, r)
                else:
                    assert _close(got[0], r.out)
                    for k, v in got_grads.items():
                        assert _close(v, getattr(r, names[k])), k
            return check
        return ref
    c.append(case("segment_attention logits H=2 F=4", {"feat": normal(440, SEG_ROWS, 2, 4), "logits": normal(441, SEG_ROWS, 2, scale=3.0)},
                  lambda s, t: [ops.segment_attention(s, t["feat"], logits=t["logits"], total=SEG_ROWS)], [normal(442, len(SEG_LENS), 2, 4)],
                  exact=False, ref=seg_attention_ref("gate"), graph="segments", idtypes=(None,)))
    c.append(case("segment_attention query H=2 F=4", {"feat": normal(443, SEG_ROWS, 2, 4), "query": normal(444, len(SEG_LENS), 2, 4)},
                  lambda s, t: [ops.segment_attention(s, t["feat"], query=t["query"], scale=0.37, total=SEG_ROWS)], [normal(445, len(SEG_LENS), 2, 4)],
                  exact=False, ref=seg_attention_ref("query"), graph="segments", idtypes=(None,)))
    c.append(case("segment_topk k=2 D=8", {"feat": ints(450, SEG_ROWS, 8)}, lambda s, t: list(ops.segment_topk(s, t["feat"], 2, sortby=0, total=SEG_ROWS)),
                  [ints(451, len(SEG_LENS), 2, 8)], graph="segments", idtypes=(None,)))
    c.append(case("segment_broadcast D=8", {"value": ints(460, len(SEG_LENS), 8)}, lambda s, t: [ops.segment_broadcast(s, t["value"], SEG_ROWS)],
                  [ints(461, SEG_ROWS, 8)], graph="segments", terms=max(SEG_LENS), idtypes=(None,)))

    # ---- one fused layer: the square graph (power-of-two in-degrees: means, and with them every sum, stay exact)
    # every value is a multiple of 1 / (2 HUB), the reciprocal of the longest row: `terms` counts in those units -- the longest sum (the
    # reversed aggregation over a source's out-edges, the weight gradient over the nodes, a GEMM's 8 columns) times 2 HUB
    sn = SQUARE[2]
    sq_terms = 2 * HUB * 2 * int(max(np.bincount(SQUARE[0]).max(), sn, 8))

    def sage(g, t):
        y = ops.sage_mean_layer(g, t["h"], t["w_self"], t["w_neigh"], t["bias"], cat=None)
        assert y is not None, "sage_mean_layer declined the operands"
        return [y]
    c.append(case("sage_mean_layer K=8 M=4", {"h": ints(470, sn, 8, bound=2), "w_self": ints(471, 4, 8, bound=2), "w_neigh": ints(472, 4, 8, bound=2),
                                               "bias": ints(473, 4, bound=2)},
                  sage, [ints(474, sn, 4, bound=2)], graph="square", terms=sq_terms, backends=("gpu",),
                  idtypes=(torch.int32,)))   # ops._fused_layer_operands: the fused layer exists for int32 graphs only (None otherwise)
    return {k.name: k for k in c}


def batch_norm_case(name, n, C, seed):
    def call(g, t):
        bn = mg.nn.BatchNorm1d(C).to(t["x"].device)
        bn._parameters["weight"], bn._parameters["bias"] = t["weight"], t["bias"]   # the leaves themselves, in the layout they lie in
        return [bn(t["x"])]

    def ref(values, ups, g):
        outs, grads, _ = _autograd_ref(lambda x, weight, bias: F.batch_norm(x, None, None, weight, bias, True, 0.1, 1e-5), values, ups)
        top = {k: float(v.abs().max()) for k, v in grads.items()}

        def check(got, got_grads, on_gpu, scales=None):                                         # tests/test_gpu_parity.test_batch_norm_matches_torch
            assert _maxerr(got[0], outs[0]) < 2e-4 * float(outs[0].abs().max())
            for k in ("x", "weight", "bias"):
                assert _maxerr(got_grads[k], grads[k]) < 5e-6 + 5e-4 * (scales or top)[k], k
        check.top = top
        return check
    return case(name, {"x": normal(seed, n, C, scale=2.0) + 0.5, "weight": torch.rand(C, generator=torch.Generator().manual_seed(seed + 1)) + 0.5,
                       "bias": normal(seed + 2, C, scale=0.3)}, call, [normal(seed + 3, n, C)], exact=False, ref=ref, cancels=True)


CASES = build_cases()
TALL = {k.name: k for k in (
    case("linear tall", {"x": ints(500, TALL_N, TALL_K, bound=2), "weight": ints(501, TALL_M, TALL_K, bound=2), "bias": ints(502, TALL_M, bound=2)},
         lambda g, t: [ops.linear(t["x"], t["weight"], t["bias"])], [ints(503, TALL_N, TALL_M, bound=2)], terms=TALL_N),
    case("linear_sum tall", {"x1": ints(510, TALL_N, TALL_K, bound=2), "weight1": ints(511, TALL_M, TALL_K, bound=2),
                             "x2": ints(512, TALL_N, TALL_K, bound=2), "weight2": ints(513, TALL_M, TALL_K, bound=2), "bias": ints(514, TALL_M, bound=2)},
         lambda g, t: [ops.linear_sum(t["x1"], t["weight1"], t["x2"], t["weight2"], t["bias"])], [ints(515, TALL_N, TALL_M, bound=2)], terms=2 * TALL_N),
    case("bias_add tall", {"x": ints(520, TALL_N, TALL_M, bound=2), "bias": ints(521, TALL_M, bound=2)},
         lambda g, t: [ops.bias_add(t["x"], t["bias"])], [ints(522, TALL_N, TALL_M, bound=2)], terms=TALL_N),
    batch_norm_case("BatchNorm1d tall", TALL_N, TALL_M, 530))}
TALL_LAYOUTS = ("colblock", "offset4")
GRAD = "grad"          # the slot name of the upstream gradient(s)


def slots_of(k):
    return list(k.slots) + [GRAD]


def shape_of(k, slot):
    return tuple(k.ups[0].shape) if slot == GRAD else tuple(k.slots[slot].shape)


# Every (case, slot, layout) that is NOT run, with the reason.  Only layouts that cannot be formed are here: no operator of the table
# documents that it rejects a layout torch accepts.
#   transposed  a 1-D operand (a bias, a scale per edge) has no second dimension to transpose
#   expanded    needs equal rows.  It is run for every upstream gradient (what `.sum().backward()` delivers) and for the per-edge scale and
#               weight operands, with the case's values replaced by their first row; for every other operand the rows must differ: equal
#               feature rows make every neighbourhood's max, softmax and variance degenerate and would hide a misattributed row
EXCLUDED = {}
for _k in CASES.values():
    for _slot in slots_of(_k):
        if len(shape_of(_k, _slot)) < 2:
            EXCLUDED[(_k.name, _slot, "transposed")] = "a 1-D operand has no second dimension to transpose"
        if _slot != GRAD and _slot not in _k.weights:
            EXCLUDED[(_k.name, _slot, "expanded")] = "rows must differ"
# the restatement of tests/test_multi_aggregate.py takes no var / std gradient on its ill-conditioned elements (rows of one edge): the
# gradient's rows differ by construction
EXCLUDED[("multi_aggregate mean var std D=8", GRAD, "expanded")] = "rows must differ: the upstream gradient is zero on the restatement's ill-conditioned rows"

TABLE = [(k.name, slot, tuple(L for L in layouts.NAMES if (k.name, slot, L) not in EXCLUDED)) for k in CASES.values() for slot in slots_of(k)]
CELLS = [(name, slot, L) for name, slot, Ls in TABLE for L in Ls]
TALL_CELLS = [(k.name, slot, L) for k in TALL.values() for slot in slots_of(k) for L in TALL_LAYOUTS]
# an expanded gradient (stride 0 along the rows, unit column stride) on its way into mgx_xty: walked by max(stride, width) it would be
# read past its single row -- HipBackend._row_walkable copies it
TALL_CELLS += [(name, GRAD, "expanded") for name in ("linear tall", "linear_sum tall")]


# ----------------------------------------------------------------------------- running one cell
def values_for(k, slot, layout):
    """(slot values, upstream gradients) of the cell: the case's own, or -- `expanded` -- with the varied operand's rows all equal to its first"""
    values, ups = dict(k.slots), list(k.ups)
    if layout == "expanded":
        def flat(v):
            return v[:1].expand_as(v).contiguous()
        if slot == GRAD:
            ups = [flat(u) for u in ups]
        else:
            values[slot] = flat(values[slot])
    return values, ups


def assert_exact_precondition(k, values, ups):
    """every sum of the case stays exact in fp32: (terms of the longest sum) x (largest |operand| of each slot and of the gradient)"""
    bound = k.terms
    for v in list(values.values()) + list(ups):
        bound *= max(float(v.abs().max()), 1.0)
    assert bound < xl.LIMIT, "inputs too large for exact fp32 sums: %g" % bound


def structure_for(k, dev, idtype, seglen_layout="dense"):
    if k.graph == "segments":
        return layouts.make(seglen_layout, torch.tensor(SEG_LENS), dev).view
    return graph_on(k.graph, idtype, dev) if k.graph else None


def run(k, dev, idtype, values, ups, slot=None, layout="dense", seglen_layout="dense"):
    """one call of case k with `slot` (an operand, GRAD or None) in `layout`, everything else dense: (outputs, {slot: gradient}); asserts
    (c) and (d)"""
    g = structure_for(k, dev, idtype, seglen_layout)
    laid = {s: layouts.make(layout if s == slot else "dense", v, dev) for s, v in values.items()}
    laid_up = [layouts.make(layout if slot == GRAD else "dense", u, dev) for u in ups]
    leaves = {s: L.view.detach().requires_grad_(s not in k.nograd) for s, L in laid.items()}
    for s, L in laid.items():
        assert leaves[s].data_ptr() == L.view.data_ptr() and leaves[s].stride() == L.view.stride()
    held = [(L, L.snapshot()) for L in list(laid.values()) + laid_up]
    if k.seeded:
        torch.manual_seed(1234)
        calls, ops.ReluDropout._calls = ops.ReluDropout._calls, 0
    try:
        outs = k.call(g, leaves)
    finally:
        if k.seeded:
            ops.ReluDropout._calls = calls
    torch.autograd.backward(outs[:len(ups)], [L.view for L in laid_up])
    grads = {}
    for s, leaf in leaves.items():
        if s in k.nograd:
            assert leaf.grad is None
            continue
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape, (s, None if leaf.grad is None else tuple(leaf.grad.shape))   # (d)
        grads[s] = leaf.grad.detach()
    for L, snap in held:                                                           # (c)
        assert L.unchanged(snap) and L.guards_hold(), "an operand or its guard elements changed (%s)" % L.name
    return [o.detach() for o in outs], grads


_baseline = {}


def baseline(k, dev, idtype, flat_slot, values, ups):
    """the all-dense call of these values: once per (case, device, id width, which operand has equal rows)"""
    key = (k.name, dev, idtype, flat_slot)
    if key not in _baseline:
        _baseline[key] = run(k, dev, idtype, values, ups)
    return _baseline[key]


_checks = {}


def check_for(k, dev, idtype, flat_slot, values, ups):
    """the reference of an exact=False case: built once per set of values (on the host, from the fp32 inputs)"""
    key = (k.name, flat_slot)
    if key not in _checks:
        _checks[key] = k.ref(values, ups, None)
    return _checks[key]


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(got, want), "%s: %d elements differ from the all-dense call" % (what, int((got != want).sum()))


def run_cell(k, dev, slot, layout, seglen_layout="dense"):
    values, ups = values_for(k, slot, layout)
    flat_slot = slot if layout == "expanded" else None
    if k.exact and not k.seeded:
        assert_exact_precondition(k, values, ups)
    for idtype in k.idtypes:
        outs, grads = run(k, dev, idtype, values, ups, slot, layout, seglen_layout)                    # (a)
        if k.exact or k.seeded:                                                                            # (b)
            want_outs, want_grads = baseline(k, dev, idtype, flat_slot, values, ups)
            assert len(outs) == len(want_outs) and sorted(grads) == sorted(want_grads)
            for i, (a, b) in enumerate(zip(outs, want_outs)):
                same(a, b, "output %d" % i)
            for s in grads:
                same(grads[s], want_grads[s], "gradient of %s" % s)
            if k.seeded:
                assert torch.equal(outs[0] == 0, want_outs[0] == 0), "another dropout mask"
        else:
            scales = check_for(k, dev, idtype, None, k.slots, k.ups).top if k.cancels and flat_slot == GRAD else None
            check_for(k, dev, idtype, flat_slot, values, ups)(outs, grads, dev != "cpu", scales)


@pytest.fixture()
def cpu_on():
    was = mg.enable_cpu_backend(True)
    try:
        yield
    finally:
        mg.enable_cpu_backend(was)


def ids(cells):
    return ["%s-%s-%s" % c for c in cells]


def on(backend, cells, table):
    return [c for c in cells if backend in table[c[0]].backends]


# ----------------------------------------------------------------------------- the helpers themselves, and the table
@pytest.mark.parametrize("shape", [(6, 8), (6, 2, 4), (5, 7), (9,), (6, 1)])
def test_layouts_hold_the_values_and_are_what_their_names_say(shape):
    v = torch.arange(float(np.prod(shape))).view(shape) - 3.0
    for name in layouts.NAMES:
        val = v[:1].expand_as(v).contiguous() if name == "expanded" else v
        if name == "transposed" and len(shape) < 2:
            with pytest.raises(layouts.LayoutError):
                layouts.make(name, val)
            continue
        L = layouts.make(name, val)
        assert torch.equal(L.view, val) and tuple(L.view.shape) == shape
        assert layouts.as_named(name, L, shape) is None, (name, layouts.as_named(name, L, shape))
        assert L.guards_hold() and int(L.guard.sum()) == L.buf.numel() - (val[:1].numel() if name == "expanded" else val.numel())
        snap = L.snapshot()
        assert L.unchanged(snap)
        if bool(L.guard.any()):                                                    # a write beside the view is seen
            L.buf.view(-1)[int(torch.nonzero(L.guard)[0])] = 1.0
            assert not L.unchanged(snap) and not L.guards_hold()
        leaf = L.view.detach().requires_grad_(True)
        assert leaf.stride() == L.view.stride() and leaf.data_ptr() == L.view.data_ptr()
    with pytest.raises(layouts.LayoutError):
        layouts.make("expanded", v)                                                # rows differ
    lens = layouts.make("alt_rows", torch.tensor(SEG_LENS))
    assert torch.equal(lens.view, torch.tensor(SEG_LENS)) and lens.view.stride() == (2,) and lens.guards_hold()


def test_backward_hands_the_upstream_gradient_over_as_it_lies():
    """autograd does not repack a gradient on its way into a Function: the layout the test gives is the layout the operator's backward sees"""
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, dy):
            seen.append((dy.stride(), dy.data_ptr()))
            return dy

    for name in layouts.NAMES:
        v = torch.ones(6, 8)
        L = layouts.make(name, v)
        Probe.apply(v.clone().requires_grad_(True)).backward(L.view)
        assert seen[-1] == (L.view.stride(), L.view.data_ptr()), name


def test_every_slot_meets_every_layout_or_is_excluded():
    cells = set(CELLS)
    assert len(cells) == len(CELLS)
    for k in CASES.values():
        assert k.backends and set(k.backends) <= {"cpu", "gpu"}
        for slot in slots_of(k):
            for L in layouts.NAMES:
                key = (k.name, slot, L)
                assert (key in cells) != (key in EXCLUDED), key
                if key in EXCLUDED:                                                # an exclusion is a layout that cannot be formed
                    assert isinstance(EXCLUDED[key], str) and EXCLUDED[key]
                    if L == "transposed":
                        with pytest.raises(layouts.LayoutError):
                            layouts.make(L, k.ups[0] if slot == GRAD else k.slots[slot])
                    else:
                        assert L == "expanded"
                        vals = k.ups if slot == GRAD else [k.slots[slot]]
                        for v in vals:
                            with pytest.raises(layouts.LayoutError):
                                layouts.make(L, v)
    assert set(EXCLUDED) <= {(k.name, s, L) for k in CASES.values() for s in slots_of(k) for L in layouts.NAMES}
    # every operator and form the matrix is meant to hold
    for word in ("gspmm copy_u sum", "gspmm copy_u mean", "gspmm copy_u max", "gspmm u_mul_e sum [E,H,1]", "gspmm u_mul_e sum [E,H,F]", "gspmm u_add_e sum",
                 "gspmm copy_e sum", "gsddmm u_add_v", "gsddmm u_mul_e", "gsddmm u_dot_v", "edge_softmax", "gat_attention", "gat_fused", "dot_attention H",
                 "dot_attention k is v", "gine_sum", "multi_aggregate sum max min", "multi_aggregate mean var std", "rel_gspmm", "head_dot one vector",
                 "head_dot two vectors", "bias_add", "relu_dropout", "linear K", "linear_sum", "BatchNorm1d", "segment_reduce sum", "segment_reduce mean",
                 "segment_reduce max", "segment_softmax", "segment_attention logits", "segment_attention query", "segment_topk", "segment_broadcast",
                 "sage_mean_layer"):
        assert any(name.startswith(word) for name in CASES), word


# ----------------------------------------------------------------------------- the matrix: CPU backend
@pytest.mark.parametrize("name,slot,layout", on("cpu", CELLS, CASES), ids=ids(on("cpu", CELLS, CASES)))
def test_matrix_on_the_cpu_backend(cpu_on, name, slot, layout):
    run_cell(CASES[name], "cpu", slot, layout)


@pytest.mark.parametrize("name,slot,layout", on("cpu", TALL_CELLS, TALL), ids=ids(on("cpu", TALL_CELLS, TALL)))
def test_tall_inputs_on_the_cpu_backend(cpu_on, name, slot, layout):
    run_cell(TALL[name], "cpu", slot, layout)


SEGMENT_CASES = [k.name for k in CASES.values() if k.graph == "segments"]


@pytest.mark.parametrize("name", SEGMENT_CASES)
def test_segment_lengths_as_every_other_element_on_the_cpu_backend(cpu_on, name):
    run_cell(CASES[name], "cpu", None, "dense", seglen_layout="alt_rows")


def layer_on_a_column_block(dev, make_layer, width=8):
    """layer(block, feat) with feat a column block of a wider matrix against the same call on a dense copy: the 1e-4 of the tensor's
    scale that tests/test_gpu_parity.py holds composed layers to (the kernels are the same ones: in practice the same bits)"""
    g = graph_on("block", torch.int32, dev)
    torch.manual_seed(5)
    layer = make_layer().to(dev)
    value, up = normal(600, BLOCK[2], width), None
    got = {}
    for layout in ("dense", "colblock"):
        L = layouts.make(layout, value, dev)
        snap = L.snapshot()
        feat = L.view.detach().requires_grad_(True)
        layer.zero_grad()
        y = layer(g, feat)
        up = normal(601, *y.shape).to(dev) if up is None else up
        y.backward(up)
        assert feat.grad.shape == feat.shape and L.unchanged(snap) and L.guards_hold()
        got[layout] = [y.detach(), feat.grad.detach()] + [p.grad.detach().clone() for p in layer.parameters()]
    for a, b in zip(got["colblock"], got["dense"]):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


LAYERS = {"SAGEConv mean": lambda: mg.nn.SAGEConv(8, 4, "mean"),
          "GATConv H=2": lambda: mg.nn.GATConv(8, 4, 2, allow_zero_in_degree=True),
          "GraphConv": lambda: mg.nn.GraphConv(8, 4, allow_zero_in_degree=True)}


@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_layers_on_a_column_block_on_the_cpu_backend(cpu_on, layer):
    layer_on_a_column_block("cpu", LAYERS[layer])


# ----------------------------------------------------------------------------- the matrix: device
@pytest.mark.gpu
@pytest.mark.parametrize("name,slot,layout", on("gpu", CELLS, CASES), ids=ids(on("gpu", CELLS, CASES)))
def test_matrix_on_the_device(name, slot, layout):
    run_cell(CASES[name], DEV, slot, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("name,slot,layout", on("gpu", TALL_CELLS, TALL), ids=ids(on("gpu", TALL_CELLS, TALL)))
def test_tall_inputs_on_the_device(name, slot, layout):
    run_cell(TALL[name], DEV, slot, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEGMENT_CASES)
def test_segment_lengths_as_every_other_element_on_the_device(name):
    run_cell(CASES[name], DEV, None, "dense", seglen_layout="alt_rows")


@pytest.mark.gpu
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_layers_on_a_column_block_on_the_device(layer):
    layer_on_a_column_block(DEV, LAYERS[layer])
