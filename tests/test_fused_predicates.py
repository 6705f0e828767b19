"""The contract every `X_fused` predicate of mi355x_graph.ops keeps with its operator `X`:

  * operands the operator rejects: the operator raises a DGLError of its own (its name in the text, so that no backend's error can stand
    in for it -- a CPU backend is installed and the accepted set runs beside every rejected one) and the predicate says False, never raises;
  * operands the operator accepts: the predicate says which path the operator takes -- on the CPU always the composed one, whose values are
    checked against the restatement of the operator's own test file (imported, not repeated here); on the device the backend's fused
    wrapper is counted: one call when the predicate says True, none when it says False, and the operator's result is, bit for bit, that of
    the named path called directly (the autograd Function / backend wrapper, or the composition);
  * the predicates of the segment operators never wait for the device when the caller passes the row count (and max_len for fps).

Shapes: a 5-node, 8-edge graph or two segments of 3 and 4 rows, D = 4, H = 1, k = 2.  The point coordinates, x, w and scale are small
integers, so every sum of the summing operators is exact on both paths, which must therefore also agree with each other (torch.equal);
the two softmax operators' paths agree with each other as their own CPU tests compare them (rtol 1e-5, atol 1e-6: a handful of fp32
roundings over at most 4 terms)."""
import functools
import types

import numpy as np
import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import config, ops, sparse
import oracle_backend
import test_ball_query as t_ball
import test_dot_attention as t_dot
import test_fps as t_fps
import test_gine as t_gine
import test_knn as t_knn
import test_knn_query as t_knnq
import test_multi_aggregate as t_multi
import test_readout as t_readout
import test_rel_spmm as t_rel
import test_segment_topk as t_topk

DEV = "cuda:0"
SRC = np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.int64)
DST = np.array([1, 2, 3, 4, 0, 2, 2, 1], dtype=np.int64)
N, E, D, K = 5, 8, 4, 2
LENS, QUERY_LENS = (3, 4), (2, 3)
ROWS, QUERY_ROWS = sum(LENS), sum(QUERY_LENS)
AGGS = ("sum", "max", "min")


def ints(*shape, seed=0):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).float()


def case(op, pred, ok, bad, check, kernel, switch, direct=None, exact=True):
    """ok: (args, kwargs) of an accepted call; bad: {label: (args, kwargs)} of rejected ones, each one edit of an accepted call;
    direct(fused), where the two paths round differently: the fused (True) or composed (False) path of the accepted call, without the operator."""
    return types.SimpleNamespace(op=op, pred=pred, ok=ok, bad=bad, check=check, kernel=kernel, switch=switch, direct=direct, exact=exact, also=())


def edits(ok, **changes):
    """{label: (args, kwargs)}: `ok` with positional argument i replaced (label=(i, value)) or a keyword set (label=(name, value))"""
    args, kwargs = ok
    out = {}
    for label, (where, value) in changes.items():
        if isinstance(where, int):
            out[label] = (args[:where] + (value,) + args[where + 1:], kwargs)
        else:
            out[label] = (args, dict(kwargs, **{where: value}))
    return out


def close(got, want):
    return torch.allclose(got.detach().cpu().double(), want, rtol=1e-5, atol=1e-6)


@functools.lru_cache(maxsize=None)
def cases(device):
    """name -> case, operands on `device`; built once and never modified"""
    g = mg.graph((torch.from_numpy(SRC), torch.from_numpy(DST)), num_nodes=N).int().to(device)
    seglen, qlen = torch.tensor(LENS).to(device), torch.tensor(QUERY_LENS).to(device)
    meta = torch.empty(2, dtype=torch.int64, device="meta")
    x, w, s = ints(N, D, seed=1).to(device), ints(E, D, seed=2).to(device), ints(E, seed=3).to(device)
    pts, qpts = ints(ROWS, D, seed=4).to(device), ints(QUERY_ROWS, D, seed=5).to(device)
    gen = torch.Generator().manual_seed(6)
    q, k, v = (torch.randn(N, 1, D, generator=gen).to(device) for _ in range(3))
    feat, logits = torch.randn(ROWS, 1, D, generator=gen).to(device), torch.randn(ROWS, 1, generator=gen).to(device)
    rel_w = ints(E, 2, seed=7).to(device)
    centers = torch.tensor([0, 4, 6, 2]).to(device)
    c = {}

    ok = ((g, q, k, v), {})
    c["dot_attention"] = case(
        ops.dot_attention, ops.dot_attention_fused, ok,
        edits(ok, no_graph=(0, None), q_2d=(1, q[:, 0]), k_no_tensor=(2, None), v_double=(3, v.double()), q_rows=(1, q[:4]), k_rows=(2, k[:4]), v_rows=(3, v[:4]), k_width=(2, k[:, :, :2]), v_heads=(3, v.view(N, 2, 2))),
        lambda out: close(out, t_dot.Restated(SRC, DST, N, N, q, k, v, D ** -0.5).out), "dot_attention_fwd", "DOT_ATTENTION_FUSED",
        lambda fused: ops.DotAttention.apply(g._index, q, k, v, D ** -0.5) if fused else t_dot.composition(g, q, k, v, D ** -0.5), exact=False)

    ok = ((g, x, w, s), {})
    c["gine_sum"] = case(
        ops.gine_sum, ops.gine_sum_fused, ok,
        edits(ok, no_graph=(0, 3), x_3d=(1, x.view(N, 2, 2)), w_none=(2, None), x_double=(1, x.double()), w_rows=(2, w[:7]), w_width=(2, w[:, :2]),
              scale_shape=(3, s.view(4, 2)), scale_list=(3, [1.0] * E), scale_double=(3, s.double()), scale_grad=(3, s.clone().requires_grad_(True))),
        lambda out: close(out, t_gine.Restated(SRC, DST, N, N, x, w, s).out), "gine_fwd", "GINE_FUSED")

    ok = ((g, x, AGGS, w), {})
    c["multi_aggregate"] = case(
        ops.multi_aggregate, ops.multi_aggregate_fused, ok,
        edits(ok, no_graph=(0, "g"), x_3d=(1, x.view(N, 2, 2)), x_double=(1, x.double()), x_rows=(1, x[:4]), w_3d=(3, w.view(E, 2, 2)),
              w_double=(3, w.double()), w_rows=(3, w[:7]), names_str=(2, "sum"), names_empty=(2, ()), names_unknown=(2, ("sum", "median")),
              names_repeated=(2, ("sum", "sum")), eps_text=("eps", "small"), eps_zero=("eps", 0.0), eps_inf=("eps", float("inf"))),
        lambda out: t_multi.check_forward(out, AGGS, t_multi.Restated(SRC, DST, N, N, x, w, t_multi.storage_rank(g))) is None,
        "multi_agg_fwd", "MULTI_AGG_FUSED")

    ok = ((seglen, feat), dict(logits=logits, total=ROWS))
    ok_query = ((seglen, feat), dict(query=torch.randn(2, 1, D, generator=gen).to(device), total=ROWS))
    offsets = ops._offsets_of(seglen, device)
    c["segment_attention"] = case(
        ops.segment_attention, ops.segment_attention_fused, ok,
        dict(edits(ok_query, query_segments=("query", feat[:3]), query_2d=("query", feat[:2, 0]), query_list=("query", [[1.0] * D] * 2),
                   query_double=("query", feat[:2].double()), query_device=("query", torch.empty(2, 1, D, device="meta"))),
             **edits(ok, feat_2d=(1, feat[:, 0]), feat_list=(1, [1.0]), feat_double=(1, feat.double()), both=("query", feat[:2]), neither=("logits", None),
              logits_double=("logits", logits.double()), logits_rows=("logits", logits[:6]), logits_3d=("logits", logits.unsqueeze(-1)),
              logits_device=("logits", torch.empty(ROWS, 1, device="meta")), seglen_list=(0, list(LENS)), seglen_2d=(0, seglen.view(1, 2)),
              total=("total", ROWS - 1))),
        lambda out: t_readout.check_forward(out, t_readout.Restated(LENS, feat, logits)) is None,
        "segment_attention_fwd", "SEGMENT_ATTENTION_FUSED",
        lambda fused: (ops.SegmentAttention.apply(feat, logits, None, offsets, 1.0) if fused
                       else ops._segment_attention_composed(offsets, feat, logits, None, 1.0, ROWS)), exact=False)

    c["segment_attention"].also = (ok_query,)                 # query mode: the accepted call its query_* variants edit

    def topk_check(out):
        ref = t_topk.Restated(LENS, pts, K, 0, True)
        return torch.equal(out[1].cpu(), ref.index) and torch.equal(t_topk.bits(out[0]), t_topk.bits(ref.values))

    ok = ((seglen, pts, K), dict(sortby=0, total=ROWS))
    c["segment_topk"] = case(
        ops.segment_topk, ops.segment_topk_fused, ok,
        edits(ok, feat_3d=(1, pts.view(ROWS, 2, 2)), feat_list=(1, [1.0, 2.0]), feat_double=(1, pts.double()), no_columns=(1, pts[:, :0]),
              k_zero=(2, 0), k_bool=(2, True), k_float=(2, 2.5), sortby_high=("sortby", D), sortby_float=("sortby", 1.0), sortby_bool=("sortby", True),
              seglen_list=(0, list(LENS)), seglen_device=(0, meta), total=("total", ROWS + 1)),
        topk_check, "segment_topk_fwd", "SEGMENT_TOPK_FUSED")

    ok = ((seglen, pts, K), dict(total=ROWS, return_dist=True))
    c["segment_knn"] = case(
        ops.segment_knn, ops.segment_knn_fused, ok,
        edits(ok, x_1d=(1, pts[:, 0]), x_none=(1, None), x_double=(1, pts.double()), no_columns=(1, pts[:, :0]), k_zero=(2, 0), k_bool=(2, True),
              seglen_list=(0, list(LENS)), seglen_2d=(0, seglen.view(2, 1)), seglen_device=(0, meta), total=("total", ROWS - 1)),
        lambda out: t_knn.check_exact(out[0], out[1], t_knn.Restated(LENS, pts), K) is None, "segment_knn", "KNN_FUSED")

    ok = ((seglen, pts, qlen, qpts, K), dict(ref_total=ROWS, query_total=QUERY_ROWS, return_dist=True, return_weight=True))
    c["segment_knn_query"] = case(
        ops.segment_knn_query, ops.segment_knn_query_fused, ok,
        edits(ok, x_1d=(1, pts[:, 0]), y_list=(3, [[0.0] * D]), y_double=(3, qpts.double()), y_device=(3, torch.empty(QUERY_ROWS, D, device="meta")),
              widths=(3, qpts[:, :3]), no_columns=(1, pts[:, :0]), k_bool=(4, True), k_zero=(4, 0), eps_negative=("eps", -1.0),
              eps_inf=("eps", float("inf")), eps_bool=("eps", True), segments=(2, torch.tensor([QUERY_ROWS]).to(device)),
              seglen_list=(0, list(LENS)), query_seglen_2d=(2, qlen.view(1, 2)), seglen_device=(2, meta), ref_total=("ref_total", ROWS + 1),
              query_total=("query_total", QUERY_ROWS - 1)),
        lambda out: t_knnq.check_exact(out, t_knnq.Restated(LENS, pts, QUERY_LENS, qpts), K) is None, "segment_knn_query", "KNN_QUERY_FUSED")

    ok = ((seglen, pts, K), dict(total=ROWS, max_len=max(LENS), return_dist=True))
    c["segment_fps"] = case(
        ops.segment_fps, ops.segment_fps_fused, ok,
        edits(ok, x_3d=(1, pts.view(ROWS, 2, 2)), x_double=(1, pts.double()), no_columns=(1, pts[:, :0]), npoints_zero=(2, 0), npoints_bool=(2, True),
              seglen_list=(0, list(LENS)), seglen_device=(0, meta), start_float=("start", 1.5), start_int32=("start", torch.zeros(2, dtype=torch.int32).to(device)),
              start_length=("start", torch.zeros(3, dtype=torch.int64).to(device)), max_len_negative=("max_len", -1), max_len_bool=("max_len", True),
              total=("total", ROWS - 1)),
        lambda out: t_fps.check_exact(out[0], out[1], t_fps.restated(LENS, pts, K), K) is None, "segment_fps", "FPS_FUSED")

    def ball_check(out):
        index, count = t_ball.restated(LENS, pts, centers.cpu(), 2.0, K, True)
        return torch.equal(out[0].cpu(), index) and torch.equal(out[1].cpu(), count)

    ok = ((seglen, pts, centers, 2.0, K), dict(total=ROWS))
    c["segment_ball_query"] = case(
        ops.segment_ball_query, ops.segment_ball_query_fused, ok,
        edits(ok, x_1d=(1, pts[:, 0]), x_double=(1, pts.double()), no_columns=(1, pts[:, :0]), neighbors_bool=(4, True), neighbors_zero=(4, 0),
              centers_float=(2, centers.float()), centers_2d=(2, centers.view(2, 2)), centers_list=(2, [0, 4]), radius_negative=(3, -1.0),
              radius_text=(3, "far"), radius_bool=(3, True), radius_nan=(3, float("nan")), pad=("pad", "last"), seglen_list=(0, list(LENS)),
              seglen_device=(0, meta), total=("total", ROWS + 1)),
        ball_check, "segment_ball_query", "BALL_QUERY_FUSED")

    ok = ((g, x, rel_w), {})
    c["rel_gspmm"] = case(
        lambda *a: ops.rel_gspmm(*a, reduce="sum"), ops.rel_gspmm_fused, ok,
        edits(ok, no_graph=(0, None), x_1d=(1, x[:, 0]), w_3d=(2, rel_w.unsqueeze(-1)), w_list=(2, [1.0])),
        lambda out: torch.allclose(out, t_rel.loop_rel_gspmm(g, x, rel_w, "sum"), rtol=1e-5, atol=1e-6), "spmm_rel", None)
    return c


NAMES = ("dot_attention", "gine_sum", "multi_aggregate", "segment_attention", "segment_topk", "segment_knn", "segment_knn_query", "segment_fps",
         "segment_ball_query", "rel_gspmm")
SEGMENT_NAMES = tuple(n for n in NAMES if n.startswith("segment_"))


def call(fn, operands):
    return fn(*operands[0], **operands[1])


def tensors(out):
    return [t for t in (out if isinstance(out, tuple) else (out,)) if t is not None]


@pytest.fixture
def checker():
    oracle_backend.install()
    yield
    oracle_backend.uninstall()


def check_rejected(c, name):
    """the accepted calls run; every rejected one raises the operator's own DGLError -- its name is in the text (the graph check: the type it
    wants), which no backend's error carries -- and the predicate says False without raising"""
    for operands in (c.ok,) + c.also:
        call(c.op, operands)
    assert len(c.bad) >= 3
    for label, operands in c.bad.items():
        with pytest.raises(mg.DGLError, match="expected a DGLGraph" if label == "no_graph" else name):
            call(c.op, operands)
        assert call(c.pred, operands) is False, label


@pytest.mark.parametrize("name", NAMES)
def test_rejected_operands_raise_and_the_predicate_says_false(checker, name):
    check_rejected(cases("cpu")[name], name)


def test_rel_gspmm_rejects_a_reduce_the_predicate_is_not_told(checker):
    g, x, w = cases("cpu")["rel_gspmm"].ok[0]
    ops.rel_gspmm(g, x, w, "mean")
    with pytest.raises(mg.DGLError, match="rel_gspmm: reduce"):
        ops.rel_gspmm(g, x, w, "max")


@pytest.mark.parametrize("name", NAMES)
def test_accepted_operands_compose_on_the_cpu_and_match_the_restatement(checker, name):
    c = cases("cpu")[name]
    assert call(c.pred, c.ok) is False
    assert c.check(call(c.op, c.ok))


# ----------------------------------------------------------------------------- GPU
def counted(monkeypatch, c):
    """the list the backend's fused wrapper of case c appends to, once per call"""
    backend, calls = type(sparse.backend_for(torch.zeros(1, device=DEV))), []
    inner = getattr(backend, c.kernel)

    def wrapper(self, *args, **kwargs):
        calls.append(c.kernel)
        return inner(self, *args, **kwargs)

    monkeypatch.setattr(backend, c.kernel, wrapper)         # on the class, as the neighbouring tests do: undone, nothing is left on the instance
    return calls


def run_counted(c, calls, operands):
    """(the predicate's answer, the operator's result) of one call that took the path the predicate named"""
    fused = call(c.pred, operands)
    assert fused in (True, False)
    del calls[:]
    out = call(c.op, operands)
    assert len(calls) == (1 if fused else 0), (fused, calls)
    return fused, tensors(out)


def same(c, got, want):
    """the two paths against each other"""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        if c.exact:
            assert torch.equal(a, b)                    # no NaN in these results; -0.0 == 0.0
        else:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def bit_equal_to_the_named_path(c, fused, out):
    """the operator's result against the path the predicate named, called directly: the same kernels or operators on the same operands"""
    if c.direct is not None:
        want = tensors(c.direct(fused))
        assert len(out) == len(want)
        for a, b in zip(out, want):
            assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_predicate_names_the_path_the_operator_takes(monkeypatch, name):
    c = cases(DEV)[name]
    calls = counted(monkeypatch, c)
    fused, out_fused = run_counted(c, calls, c.ok)
    assert fused is True
    bit_equal_to_the_named_path(c, True, out_fused)
    if c.switch is not None:
        monkeypatch.setattr(config, c.switch, False)
        unfused, out_composed = run_counted(c, calls, c.ok)
        assert unfused is False
        bit_equal_to_the_named_path(c, False, out_composed)
        same(c, out_fused, out_composed)
        monkeypatch.setattr(config, c.switch, True)
    check_rejected(c, name)                             # rejected on the device as on the host


@pytest.mark.gpu
@pytest.mark.parametrize("name,positions", [("gine_sum", (1, 2)), ("multi_aggregate", (1, 3))])
def test_a_contiguous_view_at_a_4_byte_offset_is_not_fused(monkeypatch, name, positions):
    c = cases(DEV)[name]
    calls = counted(monkeypatch, c)
    _, out_fused = run_counted(c, calls, c.ok)
    for i in positions:
        t = c.ok[0][i]
        odd = torch.zeros(t.numel() + 1, device=DEV)[1:].view(t.shape).copy_(t)
        assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
        operands = (c.ok[0][:i] + (odd,) + c.ok[0][i + 1:], c.ok[1])
        unfused, out = run_counted(c, calls, operands)
        assert unfused is False
        same(c, out_fused, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEGMENT_NAMES)
def test_segment_predicates_do_not_wait_for_the_device(name):
    c = cases(DEV)[name]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fused = call(c.pred, c.ok)                      # every row count (and max_len) is given: nothing to read back
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert fused is True
