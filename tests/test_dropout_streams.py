"""Every dropout mask the library draws on the device, against a host restatement of its definition (tests/dropout_streams.py):

  relu + dropout   mgx_relu_dropout_fwd / _strided / _counter (csrc/elementwise.hip) and the activation epilogue of mgx_rows_gemm
                   (csrc/rowsgemm.hip): y, the stored mask bytes and dx, bit for bit -- nothing in them is rounded differently on
                   the host.  NaN rule: the relu test is !(x <= 0), so a NaN at a kept position stays NaN with its mask bit set.
  attention dropout of the fused GAT ROW kernels (csrc/gatfused.hip), keyed (seed, edge id, head): outputs and gradients against an
                   fp64 reference that applies the restated mask, on a graph whose edge ids are a real permutation in both CSRs.

The CPU part (unmarked) pins the restatement itself: splitmix64's published sequence, the same mixer as test_gat_fused.pair_keep,
and the keep-share conditions the GPU tests impose."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import dropout_streams as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ROWS, COLS = 256, 64
PS = (0.1, 0.5, 0.9)
POSITIONS = ((0, 0), (12345, 777), (2 ** 64 - 1, ds.call_offset(5)))
P_LAST = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
SPECIALS = np.array([-0.0, 0.0, 1e-40, np.inf, -np.inf, np.nan], dtype=np.float32)  # (1e-40: a float32 denormal)


# ------------------------------------------------------------------------------------------------------------------ the CPU part
def test_splitmix64_published_sequence():
    """The first three outputs of SplitMix64 from state 0 (the reference implementation's sequence): the state advances by the
    golden-ratio increment, which splitmix64(z) adds itself, so they are splitmix64 of 0, one and two increments."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = ds.splitmix64(np.array([0, ds.STEP, (2 * ds.STEP) & ds.M64], dtype=np.uint64))
    assert [int(v) for v in got] == want
    assert int(ds.splitmix64(0)) == want[0]


def test_stream_positions_wrap_as_the_kernels_do():
    assert ds.call_offset(0) == 0 and ds.call_offset(1) == ds.STEP & ds.M63 and ds.call_offset(5) == (5 * ds.STEP) % 2 ** 64 % 2 ** 63
    assert ds.counter_offset(1 << 20) == ((ds.STEP << 20) % 2 ** 64) % 2 ** 63
    assert ds.counter_offset(-3) == ds.counter_offset(2 ** 64 - 3)                 # an int64 counter is read as uint64
    assert ds.gat_call_seed(2 ** 64 - 1, 3) == (2 ** 64 - 1) ^ ((3 * ds.STEP) % 2 ** 64)
    assert ds.drop_below(0.0) == 0 and ds.drop_below(0.5) == 1 << 31 and ds.drop_below(P_LAST) == 2 ** 32 - 256
    assert ds.drop_below(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)           # from the float argument, not the double
    # (offset + i) * 2 wraps modulo 2^64 inside a tensor that starts at 2^63 - 3: float4 number 3 draws counter 0
    a, b = ds.relu_dropout_keep(99, 2 ** 63 - 3, 8, 0.5), ds.relu_dropout_keep(99, 0, 5, 0.5)
    assert np.array_equal(a[3:], b)


def test_gat_hash_is_the_mixer_of_pair_keep():
    """gat_hash(seed, source, destination + rank * 0x9E3779B1) against test_gat_fused.pair_keep (the tile walks' restatement, which
    returns only the comparison with the threshold): the same bit at 64 thresholds for 20,000 random keys."""
    from test_gat_fused import pair_keep
    rng = np.random.default_rng(1)
    n = 20000
    src, dst = rng.integers(0, 1 << 24, n), rng.integers(0, 1 << 31, n)
    rank = rng.integers(0, 128, n)
    for seed in (0, 7, 2 ** 64 - 1, 0x123456789ABCDEF0):
        h = ds.gat_hash(seed, src, (dst + rank * 0x9E3779B1) & 0xFFFFFFFF)
        assert h.dtype == np.uint32
        for t in [0, 1, 2 ** 32 - 1, 2 ** 31] + [int(v) for v in rng.integers(0, 2 ** 32, 60)]:
            p = t / 4294967296.0  # exact in a double: pair_keep's threshold is t again
            assert np.array_equal(h >= np.uint32(t), pair_keep(seed, dst, src, rank, p))


def test_gat_edge_keep_is_keyed_by_edge_and_head():
    keep = ds.gat_edge_keep(77, 500, 4, 0.3)
    assert keep.shape == (500, 4) and keep.dtype == bool
    assert bool(keep[17, 2]) == bool(ds.gat_hash(77, 17, 2) >= np.uint32(ds.drop_below(0.3)))
    assert not np.array_equal(keep[:, 0], keep[:, 1])


def keep_share_within_6_sigma(bits, p):
    """The conditions the GPU tests impose on a [rows, cols] array of keep bits: whole-tensor share and every column's share within
    6 sigma of 1 - p, sigma = sqrt(p (1 - p) / n) (caps from the binomial distribution, not measurements)."""
    whole = abs(bits.mean() - (1 - p)) < 6 * (p * (1 - p) / bits.size) ** 0.5
    cols = np.abs(bits.mean(0) - (1 - p)).max() < 6 * (p * (1 - p) / bits.shape[0]) ** 0.5
    return bool(whole and cols)


@pytest.mark.parametrize("p", PS)
def test_restatement_meets_the_keep_share_conditions(p):
    for seed, offset in POSITIONS:
        bits = ds.relu_dropout_keep(seed, offset, ROWS * COLS // 4, p).reshape(ROWS, COLS)
        assert keep_share_within_6_sigma(bits, p), (p, seed, offset)


def test_mask_bytes_and_reference_on_special_values():
    x = np.tile(SPECIALS, 4)[:24].reshape(6, 4).copy()
    keep = np.ones((6, 4), bool)
    keep[3:] = False
    m = ds.mask_bytes(keep, x)
    pos = ds.relu_positive(x)
    assert pos.tolist() == [[v in (2, 3, 5) for v in (np.arange(4 * r, 4 * r + 4) % 6)] for r in range(6)]  # denormal, +Inf, NaN
    assert m[3:].tolist() == [0, 0, 0] and m[0] == 4 + 8 and np.array_equal(ds.mask_bits(m, x.shape), keep & pos)


# ------------------------------------------------------------------------------------------------------------------ the GPU part
gpu = pytest.mark.gpu


def backend():
    from mi355x_graph import sparse
    return sparse.backend_for(torch.zeros(1, device=DEV))


@functools.lru_cache(maxsize=None)
def host_matrix(rows, cols, seed):
    return np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32)  # shared: callers copy before they write


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(t, a):
    """Bit-for-bit equality of a device tensor with a host array without NaNs."""
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


def check_forward_backward(x, p, seed, offset, y, mask, what):
    """y and the mask bytes against the restatement of (seed, offset); then dx of a fixed dy under that mask."""
    want_y, want_m = ds.relu_dropout_reference(x, seed, offset, p)
    assert same(mask, want_m), ("mask",) + what
    assert same(y, want_y), ("y",) + what
    dy = host_matrix(x.shape[0], x.shape[1], 4321)
    dx = backend().relu_dropout_bwd(dev(dy), mask, p)
    assert same(dx, np.where(ds.mask_bits(want_m, x.shape), dy * ds.keep_scale(p), np.float32(0.0)).astype(np.float32)), ("dx",) + what


@gpu
@pytest.mark.parametrize("p,seed,offset",
                         [(p, s, o) for p in PS for s, o in POSITIONS]
                         + [(0.5, 12345, 2 ** 63 - 3), (0.5, 12345, 2 ** 62 + 1), (0.0, 12345, 777), (P_LAST, 12345, 777)])
def test_dense_forward_draws_the_restated_mask(p, seed, offset):
    """mgx_relu_dropout_fwd on 256 x 64: three p at three stream positions, offsets at which (offset + i) * 2 passes 2^64 / 2^63
    inside the tensor, and the ends of the admitted range of p (0: relu alone; the last float32 below 1: scale 2^24)."""
    x = host_matrix(ROWS, COLS, 11)
    y, mask = backend().relu_dropout_fwd(dev(x), p, seed, offset)
    check_forward_backward(x, p, seed, offset, y, mask, (p, seed, offset))
    if p in PS and (seed, offset) in POSITIONS:  # the bits alone (an all-positive input): exact, and within the binomial caps
        _, bits = backend().relu_dropout_fwd(torch.ones(ROWS, COLS, device=DEV), p, seed, offset)
        got = ds.mask_bits(bits.cpu().numpy(), (ROWS, COLS))
        assert np.array_equal(got, ds.relu_dropout_keep(seed, offset, ROWS * COLS // 4, p).reshape(ROWS, COLS))
        assert keep_share_within_6_sigma(got, p)
    if p == 0.0:
        assert same(y, np.maximum(x, np.float32(0.0)))


@gpu
def test_second_trip_of_the_grid_stride_loop():
    """The launch is capped at 256 * 32 blocks of kBlock threads: 1000 float4s more than one trip covers.  The whole mask and y,
    and separately the part behind the first trip, so that a failure names the loop."""
    text = open(os.path.join(ROOT, "dgl-0.5-benchmark_amd", "csrc", "common.h")).read()
    k_block = int(re.search(r"constexpr int kBlock = (\d+);", text).group(1))
    first = 256 * 32 * k_block
    n4 = first + 1000
    x = np.random.default_rng(3).standard_normal(4 * n4).astype(np.float32)
    p, seed, offset = 0.5, 2 ** 64 - 1, ds.call_offset(2)
    y, mask = backend().relu_dropout_fwd(dev(x), p, seed, offset)
    want_y, want_m = ds.relu_dropout_reference(x, seed, offset, p)
    y, mask = y.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(mask[:first], want_m[:first]) and np.array_equal(y[:4 * first], want_y[:4 * first]), "first trip"
    assert np.array_equal(mask[first:], want_m[first:]) and np.array_equal(y[4 * first:], want_y[4 * first:]), "second trip of the loop"
    assert 400 < int((mask[first:] != 0).sum()) <= 1000  # the tail was written, not left as it was


@gpu
@pytest.mark.parametrize("cols", [4, 64, 100])
def test_strided_forward_is_keyed_by_the_dense_element_number(cols):
    """x a row-strided view, `out` a column block of a wider matrix, x_stride != y_stride: mask and values of the dense call."""
    rows, p, seed, offset = 37, 0.5, 12345, 777
    x = host_matrix(rows, cols, 5 + cols)
    wide_x = torch.full((rows, cols + 8), -3.0, device=DEV)
    wide_x[:, 4:4 + cols] = dev(x)
    wide_y = torch.full((rows, 2 * cols + 8), 7.0, device=DEV)
    xv, out = wide_x[:, 4:4 + cols], wide_y[:, cols:2 * cols]
    assert xv.stride(0) != out.stride(0) and not xv.is_contiguous()
    y, mask = backend().relu_dropout_fwd(xv, p, seed, offset, out=out)
    assert y.data_ptr() == out.data_ptr()
    check_forward_backward(x, p, seed, offset, y, mask, (cols,))
    assert bool((wide_y[:, :cols] == 7.0).all()) and bool((wide_y[:, 2 * cols:] == 7.0).all())


@gpu
@pytest.mark.parametrize("value", [1 << 20, (1 << 20) + 1, (1 << 62) + 12345, -3])
def test_counter_form_reads_its_offset_from_the_device(value):
    """mgx_relu_dropout_fwd_counter, run eagerly: offset = (counter * 0x9E3779B97F4A7C15 mod 2^64) mod 2^63, the `offset` argument
    is ignored.  1 << 20 is where ops._capture_counter starts; every product here passes 2^64; -3 is 2^64 - 3 to the kernel."""
    x = host_matrix(ROWS, COLS, 11)
    p, seed = 0.5, 2 ** 64 - 1
    counter = torch.full((1,), value, dtype=torch.int64, device=DEV)
    y, mask = backend().relu_dropout_fwd(dev(x), p, seed, 999, counter=counter)
    assert int(counter) == value
    check_forward_backward(x, p, seed, ds.counter_offset(value), y, mask, (value,))


@gpu
def test_operator_calls_walk_the_stream_and_backward_zeroes_behind_cleared_bits():
    """ops.relu_dropout after torch.manual_seed(s) with the call counter at 0: calls 0, 1, 2 draw the masks of call_offset(0 .. 2)
    under seed torch.initial_seed().  Backward: where(bit, dy * scale, 0) exactly -- +Inf and NaN in dy behind cleared bits give 0."""
    from mi355x_graph import ops
    p = 0.5
    x = host_matrix(ROWS, COLS, 11)
    held = ops.ReluDropout._calls
    try:
        torch.manual_seed(2024)
        ops.ReluDropout._calls = 0
        seed = torch.initial_seed() & ds.M64
        assert seed == 2024
        for k in range(3):
            xg = dev(x).requires_grad_(True)
            y = ops.relu_dropout(xg, p, True)
            want_y, want_m = ds.relu_dropout_reference(x, seed, ds.call_offset(k), p)
            assert same(y.detach(), want_y), k
            bits = ds.mask_bits(want_m, x.shape)
            dy = host_matrix(ROWS, COLS, 4321).copy()
            clear = np.flatnonzero(~bits.ravel())
            dy.ravel()[clear[0::3]] = np.inf
            dy.ravel()[clear[1::3]] = np.nan
            y.backward(dev(dy))
            with np.errstate(invalid="ignore"):
                want = np.where(bits, dy * ds.keep_scale(p), np.float32(0.0)).astype(np.float32)
            assert not np.isnan(want).any() and same(xg.grad, want), k
        assert ops.ReluDropout._calls == 3
    finally:
        ops.ReluDropout._calls = held


def bits_equal_nan(got, a):
    """NaN where NaN is expected, every other element bit for bit (signed zeros included)."""
    got, a = np.ascontiguousarray(got), np.ascontiguousarray(a)
    nan = np.isnan(a)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], a.view(np.uint32)[~nan])


def same_with_nan(t, a):
    """As same(), for arrays with NaNs."""
    return bits_equal_nan(t.cpu().numpy(), a)


@gpu
def test_special_values_dense_producer():
    """-0, +0, a denormal, +Inf, -Inf and NaN, each at a kept and at a dropped position of the stream.  A NaN at a kept position is
    NaN with its mask bit SET (the backward passes dy * scale there), at a dropped position 0 with a clear bit; zeros and -Inf are
    0 with a clear bit either way; the denormal and +Inf are positive values."""
    p, seed, offset = 0.5, 12345, 777
    x = host_matrix(ROWS, COLS, 11).copy()
    keep = ds.relu_dropout_keep(seed, offset, x.size // 4, p).ravel()
    kept, dropped = np.flatnonzero(keep)[100:100 + 6], np.flatnonzero(~keep)[100:100 + 6]
    x.ravel()[kept] = SPECIALS
    x.ravel()[dropped] = SPECIALS
    y, mask = backend().relu_dropout_fwd(dev(x), p, seed, offset)
    want_y, want_m = ds.relu_dropout_reference(x, seed, offset, p)
    assert same(mask, want_m) and same_with_nan(y, want_y)
    got, bits = y.cpu().numpy().ravel(), ds.mask_bits(mask.cpu().numpy(), x.shape).ravel()
    assert bits[kept].tolist() == [False, False, True, True, False, True] and not bits[dropped].any()
    assert np.isnan(got[kept[5]]) and got[kept[3]] == np.inf and got[kept[2]] == np.float32(1e-40) * np.float32(2.0)
    assert np.array_equal(got[dropped].view(np.uint32), np.zeros(6, np.uint32))  # +0.0, whatever was dropped
    assert np.array_equal(got[kept[[0, 1, 4]]].view(np.uint32), np.zeros(3, np.uint32))
    dy = host_matrix(ROWS, COLS, 4321)
    dx = backend().relu_dropout_bwd(dev(dy), mask, p).cpu().numpy().ravel()
    assert dx[kept[5]] == dy.ravel()[kept[5]] * np.float32(2.0) and dx[dropped[5]] == 0.0


@gpu
def test_special_values_rows_gemm_epilogue():
    """The same rule in the activation epilogue of mgx_rows_gemm: a NaN row of A gives a row that is NaN at its kept positions (bits
    set) and 0 at the dropped ones; rows of zeros in A pass the bias -- which holds the special values -- to the activation alone.
    Mask and values are the restatement applied to the product mgx_rows_gemm stores for the same operands."""
    be = backend()
    n, K, M = 301, 128, 64
    p, seed, offset = 0.5, 12345, 777
    a = host_matrix(n, K, 21).copy()
    w, bias = host_matrix(M, K, 22), host_matrix(1, M, 23)[0].copy()
    zero_rows, nan_row = np.arange(40, 56), 77
    a[zero_rows] = 0.0
    a[nan_row, 5] = np.nan
    bias[8:20] = np.tile(SPECIALS, 2)
    z = be.rows_gemm(dev(a), dev(w), b_transposed=True, bias=dev(bias))
    zh = z.cpu().numpy()
    assert np.isnan(zh[nan_row]).all() and int(np.isnan(zh).sum()) == M + 2 * (n - 1)  # (the bias carries NaN into two columns)
    assert bits_equal_nan(zh[zero_rows][:, 8:20], np.tile(bias[8:20] + np.float32(0.0), (zero_rows.size, 1)))
    wide = torch.full((n, 2 * M), 7.0, device=DEV)
    y, mask = be.rows_gemm_relu_dropout(dev(a), dev(w), True, dev(bias), p, seed, offset, out=wide[:, M:])
    want_y, want_m = ds.relu_dropout_reference(zh, seed, offset, p)
    assert same(mask, want_m) and same_with_nan(y, want_y) and bool((wide[:, :M] == 7.0).all())
    y2, mask2 = be.relu_dropout_fwd(z, p, seed, offset)  # the two producers: the same bits as each other
    assert torch.equal(mask, mask2) and same_with_nan(y2, want_y)
    keep = ds.relu_dropout_keep(seed, offset, n * M // 4, p).reshape(n, M)
    got, bits = y.cpu().numpy(), ds.mask_bits(mask.cpu().numpy(), (n, M))
    assert np.array_equal(np.isnan(got[nan_row]), keep[nan_row]) and np.array_equal(bits[nan_row], keep[nan_row])
    assert 16 < int(keep[nan_row].sum()) < 48 and np.array_equal(got[nan_row][~keep[nan_row]].view(np.uint32), np.zeros(int((~keep[nan_row]).sum()), np.uint32))
    for j, positive in enumerate([False, False, True, True, False, True]):  # every special value met a kept and a dropped position
        cols = [8 + j, 14 + j]
        k = keep[zero_rows][:, cols]
        assert k.any() and not k.all()
        assert np.array_equal(bits[zero_rows][:, cols], k & positive)


@gpu
def test_sparsity_consumers_count_nan_as_nonzero():
    """What derives sparsity from an activation treats NaN as a value, never as a zero: mgx_row_nonzero_bits, mgx_rows_slots_pack and
    mgx_rows_pack_count (dist.SparseHalo's bitmaps) all test `!= 0`."""
    be = backend()
    x = torch.zeros(40, 64, device=DEV)
    x[3, 9] = float("nan")
    words = be.row_nonzero_bits(x).cpu().numpy().view(np.uint32)
    assert words.tolist() == [1 << 3, 0]
    slots, overflow = be.rows_slots_pack(x)
    s = slots.cpu().numpy().view(np.uint32)
    assert int(overflow) == 0 and s[3, 0] == 0x00404009 and np.isnan(s[3, 1:2].view(np.float32)[0])  # column 9 in group 0, its value
    assert (s[np.arange(40) != 3, 0] == 0x00404040).all()
    assert be.rows_pack_supported(x)
    masks, counts = be.rows_pack_count(x, None)
    assert counts.cpu().numpy().tolist() == [1 if r == 3 else 0 for r in range(40)] and int(masks[3, 0]) != 0


# ---- attention dropout of the fused GAT row kernels
GAT_N = 300
SLOPE = 0.2


@functools.lru_cache(maxsize=None)
def gat_edges():
    """~300 nodes: hubby_graph's random part, a destination and a source of 700 edges (above the plan's split threshold of 256, so
    hub chunks run in both CSRs; 700 edges among 300 nodes are parallel edges by themselves), five more parallel copies of one
    edge, nodes 0 .. 4 without in-edges -- and the edge list SHUFFLED, so that neither CSR holds the edges in id order."""
    from test_gat_fused import hubby_graph
    src, dst = hubby_graph(GAT_N, 12 * GAT_N, seed=3, hub_deg=700)
    src, dst = np.concatenate([src, np.full(5, 3)]), np.concatenate([dst, np.full(5, 20)])
    perm = np.random.default_rng(9).permutation(src.shape[0])
    src, dst = src[perm], dst[perm]
    assert not np.isin(dst, np.arange(5)).any()
    return src, dst


def gat_reference(src, dst, feat, attn, el, er, keep, p, w, grads=True):
    """fp64: out[v,h,:] = sum_e keep[e,h] / (1 - p) softmax_v(leaky_relu(el[u] + er[v]))[e,h] feat[u,h,:] and the gradients of
    <out, w> by autograd.  attn given: el = <feat, attn> is part of the expression (its gradient flows into feat and attn)."""
    n, H = feat.shape[0], feat.shape[1]
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    feat = torch.from_numpy(feat).double().requires_grad_(grads)
    er = torch.from_numpy(er).double().requires_grad_(grads)
    if attn is not None:
        first = torch.from_numpy(attn).double().requires_grad_(grads)
        el2 = (feat * first).sum(-1)
    else:
        first = torch.from_numpy(el).double().requires_grad_(grads)
        el2 = first.view(n, H)
    z = torch.nn.functional.leaky_relu(el2[s] + er.view(n, H)[d], SLOPE)
    top = torch.full((n, H), -np.inf, dtype=torch.float64).scatter_reduce(0, d.view(-1, 1).expand(-1, H), z.detach(), "amax")
    ex = torch.exp(z - top[d])
    a = ex / torch.zeros(n, H, dtype=torch.float64).index_add(0, d, ex)[d]
    a = a * torch.from_numpy(keep).double() / (1.0 - p)
    out = torch.zeros(feat.shape, dtype=torch.float64).index_add(0, d, a.unsqueeze(-1) * feat[s])
    if not grads:
        return [out]
    (out * torch.from_numpy(w).double()).sum().backward()
    return [out.detach(), feat.grad, first.grad, er.grad]


@gpu
@pytest.mark.parametrize("p", [0.3, 0.6])
@pytest.mark.parametrize("H,Fd,elk", [(1, 4, False), (8, 8, False), (4, 16, False), (2, 64, False), (8, 16, True)],
                         ids=["1x4-lph1", "8x8-lph2", "4x16-lph4-quad", "2x64-lph16-quad", "8x16-el-in-kernel"])
def test_gat_row_kernels_draw_the_restated_mask(H, Fd, elk, p, monkeypatch):
    """The row form of gat_fused with attn_drop against fp64 with keep = gat_edge_keep(gat_call_seed(seed, k), E, H, p): outputs and
    the gradients of feat, el (attn_l in the el-in-kernel case) and er, for call 0 and call 1 of a seeded run; at H > 1 the
    reference with the NEXT head's mask must NOT match, so a head-blind mask would be seen.  Tolerance: test_gat_fused.RTOL (1e-4)
    of each tensor's largest magnitude; the measured maxima against fp64 are printed before the assertion (on an MI355X: at most
    2.4e-7 for out, 6.2e-7 for d_feat, 6.6e-7 for d_el / d_attn_l and 1.3e-6 for d_er over all cases)."""
    from mi355x_graph import ops
    from test_gat_fused import RTOL, mk
    monkeypatch.setenv("MGX_GAT_TILE", "0")
    src, dst = gat_edges()
    E, n = src.shape[0], GAT_N
    g = mk(n, n, src, dst)
    rng = np.random.default_rng(H * 100 + Fd)
    feat = rng.standard_normal((n, H, Fd)).astype(np.float32)
    attn = (rng.standard_normal((1, H, Fd)) * 0.5).astype(np.float32) if elk else None
    el = rng.standard_normal((n, H, 1)).astype(np.float32)
    er = rng.standard_normal((n, H, 1)).astype(np.float32)
    w = rng.standard_normal((n, H, Fd)).astype(np.float32)
    held = ops.GATFused._calls
    try:
        torch.manual_seed(31)
        ops.GATFused._calls = 0
        for k in range(2):
            f_, r_ = dev(feat).requires_grad_(True), dev(er).requires_grad_(True)
            if elk:
                first = dev(attn).requires_grad_(True)
                out = ops.gat_fused(g, f_, (f_ * first).sum(-1, keepdim=True), r_, SLOPE, p, True, attn_l=first)
            else:
                first = dev(el).requires_grad_(True)
                out = ops.gat_fused(g, f_, first, r_, SLOPE, p, True)
            assert out.grad_fn.backward_cache[-1] == "row"
            (out * dev(w)).sum().backward()
            got = [out.detach(), f_.grad, first.grad, r_.grad]
            keep = ds.gat_edge_keep(ds.gat_call_seed(31, k), E, H, p)
            want = gat_reference(src, dst, feat, attn, el, er, keep, p, w)
            for name, a_, b_ in zip(("out", "d_feat", "d_attn_l" if elk else "d_el", "d_er"), got, want):
                err, scale = float((a_.cpu().double() - b_.view(a_.shape)).abs().max()), float(b_.abs().max())
                print("gat row form H=%d F=%d p=%g call %d %s: max err %.3g of scale %.3g = %.3g relative" % (H, Fd, p, k, name, err, scale, err / scale))
                assert err <= RTOL * scale, (name, k, err, scale)
            assert bool((got[0][:5] == 0).all())  # rows without in-edges
            if H > 1:
                other = gat_reference(src, dst, feat, attn, el, er, np.roll(keep, -1, axis=1), p, w, grads=False)[0]
                assert float((got[0].cpu().double() - other).abs().max()) > 100 * RTOL * float(other.abs().max()), "a head-blind mask would pass"
        assert ops.GATFused._calls == 2
    finally:
        ops.GATFused._calls = held
    csc, csr = g._index.csc(), g._index.csr()
    assert not (isinstance(csc._tile_plan, dict) and "gat" in csc._tile_plan), "the tile walk was taken"
    for c in (csc, csr):  # edge ids are a real permutation, and a hub chunk ran, in both CSRs
        assert c.eids is not None and not torch.equal(c.eids.cpu().long(), torch.arange(E))
        assert c.plan() is not None and c.plan().num_slots > 0
