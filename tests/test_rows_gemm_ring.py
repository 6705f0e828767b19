"""mgx_rows_gemm (csrc/rowsgemm.hip) at the sizes where its rolling operand buffer and the staged loads of contiguous unaligned
rows can go wrong: a wave with zero, one, two and three tiles, ragged last tiles, a tile that would receive another tile's chunk,
K = 47 through the staged and through the row-strided loads.  S = the rows one sweep of the grid covers, asked from the library."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-0.5-benchmark_amd"))
import mi355x_graph as mg  # noqa: E402,F401
from mi355x_graph import sparse  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (K, M, B transposed): forward layers 1 and 2, backward layers 2 and 3 of the products model
SHAPES = [(200, 64, True), (128, 64, True), (64, 128, False), (47, 128, False)]
ROWS = {"1": lambda S: 1, "15": lambda S: 15, "16": lambda S: 16, "17": lambda S: 17, "129": lambda S: 129, "S-1": lambda S: S - 1,
        "S+1": lambda S: S + 1, "S+16*8+3": lambda S: S + 16 * 8 + 3, "2S+17": lambda S: 2 * S + 17}
P, SEED, OFFSET = 0.3, 12345, 777


def backend():
    return sparse.backend_for(torch.zeros(1, device=DEV))


def sweep(K, M, act):
    S = backend().rows_gemm_sweep_rows(K, M, K, act)
    assert S > 0 and S % 128 == 0, (K, M, act, S)   # whole workgroups of 8 waves x 16 rows
    return S


@functools.lru_cache(maxsize=2)
def problem(K, M, bt):
    """The longest matrix any case of this shape needs, and its fp64 product: computed once, shared, never written."""
    n = 2 * max(sweep(K, M, False), sweep(K, M, True)) + 17
    gen = torch.Generator(device=DEV).manual_seed(K * 1000 + M)
    a = torch.randn(n, K, device=DEV, generator=gen)
    b = torch.randn((M, K) if bt else (K, M), device=DEV, generator=gen)
    bias = torch.randn(M, device=DEV, generator=gen)
    rs = torch.rand(n, device=DEV, generator=gen) + 0.25
    bd = b.double().t() if bt else b.double()
    ref = a.double() @ bd + bias.double()
    bound = a.double().abs() @ bd.abs() + bias.double().abs()
    return a, b, bias, rs, ref, bound


def mask_bits(mask, n, M):
    shifts = torch.arange(4, device=mask.device, dtype=torch.uint8)
    return ((mask.view(n, M // 4, 1) >> shifts) & 1).view(n, M).bool()


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("act", [False, True], ids=["plain", "relu_dropout"])
@pytest.mark.parametrize("K,M,bt", SHAPES)
def test_row_counts_match_fp64_and_rerun_bitwise(K, M, bt, act, rows):
    be = backend()
    a, b, bias, rs, ref, bound = problem(K, M, bt)
    n = ROWS[rows](sweep(K, M, act))
    a = a[:n]
    ref, bound = ref[:n], bound[:n]
    if act:
        y, mask = be.rows_gemm_relu_dropout(a, b, bt, bias, P, SEED, OFFSET)
        y2, mask2 = be.rows_gemm_relu_dropout(a, b, bt, bias, P, SEED, OFFSET)
        assert torch.equal(y, y2) and torch.equal(mask, mask2)
        keep = mask_bits(mask, n, M)
        scale = 1.0 / (1.0 - P)
        err = (y.double() - torch.where(keep, ref, torch.zeros_like(ref)) * scale).abs()
        assert bool((err <= 1e-5 * bound * scale + 1e-30).all()), (K, M, n, float((err / (bound + 1e-30)).max()))
        assert bool((ref[keep] >= -1e-5 * bound[keep]).all())           # only positive pre-activations are kept
        assert 0.2 < float(keep.float().mean()) < 0.5 or n < 64           # about (1 - p) / 2
    else:
        sf = M // 2
        out = be.rows_gemm(a, b, b_transposed=bt, bias=bias, row_scale=rs[:n], scale_from=sf)
        assert torch.equal(out, be.rows_gemm(a, b, b_transposed=bt, bias=bias, row_scale=rs[:n], scale_from=sf))
        ref, bound = ref.clone(), bound.clone()
        ref[:, sf:] *= rs[:n].double().view(-1, 1)
        bound[:, sf:] *= rs[:n].double().view(-1, 1)
        err = (out.double() - ref).abs()
        assert bool((err <= 1e-5 * bound + 1e-30).all()), (K, M, n, float((err / (bound + 1e-30)).max()))


@pytest.mark.parametrize("act", [False, True], ids=["plain", "relu_dropout"])
@pytest.mark.parametrize("K,M,bt", SHAPES)
def test_rows_do_not_depend_on_their_position(K, M, bt, act):
    """Rows [s, e) of the product of the whole matrix == the product of those rows alone (they sit in other tiles of other waves
    there): a tile that received a chunk of another tile would differ."""
    be = backend()
    a, b, bias, rs, _, _ = problem(K, M, bt)
    S = sweep(K, M, act)
    s, e = S + 48, 2 * S + 5
    assert s % 16 == 0 and e % 16 != 0 and e <= a.shape[0]
    if act:
        whole, wmask = be.rows_gemm_relu_dropout(a, b, bt, bias, P, SEED, OFFSET)
        part, pmask = be.rows_gemm_relu_dropout(a[s:e], b, bt, bias, P, SEED, OFFSET + s * (M // 4))   # the same random stream positions
        assert torch.equal(wmask[s * (M // 4):e * (M // 4)], pmask)
    else:
        whole = be.rows_gemm(a, b, b_transposed=bt, bias=bias, row_scale=rs, scale_from=M // 2)
        part = be.rows_gemm(a[s:e], b, b_transposed=bt, bias=bias, row_scale=rs[s:e], scale_from=M // 2)
    assert torch.equal(whole[s:e], part)


def test_k47_staged_loads_equal_row_strided_loads_bitwise():
    be = backend()
    K, M = 47, 128
    a, b, bias, rs, _, _ = problem(K, M, False)
    n = sweep(K, M, False) + 16 * 8 + 3
    wide = torch.zeros(n, 56, device=DEV)
    wide[:, :K] = a[:n]
    assert a[:n].is_contiguous() and a.data_ptr() % 16 == 0 and wide[:, :K].stride(0) == 56
    staged = be.rows_gemm(a[:n], b, bias=bias, row_scale=rs[:n], scale_from=M // 2)
    strided = be.rows_gemm(wide[:, :K], b, bias=bias, row_scale=rs[:n], scale_from=M // 2)
    assert torch.equal(staged, strided)


def test_k47_misaligned_matrix_matches_fp64():
    be = backend()
    K, M = 47, 128
    a, b, bias, _, ref, bound = problem(K, M, False)
    n = sweep(K, M, False) + 16 * 8 + 3
    flat = torch.zeros(n * K + 4, device=DEV)
    view = flat[1:1 + n * K].view(n, K)
    view.copy_(a[:n])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    out = be.rows_gemm(view, b, bias=bias)
    err = (out.double() - ref[:n]).abs()
    assert bool((err <= 1e-5 * bound[:n] + 1e-30).all()), float((err / (bound[:n] + 1e-30)).max())
    assert torch.equal(out, be.rows_gemm(a[:n], b, bias=bias))   # the same sums whichever loads fetched the rows


@pytest.mark.parametrize("n", [5, 16 * 9 + 5, 16 * 8 * 3 + 15])
def test_k47_ragged_last_tile_reads_no_row_beyond_n(n):
    """A as the last rows of its allocation, and A followed by a row of NaN: the rows of the last, ragged tile come out as from a
    matrix of their own, so nothing beyond row n was taken for one of them."""
    be = backend()
    K, M = 47, 128
    a, b, bias, _, ref, bound = problem(K, M, False)
    alone = be.rows_gemm(a[:n].clone(), b, bias=bias)
    err = (alone.double() - ref[:n]).abs()
    assert bool((err <= 1e-5 * bound[:n] + 1e-30).all())
    tail = torch.full((16 + n, K), float("nan"), device=DEV)   # [16 rows of NaN | A]: A ends where the allocation ends
    tail[16:] = a[:n]
    head = torch.full((n + 1, K), float("nan"), device=DEV)    # [A | one row of NaN]
    head[:n] = a[:n]
    for view in (tail[16:], head[:n]):
        assert view.is_contiguous() and view.data_ptr() % 16 == 0
        out = be.rows_gemm(view, b, bias=bias)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, alone)
