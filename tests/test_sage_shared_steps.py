"""The host-side steps every form of the SAGE layer over a CatBuffer shares (mi355x_graph.ops): the resident input and the generation
check of CatBuffer, the cache of what is derived from a row list, and the position in the dropout stream.  Plain torch on CPU tensors."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dgl-0.5-benchmark_amd")
sys.path.insert(0, PKG)
from mi355x_graph import DGLError, config, ops  # noqa: E402

N, K = 12, 4
SENTINEL = -7.0


def _copied(cat, h):
    """take_input(h) with a sentinel in the left half beforehand: True when h was copied over it, False when it still stands there"""
    cat.left.fill_(SENTINEL)
    before = cat.generation
    with torch.no_grad():  # as inside an autograd node's forward
        cat.take_input(h)
    assert cat.generation == before + 1
    if torch.equal(cat.left, h.detach()):
        return True
    assert bool((cat.left == SENTINEL).all())
    return False


def test_an_input_elsewhere_is_copied_once_and_again_after_a_write():
    cat = ops.CatBuffer(N, K, "cpu")
    h = torch.rand(N, K)
    assert not cat.is_resident(h)
    assert _copied(cat, h)
    assert cat.is_resident(h) and cat.static_key[0] is h
    assert not _copied(cat, h)            # the same object at the same version
    assert not _copied(cat, h)
    h.add_(1.0)
    assert not cat.is_resident(h)
    assert _copied(cat, h)                # written in place since
    assert not _copied(cat, h)
    other = h.clone()                     # equal values, another object
    assert _copied(cat, other)
    assert _copied(cat, h)
    assert cat.generation == 7


def test_an_input_that_takes_a_gradient_is_copied_every_time():
    cat = ops.CatBuffer(N, K, "cpu")
    h = torch.rand(N, K, requires_grad=True)
    assert _copied(cat, h) and cat.static_key is None
    assert _copied(cat, h) and cat.static_key is None
    const = torch.rand(N, K)
    assert _copied(cat, const) and not _copied(cat, const)
    assert _copied(cat, h) and cat.static_key is None   # ... and it is not remembered in place of the constant one
    assert _copied(cat, const)


def test_without_the_static_switch_every_pass_copies(monkeypatch):
    monkeypatch.setattr(config, "SAGE_STATIC_CAT", False)
    cat = ops.CatBuffer(N, K, "cpu")
    h = torch.rand(N, K)
    assert _copied(cat, h) and _copied(cat, h) and _copied(cat, h)
    assert cat.generation == 3


def test_the_left_half_itself_is_never_copied():
    cat = ops.CatBuffer(N, K, "cpu")
    h = cat.left
    assert cat.holds(h)
    for expect in (1, 2):
        cat.left.fill_(SENTINEL)
        cat.take_input(h)
        assert cat.generation == expect and bool((cat.left == SENTINEL).all()) and cat.static_key is None


def test_a_second_forward_pass_fails_the_generation_check():
    cat = ops.CatBuffer(N, K, "cpu")
    h = torch.rand(N, K)
    cat.take_input(h)
    saved = cat.generation
    cat.check_generation(saved)
    cat.take_input(h)
    with pytest.raises(DGLError, match="SAGE_CAT") as e:
        cat.check_generation(saved)
    assert "MGX_" not in str(e.value)
    cat.check_generation(cat.generation)


@pytest.fixture
def row_caches():
    saved = [(c, dict(c)) for c in (ops._ROW_BITS, ops._ROW_INV_DEG, ops._ROW_POS)]
    for c, _ in saved:
        c.clear()
    yield
    for c, was in saved:
        c.clear()
        c.update(was)


def test_row_positions_are_kept_per_list_object_and_version(row_caches):
    rows = torch.tensor([5, 0, 3], dtype=torch.int64)
    pos = ops._row_pos(rows, 7)
    assert pos.tolist() == [1, -1, -1, 2, -1, 0, -1]
    assert ops._row_pos(rows, 7) is pos
    assert ops._row_pos(rows, 8) is not pos and ops._row_pos(rows, 8).shape[0] == 8
    assert ops._row_pos(rows, 7) is pos                     # another N is another entry, not a replacement
    rows[0] = 6                                             # written in place: same address, next version
    again = ops._row_pos(rows, 7)
    assert again is not pos and again.tolist() == [1, -1, -1, 2, -1, -1, 0]
    twin = rows.clone()                                     # an equal list in another tensor object
    assert ops._row_pos(twin, 7) is not again and torch.equal(ops._row_pos(twin, 7), again)
    assert ops._row_pos(rows, 7) is again


def test_row_factors_also_depend_on_the_identity_of_the_degree_vector(row_caches):
    rows = torch.tensor([4, 1], dtype=torch.int64)
    inv = torch.tensor([1.0, 0.5, 0.25, 0.125, 0.0625])
    got = ops._row_inv_deg(rows, inv)
    assert got.tolist() == [0.0625, 0.5]
    assert ops._row_inv_deg(rows, inv) is got
    view = inv.view(5)                                      # same address, another object
    assert view.data_ptr() == inv.data_ptr()
    other = ops._row_inv_deg(rows, view)
    assert other is not got and torch.equal(other, got)
    rows[1] = 2
    assert ops._row_inv_deg(rows, view).tolist() == [0.0625, 0.25]


def test_each_row_cache_is_emptied_on_its_own_above_eight_entries(row_caches):
    inv = torch.rand(64)
    lists = [torch.tensor([i, i + 1], dtype=torch.int64) for i in range(30)]
    for i, rows in enumerate(lists):
        ops._row_pos(rows, 64)
        assert 1 <= len(ops._ROW_POS) <= 9
        if i < 5:
            ops._row_inv_deg(rows, inv)
    assert len(ops._ROW_INV_DEG) == 5 and len(ops._ROW_BITS) == 0
    assert ops._row_pos(lists[-1], 64) is ops._row_pos(lists[-1], 64)


def test_the_dropout_stream_advances_by_one_constant_per_call():
    start = ops.ReluDropout._calls
    try:
        torch.manual_seed(77)
        seed_a, a = ops._dropout_stream_position()
        seed_b, b = ops._dropout_stream_position()
        assert ops.ReluDropout._calls == start + 2
        assert seed_a == seed_b == 77
        assert 0 <= a < 2 ** 63 and 0 <= b < 2 ** 63
        assert (b - a) % 2 ** 63 == 0x9E3779B97F4A7C15 % 2 ** 63
        assert a == (start * 0x9E3779B97F4A7C15) % 2 ** 63
    finally:
        ops.ReluDropout._calls = start
