"""mgx_spmm_copy_u_slots_init as a dense INIT walk with a per-edge slot probe (csrc/spmm_slots.inc, spmm_probe_init_kernel): bit patterns
against mgx_spmm_copy_u_strided_init on the same CSR and plan, on a hand-made graph that puts ONE live source at every position of the
predicate that can go wrong -- each lane group, each step of a group's walk, each 64-edge chunk, the 256-edge partials of a split row --
with every other source of that row empty; hub rows whose live sources sit in the last chunk only or nowhere in the first; rows without
edges before, between and after rows with live edges in runs that cover a wave's and a workgroup's whole stretch (the look-ahead over
chunks); the short items of a forced two-part plan with the live edge at each position; two calls on one CSR with the live set swapped;
and live rows of 1, 24 and 25 non-zeros and with Inf / NaN.  A row with a single live source has a result that needs no reference at all:
fl(initial value + that source row)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dgl-0.5-benchmark_amd")
sys.path.insert(0, PKG)
from mi355x_graph import _lib, schedule, sparse  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, D = 4096, 64
DEGS = [1, 4, 15, 16, 17, 63, 64, 65, 129, 256, 257]
POSITIONS = [0, 1, 3, 4, 15, 16, 63, 64]
ZERO_RUNS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 33, 64, 70]   # rows without edges in front of a row with a live edge
HUB_TAIL, HUB_HEAD = 1100, 1030


def _be():
    return sparse.backend_for(torch.zeros(1, device=DEV))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _world():
    """(indptr, indices, single, live_a, live_b): `single` = [(row, position, source)] for the rows with exactly one live source under the
    live set `live_a`; `live_b` is disjoint from it (the swapped set)."""
    rng = np.random.default_rng(23)
    ids = np.arange(N)
    live_a, live_b = ids[ids % 8 == 3], ids[ids % 8 == 5]
    dead = ids[(ids % 8 != 3) & (ids % 8 != 5)]
    specs = []   # (degree, live positions)
    for d in DEGS:
        for p in sorted(set(q for q in POSITIONS + [d - 1] if q < d)):
            specs.append((d, [p]))
    n_long = len(specs)
    for d in range(1, 17):   # the short items of the two-part plan, the live edge at each position
        for p in range(d):
            specs.append((d, [p]))
    rows = []    # per destination row: (degree, live positions, or None = 8 % of the positions at random)
    for i, s in enumerate(specs):
        rows += [(0, [])] * (ZERO_RUNS[i % len(ZERO_RUNS)] if i < n_long else i % 4)
        rows.append(s)
    rows += [(0, [])] * 40
    rows.append((HUB_TAIL, [HUB_TAIL - 1, HUB_TAIL - 2, HUB_TAIL - 5]))                          # live in the last chunk only
    rows.append((HUB_HEAD, sorted(rng.choice(np.arange(300, HUB_HEAD), 200, replace=False))))   # nothing live in the first chunks
    rows += [(0, [])] * 3
    assert len(rows) < N - 200
    fill = [0, 3, 40, 70, 130]
    while len(rows) < N - 17:
        rows.append((fill[int(rng.integers(0, len(fill)))], None))
    rows += [(0, [])] * (N - len(rows))   # the last workgroup's stretch ends in rows without edges
    indptr = np.zeros(N + 1, dtype=np.int64)
    chunks, single = [], []
    for r, (d, live) in enumerate(rows):
        idx = rng.choice(dead, d)
        if live is None:
            live = np.nonzero(rng.random(d) < 0.08)[0]
        for p in live:
            idx[p] = rng.choice(live_a)
        if len(live) == 1:
            single.append((r, int(live[0]), int(idx[live[0]])))
        chunks.append(idx)
        indptr[r + 1] = indptr[r] + d
    assert len(single) >= len(specs)
    return indptr, np.concatenate(chunks), single, live_a, live_b


def _csr(form, indptr, indices):
    csr = sparse.CsrView(N, N, torch.from_numpy(indptr).to(torch.int32).to(DEV), torch.from_numpy(indices).to(torch.int32).to(DEV), None)
    plan = csr.plan()
    assert plan is not None and plan.num_hubs >= 2
    if form == "two-part":   # forced the way tests/test_head_slots.py forces one
        split = schedule.split_short_items(csr, plan, any_share=True, limit=16)
        assert split is not None and split[0].rest is not None
        csr._short = {nb: split[0] for nb in (2, 4, 8, 16, 32, 64)}
        assert csr.spmm_plan_for(D) == (split[0], True)
    else:
        csr._short = {nb: None for nb in (2, 4, 8, 16, 32, 64)}
        assert csr.spmm_plan_for(D) == (plan, False)
    assert csr.tile_plan(D) is None
    return csr


def _source(live, kind):
    """[N, 64], zero outside `live`; live row i holds (1, 5, 24, 25, 64)[i % 5] non-zeros at random columns (valued and flagged slots)."""
    gen = torch.Generator(device=DEV).manual_seed(31)
    dense = torch.randn(N, D, device=DEV, generator=gen)
    dense[dense == 0] = 1.0
    u = torch.zeros(N, D, device=DEV)
    lv = torch.from_numpy(live).to(DEV)
    counts = (1, 24, 25) if kind == "1 / 24 / 25 non-zeros" else (1, 5, 24, 25, 64)
    for i, k in enumerate(counts):
        r = lv[i::len(counts)]
        cols = torch.rand(r.shape[0], D, device=DEV, generator=gen).argsort(dim=1)[:, :k]
        u[r.view(-1, 1), cols] = dense[r.view(-1, 1), cols]
    if kind == "inf and nan":
        # One column per special value, as in tests/test_head_slots.py: +Inf and -Inf never meet in a column, so every NaN of the result
        # has the one bit pattern 0x7fc00000.  Where NaNs of both signs meet, IEEE 754 leaves the result's sign to the operand order of
        # the add instruction, and the dense kernel's own instructions differ in it from one value buffer to the other (measured: six
        # elements 0xffc00000 against 0x7fc00000 with the specials at each row's first non-zero column) -- no property of either sum.
        u[lv[0::3], 3] = float("inf")
        u[lv[1::3], 40] = float("-inf")
        u[lv[2::3], 63] = float("nan")
    return u


@pytest.fixture(scope="module")
def world():
    indptr, indices, single, live_a, live_b = _world()
    gen = torch.Generator(device=DEV).manual_seed(32)
    rows = torch.nonzero(torch.rand(N, device=DEV, generator=gen) < 0.3).flatten()
    rows = rows[torch.randperm(rows.shape[0], device=DEV, generator=gen)].contiguous()   # unsorted, distinct; rows without edges among them
    pos = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    pos[rows] = torch.arange(rows.shape[0], dtype=torch.int64, device=DEV)
    init = torch.randn(rows.shape[0], D, device=DEV, generator=gen)
    deg = np.diff(indptr)
    assert bool((pos[torch.from_numpy(np.nonzero(deg == 0)[0]).to(DEV)] >= 0).any())
    return {"indptr": indptr, "indices": indices, "single": single, "live_a": live_a, "live_b": live_b, "pos": pos, "init": init,
            "csr": {f: _csr(f, indptr, indices) for f in ("natural", "two-part")}}


def _both(w, form, u, slots=None):
    be, csr = _be(), w["csr"][form]
    want = be.spmm_copy_u_strided_init(csr, "sum", u, w["init"], w["pos"], torch.full((N, D), float("nan"), device=DEV))
    assert want is not None and _lib.lib().mgx_last_spmm_kernel() == (b"rowgroup32" if form == "two-part" else b"rowwave32")
    if slots is None:
        slots = be.rows_slots_pack(u)[0]
    got = be.spmm_copy_u_slots_init(csr, "sum", u, slots, w["init"], w["pos"], torch.full((N, D), float("nan"), device=DEV))
    assert got is not None and _lib.lib().mgx_last_spmm_kernel() == b"slots"
    return got, want


@pytest.mark.parametrize("form", ["natural", "two-part"])
def test_one_live_source_at_every_position(world, form):
    """(a), (b), (c), (e): the dense call's bits in every row, and in the rows with one live source the sum that needs no reference."""
    w = world
    u = _source(w["live_a"], "mixed")
    got, want = _both(w, form, u)
    diff = torch.nonzero((_bits(got) != _bits(want)).any(dim=1)).flatten()
    print("%s: %d rows differ" % (form, diff.numel()))
    assert diff.numel() == 0, (form, diff[:10].tolist())
    r = torch.tensor([s[0] for s in w["single"]], device=DEV)
    src = torch.tensor([s[2] for s in w["single"]], device=DEV)
    start = torch.zeros(N, D, device=DEV)
    start[w["pos"] >= 0] = w["init"][w["pos"][w["pos"] >= 0]]
    assert torch.equal(got[r], start[r] + u[src])
    deg = torch.from_numpy(np.diff(w["indptr"])).to(DEV)
    assert torch.equal(got[deg == 0], start[deg == 0])   # a row without edges is its initial value (or +0.0f)


@pytest.mark.parametrize("form", ["natural", "two-part"])
def test_swapped_live_set_on_the_same_csr(world, form):
    """(d): the rows that were live are cleared, others become live, the slots of both lists are packed again; no flag survives."""
    w = world
    be = _be()
    u = _source(w["live_a"], "mixed")
    slots = be.rows_slots_pack(u)[0]
    got, want = _both(w, form, u, slots)
    assert torch.equal(_bits(got), _bits(want))
    la, lb = torch.from_numpy(w["live_a"]).to(DEV), torch.from_numpy(w["live_b"]).to(DEV)
    u.index_fill_(0, la, 0.0)
    u[lb] = _source(w["live_b"], "mixed")[lb]
    be.rows_slots_pack_rows(u, la, slots)
    be.rows_slots_pack_rows(u, lb, slots)
    assert torch.equal(slots, be.rows_slots_pack(u)[0])
    got2, want2 = _both(w, form, u, slots)
    assert torch.equal(_bits(got2), _bits(want2))
    r = torch.tensor([s[0] for s in w["single"]], device=DEV)   # their one source is dead now: the initial value alone
    start = torch.zeros(N, D, device=DEV)
    start[w["pos"] >= 0] = w["init"][w["pos"][w["pos"] >= 0]]
    assert torch.equal(got2[r], start[r])
    assert not torch.equal(_bits(got2), _bits(got))


@pytest.mark.parametrize("kind", ["1 / 24 / 25 non-zeros", "inf and nan"])
@pytest.mark.parametrize("form", ["natural", "two-part"])
def test_slot_capacity_and_specials(world, form, kind):
    """(f): live rows at the slot's capacity from both sides (24 values, 25 = the flag) and live rows that hold Inf / NaN."""
    w = world
    u = _source(w["live_a"], kind)
    if kind == "inf and nan":
        assert bool(torch.isnan(u).any()) and bool(torch.isinf(u).any())
    got, want = _both(w, form, u)
    bad = torch.nonzero(_bits(got) != _bits(want))
    print("%s / %s: %d elements differ" % (form, kind, bad.shape[0]),
          [(int(r), int(c), hex(int(_bits(got)[r, c]) & 0xffffffff), hex(int(_bits(want)[r, c]) & 0xffffffff)) for r, c in bad[:8].tolist()])
    assert bad.shape[0] == 0
    if kind == "inf and nan":
        assert bool(torch.isnan(got).any())
