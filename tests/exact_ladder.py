"""Helpers of tests/test_exact_structure.py: the degree-ladder graph and exact (order-independent) comparisons.

Small signed integers stored as fp32 add exactly in ANY association while every partial sum stays below 2^24, so a kernel that
reduces such terms must reproduce an int64 reference bit for bit -- a lost, doubled or misattributed edge of value 1 on a 21 000-edge
row is a mismatch, where a 1e-4 relative bound is blind to it."""
import numpy as np

from mi355x_graph import config

LIMIT = 1 << 24          # below this every integer is an fp32 value, and so is every partial sum of terms whose |.| sum stays below it
BASE_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
                1023, 1024, 1025, 2047, 2048, 2049, 4097]
LONGEST = 21000


def split_thresholds():
    """Every hub threshold in play: the default, the two the fuzz patches in, and the tile kernel's."""
    return sorted({int(config.HUB_SPLIT), 64, 1024, int(config.TILE_HUB_SPLIT)})


def around(S):
    return [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 1]


def min_rows():
    """More rows than one tile of the widest TILE_CONFIG entry (consumers x nacc x rows per step)."""
    return max(c[0] * c[1] * (64 >> lg) for lg, c in config.TILE_CONFIG.items()) + 1


def ladder_lengths(seed=0, repeats=None, thresholds=None, longest=LONGEST, base=None):
    """Row lengths of the ladder graph: the rungs repeated until there are more rows than one tile (and than a 64-row block), shuffled,
    one row of `longest` edges; hub rows first (two adjacent) and last."""
    thresholds = split_thresholds() if thresholds is None else thresholds
    rungs = list(BASE_LENGTHS if base is None else base)
    for S in thresholds:
        rungs += around(S)
    if repeats is None:
        repeats = -(-min_rows() // len(rungs))
    rng = np.random.default_rng(seed)
    lens = np.array(rungs * repeats, np.int64)
    rng.shuffle(lens)
    top = 3 * max(thresholds) + 1
    first = int(np.nonzero(lens == top)[0][0])
    lens = np.delete(lens, first)
    tail = int(np.nonzero(lens == 2 * max(thresholds) + 1)[0][0])
    last = lens[tail]
    lens = np.delete(lens, tail)
    head = [longest, top] if longest else [top]
    return np.concatenate([np.array(head, np.int64), lens, np.array([last], np.int64)])


def ladder_graph(seed=0, bipartite=False, repeats=None, thresholds=None, longest=LONGEST, hub_source_edges=5000, base=None):
    """(src, dst, n_src, n_dst) int64: destination v has ladder_lengths()[v] in-edges, in a shuffled edge order (edge ids are not CSR
    positions); sources are random with duplicates, one source is gathered by `hub_source_edges` edges, the last 40 by nobody."""
    lens = ladder_lengths(seed, repeats, thresholds, longest, base)
    n_dst = int(lens.shape[0])
    n_src = n_dst + 611 if bipartite else n_dst
    rng = np.random.default_rng(seed + 1)
    dst = np.repeat(np.arange(n_dst, dtype=np.int64), lens)
    src = rng.integers(0, n_src - 40, dst.shape[0]).astype(np.int64)
    k = min(hub_source_edges, dst.shape[0] // 4)
    src[rng.choice(dst.shape[0], k, replace=False)] = 3
    perm = rng.permutation(dst.shape[0])
    return src[perm], dst[perm], n_src, n_dst


def ints(rng, shape, bound):
    """Signed integers in [-bound, bound] as fp32, zeros included."""
    return rng.integers(-bound, bound + 1, shape).astype(np.float32)


_sorted = {}


def _by_row(dst, n_dst):
    """(edge order sorted by destination, start of every non-empty row, which rows are non-empty), computed once per edge list."""
    key = (id(dst), n_dst)
    if key not in _sorted or _sorted[key][0] is not dst:
        while len(_sorted) >= 8:                       # a handful of edge lists are live at a time: the oldest entry goes
            _sorted.pop(next(iter(_sorted)))
        counts = np.bincount(dst, minlength=n_dst)
        _sorted[key] = (dst, np.argsort(dst, kind="stable"), (np.cumsum(counts) - counts)[counts > 0], counts > 0)
    return _sorted[key][1:]


def reduce_rows(dst, n_dst, term, D, absolute=False, chunk=32, both=False):
    """out[v, k] = sum over edges e with dst[e] == v of term(columns)[e, k] in int64; term(slice) -> [nnz, len(slice)] integers.
    (np.add.at's result -- test_reduce_rows_is_np_add_at -- computed from the edge list sorted by destination, in column chunks.)
    absolute: the sum of |terms|; both: (sums, sums of |terms|) from one pass."""
    order, starts, live = _by_row(dst, n_dst)
    out = np.zeros((n_dst, D), np.int64)
    mag = np.zeros((n_dst, D), np.int64) if both else None
    if order.shape[0] == 0:
        return (out, mag) if both else out
    for c0 in range(0, D, chunk):
        t = np.asarray(term(slice(c0, min(D, c0 + chunk))))[order].astype(np.int64)
        if both:
            mag[live, c0:c0 + t.shape[1]] = np.add.reduceat(np.abs(t), starts, axis=0)
        elif absolute:
            t = np.abs(t)
        out[live, c0:c0 + t.shape[1]] = np.add.reduceat(t, starts, axis=0)
    return (out, mag) if both else out


def exact_pair(dst, n_dst, term, D, with_mag=False):
    """The int64 sums, after asserting the precondition of a bit-exact comparison: the sum of |terms| of every output element is
    below 2^24 (with_mag: those sums of |terms| too)."""
    out, mag = reduce_rows(dst, n_dst, term, D, both=True)
    assert int(mag.max(initial=0)) < LIMIT, "inputs too large for exact fp32 sums: %d" % int(mag.max())
    return (out, mag) if with_mag else out


def assert_exact(got, want_int, what=""):
    got = np.asarray(got)
    want = want_int.astype(np.float32).reshape(got.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ, first at %s: got %r, want %r" % (what, bad.shape[0], bad[0].tolist(),
                                                                                         got[tuple(bad[0])], want[tuple(bad[0])]))


def mean_of(int_sum, deg):
    shape = (-1,) + (1,) * (int_sum.ndim - 1)
    return int_sum.astype(np.float32) / np.maximum(deg, 1).astype(np.float32).reshape(shape)


def assert_mean(got, int_sum, deg, what=""):
    """An exact numerator and ONE fp32 division or reciprocal-multiply: within 4 ulp of float32(sum) / float32(deg); isolated rows 0."""
    got = np.asarray(got)
    want = mean_of(int_sum, deg).reshape(got.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = err > 4.0 * np.spacing(np.abs(want)).astype(np.float64)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d means beyond 4 ulp, first at %s: got %r, want %r" % (what, int(bad.sum()), list(i), got[i], want[i]))
    assert not got[deg == 0].any(), "%s: isolated rows must be exactly 0" % what


def within_ulp(got, want, ulps):
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)


def old_metric(got, want):
    """The suite's earlier comparison (tests/test_tile_spmm.rel)."""
    a, b = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-5)))


def rank_in_row(dst, key):
    """Rank of every edge among the edges of its destination when those are ordered by `key` (a permutation of the edge ids)."""
    order = np.lexsort((key, dst))
    counts = np.bincount(dst)
    starts = np.cumsum(counts) - counts
    rank = np.empty(dst.shape[0], np.int64)
    rank[order] = np.arange(dst.shape[0]) - np.repeat(starts, counts)
    return rank
