"""Helpers of tests/test_value_edges.py: the private-source graph, value patterns and plain numpy fp64 references over the COO list.

Every reference here is a function of the fp32 inputs the kernels see: the logit sums and the leaky-relu product are formed in fp32
first (the kernels' own single operations, IEEE-exact), everything after that in fp64."""
import numpy as np

import exact_ladder as xl

ROW_LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000]


# ============================================================================= max / min: the first extremum in storage order wins
def first_extremum(dst, n_dst, term, red):
    """What a strict compare (`>` for max, `<` for min) started from the identity (-inf | +inf) and walked in CSR storage order leaves,
    per (row, column) of term [nnz, K] float32: (values float32, winning edge id, is-a-tie).  The CSR the library builds from COO is
    stable, so storage order inside a row is edge-id order: np.lexsort with the edge id as the final key.  A NaN never wins; a term
    equal to the identity never wins either (the compare never fires): value = identity, arg = -1.  Empty rows: 0, -1.
    tie[v, k]: at least two edges of the row carry the winning value."""
    nnz, K = term.shape
    ident = np.float32(-np.inf if red == "max" else np.inf)
    key = term.astype(np.float64)
    key[np.isnan(key)] = ident
    ranked = -key if red == "max" else key           # ascending: the extremum first; -0.0 and +0.0 compare equal
    counts = np.bincount(dst, minlength=n_dst)
    starts = (np.cumsum(counts) - counts)
    live = counts > 0
    eid = np.arange(nnz)
    val = np.zeros((n_dst, K), np.float32)
    arg = np.full((n_dst, K), -1, np.int64)
    tie = np.zeros((n_dst, K), bool)
    for k in range(K):
        order = np.lexsort((eid, ranked[:, k], dst))
        win = order[starts[live]]
        never = key[win, k] == ident
        val[live, k] = np.where(never, ident, term[win, k])
        arg[live, k] = np.where(never, -1, win)
        best = np.full(n_dst, np.nan)
        best[live] = np.where(never, np.nan, key[win, k])
        tie[:, k] = np.bincount(dst, weights=(key[:, k] == best[dst]).astype(np.float64), minlength=n_dst) >= 2
    return val, arg, tie


def edge_tie_values(dst, n_dst, K, seed, big=50):
    """[nnz, K] integer-valued fp32 with deliberate ties, by row class (row % 5) and by storage rank:
    0: every edge of the row equal; 1: ReLU-like, three quarters zeros and small positives; 2: the row's first and last edge share the
    extremum (the maximum in even columns, the minimum in odd ones), everything between distinct; 3: the extremum on both sides of
    every 64-edge boundary (ranks 63 | 64, 127 | 128, ...; short rows: first and last); 4: integers in [-2, 2]."""
    rng = np.random.default_rng(seed)
    nnz = dst.shape[0]
    rank = xl.rank_in_row(dst, np.arange(nnz))
    lens = np.bincount(dst, minlength=n_dst)[dst]
    cls = dst % 5
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)[None, :]
    out = np.zeros((nnz, K))
    out[:] = ((dst * 7) % 23 - 11)[:, None]                                                   # class 0
    relu = rng.integers(1, 4, (nnz, K)) * (rng.random((nnz, K)) < 0.25)
    out = np.where((cls == 1)[:, None], relu, out)
    inner = np.stack([xl.rank_in_row(dst, rng.permutation(nnz)) for _ in range(K)], 1) % (2 * big - 1) - (big - 1)   # |.| < big
    ends = ((rank == 0) | (rank == lens - 1))[:, None]
    out = np.where((cls == 2)[:, None], np.where(ends, big * sign, inner), out)
    edge64 = ((rank % 64 == 63) & (rank + 1 < lens)) | ((rank % 64 == 0) & (rank > 0))
    both = np.where(lens > 64, edge64, (rank == 0) | (rank == lens - 1))[:, None]
    out = np.where((cls == 3)[:, None], np.where(both, big * sign, inner), out)
    out = np.where((cls == 4)[:, None], rng.integers(-2, 3, (nnz, K)), out)
    return out.astype(np.float32)


def edge_special_values(dst, n_dst, seed):
    """[nnz, 6] fp32 columns of signed zeros, infinities and NaN, by row class:
    0: +0.0 / -0.0 at random; 1: -0.0 first in storage order, +0.0 after it; 2: row % 4 -- one +inf among integers | one -inf among
    integers | all -inf | all +inf; 3: row % 3 -- all NaN | one NaN (the row's first edge when the row is odd) among integers | NaN
    first, then +inf and -inf among integers; 4: all -inf; 5: all NaN."""
    rng = np.random.default_rng(seed)
    nnz = dst.shape[0]
    rank = xl.rank_in_row(dst, np.arange(nnz))
    lens = np.bincount(dst, minlength=n_dst)[dst]
    ints = rng.integers(-5, 6, (nnz, 6)).astype(np.float32)
    pick = (rng.integers(0, 1 << 30, n_dst)[dst] % lens)                 # one rank per row
    out = ints.copy()
    out[:, 0] = np.where(rng.random(nnz) < 0.5, np.float32(0.0), np.float32(-0.0))
    out[:, 1] = np.where(rank == 0, np.float32(-0.0), np.float32(0.0))
    c4 = dst % 4
    out[:, 2] = np.where(c4 == 0, np.where(rank == pick, np.inf, ints[:, 2]),
                         np.where(c4 == 1, np.where(rank == pick, -np.inf, ints[:, 2]), np.where(c4 == 2, -np.inf, np.inf)))
    c3 = dst % 3
    one_nan = np.where(dst % 2 == 1, rank == 0, rank == pick)
    mixed = np.where(rank == 0, np.nan, np.where(rank == 1, np.inf, np.where(rank == 2, -np.inf, ints[:, 3])))
    out[:, 3] = np.where(c3 == 0, np.nan, np.where(c3 == 1, np.where(one_nan, np.nan, ints[:, 3]), mixed))
    out[:, 4] = -np.inf
    out[:, 5] = np.nan
    return out.astype(np.float32)


def node_tie_values(n, K, seed):
    """[n, K + 5] fp32 per-source values for a graph with shared sources: K columns of ties (even: integers in [-2, 2]; odd: ReLU-like,
    three quarters zeros), then signed zeros, a column with a few +-inf / NaN sources, all -inf, all +inf, all NaN."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-2, 3, (n, K + 5)).astype(np.float32)
    relu = (rng.integers(1, 4, (n, K)) * (rng.random((n, K)) < 0.25)).astype(np.float32)
    X[:, 1:K:2] = relu[:, 1:K:2]
    X[:, K] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
    some = rng.permutation(n)
    X[some[:n // 50 + 1], K + 1] = np.inf
    X[some[n // 50 + 1:2 * (n // 50 + 1)], K + 1] = -np.inf
    X[some[2 * (n // 50 + 1):3 * (n // 50 + 1)], K + 1] = np.nan
    X[:, K + 2], X[:, K + 3], X[:, K + 4] = -np.inf, np.inf, np.nan
    return X


# ============================================================================= softmax family
def private_graph(seed=0):
    """(src, dst, n_src, n_dst) with n_src == nnz: every edge has a source of its own, so el[u] is a per-edge logit.  Rows of every
    length in ROW_LENGTHS and three empty rows (first, in the middle, last), in a shuffled edge order."""
    lens = np.array([0] + ROW_LENGTHS[:9] + [0] + ROW_LENGTHS[9:] + [0], np.int64)
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(lens.shape[0], dtype=np.int64), lens)
    dst = dst[rng.permutation(dst.shape[0])]
    src = rng.permutation(dst.shape[0]).astype(np.int64)
    return src, dst, int(dst.shape[0]), int(lens.shape[0])


def leaky32(t, slope):
    """The kernels' logit from the fp32 sum t: one fp32 multiply on the negative side."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(t > 0, t, t * np.float32(slope)).astype(np.float32)


def softmax_reference(dst, n_dst, z, da=None):
    """fp64 edge softmax of fp32 logits z [nnz, H] over the edges of every destination: a (and, given da: dz and the sum of |terms| of
    dz, the row scale of close_rows).  -inf logits get exactly 0; a row of nothing but -inf is NaN, as torch.softmax gives."""
    z64 = np.asarray(z, np.float64)
    H = z64.shape[1]
    m = np.full((n_dst, H), -np.inf)
    np.maximum.at(m, dst, z64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(z64 - m[dst])
        s = np.zeros((n_dst, H))
        np.add.at(s, dst, e)
        a = e / s[dst]
    if da is None:
        return a
    da64 = np.asarray(da, np.float64)
    dot, mag = np.zeros((n_dst, H)), np.zeros((n_dst, H))
    np.add.at(dot, dst, a * da64)
    np.add.at(mag, dst, np.abs(a * da64))
    return a, a * (da64 - dot[dst]), a * (np.abs(da64) + mag[dst])


def below_top(dst, n_dst, z):
    """z - (the maximum of its row and head) in fp64, [nnz, H]; NaN on rows of nothing but -inf."""
    z64 = np.asarray(z, np.float64)
    m = np.full((n_dst, z64.shape[1]), -np.inf)
    np.maximum.at(m, dst, z64)
    with np.errstate(invalid="ignore"):
        return z64 - m[dst]


def gat_reference(G, el, er, slope, feat=None, up=None, da=None):
    """One GAT layer's message passing in fp64 from fp32 operands: el [n_src, H], er [n_dst, H], feat [n_src, H, F], upstream gradient
    up [n_dst, H, F] (or, without feat, the attention alone with an upstream da [nnz, H]).  Returns a dict of references and, beside
    every reduced one, the sum of |terms| reduced into each element (`*_mag`)."""
    src, dst, n_src, n_dst = G
    with np.errstate(invalid="ignore"):
        t = (el[src] + er[dst]).astype(np.float32)                       # the fp32 sum the kernels form
    z = leaky32(t, slope)
    lrelu = np.where(t > 0, 1.0, float(np.float32(slope)))
    H = z.shape[1]
    r = {"z": z}
    if feat is None:
        a, dz, bound = softmax_reference(dst, n_dst, z, da)
    else:
        a = softmax_reference(dst, n_dst, z)
        f64, u64 = feat.astype(np.float64), up.astype(np.float64)
        F = f64.shape[2]
        r["out"], r["out_mag"] = np.zeros((n_dst, H, F)), np.zeros((n_dst, H, F))
        np.add.at(r["out"], dst, a[:, :, None] * f64[src])
        np.add.at(r["out_mag"], dst, a[:, :, None] * np.abs(f64[src]))
        r["dfeat"], r["dfeat_mag"] = np.zeros((n_src, H, F)), np.zeros((n_src, H, F))
        np.add.at(r["dfeat"], src, a[:, :, None] * u64[dst])
        np.add.at(r["dfeat_mag"], src, a[:, :, None] * np.abs(u64[dst]))
        da64 = (f64[src] * u64[dst]).sum(-1)
        da_mag = (np.abs(f64[src]) * np.abs(u64[dst])).sum(-1)
        dot, dot_mag = np.zeros((n_dst, H)), np.zeros((n_dst, H))
        np.add.at(dot, dst, a * da64)
        np.add.at(dot_mag, dst, a * da_mag)
        dz, bound = a * (da64 - dot[dst]), a * (da_mag + dot_mag[dst])
    r["a"] = a
    dt = dz * lrelu
    for name, idx, n in (("del", src, n_src), ("der", dst, n_dst)):
        r[name], r[name + "_mag"] = np.zeros((n, H)), np.zeros((n, H))
        np.add.at(r[name], idx, dt)
        np.add.at(r[name + "_mag"], idx, bound)
    return r


def chunk_edges(L, splits=(64, 256)):
    """The first and the last rank of every hub chunk of a row of L edges, for every split threshold that makes it a hub row."""
    ranks = set()
    for s in splits:
        if L > s:
            for b in range(0, L, s):
                ranks |= {b, min(b + s, L) - 1}
    return sorted(ranks)


def dominant_ranks(L):
    """Where the dominant edge of a row of L edges goes, one placement per round: rank 0, the last rank, 63, 64, 65, chunk edges."""
    return sorted({r for r in [0, L - 1, 63, 64, 65] + chunk_edges(L) if 0 <= r < L})


def logit_pattern(name, dst, n_dst, H, seed, rnd=0):
    """[nnz, H] fp32 logits by the rank of the edge inside its row (section 2 of the module docstring of test_value_edges.py)."""
    rng = np.random.default_rng(seed)
    nnz = dst.shape[0]
    rank = xl.rank_in_row(dst, np.arange(nnz))
    lens = np.bincount(dst, minlength=n_dst)
    if name.startswith("shift"):
        c = {"shift+90": 90.0, "shift-90": -90.0, "shift+3e4": 3e4, "shift-3e4": -3e4}[name]
        return (rng.standard_normal((nnz, H)) * 3 + c).astype(np.float32)
    if name in ("ramp up", "ramp down"):
        return ((25.0 if name == "ramp up" else -25.0) * rank)[:, None].repeat(H, 1).astype(np.float32)
    if name == "dominant":
        z = rng.standard_normal((nnz, H)).astype(np.float32)
        spots = [dominant_ranks(L) for L in lens.tolist()]
        for h in range(H):
            where = np.array([c[(rnd + h) % len(c)] if c else -1 for c in spots])
            z[rank == where[dst], h] = 200.0
        return z
    if name == "underflow":                       # half the edges far below the row's top, rank 0 among them in every other row
        z = rng.standard_normal((nnz, H)).astype(np.float32)
        low = (rng.random((nnz, H)) < 0.5) | ((rank == 0) & (dst % 2 == 0))[:, None]
        low &= (rank != lens[dst] - 1)[:, None]                                           # the last edge stays on top
        return np.where(low, z - np.float32(120.0) - np.abs(z) * np.float32(10.0), z).astype(np.float32)
    if name == "ties at 88":
        return np.full((nnz, H), 88.0, np.float32)
    raise KeyError(name)


PATTERNS = ("shift+90", "shift-90", "shift+3e4", "shift-3e4", "ramp up", "ramp down", "dominant", "underflow", "ties at 88")


def masked_ranks(L, placement, rng):
    """Which ranks of a row of L >= 2 edges are masked: about 30 % (at least a quarter, never all).  head: from rank 0 on (rows of 214
    edges and more lose their whole first 64-edge step, the 1000-edge row its whole first hub chunk); tail: up to the last rank;
    stride: every fourth rank from 0 -- the whole share of a lane group wherever 4, 8 or 16 groups split a row -- and as many ranks
    = 2 mod 4 as the count needs; scattered: at random."""
    k = min(L - 1, max(-(-L // 4), int(0.3 * L + 0.5)))
    if placement == "head":
        return np.arange(k)
    if placement == "tail":
        return np.arange(L - k, L)
    if placement == "stride":
        first = np.arange(0, L, 4)
        if first.shape[0] > k:                       # L = 2, 3, 5 ...: ceil(L / 4) can reach L - 1 only through the cap above
            first = first[:k]
        return np.concatenate([first, np.arange(2, L, 4)[:k - first.shape[0]]])
    return rng.permutation(L)[:k]


PLACEMENTS = ("head", "tail", "stride", "scattered")


def masked_logits(dst, n_dst, H, seed, rnd):
    """(z [nnz, H] fp32 with -inf on the masked edges, masked [nnz, H] bool).  Head h takes placement (h + rnd) % 4.  The unmasked edges
    of a row carry the same N(0, 3) values in the same order whatever the placement: values are dealt by rank among the unmasked."""
    nnz = dst.shape[0]
    rank = xl.rank_in_row(dst, np.arange(nnz))
    lens = np.bincount(dst, minlength=n_dst)
    order = np.argsort(dst, kind="stable")                              # CSR position -> edge id
    starts = np.cumsum(lens) - lens
    z = np.zeros((nnz, H), np.float32)
    masked = np.zeros((nnz, H), bool)
    for h in range(H):
        place = PLACEMENTS[(h + rnd) % 4]
        for v, L in enumerate(lens.tolist()):
            if L == 0:
                continue
            vals = (np.random.default_rng([seed, v, h]).standard_normal(L) * 3).astype(np.float32)
            rows = order[starts[v]:starts[v] + L]                       # edge ids by rank
            if L >= 2:
                gone = np.zeros(L, bool)
                gone[masked_ranks(L, place, np.random.default_rng([seed, v, h, 1]))] = True
                zr = np.full(L, -np.inf, np.float32)
                zr[~gone] = vals[:int((~gone).sum())]
                z[rows, h], masked[rows, h] = zr, gone
            else:
                z[rows, h] = vals
    assert np.array_equal(rank[order], np.concatenate([np.arange(L) for L in lens.tolist()]))
    return z, masked


# ============================================================================= non-finite sources
def float_rows_sum(dst, n_dst, term):
    """Row sums of fp32 terms [nnz, D] in fp64, IEEE classes included: a NaN term or +inf and -inf together give NaN, an infinity
    alone gives itself.  For integer terms below 2^24 in total the finite sums are exact in any order."""
    order = np.argsort(dst, kind="stable")
    counts = np.bincount(dst, minlength=n_dst)
    live = counts > 0
    out = np.zeros((n_dst, term.shape[1]))
    with np.errstate(invalid="ignore"):
        out[live] = np.add.reduceat(np.asarray(term, np.float64)[order], (np.cumsum(counts) - counts)[live], axis=0)
    return out


def fed_rows(src, dst, n_dst, sources):
    """Mask of the destinations that receive at least one edge from `sources`."""
    fed = np.zeros(n_dst, bool)
    fed[dst[np.isin(src, sources)]] = True
    return fed


def sources_feeding(src, dst, n_src, n_dst, lo=0.01, hi=0.10, count=2, avoid=()):
    """`count` sources whose destinations are between lo and hi of all destinations, the ones feeding the most first."""
    pairs = np.unique(src * n_dst + dst)
    per = np.bincount(pairs // n_dst, minlength=n_src)
    ok = np.nonzero((per >= lo * n_dst) & (per <= hi * n_dst))[0]
    ok = [int(u) for u in ok[np.argsort(-per[ok], kind="stable")] if int(u) not in avoid]
    assert len(ok) >= count, "no %d sources feed between %g and %g of the destinations" % (count, lo, hi)
    return ok[:count]
