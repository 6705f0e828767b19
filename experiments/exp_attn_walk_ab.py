"""Two builds of libmi355x_graph.so in ONE process: the attention walks (csrc/gatfused.hip + gat_tile.inc, csrc/dotattn.hip) of a
parent build against this tree's, for a change that must not change a bit or a microsecond (the walk skeleton moved to plan_walk.h).

  bits    mgx_gat_fused_fwd/bwd (attn_drop 0 and 0.5; the 8 x 16 layer with el formed in the kernel, the ragged 1 x 41 layer),
          mgx_gat_tile_fwd/bwd where a tile plan exists, mgx_dot_attention_fwd/bwd (k, v separate and aliased) on the hub graphs of
          tests/test_gat_fused.py and tests/test_dot_attention.py at those tests' sizes, hub rows split at 64 and at 256, plus one
          +-3e4 shifted-logit, one -inf-masked and one NaN-logit input: every output and every stat / nstat array compared as int32.
  speed   median call times (HIP events, the builds alternate call by call) of the three walks of each family on the arxiv-shaped
          and reddit-shaped stand-ins, in several rounds; the parent is loaded TWICE (a copy of the file), and the range of the round
          medians of its two loads -- parent against parent in the same run -- is the margin the new build's median is held against.

    python experiments/exp_attn_walk_ab.py --parent /path/to/parent/libmi355x_graph.so [--mode bits|speed|both] [--out FILE] [--rounds 7] [--reps 20]
"""
import argparse
import ctypes
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dgl-0.5-benchmark_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import dgl  # noqa: E402,F401
from mi355x_graph import _lib, config, sparse  # noqa: E402
from kernel_bench import get_graph  # noqa: E402

DEV = torch.device("cuda:0")
GAT_SHAPES = [(900, 1, 16), (900, 8, 16), (700, 4, 8), (500, 2, 64), (300, 1, 4), (600, 3, 16), (400, 1, 256), (400, 16, 4), (350, 2, 128),
              (800, 1, 41), (500, 1, 7), (400, 1, 100), (300, 1, 5), (300, 1, 253), (800, 1, 16), (300, 4, 4), (400, 1, 102)]
DOT_SHAPES = [(300, 1, 4), (900, 1, 16), (700, 4, 8), (900, 8, 16), (500, 2, 64), (400, 1, 64), (600, 4, 64), (500, 3, 16), (400, 5, 8), (300, 3, 4)]
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def load(path):
    handle = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def use(handle):
    _lib._lib = handle  # every call of sparse.HipBackend goes through _lib.lib()


def hubby_graph(n, nnz, seed, hub_deg=3000):
    """tests/test_gat_fused.py's: conftest.random_graph + one hub destination + one hub source + destinations 0..4 without in-edges"""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n + 1) ** 0.9
    w[rng.integers(0, n, size=max(1, n // 8))] = 0.0
    w /= w.sum()
    dst = rng.choice(n, size=nnz, p=w)
    src = rng.integers(0, n, size=nnz)
    rng = np.random.default_rng(seed)
    keep = dst >= 5
    src, dst = src[keep], dst[keep]
    hs = rng.integers(0, n, hub_deg)
    src = np.concatenate([src, hs, np.full(hub_deg, 7)])
    dst = np.concatenate([dst, np.full(hub_deg, 11), rng.integers(5, n, hub_deg)])
    return src.astype(np.int64), dst.astype(np.int64)


def views(src, dst, n, split, tile):
    os.environ["MGX_SCHEDULE"] = "natural"
    os.environ["MGX_TILE"] = os.environ["MGX_GAT_TILE"] = "1" if tile else "0"
    config.HUB_SPLIT = split
    s, d = torch.from_numpy(src).int().to(DEV), torch.from_numpy(dst).int().to(DEV)
    return sparse.coo_to_csr(n, n, d, s), sparse.coo_to_csr(n, n, s, d)  # in-CSR, out-CSR


def gat_run(be, csc, csr, feat, el, er, up, p, attn_l):
    out, nstat, form = be.gat_fused_fwd(csc, feat, el, er, 0.2, p, 1234, attn_l=attn_l, csr=csr)
    fwd_stat = nstat.clone()
    d_feat, d_el, d_er = be.gat_fused_bwd(csc, csr, feat, el, 0.2, p, 1234, out, up, nstat, True, attn_l=attn_l, form=form)
    return form, [out, fwd_stat, nstat, d_feat, d_el, d_er]


def dot_run(be, csc, csr, q, k, v, up):
    out, stat = be.dot_attention_fwd(csc, q, k, v, 0.37)
    fwd_stat = stat.clone()
    dq, dk, dv = be.dot_attention_bwd(csc, csr, q, k, v, 0.37, out, up, stat, True, True, True)
    return "dot", [out, fwd_stat, stat, dq, dk, dv]


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def bits(builds):
    be = sparse.backend_for(torch.zeros(1, device=DEV))
    parent, new = builds["parent"], builds["new"]
    n_cmp = n_bad = 0

    def compare(what, fn):
        nonlocal n_cmp, n_bad
        use(parent)
        form, a = fn()
        use(new)
        form2, b = fn()
        ok = form == form2 and same_bits(a, b)
        n_cmp += 1
        n_bad += not ok
        nonfinite = sum(int((~torch.isfinite(x)).sum()) for x in b)
        say("%-66s %-5s %s%s" % (what, form, "bit-identical" if ok else "DIFFERENT", "  (%d non-finite values)" % nonfinite if nonfinite else ""))

    for split in (64, 256):
        for n, H, F in GAT_SHAPES:
            src, dst = hubby_graph(n, 40 * n, seed=H * 100 + F)
            gen = torch.Generator(device=DEV).manual_seed(H + F)
            feat = torch.randn(n, H, F, device=DEV, generator=gen)
            up = torch.randn(n, H, F, device=DEV, generator=gen)
            er = torch.randn(n, H, device=DEV, generator=gen) * 2
            attn_l = torch.randn(H, F, device=DEV, generator=gen) if (H, F) == (8, 16) else None   # el formed in the kernel
            el = (feat * attn_l).sum(-1) if attn_l is not None else torch.randn(n, H, device=DEV, generator=gen) * 2
            inputs = [("plain", el)]
            if (H, F) in ((1, 16), (4, 8), (1, 41)):
                shifted, masked, nan = el + 3e4, el.clone(), el.clone()
                shifted[::2] = el[::2] - 3e4
                masked[torch.rand(n, H, device=DEV, generator=gen) < 0.3] = -float("inf")
                nan[3], nan[n // 2, H - 1] = float("nan"), float("nan")
                inputs += [("+-3e4", shifted), ("-inf masked", masked), ("NaN logit", nan)]
            for tile in ([False, True] if H == 1 and F % 4 == 0 and F <= 16 else [False]):
                csc, csr = views(src, dst, n, split, tile)
                if tile and (csc.gat_tile_plan(F) is None or csr.gat_tile_plan(F) is None):
                    say("gat n=%d H=%d F=%d split=%d: no tile plan" % (n, H, F, split))
                    continue
                assert csc.plan().num_hubs >= 1 and csr.plan().num_hubs >= 1
                for name, e in inputs:
                    for p in (0.0, 0.5):
                        compare("gat  n=%d H=%d F=%d split=%d p=%.1f %s%s" % (n, H, F, split, p, name, " attn_l" if attn_l is not None else ""),
                                lambda: gat_run(be, csc, csr, feat, e.contiguous(), er, up, p, attn_l))
        for n, H, F in DOT_SHAPES:
            src, dst = hubby_graph(n, 40 * n, seed=H * 100 + F)
            csc, csr = views(src, dst, n, split, False)
            gen = torch.Generator(device=DEV).manual_seed(H * 7 + F)
            q, k, v, up = (torch.randn(n, H, F, device=DEV, generator=gen) for _ in range(4))
            inputs = [("plain", q, k)]
            if (H, F) in ((1, 16), (4, 8), (4, 64)):
                big, inf, nan = k * 3e4, k.clone(), k.clone()
                inf[::3] = -float("inf")                                  # q . k = -+inf or NaN by the sign of q: masked and NaN logits
                nan[3], nan[n // 2, H - 1, 0] = float("nan"), float("nan")
                inputs += [("+-3e4", q, big), ("-inf masked", q.abs(), inf), ("NaN logit", q, nan)]
            for name, qq, kk in inputs:
                compare("dot  n=%d H=%d F=%d split=%d %s k, v separate" % (n, H, F, split, name), lambda: dot_run(be, csc, csr, qq, kk, v, up))
                compare("dot  n=%d H=%d F=%d split=%d %s k is v" % (n, H, F, split, name), lambda: dot_run(be, csc, csr, qq, kk, kk, up))
    say("%d comparisons, %d different" % (n_cmp, n_bad))
    return n_bad


def timed(fns, rounds, reps):
    """fns: {build: callable}; 3 warm-up calls each, then `rounds` rounds in which the builds alternate call by call for `reps` calls
    each -> {build: [the median of every round]} in ms"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name in fns}
    for _ in range(rounds):
        evs = {name: [] for name in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                evs[name].append((a, b))
        torch.cuda.synchronize()
        for name, pairs in evs.items():
            t = sorted(a.elapsed_time(b) for a, b in pairs)
            res[name].append(t[len(t) // 2])
    return res


def speed(builds, rounds, reps, scale):
    """Per row: every build's median over its rounds' medians [the least .. the largest round median].  The parents' spread is the range
    of the 2 x rounds round medians of the two loads of the parent; the new build fails a row when its median lies above that range."""
    be = sparse.backend_for(torch.zeros(1, device=DEV))
    os.environ.pop("MGX_SCHEDULE", None)
    os.environ.pop("MGX_TILE", None)
    os.environ.pop("MGX_GAT_TILE", None)
    config.HUB_SPLIT = 256
    slow = 0
    say("%-50s %-26s %-26s %-26s %s" % ("call (ms; %d rounds of %d calls, builds alternate)" % (rounds, reps), "parent", "parent again", "new",
                                        "parents' spread, verdict"))

    def row(what, make):
        nonlocal slow
        fns = {}
        for name, handle in builds.items():
            fns[name] = (lambda h=handle: (use(h), make())[1])
        t = timed(fns, rounds, reps)
        both = t["parent"] + t["parent again"]
        lo, hi = min(both), max(both)
        nw = sorted(t["new"])[rounds // 2]
        slow += nw > hi
        cells = ("%7.3f [%7.3f .. %7.3f]" % (sorted(t[k])[rounds // 2], min(t[k]), max(t[k])) for k in ("parent", "parent again", "new"))
        say("%-50s %-26s %-26s %-26s [%.3f .. %.3f] %s" % (what, *cells, lo, hi, "within" if nw <= hi else "SLOWER: %.3f above" % (nw - hi)))

    cases = [("arxiv", sh, "dot") for sh in ((1, 16), (8, 16), (4, 64))] + [("reddit-small", sh, "dot") for sh in ((1, 16), (8, 16), (4, 64))]
    cases += [("reddit", (1, 16), "gat"), ("reddit", (1, 41), "gat")]
    graphs = {}
    for name, (H, F), fam in cases:
        if name not in graphs:
            graphs.clear()
            g = get_graph(name, DEV, scale).int().formats(["csr", "csc"]).to(DEV)
            graphs[name] = (g._index.csc(), g._index.csr(), g.number_of_nodes())
        csc, csr, n = graphs[name]
        gen = torch.Generator(device=DEV).manual_seed(H * 100 + F)
        up = torch.randn(n, H, F, device=DEV, generator=gen)
        if fam == "dot":
            q, k, v = (torch.randn(n, H, F, device=DEV, generator=gen) for _ in range(3))
            use(builds["new"])
            out, stat = be.dot_attention_fwd(csc, q, k, v, F ** -0.5)
            row("dot %s (%d,%d) forward" % (name, H, F), lambda: be.dot_attention_fwd(csc, q, k, v, F ** -0.5))
            row("dot %s (%d,%d) backward, destination walk" % (name, H, F),
                lambda: be.dot_attention_bwd(csc, csr, q, k, v, F ** -0.5, out, up, stat, True, False, False))
            row("dot %s (%d,%d) backward, source walk" % (name, H, F),
                lambda: be.dot_attention_bwd(csc, csr, q, k, v, F ** -0.5, out, up, stat, False, True, True))
        else:
            feat = torch.randn(n, H, F, device=DEV, generator=gen)
            el, er = torch.randn(n, H, device=DEV, generator=gen), torch.randn(n, H, device=DEV, generator=gen)
            p = 0.6
            use(builds["new"])
            out, nstat, form = be.gat_fused_fwd(csc, feat, el, er, 0.2, p, 7, csr=csr)
            row("gat %s (%d,%d) p=%.1f %s forward" % (name, H, F, p, form), lambda: be.gat_fused_fwd(csc, feat, el, er, 0.2, p, 7, csr=csr))
            row("gat %s (%d,%d) p=%.1f %s backward, dst walk" % (name, H, F, p, form),
                lambda: be.gat_fused_bwd(csc, csr, feat, el, 0.2, p, 7, out, up, nstat, False, form=form))
            row("gat %s (%d,%d) p=%.1f %s backward, both walks" % (name, H, F, p, form),
                lambda: be.gat_fused_bwd(csc, csr, feat, el, 0.2, p, 7, out, up, nstat, True, form=form))
    say("%d rows slower than the parents' spread allows" % slow)
    return slow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libmi355x_graph.so of the parent commit")
    ap.add_argument("--new", default=_lib.LIB_PATH)
    ap.add_argument("--mode", choices=["bits", "speed", "both"], default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls of every build per round")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_attn_walk_ab.py runs on the GPU; none is visible")
    tmp = tempfile.mkdtemp()
    again = os.path.join(tmp, "libmi355x_graph_parent_again.so")  # dlopen of one path twice gives one library: a copy is a second one
    shutil.copy(args.parent, again)
    builds = {"parent": load(args.parent), "parent again": load(again), "new": load(args.new)}
    prop = torch.cuda.get_device_properties(0)
    say("experiments/exp_attn_walk_ab.py -- device '%s' (%s, %d CUs)" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count))
    bad = 0
    if args.mode in ("bits", "both"):
        bad += bits(builds)
    if args.mode in ("speed", "both"):
        bad += speed(builds, max(args.rounds, 3), max(args.reps, 10), args.scale)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
