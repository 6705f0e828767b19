"""Two builds of libmi355x_graph.so in ONE process: csrc/xty.hip of a parent build against this tree's, for a change that must not
change a bit or a microsecond (one dword walk body, one partial-sum finish, one wrapper call path; docs/LOG_xty_body.md).

  bits    standard-normal operands, outputs and column sums compared as int32: backend.xty with and without column sums at every shape
          of tests/test_exact_structure.py's XTY_SHAPES and XTY_COLSUM_SHAPES, the 64 dword instantiations and the misaligned view of
          that file, the row-list and position-map forms at tests/test_head_rows.py's shapes, one position map with Inf and NaN in rows
          of b that meet zero rows of a, and mgx_xty_colsum_masked at tests/test_xty_masked.py's (n, K, p) grid.
  speed   median call times (HIP events, the builds alternate call by call) at the workloads' shapes, in several rounds; the parent is
          loaded TWICE (a copy of the file), and the range of the round medians of its two loads -- parent against parent in the same
          run -- is the margin the new build's median is held against.

    python experiments/exp_xty_ab.py --parent /path/to/parent/libmi355x_graph.so [--mode bits|speed|both] [--out FILE] [--rounds 7] [--reps 20]
"""
import argparse
import ctypes
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dgl-0.5-benchmark_amd"))
import torch  # noqa: E402
from mi355x_graph import _lib, sparse  # noqa: E402

DEV = torch.device("cuda:0")
XTY_SHAPES = [(0, 3, 5), (1, 1, 1), (5, 64, 128), (1000, 47, 64), (70001, 64, 100), (300000, 16, 7), (123457, 33, 113), (65536, 64, 64),
              (70000, 256, 128), (66000, 200, 300), (3000, 65, 129), (80000, 128, 602), (70000, 256, 1024), (50, 256, 1000),
              (169343, 256, 512), (0, 200, 300)]
XTY_COLSUM_SHAPES = [(70001, 64, 128), (65537, 64, 200), (100000, 47, 128), (70000, 64, 64), (66000, 16, 100), (5000, 64, 128),
                     (70000, 64, 72), (70000, 128, 128), (0, 64, 128)]
MASKED_NS, MASKED_KS, MASKED_PS = [1, 15, 16, 17, 4099, 70001], [64, 72, 128, 200, 256], [0.0, 0.5]
N_PRODUCTS, TRAIN_PRODUCTS = 2449029, 196615
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


def flat(res):
    """a backend result (tensor, tuple of tensors or None) as a list of tensors"""
    return [] if res is None else [res] if torch.is_tensor(res) else list(res)


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def rand(gen, *shape):
    return torch.randn(*shape, device=DEV, generator=gen)


def subset(n, R, gen):
    return torch.randperm(n, device=DEV, generator=gen)[:R].sort().values


def bits(builds):
    be = sparse.backend_for(torch.zeros(1, device=DEV))
    parent, new = builds["parent"], builds["new"]
    n_cmp = n_bad = 0

    def compare(what, fn):
        nonlocal n_cmp, n_bad
        use(parent)
        a = flat(fn())
        use(new)
        b = flat(fn())
        ok = same_bits(a, b)
        n_cmp += 1
        n_bad += not ok
        nonfinite = sum(int((~torch.isfinite(x)).sum()) for x in b)
        say("%-74s %s%s%s" % (what, "bit-identical" if ok else "DIFFERENT", "" if a else "  (no kernel: None from both)" if ok else "",
                              "  (%d non-finite values)" % nonfinite if nonfinite else ""))

    for n, M, K in XTY_SHAPES + XTY_COLSUM_SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(n + M + K)
        a, b = rand(gen, n, M), rand(gen, n, K)
        compare("xty                     n=%d %dx%d" % (n, M, K), lambda: be.xty(a, b))
        compare("xty colsum              n=%d %dx%d" % (n, M, K), lambda: be.xty(a, b, colsum=True))
        wide = torch.cat([a, torch.full((n, 8), 5.0, device=DEV)], 1)
        compare("xty colsum, strided a   n=%d %dx%d" % (n, M, K), lambda: be.xty(wide[:, :M], b, colsum=True))
    for n in (37, 4117):
        gen = torch.Generator(device=DEV).manual_seed(n)
        a64, b128 = rand(gen, n, 64), rand(gen, n, 128)
        for mt in range(1, 5):
            for kt in range(1, 9):
                a, b = a64[:, :16 * mt - 3].contiguous(), b128[:, :16 * kt - 1].contiguous()
                compare("xty dword <%d,%d>         n=%d %dx%d" % (mt, kt, n, a.shape[1], b.shape[1]), lambda: be.xty(a, b))
        if n == 4117:
            compare("xty misaligned b        n=%d 64x64" % n, lambda: be.xty(a64, b128[:, 1:65]))
            compare("xty colsum misaligned b n=%d 64x64" % n, lambda: be.xty(a64, b128[:, 1:65], colsum=True))
    for R in (5000, 17):
        for cols in ((0, 128), (0, 64), (64, 128)):
            gen = torch.Generator(device=DEV).manual_seed(R + cols[0] + cols[1])
            b = rand(gen, 20000, 128)[:, cols[0]:cols[1]]
            a, rows = rand(gen, R, 47), subset(20000, R, gen)
            for colsum in (False, True):
                compare("xty row list%s     R=%d cols %d..%d" % (" colsum" if colsum else "       ", R, *cols), lambda: be._xty_rows(a, b, rows, colsum))
                compare("xty(rows=)%s       R=%d cols %d..%d" % (" colsum" if colsum else "       ", R, *cols), lambda: be.xty(a, b, colsum=colsum, rows=rows))
    n = 70001
    for R in (5600, 17, 1):
        for cols in ((0, 128), (64, 128)):
            gen = torch.Generator(device=DEV).manual_seed(7 * R + cols[0])
            b = rand(gen, n, 128)[:, cols[0]:cols[1]]
            a, rows = rand(gen, R, 47), subset(n, R, gen)
            pos = torch.full((n,), -1, dtype=torch.int64, device=DEV)
            pos[rows] = torch.arange(R, device=DEV)
            for colsum in (False, True):
                compare("xty position map%s R=%d cols %d..%d" % (" colsum" if colsum else "       ", R, *cols), lambda: be.xty_pos(a, pos, b, colsum=colsum))
            if R == 5600 and cols == (0, 128):
                bad = b.clone()
                zero_rows = (pos < 0).nonzero().flatten()
                bad[zero_rows[::3]] = float("inf")
                bad[zero_rows[1::3], ::2] = float("nan")
                compare("xty position map colsum, Inf / NaN in b on zero rows of a", lambda: be.xty_pos(a, pos, bad, colsum=True))
    for n in MASKED_NS:
        for p in MASKED_PS:
            gen = torch.Generator(device=DEV).manual_seed(1000 * n + int(p * 10))
            use(new)
            _, mask = be.relu_dropout_fwd(rand(gen, n, 64), p, 4242 + n, 77)
            wide, bwide = rand(gen, n, 128), rand(gen, n, 264)
            for K in MASKED_KS:
                compare("xty masked              n=%d K=%d p=%.1f" % (n, K, p), lambda: be.xty_masked(wide[:, :64].contiguous(), mask, p, bwide[:, :K].contiguous()))
                compare("xty masked, strided     n=%d K=%d p=%.1f" % (n, K, p), lambda: be.xty_masked(wide[:, :64], mask, p, bwide[:, :K]))
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


def speed(builds, rounds, reps):
    """Per row: every build's median over its rounds' medians [the least .. the largest round median].  The parents' spread is the range
    of the 2 x rounds round medians of the two loads of the parent; the new build fails a row when its median lies above that range."""
    be = sparse.backend_for(torch.zeros(1, device=DEV))
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

    gen = torch.Generator(device=DEV).manual_seed(1)
    n = N_PRODUCTS
    a, b = rand(gen, n, 64), rand(gen, n, 200)
    b100 = b[:, :100].contiguous()
    row("n=%d 64x100 colsum (16-byte loads)" % n, lambda: be.xty(a, b100, colsum=True))
    del b100
    row("n=%d 64x200 colsum (two launches)" % n, lambda: be.xty(a, b, colsum=True))
    use(builds["new"])
    _, mask = be.relu_dropout_fwd(rand(gen, n, 64), 0.5, 4242, 77)
    row("n=%d masked K=200 p=0.5" % n, lambda: be.xty_masked(a, mask, 0.5, b))
    del a, mask
    buf = b[:, :128]                                         # a [n, 128] view of the layer buffer, row stride 200
    dy, rows = rand(gen, TRAIN_PRODUCTS, 47), subset(n, TRAIN_PRODUCTS, gen)
    row("R=%d 47x128 colsum, loss-row list" % TRAIN_PRODUCTS, lambda: be._xty_rows(dy, buf, rows, True))
    pos = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    pos[rows] = torch.arange(TRAIN_PRODUCTS, device=DEV)
    row("n=%d 47x128 colsum, position map" % n, lambda: be.xty_pos(dy, pos, buf, colsum=True))
    del b, buf, dy, rows, pos
    for n, M, K, what in ((169343, 256, 512, "grid"), (232965, 128, 602, "grid"), (300000, 16, 7, "dword"), (123457, 33, 113, "dword")):
        a, b = rand(gen, n, M), rand(gen, n, K)
        row("n=%d %dx%d (%s)" % (n, M, K, what), lambda: be.xty(a, b))
    say("%d rows slower than the parents' spread allows" % slow)
    return slow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libmi355x_graph.so of the parent commit")
    ap.add_argument("--new", default=_lib.LIB_PATH)
    ap.add_argument("--mode", choices=["bits", "speed", "both"], default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls of every build per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_xty_ab.py runs on the GPU; none is visible")
    tmp = tempfile.mkdtemp()
    again = os.path.join(tmp, "libmi355x_graph_parent_again.so")  # dlopen of one path twice gives one library: a copy is a second one
    shutil.copy(args.parent, again)
    builds = {"parent": load(args.parent), "parent again": load(again), "new": load(args.new)}
    prop = torch.cuda.get_device_properties(0)
    say("experiments/exp_xty_ab.py -- device '%s' (%s, %d CUs)" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count))
    bad = 0
    if args.mode in ("bits", "both"):
        bad += bits(builds)
    if args.mode in ("speed", "both"):
        bad += speed(builds, max(args.rounds, 3), max(args.reps, 10))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
