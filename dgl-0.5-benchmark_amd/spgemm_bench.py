"""Sparse x sparse product benchmark: ops.spgemm fused (csrc/spgemm.hip) against the composition it replaces.

Forward (weighted), and forward + backward (d wa, d wb), of C = A B on
  gcmc      user-item times item-user at MovieLens-100K's sizes (943 x 1682, 50 k ratings, popularity-skewed items)
  metapath  author -> paper -> subject -> venue on a synthetic heterograph, two products (dgl.metapath_reachable_graph's chain, weighted)
  products  A A on 16 k sampled rows of a 200 k-node graph of ~25 edges per node
  rmat      A A on 2048 sampled rows and the 16 longest of an R-MAT graph, scale 16, 400 k edges: hub rows above T2
  molhiv    A A on a batch of 2048 molecule graphs: many tiny rows
as
  fused     config.SPGEMM_FUSED = True: hash tables and column windows in LDS, no product written to memory
  composed  config.SPGEMM_FUSED = False: repeat_interleave -> unique -> index_add over every product
--sweep times the fused forward of rmat and products for config.SPGEMM_T1 / _T2 / _W.
Timing: HIP events around every call after --warmup discarded ones; median / min / max of --reps calls in microseconds; peak memory
above what is allocated before the call.  Both forms run in one process and are compared before they are timed.  The script only reports."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgl  # noqa: E402,F401
from gatv2_bench import molhiv_batch, peak_mib  # noqa: E402
from nnconv_bench import timed  # noqa: E402
from mi355x_graph import config, ops  # noqa: E402
import mi355x_graph as mg  # noqa: E402


def block(src, dst, n, m, dev):
    return mg.create_block((src, dst), n, m, idtype=torch.int32, device=dev)


def gcmc_pair(dev):
    gen = torch.Generator().manual_seed(0)
    users, items, E = 943, 1682, 50000
    item = torch.multinomial(1.0 / torch.arange(1, items + 1).float() ** 0.8, E, replacement=True, generator=gen)
    user = torch.randint(0, users, (E,), generator=gen)
    return [(block(user, item, users, items, dev), block(item, user, items, users, dev))]


def metapath_chain(dev):
    gen = torch.Generator().manual_seed(1)
    a, p, s, v = 20000, 40000, 2000, 300
    draw = lambda n, m, e: (torch.randint(0, n, (e,), generator=gen), torch.randint(0, m, (e,), generator=gen))
    ap, ps, sv = block(*draw(a, p, 80000), a, p, dev), block(*draw(p, s, 80000), p, s, dev), block(*draw(s, v, 8000), s, v, dev)
    return [(ap, ps), (ops.spgemm(ap, ps)[0], sv)]


def row_sample(src, dst, n, rows, dev):
    """(the rows `rows` of the n x n adjacency as a block, the whole adjacency)"""
    new = torch.full((n,), -1, dtype=torch.long)
    new[rows] = torch.arange(len(rows))
    keep = new[src] >= 0
    return [(block(new[src[keep]], dst[keep], len(rows), n, dev), block(src, dst, n, n, dev))]


def products_pair(dev):
    gen = torch.Generator().manual_seed(2)
    n, E = 200000, 5000000
    src, dst = torch.randint(0, n, (E,), generator=gen), (torch.rand(E, generator=gen) ** 2 * n).long().clamp(max=n - 1)
    return row_sample(src, dst, n, torch.randperm(n, generator=gen)[:16384], dev)


def rmat_pair(dev, scale=16, E=400000):
    gen = torch.Generator().manual_seed(3)
    src, dst = torch.zeros(E, dtype=torch.long), torch.zeros(E, dtype=torch.long)
    for _ in range(scale):  # quadrant probabilities 0.57, 0.19, 0.19, 0.05
        q = torch.multinomial(torch.tensor([0.57, 0.19, 0.19, 0.05]), E, replacement=True, generator=gen)
        src, dst = src * 2 + q // 2, dst * 2 + q % 2
    n = 2 ** scale
    hubs = torch.bincount(src, minlength=n).argsort(descending=True)[:16]
    rest = torch.randperm(n, generator=gen)[:2048]
    return row_sample(src, dst, n, torch.unique(torch.cat([hubs, rest])), dev)


def molhiv_pair(dev):
    g = molhiv_batch(2048, dev)
    return [(g, g)]


def forms(pairs, compare=True):
    dev = pairs[0][0].device
    gen = torch.Generator(device=dev).manual_seed(7)
    ws = [tuple(torch.randn(g.number_of_edges(), device=dev, generator=gen).requires_grad_(True) for g in pair) for pair in pairs]
    csr = [(a._index.csr(), b._index.csr()) for a, b in pairs]
    products = sum(int((b.indptr[1:] - b.indptr[:-1]).long()[a.indices.long()].sum()) for a, b in csr)

    def fwd():
        with torch.no_grad():
            return [ops.spgemm(a, b, wa, wb)[1] for (a, b), (wa, wb) in zip(pairs, ws)]

    def fwd_bwd():
        out = [ops.spgemm(a, b, wa, wb)[1] for (a, b), (wa, wb) in zip(pairs, ws)]
        return torch.autograd.grad(sum((o * o).sum() for o in out), [w for pair in ws for w in pair])

    assert all(ops.spgemm_fused(a, b, wa, wb) for (a, b), (wa, wb) in zip(pairs, ws))
    got = fwd() + list(fwd_bwd())
    extra = {"rows": sum(a.num_rows for a, _ in csr), "nnz_a": sum(a.nnz for a, _ in csr), "nnz_b": sum(b.nnz for _, b in csr),
             "products": products, "nnz_c": sum(len(o) for o in got[:len(pairs)])}
    if compare and products <= 80000000:  # the composition holds ~10 arrays of that length
        config.SPGEMM_FUSED = False
        want = fwd() + list(fwd_bwd())
        config.SPGEMM_FUSED = True
        extra["max_rel_diff"] = max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(got, want))
    return {"fwd": fwd, "fwd_bwd": fwd_bwd}, extra


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--shapes", default="gcmc,metapath,products,rmat,molhiv")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:%d" % args.device)
    torch.cuda.set_device(dev)
    build = {"gcmc": gcmc_pair, "metapath": metapath_chain, "products": products_pair, "rmat": rmat_pair, "molhiv": molhiv_pair}
    recs = []
    for name in args.shapes.split(","):
        pairs = build[name](dev)
        if args.sweep:
            for t1, t2, w in ((256, 2048, 4096), (128, 2048, 4096), (512, 2048, 4096), (256, 1024, 4096), (256, 4096, 4096), (256, 2048, 2048),
                              (256, 2048, 7168)):
                config.SPGEMM_T1, config.SPGEMM_T2, config.SPGEMM_W = t1, t2, w
                fn = forms(pairs, compare=False)[0]["fwd"]
                recs.append(dict(shape=name, T1=t1, T2=t2, W=w, **timed(fn, args)))
                print(json.dumps(recs[-1]), flush=True)
            continue
        fns, extra = forms(pairs)
        rec = dict(extra, shape=name)
        for form, fused in (("fused", True), ("composed", False)):
            if not fused and "max_rel_diff" not in extra:
                continue
            config.SPGEMM_FUSED = fused
            for what, fn in fns.items():
                rec["%s_%s" % (form, what)] = dict(timed(fn, args), peak_mib=peak_mib(fn))
        config.SPGEMM_FUSED = True
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
