"""ops.dot_attention: the fused walks of csrc/dotattn.hip against the composition u_dot_v -> edge_softmax -> u_mul_e/sum (the operators
as they were before the fused path existed), forward and forward + backward, on the arxiv-shaped and reddit-small stand-ins of
kernel_bench.py.  (H, F) = (1, 16), (8, 16), (4, 64), each with separate k and v and with k and v aliased.

Method: HIP events around one call, 3 warm-up calls of each form, then the two forms ALTERNATE for `--reps` (>= 20) timed calls each;
the median is reported with min and max.  These are CALL times: the window holds the kernels, the launch gaps between them and the
allocator's work, which is what a user of the operator waits for; no kernel trace is taken here.  "call TB/s" = the algorithmic bytes
of the FUSED form (every operand once, index arrays once per walk) over the fused call time: a call-level rate, not a kernel's.  Peak memory (torch.cuda.max_memory_allocated above what is resident before the call) for both
forms on every row (the last row is the largest shape run).

    python experiments/exp_dot_attention.py [--out FILE] [--reps 20] [--scale 1.0] [--datasets arxiv,reddit-small]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dgl-0.5-benchmark_amd"))
import torch  # noqa: E402
import dgl  # noqa: E402,F401
from mi355x_graph import config, ops  # noqa: E402
from kernel_bench import get_graph  # noqa: E402

SHAPES = ((1, 16), (8, 16), (4, 64))


def fused_bytes(n_src, n_dst, nnz, H, F, aliased):
    D, idx = H * F, 4 * (n_dst + 1) + 4 * nnz
    kv = (1 if aliased else 2) * n_src * D * 4
    fwd = idx + n_dst * D * 4 + kv + n_dst * D * 4 + n_dst * H * 16                       # q, k, v -> out, stat
    dst_walk = idx + 3 * n_dst * D * 4 + kv + n_dst * D * 4 + 2 * n_dst * H * 16           # q, out, dout, k, v -> dq; stat read + t written
    src_walk = 4 * (n_src + 1) + 4 * nnz + kv + 2 * n_dst * D * 4 + n_dst * H * 16 + 2 * n_src * D * 4   # k, v, q, dout, stat -> dk, dv
    return fwd, fwd + dst_walk + src_walk


def timed_pair(fns, reps):
    """fns: {name: callable}; warm-up, then the callables alternate; -> {name: (median, min, max)} in ms"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    evs = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[name].append((a, b))
    torch.cuda.synchronize()
    res = {}
    for name, pairs in evs.items():
        t = sorted(a.elapsed_time(b) for a, b in pairs)
        res[name] = (t[len(t) // 2], t[0], t[-1])
    return res


def with_form(fused, fn):
    def run():
        config.DOT_ATTENTION_FUSED = fused
        try:
            return fn()
        finally:
            config.DOT_ATTENTION_FUSED = True
    return run


def peak_of(fn, clear):
    clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None, help="also write the table to this file")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--datasets", default="arxiv,reddit-small")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_dot_attention.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    lines = ["experiments/exp_dot_attention.py -- ops.dot_attention: fused walks (csrc/dotattn.hip) against u_dot_v -> edge_softmax -> u_mul_e/sum",
             "# device '%s' (%s, %d CUs), reps %d (call times by HIP events, median [min .. max] ms; fused / composed alternate)"
             % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, max(args.reps, 20)),
             "%-13s %-7s %-8s | %-28s %-28s %6s %9s | %-28s %-28s %6s %9s" % ("graph", "(H, F)", "k, v", "fwd fused", "fwd composed", "ratio", "call TB/s",
                                                                              "fwd+bwd fused", "fwd+bwd composed", "ratio", "call TB/s") + " | peak MiB fused / composed / one [E, H]"]
    print("\n".join(lines))
    for name in args.datasets.split(","):
        g = get_graph(name, dev, args.scale).int().formats(["csr", "csc"]).to(dev)
        n, nnz = g.number_of_nodes(), g.number_of_edges()
        for H, F in SHAPES:
            for aliased in (False, True):
                gen = torch.Generator(device=dev).manual_seed(H * 100 + F)
                q = torch.randn(n, H, F, device=dev, generator=gen).requires_grad_(True)
                k = torch.randn(n, H, F, device=dev, generator=gen).requires_grad_(True)
                v = k if aliased else torch.randn(n, H, F, device=dev, generator=gen).requires_grad_(True)
                up = torch.randn(n, H, F, device=dev, generator=gen)
                assert ops.dot_attention_fused(g, q, k, v), "the fused path does not take this shape: nothing to measure"

                def fwd():
                    with torch.no_grad():
                        return ops.dot_attention(g, q, k, v)

                def fwd_bwd():
                    q.grad = k.grad = v.grad = None
                    ops.dot_attention(g, q, k, v).backward(up)

                with torch.no_grad():  # faster and different is not faster: the two forms must agree at the size that is timed
                    a_, b_ = with_form(True, fwd)(), with_form(False, fwd)()
                    err = float((a_ - b_).abs().max() / b_.abs().max())
                    assert err < 1e-4, err
                    del a_, b_
                tf = timed_pair({"fused": with_form(True, fwd), "composed": with_form(False, fwd)}, max(args.reps, 20))
                tb = timed_pair({"fused": with_form(True, fwd_bwd), "composed": with_form(False, fwd_bwd)}, max(args.reps, 20))
                bf, bb = fused_bytes(n, n, nnz, H, F, aliased)

                def cell(t):
                    return "%8.3f [%7.3f .. %7.3f]" % t

                def clear():
                    q.grad = k.grad = v.grad = None

                pk_f, pk_c = peak_of(with_form(True, fwd_bwd), clear), peak_of(with_form(False, fwd_bwd), clear)
                line = "%-13s %-7s %-8s | %-28s %-28s %6.2f %9.2f | %-28s %-28s %6.2f %9.2f | %7.1f / %7.1f / %6.1f" % (
                    name, "(%d,%d)" % (H, F), "aliased" if aliased else "separate", cell(tf["fused"]), cell(tf["composed"]),
                    tf["composed"][0] / tf["fused"][0], bf / tf["fused"][0] / 1e9, cell(tb["fused"]), cell(tb["composed"]),
                    tb["composed"][0] / tb["fused"][0], bb / tb["fused"][0] / 1e9, pk_f / 2 ** 20, pk_c / 2 ** 20, nnz * H * 4 / 2 ** 20)
                print(line, flush=True)
                lines.append(line)
                clear()
    tail = ["", "# peak MiB: torch.cuda.max_memory_allocated of one forward + backward above what is resident before it (q, k, v, d out)"]
    print("\n".join(tail))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
