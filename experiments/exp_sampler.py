"""Where does a neighbor-sampling iteration spend its time?  (reddit shape, fan-out 10,25, batch 1000)

--modes: instead, the cost of the sampling modes beyond the uniform one (prob=, replace=True, select_topk) on a 25 k-seed frontier,
fanout 25 and 10: the device kernel of each mode against mgx_sample_neighbors at the same seeds and fanout (the yardstick: it reads no
weights) and against the torch formulation of the same mode on the device.  Median of 10 synchronised repeats after 3 warm-up calls."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dgl-0.5-benchmark_amd"))
import torch
import dgl
from mi355x_graph.datasets import NodeData
from mi355x_graph import sampling
dev = torch.device("cuda:0")
data = NodeData("reddit", device=dev)
g = dgl.add_self_loop(data.graph).int(); g.create_formats_()
nid = torch.nonzero(torch.rand(g.number_of_nodes()) < 0.66).flatten()



def modes():
    import statistics
    E = g.number_of_edges()
    gen = torch.Generator().manual_seed(0)
    w = torch.rand(E, generator=gen)
    w[torch.rand(E, generator=gen) < 0.25] = 0.0
    w = w.to(dev)
    seeds = torch.randperm(g.number_of_nodes(), generator=gen)[:25000].to(dev)
    idx = g._index
    view = idx.csc()

    def med(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(10):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def torch_sample(fanout, prob, replace):
        pos, seg = sampling._sample_torch(view, seeds, fanout, prob, replace, None)
        return sampling._triple(view, seeds, pos, seg, "in")

    def torch_topk(k):
        pos, seg, first, deg = sampling._candidates(view, seeds)
        keep = sampling._smallest_per_segment(-w[view.eids[pos].long() if view.eids is not None else pos], seg, first, k)
        return sampling._triple(view, seeds, pos[keep], seg[keep], "in")

    print("in-edges of the 25000 seeds: %d" % int(g.in_degrees(seeds).sum()))
    for fanout in (25, 10):
        base = med(lambda: sampling.sample_neighbors(g, seeds, fanout))
        print("fanout %2d  uniform, no replacement (mgx_sample_neighbors): %8.3f ms" % (fanout, base))
        for name, kern, ref in [
                ("weighted", lambda: sampling.sample_neighbors(g, seeds, fanout, prob=w), lambda: torch_sample(fanout, w, False)),
                ("replace", lambda: sampling.sample_neighbors(g, seeds, fanout, replace=True), lambda: torch_sample(fanout, None, True)),
                ("weighted + replace", lambda: sampling.sample_neighbors(g, seeds, fanout, prob=w, replace=True),
                 lambda: torch_sample(fanout, w, True)),
                ("select_topk", lambda: sampling.select_topk(g, fanout, w, nodes=seeds), lambda: torch_topk(fanout))]:
            a, b = med(kern), med(ref)
            print("fanout %2d  %-20s kernel %8.3f ms (%.2f x uniform)   torch formulation %8.3f ms (%.1f x the kernel)"
                  % (fanout, name, a, a / base, b, b / a))


if "--modes" in sys.argv:
    modes()
    sys.exit(0)
sampler = dgl.dataloading.MultiLayerNeighborSampler([10, 25])
loader = dgl.dataloading.NodeDataLoader(g, nid, sampler, batch_size=1000, shuffle=True)
for rep in range(2):
    torch.cuda.synchronize(); t0 = time.time(); n = 0
    for inp, out, blocks in loader:
        n += 1
        if n == 60: break
    torch.cuda.synchronize(); print("sampling only: %.2f ms / iteration" % ((time.time() - t0) / n * 1e3))
seeds = nid[:1000].to(dev)
for name, fn in [("sample_neighbors(25)", lambda: sampling.sample_neighbors(g, seeds, 25)),
                 ("sample+to_block", lambda: sampler.sample_blocks(g, seeds))]:
    for rep in range(2):
        torch.cuda.synchronize(); t0 = time.time()
        for _ in range(20): fn()
        torch.cuda.synchronize(); print("%s: %.2f ms" % (name, (time.time() - t0) / 20 * 1e3))
