"""dgl.dataloading.negative_sampler.Uniform (csrc/edgefind.hip: mgx_negative_sample; the torch form in mi355x_graph/linkpred.py).

The random stream is part of the interface (csrc/counter_rng.h): try t of draw (e, j) proposes
    c = (e * k + j) * 64 + t,   r = mix64(rng_seed ^ mix64(c)),   v' = ((r >> 32) * N) >> 32
so the kernel, its in-CSR and out-CSR forms, both index widths and the torch form must agree with the Python-integer restatement below
bit for bit.  Rejection (exclude_existing, exclude_self_loops) is bounded by max_tries: a source adjacent to every node fails its draws,
the pairs are dropped, and nothing loops.
"""
import ctypes

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config, linkpred, sampling
from mi355x_graph.linkpred import Uniform, negative_destinations

from test_sampling_modes import check_binomial

DEV = "cuda:0"
IDTYPES = [torch.int32, torch.int64]
M64 = (1 << 64) - 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def candidate(rng_seed, draw, t, n):
    return ((mix64((rng_seed & M64) ^ mix64(draw * 64 + t)) >> 32) * n) >> 32


def seed_of(generator_seed):
    """The rng_seed a sampler call draws from a fresh generator."""
    return sampling._rng_seed(torch.Generator().manual_seed(generator_seed))


def random_graph(n, m, seed, idtype=torch.int64, dev="cpu"):
    gen = torch.Generator().manual_seed(seed)
    s, d = torch.randint(0, n, (m,), generator=gen), torch.randint(0, n, (m,), generator=gen)
    return mg.graph((s.to(idtype), d.to(idtype)), num_nodes=n).to(dev), s, d


def run_exact_stream(dev, idtype):
    g, s, d = random_graph(1000, 5000, 2, idtype, dev)
    eids = torch.randperm(5000, generator=torch.Generator().manual_seed(3))[:200]
    for k in (1, 5):
        src, dst = Uniform(k)(g, eids.to(dev), generator=torch.Generator().manual_seed(7))
        assert src.dtype == idtype and dst.dtype == idtype
        assert torch.equal(src.cpu().long(), s[eids].repeat_interleave(k))
        rng_seed = seed_of(7)
        assert dst.tolist() == [candidate(rng_seed, i, 0, 1000) for i in range(200 * k)]
    # seeds with the top bit set, the largest node count, a later try: the sign handling of the int64 form
    big = 0xF123456789ABCDEF
    for t in (1, 63):
        got = linkpred.negative_candidates(big, torch.arange(300, device=dev), t, 2 ** 31 - 1)
        assert got.tolist() == [candidate(big, i, t, 2 ** 31 - 1) for i in range(300)]
    dst, failed = negative_destinations(g._index, s[eids].to(dev), 3, 0, 16, big)
    assert failed == 0 and dst.tolist() == [candidate(big, i, 0, 1000) for i in range(600)]
    return dst


def run_reproducible(dev):
    g, s, d = random_graph(500, 4000, 4, dev=dev)
    eids = torch.arange(300, device=dev)
    ns = Uniform(4, exclude_existing=True, exclude_self_loops=True)
    a = ns(g, eids, generator=torch.Generator().manual_seed(1))
    b = ns(g, eids, generator=torch.Generator().manual_seed(1))
    c = ns(g, eids, generator=torch.Generator().manual_seed(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[1], c[1])
    return a


EXCL_SEED = 11  # confirmed on the CPU form (which runs the same stream): zero failed draws, see run_exclusion


def exclusion_graph(dev, idtype=torch.int64):
    """64 nodes; source 0 has out-edges to nodes 0 .. 15 (itself included), edge ids 0 .. 15; every other node one out-edge."""
    s = torch.cat([torch.zeros(16, dtype=torch.int64), torch.arange(1, 64)])
    d = torch.cat([torch.arange(16), (torch.arange(1, 64) * 7 + 3) % 64])
    return mg.graph((s.to(idtype), d.to(idtype)), num_nodes=64).to(dev)


def run_exclusion(dev, form=None):
    g = exclusion_graph(dev)
    if form == "out":  # only the out-CSR materialised: the sampler then checks existence in it
        g = g.formats(["coo", "csr"])
        g._index.csr()
        assert not g._index.has_format("csc")
    eids = (torch.arange(2000) % 16).to(dev)
    ns = Uniform(8, exclude_existing=True)
    src, dst = ns(g, eids, generator=torch.Generator().manual_seed(EXCL_SEED))
    assert ns.last_failed == 0 and dst.shape[0] == 16000
    assert bool((src == 0).all())
    assert int(dst.min()) >= 16 and int(dst.max()) < 64  # no output is an edge of source 0: all on the 48 allowed nodes
    assert not bool(g.has_edges_between(src, dst).any())
    p = torch.zeros(64, dtype=torch.float64)
    p[16:] = 1.0 / 48
    check_binomial(torch.bincount(dst.cpu(), minlength=64), p, 16000)
    return dst


def run_bounded(dev):
    n = 32
    full = mg.graph((torch.zeros(n, dtype=torch.int64), torch.arange(n)), num_nodes=n).to(dev)  # node 0 is adjacent to every node
    ns = Uniform(3, exclude_existing=True, max_tries=16)
    src, dst = ns(full, torch.tensor([0, 5], device=dev), generator=torch.Generator().manual_seed(0))
    assert ns.last_failed == 6 and src.shape == (0,) and dst.shape == (0,)
    raw, failed = negative_destinations(full._index, torch.zeros(2, dtype=torch.int64, device=dev), 3, 1, 64, 123)
    assert failed == 6 and raw.tolist() == [-1] * 6
    one = mg.graph((torch.tensor([0]), torch.tensor([0])), num_nodes=1).to(dev)
    ns = Uniform(4, exclude_self_loops=True, max_tries=5)
    src, dst = ns(one, torch.tensor([0], device=dev))
    assert ns.last_failed == 4 and dst.shape == (0,)
    src, dst = Uniform(4)(one, torch.tensor([0], device=dev))  # without the flag the only node is drawn
    assert dst.tolist() == [0] * 4


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_negative_sample_rejects_bad_arguments():
    """Through ctypes, no GPU needed: the argument checks come before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    csr = ctypes.byref(_lib.MgxCsr(4, 4, 2, p, p, None, 64, 0))
    seed = ctypes.c_uint64(1)
    assert L.mgx_negative_sample(None, 0, 2, p, 0, 4, 0, 16, seed, p, p, None) == 1
    assert b"k must be at least 1, got 0" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 4, 0, 0, seed, p, p, None) == 1
    assert b"max_tries must be in [1, 64], got 0" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 4, 0, 65, seed, p, p, None) == 1
    assert b"max_tries must be in [1, 64], got 65" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 4, 1, 16, seed, p, p, None) == 1
    assert b"csr is NULL with exclude_existing" in L.mgx_last_error()
    assert L.mgx_negative_sample(csr, 0, 2, p, 1, 4, 2, 16, seed, p, p, None) == 1
    assert b"csr must be NULL without exclude_existing" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, -2, p, 1, 4, 0, 16, seed, p, p, None) == 1
    assert b"negative size" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 2 ** 31, 0, 16, seed, p, p, None) == 1
    assert b"below 2^31" in L.mgx_last_error()
    assert L.mgx_negative_sample(csr, 0, 2, p, 1, 5, 1, 16, seed, p, p, None) == 1
    assert b"exceeds the graph's destination nodes" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 4, 8, 16, seed, p, p, None) == 1
    assert b"unknown flag bits" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 4, 0, 16, seed, p, None, None) == 1
    assert b"result is NULL" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, None, 1, 4, 0, 16, seed, p, p, None) == 1
    assert b"NULL pointer" in L.mgx_last_error()
    assert L.mgx_negative_sample(None, 0, 2, p, 1, 0, 0, 16, seed, p, p, None) == 1
    assert b"no destination node" in L.mgx_last_error()
    for bad in (dict(k=0), dict(k=2, max_tries=0), dict(k=2, max_tries=65)):
        with pytest.raises(mg.DGLError):
            Uniform(**bad)


@pytest.mark.parametrize("idtype", IDTYPES)
def test_exact_stream_cpu(idtype):
    run_exact_stream("cpu", idtype)


def test_reproducible_cpu():
    run_reproducible("cpu")


def test_exclusion_cpu():
    run_exclusion("cpu")


def test_bounded_tries_cpu():
    run_bounded("cpu")


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_exact_stream_gpu(idtype, monkeypatch):
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    on = run_exact_stream(DEV, idtype)
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    assert torch.equal(on, run_exact_stream(DEV, idtype))


@pytest.mark.gpu
def test_reproducible_and_forms_agree_gpu(monkeypatch):
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    on = run_reproducible(DEV)
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    off = run_reproducible(DEV)
    cpu = run_reproducible("cpu")
    for a, b, c in zip(on, off, cpu):
        assert torch.equal(a, b) and torch.equal(a.cpu(), c)


@pytest.mark.gpu
def test_exclusion_gpu(monkeypatch):
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    a, b = run_exclusion(DEV), run_exclusion(DEV, form="out")
    assert torch.equal(a, b) and torch.equal(a.cpu(), run_exclusion("cpu"))


@pytest.mark.gpu
def test_bounded_tries_gpu(monkeypatch):
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    run_bounded(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("idtype", IDTYPES)
def test_out_csr_and_in_csr_forms_agree_gpu(idtype, monkeypatch):
    """A dense little graph (every proposal is rejected about one time in four), both flags, few tries so that some draws fail."""
    g, s, d = random_graph(50, 600, 9, idtype, DEV)
    pos_src = s[torch.arange(0, 600, 2)].to(DEV)
    monkeypatch.setattr(config, "DEVICE_LINKPRED", True)
    outs = [negative_destinations(g._index, pos_src, 6, 3, 2, 77, form=form) for form in ("out", "in")]
    monkeypatch.setattr(config, "DEVICE_LINKPRED", False)
    outs.append(negative_destinations(g._index, pos_src, 6, 3, 2, 77))
    outs.append(negative_destinations(g.to("cpu")._index, pos_src.cpu(), 6, 3, 2, 77))
    dst0, failed0 = outs[0]
    assert failed0 == int((dst0 < 0).sum()) and 0 < failed0 < dst0.shape[0] // 4
    for dst, failed in outs[1:]:
        assert failed == failed0 and torch.equal(dst.cpu(), dst0.cpu())
    src = pos_src.repeat_interleave(6)
    ok = dst0 >= 0
    assert not bool(g.has_edges_between(src[ok], dst0[ok]).any()) and not bool((src[ok] == dst0[ok]).any())
