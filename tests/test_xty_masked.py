"""mgx_xty_colsum_masked (csrc/xty.hip): the weight and bias gradient of a layer behind relu + dropout with the mask applied as the kernel
loads the output gradient -- bit for bit relu_dropout_bwd followed by xty(colsum=True), which it replaces in layer 1's backward."""
import numpy as np
import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import _lib, config, ops, sparse

from conftest import random_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

NS = [1, 15, 16, 17, 4099, 70001]   # one row; either side of the 16-row step; a second trip of some waves (> 256 x 16); 320 partitions
KS = [64, 72, 128, 200, 256]        # one block; a block + a dword tile; a full block; the workload's 128 + 72; two full blocks
PS = [0.0, 0.5]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def be():
    return sparse.backend_for(torch.zeros(1, device=DEV))


@pytest.fixture(scope="module")
def operands(be):
    """Per (n, p), made once and never written again: dy as the left half of an [n, 128] matrix, with +Inf and NaN behind cleared mask
    bits; the mask of the library's own relu_dropout_fwd; b as the left columns of an [n, 264] matrix."""
    made = {}

    def get(n, p):
        if (n, p) not in made:
            gen = torch.Generator(device=DEV).manual_seed(1000 * n + int(p * 10))
            _, mask = be.relu_dropout_fwd(torch.randn(n, 64, device=DEV, generator=gen), p, 4242 + n, 77)
            keep = ((mask.view(n, 16, 1).to(torch.int32) >> torch.arange(4, device=DEV, dtype=torch.int32)) & 1).view(n, 64).bool()
            wide = torch.randn(n, 128, device=DEV, generator=gen)
            dy = wide[:, :64]
            pick = torch.rand(n, 64, device=DEV, generator=gen)
            dy[~keep & (pick < 0.05)] = float("inf")
            dy[~keep & (pick > 0.95)] = float("nan")
            if n > 1:
                assert bool(torch.isinf(dy).any()) and bool(torch.isnan(dy).any()) and bool(torch.isfinite(dy[keep]).all())
            made[(n, p)] = (wide, mask, torch.randn(n, 264, device=DEV, generator=gen))
        return made[(n, p)]

    return get


def _composition(be, dy, mask, p, b):
    return be.xty(be.relu_dropout_bwd(dy, mask, p), b, colsum=True)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_bitwise_the_composition(be, operands, n, K, p):
    wide, mask, bwide = operands(n, p)
    dy, b = wide[:, :64].contiguous(), bwide[:, :K].contiguous()
    want, want_s = _composition(be, dy, mask, p, b)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(want_s).all())
    for name, dy_, b_ in (("contiguous", dy, b), ("dy with lddy = 128", wide[:, :64], b), ("b with ldb = 264", dy, bwide[:, :K])):
        got = be.xty_masked(dy_, mask, p, b_)
        assert got is not None, name
        out, sums = got
        assert out.shape == (64, K) and sums.shape == (64,)
        assert torch.equal(_bits(out), _bits(want)), (name, float((out - want).abs().max()))
        assert torch.equal(_bits(sums), _bits(want_s)), (name, float((sums - want_s).abs().max()))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(sums).all())


def test_against_fp64_at_the_workload_shape(be, operands):
    """n = 70001, K = 200, p = 0.5: equal to the composition, which meets the fp64 bounds of test_gpu_parity (1e-5 of the largest sum of
    magnitudes for the product, 1e-5 of each column's for the sums)."""
    wide, mask, bwide = operands(70001, 0.5)
    dy, b = wide[:, :64].contiguous(), bwide[:, :200].contiguous()
    dz = be.relu_dropout_bwd(dy, mask, 0.5)
    want, want_s = be.xty(dz, b, colsum=True)
    out, sums = be.xty_masked(dy, mask, 0.5, b)
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(sums), _bits(want_s))
    ref = dz.double().t() @ b.double()
    scale = float((dz.double().abs().t() @ b.double().abs()).max())
    err = float((out.double() - ref).abs().max())
    print("xty_masked vs fp64: max err %.3e, bound %.3e" % (err, 1e-5 * scale))
    assert err <= 1e-5 * scale
    assert bool(((sums.double() - dz.double().sum(0)).abs() <= 1e-5 * dz.double().abs().sum(0) + 1e-30).all())


def test_unsupported_operands_launch_nothing(be, monkeypatch):
    n = 1000
    dy, mask = torch.randn(n, 64, device=DEV), torch.full((n * 16,), 15, dtype=torch.uint8, device=DEV)
    launched = []
    L = _lib.lib()

    class Spy(object):
        def __getattr__(self, name):
            if name == "mgx_xty_colsum_masked":
                def call(*a):
                    st = L.mgx_xty_colsum_masked(*a)
                    launched.append(st)
                    return st
                return call
            return getattr(L, name)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    assert be.xty_masked(dy, mask, 0.5, torch.randn(n, 60, device=DEV)) is None      # below one float4 group
    assert be.xty_masked(dy, mask, 0.5, torch.randn(n, 260, device=DEV)) is None     # beyond two blocks
    assert be.xty_masked(dy, mask, 0.5, torch.randn(n, 130, device=DEV)) is None     # not a multiple of 4
    shifted = torch.randn(n * 64 + 1, device=DEV)[1:].view(n, 64)                    # 4 bytes off a 16-byte boundary
    assert shifted.data_ptr() % 16 != 0
    assert be.xty_masked(shifted, mask, 0.5, torch.randn(n, 128, device=DEV)) is None
    assert be.xty_masked(torch.randn(n, 48, device=DEV), mask, 0.5, torch.randn(n, 128, device=DEV)) is None
    assert launched == []                                                            # refused before the library was entered
    # shapes the wrapper lets through and the library has no kernel for: MGX_ERR_UNSUPPORTED, returned before any launch
    for K in (100, 132, 160):   # a block + two dword tiles; a second block below one float4 group; a second block of 32 columns
        out = torch.full((64, K), 7.0, device=DEV)
        sums = torch.full((64,), 7.0, device=DEV)
        ws = torch.empty(L.mgx_xty_masked_workspace(K) // 4, device=DEV)
        b = torch.randn(n, K, device=DEV)
        st = L.mgx_xty_colsum_masked(n, K, dy.data_ptr(), 64, mask.data_ptr(), 0.5, b.data_ptr(), K, out.data_ptr(), K, sums.data_ptr(),
                                     ws.data_ptr(), None)
        torch.cuda.synchronize()
        assert st == _lib.ERR_UNSUPPORTED and float(out.min()) == 7.0 and float(sums.min()) == 7.0
        assert be.xty_masked(dy, mask, 0.5, b) is None
    assert L.mgx_xty_masked_workspace(60) == -1 and L.mgx_xty_masked_workspace(260) == -1 and L.mgx_xty_masked_workspace(130) == -1


NL = 70001


@pytest.fixture(scope="module")
def layer_world():
    src, dst = random_graph(NL, NL, 8 * NL, seed=17, skew=True)
    g = mg.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=NL).int().formats(["csr", "csc"]).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(9)
    return {"g": g, "x": torch.randn(NL, 100, device=DEV, generator=gen),
            "params": [torch.randn(64, 100, device=DEV, generator=gen) * 0.1, torch.randn(64, 100, device=DEV, generator=gen) * 0.1,
                       torch.randn(64, device=DEV, generator=gen)],
            "dy": torch.randn(NL, 64, device=DEV, generator=gen)}


def _layer_grads(w, monkeypatch, on):
    monkeypatch.setattr(config, "XTY_MASKED", on)
    torch.manual_seed(23)
    ops.ReluDropout._calls = 0
    ws, wn, b = [p.clone().requires_grad_(True) for p in w["params"]]
    cat = ops.CatBuffer(NL, 100, DEV)
    y = ops.sage_mean_layer_act(w["g"], w["x"], ws, wn, b, cat, 0.5, None)
    assert y is not None
    y.backward(w["dy"])
    return y.detach(), [ws.grad, wn.grad, b.grad]


def test_layer_one_takes_it_and_keeps_its_gradients(layer_world, monkeypatch):
    """ops.sage_mean_layer_act on a 100-column input that takes no gradient: the three parameter gradients with the switch on are those
    with it off, bit for bit, and the on-path never runs the elementwise backward."""
    calls = {"bwd": 0, "masked": 0}
    real_bwd, real_masked = sparse.HipBackend.relu_dropout_bwd, sparse.HipBackend.xty_masked

    def spy_bwd(self, *a, **k):
        calls["bwd"] += 1
        return real_bwd(self, *a, **k)

    def spy_masked(self, *a, **k):
        r = real_masked(self, *a, **k)
        calls["masked"] += r is not None
        return r

    monkeypatch.setattr(sparse.HipBackend, "relu_dropout_bwd", spy_bwd)
    monkeypatch.setattr(sparse.HipBackend, "xty_masked", spy_masked)
    y_off, off = _layer_grads(layer_world, monkeypatch, False)
    assert calls == {"bwd": 1, "masked": 0}
    y_on, on = _layer_grads(layer_world, monkeypatch, True)
    assert calls == {"bwd": 1, "masked": 1}
    assert torch.equal(_bits(y_on), _bits(y_off))
    for name, a_, b_ in zip(("d W_self", "d W_neigh", "d bias"), on, off):
        assert a_.shape == b_.shape and torch.equal(_bits(a_), _bits(b_)), (name, float((a_ - b_).abs().max()))
    # the environment switch restores the composition too
    monkeypatch.setenv("MGX_XTY_MASKED", "0")
    _, env_off = _layer_grads(layer_world, monkeypatch, True)
    assert calls == {"bwd": 2, "masked": 1}
    assert all(torch.equal(_bits(a_), _bits(b_)) for a_, b_ in zip(env_off, off))
    monkeypatch.delenv("MGX_XTY_MASKED")
    # a backend method that declines: the layer takes the sequence it had
    monkeypatch.setattr(sparse.HipBackend, "xty_masked", lambda self, *a, **k: None)
    _, declined = _layer_grads(layer_world, monkeypatch, True)
    assert calls["bwd"] == 3
    assert all(torch.equal(_bits(a_), _bits(b_)) for a_, b_ in zip(declined, off))
