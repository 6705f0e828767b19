"""ops.segment_mha (csrc/segmha.hip) and nn.SetTransformerEncoder / SetTransformerDecoder against one fp64 restatement: a Python loop
over the segments, softmax(scale q_g k_g^T) v_g, gradients from fp64 autograd of sum(out * g).

Tolerance of the random-value tests: per tensor max|got - ref| <= 4 * max|composed fp32 - ref| + 2^-22 * max|ref|, the composed form of the
same operator on the same operands as the yardstick (docs/LOG_segment_mha.md records the ratios).  The exact-structure test has q = 0,
so that every weight is 1 / n: out and d v within (n + 4) * 2^-24 * sum|terms| per element, d k exactly 0, reruns bitwise equal."""
import copy

import pytest
import torch

import mi355x_graph as mg
from mi355x_graph import DGLError, config, nn as mnn, ops

DEV = "cuda:0"
KV = [0, 1, 15, 16, 17, 63, 64, 65, 130, 0]
QL = [3, 0, 1, 16, 17, 5, 1, 64, 2, 4]
NAMES = ("out", "d q", "d k", "d v")


def reference(q, k, v, q_seglen, kv_seglen=None, scale=None, **_):
    """the fp64 loop over segments; differentiable"""
    ql = [int(x) for x in q_seglen]
    kl = ql if kv_seglen is None else [int(x) for x in kv_seglen]
    scale, out, qb, kb = q.shape[2] ** -0.5 if scale is None else scale, [], 0, 0
    for nq, nk in zip(ql, kl):
        a = torch.softmax(torch.einsum("qhf,khf->hqk", q[qb:qb + nq], k[kb:kb + nk]) * scale, -1)
        out.append(torch.einsum("hqk,khf->qhf", a, v[kb:kb + nk]) if nk else q.new_zeros((nq,) + q.shape[1:]))
        qb, kb = qb + nq, kb + nk
    return torch.cat(out, 0)


def run(fn, q, k, v, g, dev=DEV, dtype=torch.float32):
    """(out, d q, d k, d v) of fn on fresh leaves"""
    q, k, v = (x.detach().to(dev, dtype).requires_grad_(True) for x in (q, k, v))
    out = fn(q, k, v)
    (out * g.to(dev, dtype)).sum().backward()
    return tuple(x.detach().double().cpu() for x in (out, q.grad, k.grad, v.grad))


def operands(nq, nk, H, F, integer=False, seed=0):
    gen = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.randint(-3, 4, s, generator=gen).float()) if integer else (lambda *s: torch.randn(*s, generator=gen))
    return draw(nq, H, F), draw(nk, H, F), draw(nk, H, F), draw(nq, H, F)


def check(got, yardstick, ref, names=NAMES):
    """the tolerance rule: `yardstick` is the composed fp32 form (the kernel where `got` is the composed form)"""
    for name, x, y, want in zip(names, got, yardstick, ref):
        err, yard = float((x - want).abs().max()), float((y - want).abs().max())
        print("%s: max error %.3g, yardstick %.3g, ratio %.2f" % (name, err, yard, err / max(yard, 1e-30)))
        assert yard <= 2.0 ** -12 * float(want.abs().max()), name  # (the yardstick itself is sane: fp32 sums of at most 130 terms)
        assert err <= 4 * yard + 2.0 ** -22 * float(want.abs().max()), name


def three_ways(monkeypatch, q, k, v, g, ql, kl):
    """(kernel, composed fp32, fp64 reference) of one call; the kernel must be the path taken"""
    lens = [None if x is None else torch.tensor(x, device=DEV) for x in (ql, kl)]
    call = lambda q, k, v: ops.segment_mha(q, k, v, lens[0], lens[1], q_total=q.shape[0], kv_total=k.shape[0])  # noqa: E731
    assert ops.segment_mha_fused(q.to(DEV), k.to(DEV), v.to(DEV), lens[0], lens[1], q_total=q.shape[0], kv_total=k.shape[0]) is True
    got = run(call, q, k, v, g)
    with monkeypatch.context() as m:
        m.setattr(config, "SEGMENT_MHA_FUSED", False)
        composed = run(call, q, k, v, g)
    return got, composed, run(lambda q, k, v: reference(q, k, v, ql, kl), q, k, v, g, "cpu", torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(1, 4), (3, 16), (2, 20), (4, 32), (1, 64)])
def test_values_and_gradients(monkeypatch, H, F):
    q, k, v, g = operands(sum(KV), sum(KV), H, F)
    check(*three_ways(monkeypatch, q, k, v, g, KV, None))


@pytest.mark.gpu
def test_exact_structure():
    _, k, v, g = operands(sum(KV), sum(KV), 2, 16, integer=True)
    k, q = torch.randn(k.shape, generator=torch.Generator().manual_seed(1)), torch.zeros_like(k)
    lens = torch.tensor(KV, device=DEV)
    call = lambda q, k, v: ops.segment_mha(q, k, v, lens, q_total=q.shape[0])  # noqa: E731
    assert ops.segment_mha_fused(q.to(DEV), k.to(DEV), v.to(DEV), lens, q_total=q.shape[0]) is True
    got, again = run(call, q, k, v, g), run(call, q, k, v, g)
    ref = run(lambda q, k, v: reference(q, k, v, KV), q, k, v, g, "cpu", torch.float64)
    mag = run(lambda q, k, v: reference(q, k, v, KV), q, k, v.abs(), g.abs(), "cpu", torch.float64)
    n = torch.repeat_interleave(torch.tensor(KV), torch.tensor(KV)).double().view(-1, 1, 1)
    for i in (0, 3):
        assert bool(((got[i] - ref[i]).abs() <= (n + 4) * 2.0 ** -24 * mag[i]).all()), NAMES[i]
    assert torch.equal(got[2], torch.zeros_like(got[2]))
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.gpu
def test_cross_form(monkeypatch):
    q, k, v, g = operands(sum(QL), sum(KV), 2, 16)
    got, composed, ref = three_ways(monkeypatch, q, k, v, g, QL, KV)
    check(got, composed, ref)
    qo, ko = torch.tensor([0] + QL).cumsum(0), torch.tensor([0] + KV).cumsum(0)
    for s in (0, 9):  # queries facing an empty key segment
        assert not got[0][qo[s]:qo[s + 1]].any() and not got[1][qo[s]:qo[s + 1]].any()
    assert not got[2][ko[1]:ko[2]].any() and not got[3][ko[1]:ko[2]].any()  # keys facing an empty query segment


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["qkv_blocks", "odd_offset", "host_seglen", "switch_off"])
def test_layouts_and_predicate(monkeypatch, layout):
    H, F, n = 2, 16, sum(KV)
    q, k, v, g = (x.to(DEV) for x in operands(n, n, H, F))
    lens = torch.tensor(KV, device="cpu" if layout == "host_seglen" else DEV)
    plain, fused = (q, k, v), layout in ("qkv_blocks", "host_seglen")
    if layout == "qkv_blocks":
        qkv = torch.cat([x.reshape(n, H * F) for x in plain], 1)
        q, k, v = (qkv[:, i * H * F:(i + 1) * H * F].unflatten(1, (H, F)) for i in range(3))
    elif layout == "odd_offset":
        q = torch.cat([q.new_zeros(1), q.reshape(-1)])[1:].view(n, H, F)
    elif layout == "switch_off":
        monkeypatch.setattr(config, "SEGMENT_MHA_FUSED", False)
    assert ops.segment_mha_fused(q, k, v, lens, q_total=n) is fused
    got = run(lambda q, k, v: ops.segment_mha(q, k, v, lens, q_total=n), q, k, v, g)
    monkeypatch.setattr(config, "SEGMENT_MHA_FUSED", True)
    kernel = run(lambda q, k, v: ops.segment_mha(q, k, v, lens, q_total=n), *plain, g)  # the kernel on contiguous copies
    if fused:
        assert all(torch.equal(a, b) for a, b in zip(got, kernel))
    else:  # the composed form against the kernel: the rule of test_values_and_gradients the other way round
        check(got, kernel, run(lambda q, k, v: reference(q, k, v, KV), *plain, g, "cpu", torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["fp64_q", "k_2d", "wrong_total", "v_on_cpu"])
def test_operand_errors(bad):
    q, k, v, _ = (x.to(DEV) for x in operands(sum(KV), sum(KV), 2, 16))
    lens = torch.tensor(KV)
    if bad == "fp64_q":
        q = q.double()
    elif bad == "k_2d":
        k = k.view(k.shape[0], -1)
    elif bad == "wrong_total":
        lens = lens + 1
    else:
        v = v.cpu()
    assert ops.segment_mha_fused(q, k, v, lens) is False
    with pytest.raises(DGLError):
        ops.segment_mha(q, k, v, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sab", "isab", "decoder"])
def test_layers(monkeypatch, kind):
    torch.manual_seed(0)
    lens = [1, 3, 16, 17, 40]
    import dgl
    bg = dgl.batch([mg.graph((torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)), num_nodes=n) for n in lens]).to(DEV)
    layer = (mnn.SetTransformerDecoder(32, 4, 8, 64, 1, k=2) if kind == "decoder" else
             mnn.SetTransformerEncoder(32, 4, 8, 64, block_type=kind, m=4 if kind == "isab" else None)).to(DEV).eval()
    feat, shape = torch.randn(sum(lens), 32), (5, 64) if kind == "decoder" else (sum(lens), 32)
    up = torch.randn(shape)

    def result(module, dev, dtype):
        module.zero_grad()
        out = module(bg, feat.to(dev, dtype))
        (out * up.to(dev, dtype)).sum().backward()
        weight = next(p for name, p in module.named_parameters() if name.endswith("proj_k.weight"))
        return out.detach().double().cpu(), weight.grad.detach().double().cpu()

    exact = copy.deepcopy(layer).double().cpu()
    for m in exact.modules():
        if isinstance(m, mnn.MultiHeadAttention):
            m.attend = lambda q, k, v, lx, lm, *_: reference(q, k, v, lx.tolist(), None if lm is None else lm.tolist())
    got, ref = result(layer, DEV, torch.float32), result(exact, "cpu", torch.float64)
    assert tuple(got[0].shape) == shape
    with monkeypatch.context() as m:
        m.setattr(config, "SEGMENT_MHA_FUSED", False)
        composed = result(layer, DEV, torch.float32)
    check(got, composed, ref, ("output", "d proj_k.weight"))
