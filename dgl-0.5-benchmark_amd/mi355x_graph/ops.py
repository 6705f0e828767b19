"""Autograd-aware g-SpMM / g-SDDMM / edge_softmax / segment_reduce -- the dgl.ops surface.

Signatures follow the reference call sites:
  dgl.ops.gspmm(g, op, reduce_op, lhs_data, rhs_data)            kernel/dgl-new.py:20
  dgl.ops.gsddmm(g, op, lhs_data, rhs_data, lhs_target, rhs_target)   kernel/dgl-new.py:39
  edge_softmax(graph, logits, eids=ALL, norm_by='dst')           via GATConv, main_dgl_reddit_gat.py:10
Backward formulas are DGL's: dU of a sum-SpMM is the same SpMM on the reversed
graph (out-CSR), dE is an SDDMM, etc.  `mean` is fused: the forward kernel divides by
max(in_degree, 1) and the backward SpMM scales the gathered rows by the same factor, instead of
DGL's separate elementwise divide.
Graph readout over the row segments of a batched graph: segment_reduce, segment_softmax and segment_attention (the fused
softmax-weighted sum of dgl.nn.GlobalAttentionPooling / Set2Set, csrc/segattn.hip); readout.py has DGL's sum_nodes ... softmax_nodes.
"""
import os

import torch
from torch.autograd.function import once_differentiable

from ._lib import DGLError
from . import sparse
from . import config
from .graph import DGLGraph, GraphIndex

__all__ = ["gspmm", "rel_gspmm", "gsddmm", "edge_softmax", "gat_attention", "gat_fused", "dot_attention", "dot_attention_fused", "gine_sum", "gine_sum_fused", "multi_aggregate", "multi_aggregate_fused", "segment_reduce", "segment_softmax", "segment_attention", "segment_attention_fused", "segment_topk", "segment_topk_fused", "segment_knn", "segment_knn_fused", "segment_knn_query", "segment_knn_query_fused", "segment_fps", "segment_fps_fused", "segment_ball_query", "segment_ball_query_fused", "copy_u_sum", "copy_u_mean", "u_mul_e_sum",
           "copy_e_sum", "u_add_v", "u_dot_v"]


def _torch_ops():
    """MGX_TORCH_OPS=1 (tests): EVERY raw primitive goes through torch.ops.mi355x_graph.* and the fused layer forms of this module
    are switched off, so that a model exercises exactly the registered operator surface."""
    if os.environ.get("MGX_TORCH_OPS", "auto") != "1":
        return None
    from . import torch_ops
    return torch_ops


_STREAM_STEP = 0x9E3779B97F4A7C15  # 2^64 / golden ratio: what one call moves a counter-based dropout generator on by

_NATIVE = None


def _native_ops():
    """Default route of the generic operators behind update_all() / apply_edges() on HIP tensors: the C++ dispatcher ops
    (csrc/torch_bind.cpp, TORCH_LIBRARY(mi355x_graph)) -- 5.6 us of host time per call against 13.2 us through ctypes and 22.8 us
    for a Python-registered op (experiments/exp_host_overhead.py; eager molhiv epoch 0.92 -> 0.80 s).  MGX_TORCH_OPS=0 restores
    the ctypes route; a tree without libmi355x_graph_torch.so uses it as well."""
    global _NATIVE
    if os.environ.get("MGX_TORCH_OPS", "auto") == "0":
        return None
    if _NATIVE is None:
        from . import torch_ops
        _NATIVE = torch_ops if torch_ops.NATIVE else False
    return _NATIVE or _torch_ops()


def _gspmm_over_slots(csr, op, reduce_op, X):
    """copy_u / sum|mean of a [N, 64] float32 operand over a big CSR as 128-byte slots (csrc/spmm_slots.inc) when X MAY be mostly zero:
    a relu + dropout output that reaches update_all() through plain torch modules (the reference's own model code,
    main_dgl_product_sage.py:61-64, 93-96) carries no tag, so X is packed and the overflow count decides -- this CSR's gate stops the
    probing for 64 calls whenever more than a tenth of the rows turn out to hold more than 24 non-zeros.  Exact either way.  None: not
    applicable (the caller takes the dense kernels)."""
    if (not config.PACKED_GATHER or not config.PACKED_GATHER_PROBE or op != "copy_lhs" or reduce_op not in ("sum", "mean") or X is None
            or X.dim() != 2 or X.shape[1] != 64 or not X.is_cuda or X.dtype != torch.float32 or csr.nnz < config.PACKED_GATHER_MIN_NNZ
            or X.shape[0] != csr.num_cols or X.device.type not in sparse._BACKENDS):
        return None
    be = sparse.backend_for(X)
    if not hasattr(be, "rows_slots_pack") or capture_path():
        return None
    plan, short = csr.spmm_plan_for(64)
    if short and (plan is None or plan.rest is None):
        return None
    if csr._gate is None:
        csr._gate = _SlotGate()
    gate = csr._gate
    gate.calls += 1
    if gate.calls <= gate.dense_until:
        return None
    if not X.is_contiguous():
        X = X.contiguous()
    if not be.rows_slots_supported(X, csr):
        return None
    # the decision belongs to THIS operand, so its count is read back here (one host read per probed call): which kernels a call takes
    # -- and with them the order of additions, i.e. the bits -- depends on the operands and the sequence of calls only, never on timing
    slots, overflow = be.rows_slots_pack(X)
    gate.last_fraction = float(int(overflow)) / max(int(X.shape[0]), 1)
    if gate.last_fraction > config.PACKED_GATHER_MAX_OVERFLOW:
        gate.dense_until = gate.calls + 64
        return None
    out = torch.empty((csr.num_rows, 64), dtype=torch.float32, device=X.device)
    return be.spmm_copy_u_strided(csr, reduce_op, X, out, slots=slots)


def _raw_gspmm(csr, op, reduce_op, X, Y, want_arg=False, probe=True):
    if probe and not want_arg and Y is None:
        out = _gspmm_over_slots(csr, op, reduce_op, X)
        if out is not None:
            return out, None, None
    t = _native_ops()
    if t is None or not (X if X is not None else Y).is_cuda:
        return sparse.gspmm_raw(csr, op, reduce_op, X, Y, want_arg=want_arg)
    return t.raw_gspmm(csr, op, reduce_op, X, Y, want_arg)


def _raw_gsddmm(gidx, op, X, Y, lhs_target="u", rhs_target="v"):
    t = _native_ops()
    ref = X if X is not None else Y
    if t is None or ref is None or not ref.is_cuda:
        return sparse.gsddmm_raw(gidx, op, X, Y, lhs_target, rhs_target)
    return t.raw_gsddmm(gidx, op, X, Y, lhs_target, rhs_target)


def _gidx(g):
    if isinstance(g, DGLGraph):
        return g._index
    if isinstance(g, GraphIndex):
        return g
    raise DGLError("expected a DGLGraph, got %s" % type(g))


def _reduce_grad(grad, shape):
    """Sum `grad` over the dims that were broadcast so that it has `shape` (rows excluded)."""
    grad_shape = tuple(grad.shape[1:])
    in_shape = tuple(shape[1:])
    if in_shape == grad_shape:
        return grad
    num_to_squeeze = len(grad_shape) - len(in_shape)
    in_shape = (1,) * num_to_squeeze + in_shape
    reduce_idx = [i + 1 for i, (a, b) in enumerate(zip(grad_shape, in_shape)) if a != b]
    if reduce_idx:
        grad = grad.sum(dim=tuple(reduce_idx), keepdim=True)
    return grad.view((-1,) + tuple(shape[1:]))


def _need_reduce_last_dim(ushp, eshp):
    """(N,H,F) x (E,H,1): the edge gradient is a per-head dot product."""
    return ushp[1:-1] == eshp[1:-1] and eshp[-1] == 1 and ushp[-1] > 1


def _align(a, b):
    """a and b (rows first) with their FEATURE dimensions right-aligned, the way sparse._bcast_plan aligns them for the kernels:
    (E, 4) against (E, 2, 4) becomes (E, 1, 4) -- plain torch would line the row dimension of one up with a feature dimension of
    the other."""
    nd = max(a.dim(), b.dim())

    def pad(t):
        return t if t.dim() == nd else t.reshape((t.shape[0],) + (1,) * (nd - t.dim()) + tuple(t.shape[1:]))
    return pad(a), pad(b)


def _expand(x, like):
    """x broadcast to the feature shape of `like`, feature dimensions right-aligned first (_align): the operand of a max / min
    backward `gather` may have fewer of them than the gradient, (N, 4) against (N_dst, 2, 4)."""
    return _align(x, like)[0].expand(-1, *like.shape[1:])


class GSpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gidx, op, reduce_op, X, Y):
        csc = gidx.csc()
        want_arg = reduce_op in ("max", "min")
        out, argX, argY = _raw_gspmm(csc, op, reduce_op, X, Y, want_arg=want_arg)
        ctx.backward_cache = gidx, op, reduce_op
        ctx.x_shape = None if X is None else X.shape
        ctx.y_shape = None if Y is None else Y.shape
        req_x = X is not None and X.requires_grad
        req_y = Y is not None and Y.requires_grad
        save_x = X if (req_y and op == "mul") else None
        save_y = Y if (req_x and op == "mul") or (want_arg and op == "mul") else None
        if want_arg and op == "mul":
            save_x = X
        ctx.save_for_backward(save_x, save_y, argX, argY)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dZ):
        gidx, op, reduce_op = ctx.backward_cache
        X, Y, argX, argY = ctx.saved_tensors
        dZ = dZ.contiguous()
        dX = dY = None
        summing = reduce_op in ("sum", "mean")
        if summing:
            # mean: d(sum/deg) -> scale dZ rows by 1/max(deg,1) once (one streaming pass) instead of a
            # per-edge 4-byte gather of the factor inside the reversed SpMM (measured +20 % there)
            dZs = dZ
            if reduce_op == "mean":
                inv = gidx.csc().inv_degrees()
                dZs = dZ * inv.view((-1,) + (1,) * (dZ.dim() - 1))
            if op != "copy_rhs" and ctx.needs_input_grad[3]:
                rev = gidx.csr()  # rows = src: the reversed graph's in-CSR
                if op == "mul":
                    dX, _, _ = _raw_gspmm(rev, "mul", "sum", dZs, Y)
                elif config.SPARSE_GRAD and _torch_ops() is None:
                    dX = sparse.gspmm_grad_raw(rev, dZs)  # measured variant: flags the gradient's all-zero rows and skips them
                else:  # add, copy_lhs: aggregation of the gradient over the reversed graph (a gradient is dense: not probed for slots)
                    dX = _raw_gspmm(rev, "copy_lhs", "sum", dZs, None, probe=False)[0]
                dX = _reduce_grad(dX, ctx.x_shape)
            if op != "copy_lhs" and ctx.needs_input_grad[4]:
                if op == "mul":
                    if _need_reduce_last_dim(ctx.x_shape, ctx.y_shape):
                        dY = _raw_gsddmm(gidx, "dot", X, dZs, "u", "v")
                    else:
                        dY = _raw_gsddmm(gidx, "mul", X, dZs, "u", "v")
                else:  # add, copy_rhs
                    dY = _raw_gsddmm(gidx, "copy_rhs", None, dZs, "u", "v")
                dY = _reduce_grad(dY, ctx.y_shape)
        else:  # max / min: route dZ through the arg indices; empty rows (arg = -1) contribute nothing
            if op != "copy_rhs" and ctx.needs_input_grad[3]:
                valid = (argX >= 0)
                idx = argX.clamp(min=0).long()
                g = dZ
                if op == "mul":
                    yexp = _expand(Y, dZ) if Y.shape[1:] != dZ.shape[1:] else Y
                    g = dZ * yexp.gather(0, argY.clamp(min=0).long())
                g = g * valid
                full = torch.zeros((ctx.x_shape[0],) + tuple(dZ.shape[1:]), dtype=dZ.dtype, device=dZ.device)
                full.scatter_add_(0, idx, g)
                dX = _reduce_grad(full, ctx.x_shape)
            if op != "copy_lhs" and ctx.needs_input_grad[4]:
                valid = (argY >= 0)
                idx = argY.clamp(min=0).long()
                g = dZ
                if op == "mul":
                    xexp = _expand(X, dZ) if X.shape[1:] != dZ.shape[1:] else X
                    g = dZ * xexp.gather(0, argX.clamp(min=0).long())
                g = g * valid
                full = torch.zeros((ctx.y_shape[0],) + tuple(dZ.shape[1:]), dtype=dZ.dtype, device=dZ.device)
                full.scatter_add_(0, idx, g)
                dY = _reduce_grad(full, ctx.y_shape)
        return None, None, None, dX, dY


class GSDDMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gidx, op, X, Y, lhs_target, rhs_target):
        out = _raw_gsddmm(gidx, op, X, Y, lhs_target, rhs_target)
        ctx.backward_cache = gidx, op, lhs_target, rhs_target
        ctx.x_shape = None if X is None else X.shape
        ctx.y_shape = None if Y is None else Y.shape
        req_x = X is not None and X.requires_grad
        req_y = Y is not None and Y.requires_grad
        needs_other = op in ("mul", "dot", "div")
        ctx.save_for_backward(X if (needs_other and (req_y or op == "div")) else None,
                              Y if (needs_other and (req_x or req_y)) else None)
        return out

    @staticmethod
    def _to_target(gidx, target, edge_grad):
        """Sum per-edge gradients back onto their target set."""
        if target == "e":
            return edge_grad
        view = gidx.csr() if target == "u" else gidx.csc()
        out, _, _ = _raw_gspmm(view, "copy_rhs", "sum", None, edge_grad)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dZ):
        gidx, op, lt, rt = ctx.backward_cache
        X, Y = ctx.saved_tensors
        dZ = dZ.contiguous()
        dX = dY = None
        if op != "copy_rhs" and ctx.needs_input_grad[2]:
            if op in ("add", "sub", "copy_lhs"):
                dX = GSDDMM._to_target(gidx, lt, dZ)
            elif op in ("mul", "dot", "div"):
                if lt == "u" and rt == "v" and op in ("mul", "dot"):
                    # dX[u] = sum_{e: u->v} Y[v] * dZ[e]: a mul-SpMM on the reversed graph
                    dX, _, _ = _raw_gspmm(gidx.csr(), "mul", "sum", Y, dZ)
                elif lt == "v" and rt == "u" and op in ("mul", "dot"):
                    dX, _, _ = _raw_gspmm(gidx.csc(), "mul", "sum", Y, dZ)
                else:
                    y_e = _raw_gsddmm(gidx, "copy_rhs", None, Y, lt, rt) if rt != "e" else Y
                    dz, y_e = _align(dZ, y_e)
                    ge = dz * y_e if op in ("mul", "dot") else dz / y_e
                    dX = GSDDMM._to_target(gidx, lt, ge.contiguous())
            dX = _reduce_grad(dX, ctx.x_shape)
        if op != "copy_lhs" and ctx.needs_input_grad[3]:
            if op in ("add", "copy_rhs"):
                dY = GSDDMM._to_target(gidx, rt, dZ)
            elif op == "sub":
                dY = GSDDMM._to_target(gidx, rt, (-dZ).contiguous())
            elif op in ("mul", "dot"):
                if lt == "u" and rt == "v":  # the same route as dX above
                    dY, _, _ = _raw_gspmm(gidx.csc(), "mul", "sum", X, dZ)
                elif lt == "v" and rt == "u":
                    dY, _, _ = _raw_gspmm(gidx.csr(), "mul", "sum", X, dZ)
                else:
                    x_e = _raw_gsddmm(gidx, "copy_lhs", X, None, lt, rt) if lt != "e" else X
                    dz, x_e = _align(dZ, x_e)
                    dY = GSDDMM._to_target(gidx, rt, (dz * x_e).contiguous())
            else:  # div: d(x/y)/dy = -x / y^2
                x_e = _raw_gsddmm(gidx, "copy_lhs", X, None, lt, rt) if lt != "e" else X
                y_e = _raw_gsddmm(gidx, "copy_rhs", None, Y, lt, rt) if rt != "e" else Y
                dz, x_e = _align(dZ, x_e)
                dz, y_e = _align(dz, y_e)
                dY = GSDDMM._to_target(gidx, rt, (-dz * x_e / (y_e * y_e)).contiguous())
            dY = _reduce_grad(dY, ctx.y_shape)
        return None, None, dX, dY, None, None


class EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gidx, score, norm_by):
        view = gidx.csc() if norm_by == "dst" else gidx.csr()
        t = _native_ops()
        if t is not None and score.is_cuda:
            if score.dtype != torch.float32 or score.shape[0] != view.nnz:
                raise DGLError("edge_softmax: expected float32 logits with %d rows, got %s %s" % (view.nnz, score.dtype, tuple(score.shape)))
            with torch.no_grad():
                out = torch.ops.mi355x_graph.edge_softmax_fwd(*t.csr_args(view), score.contiguous(), t.softmax_plan_handle(view))
        else:
            out = sparse.edge_softmax_fwd_raw(view, score)
        ctx.backward_cache = view
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, grad_out):
        view = ctx.backward_cache
        out, = ctx.saved_tensors
        return None, sparse.edge_softmax_bwd_raw(view, out, grad_out.contiguous()), None


class GATAttention(torch.autograd.Function):
    """a = edge_softmax(leaky_relu(el[u] + er[v])) in one launch; d el / d er by two copy_e g-SpMMs of the fused de."""

    @staticmethod
    def forward(ctx, gidx, el, er, slope):
        csc = gidx.csc()
        if el.shape[0] != csc.num_cols or er.shape[0] != csc.num_rows:  # the kernel indexes el by source id, er by row
            raise DGLError("gat_attention: expected el with %d source rows and er with %d destination rows, got %d and %d"
                           % (csc.num_cols, csc.num_rows, el.shape[0], er.shape[0]))
        shape = el.shape[1:]
        el2, er2 = el.contiguous().view(el.shape[0], -1), er.contiguous().view(er.shape[0], -1)
        a = sparse.backend_for(el2).gat_attention_fwd(csc, el2, er2, float(slope))
        ctx.backward_cache = gidx, float(slope), shape
        ctx.save_for_backward(a, el2, er2)
        return a.view((a.shape[0],) + tuple(shape))

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, da):
        gidx, slope, shape = ctx.backward_cache
        a, el2, er2 = ctx.saved_tensors
        de = sparse.backend_for(a).gat_attention_bwd(gidx.csc(), el2, er2, slope, a, da.contiguous().view(a.shape))
        d_el = d_er = None
        if ctx.needs_input_grad[1]:
            d_el, _, _ = sparse.gspmm_raw(gidx.csr(), "copy_rhs", "sum", None, de)
            d_el = d_el.view((el2.shape[0],) + tuple(shape))
        if ctx.needs_input_grad[2]:
            d_er, _, _ = sparse.gspmm_raw(gidx.csc(), "copy_rhs", "sum", None, de)
            d_er = d_er.view((er2.shape[0],) + tuple(shape))
        return None, d_el, d_er, None


def gat_attention(graph, el, er, negative_slope=0.2):
    """Fused apply_edges(u_add_v) -> leaky_relu -> edge_softmax (norm_by='dst').  el: (N_src, H[, 1]), er: (N_dst, H[, 1])."""
    if el.dtype != torch.float32 or er.dtype != torch.float32:
        raise DGLError("gat_attention expects float32 attention terms")
    if el.shape[1:] != er.shape[1:]:
        raise DGLError("gat_attention: el %s and er %s disagree" % (tuple(el.shape[1:]), tuple(er.shape[1:])))
    return GATAttention.apply(_gidx(graph), el, er, negative_slope)


class GATFused(torch.autograd.Function):
    """out[v,h,:] = sum_e dropout(softmax_{e->v}(leaky_relu(el[u] + er[v])))[e,h] * feat[u,h,:] -- GATConv's whole
    message-passing block (main_dgl_reddit_gat.py:31-55) in two launches forward and two backward, with no E-sized
    tensor: the attention of an edge is rebuilt from per-node statistics where it is needed (csrc/gatfused.hip)."""

    _calls = 0  # advances the counter-based generator: a new mask per call, reproducible after torch.manual_seed

    @staticmethod
    def forward(ctx, gidx, feat, el, er, slope, p, attn_l=None):
        csc = gidx.csc()
        H, F = int(feat.shape[1]), int(feat.shape[2])
        if attn_l is not None:  # el IS (feat * attn_l).sum(-1): the kernels may form it from the gathered row (no gradient flows
            attn_l = attn_l.detach().contiguous().view(H, F)  # through this argument: d_el goes back through el's own producer)
        if el.shape[0] != csc.num_cols or er.shape[0] != csc.num_rows or feat.shape[0] != csc.num_cols:
            raise DGLError("gat_fused: expected feat / el with %d source rows and er with %d destination rows, got %d / %d / %d"
                           % (csc.num_cols, csc.num_rows, feat.shape[0], el.shape[0], er.shape[0]))
        feat = feat.contiguous()
        el2, er2 = el.contiguous().view(el.shape[0], H), er.contiguous().view(er.shape[0], H)
        seed = 0
        if p > 0.0:
            seed = ((torch.initial_seed() & (2 ** 64 - 1)) ^ ((GATFused._calls * _STREAM_STEP) & (2 ** 64 - 1)))
            GATFused._calls += 1
        be = sparse.backend_for(feat)
        if p > 0.0 and be.name == "hip":  # training with attn_drop: the backward needs the out-CSR anyway; the forward's choice of kernel too
            out, nstat, form = be.gat_fused_fwd(csc, feat, el2, er2, float(slope), float(p), seed, attn_l, csr=gidx.csr())
        else:
            out, nstat, form = be.gat_fused_fwd(csc, feat, el2, er2, float(slope), float(p), seed, attn_l)
        ctx.backward_cache = gidx, float(slope), float(p), seed, el.shape, er.shape, attn_l, form
        ctx.save_for_backward(feat, el2, out, nstat)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_out):
        gidx, slope, p, seed, el_shape, er_shape, attn_l, form = ctx.backward_cache
        feat, el2, out, nstat = ctx.saved_tensors
        need_src = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        d_feat, d_el, d_er = sparse.backend_for(feat).gat_fused_bwd(gidx.csc(), gidx.csr(), feat, el2, slope, p, seed, out,
                                                                     d_out.contiguous(), nstat, need_src, attn_l, form=form)
        return (None, d_feat if ctx.needs_input_grad[1] else None,
                d_el.view(el_shape) if (d_el is not None and ctx.needs_input_grad[2]) else None,
                d_er.view(er_shape) if ctx.needs_input_grad[3] else None, None, None, None)


def gat_fused_supported(graph, feat):
    gidx = _gidx(graph)
    return (feat.dim() == 3 and feat.dtype == torch.float32 and feat.is_cuda and os.environ.get("MGX_GAT_FUSED", "1") == "1"
            and sparse.backend_for(feat).name == "hip"
            and sparse.backend_for(feat).gat_fused_supported(gidx.csc(), int(feat.shape[1]), int(feat.shape[2])))


def gat_fused(graph, feat, el, er, negative_slope=0.2, attn_drop=0.0, training=True, attn_l=None):
    """GATConv's u_add_v -> leaky_relu -> edge_softmax -> attn_drop -> u_mul_e/sum block.  feat (N_src, H, F),
    el (N_src, H[, 1]), er (N_dst, H[, 1]) -> (N_dst, H, F).  Check gat_fused_supported() first.
    `attn_l` (1 | -, H, F): pass it when el is exactly (feat * attn_l).sum(-1) -- multi-head layers then form el from the gathered
    feature row inside the kernels instead of gathering it (one L2 request per edge less)."""
    if feat.dtype != torch.float32 or el.dtype != torch.float32 or er.dtype != torch.float32:
        raise DGLError("gat_fused expects float32 inputs")
    p = float(attn_drop) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise DGLError("gat_fused: attn_drop must be in [0, 1), got %g" % p)
    if p > 0.0 and feat.is_cuda and capture_path():
        raise DGLError("gat_fused: attn_drop > 0 under HIP-graph capture would replay ONE dropout mask (the seed is a launch "
                       "argument); use the unfused operators there, as GATConv does")
    return GATFused.apply(_gidx(graph), feat, el, er, negative_slope, p, attn_l)


class DotAttention(torch.autograd.Function):
    """out[v,h,:] = sum_e softmax_{e->v}(scale <q[v,h,:], k[u,h,:]>)[e,h] v[u,h,:] -- dgl.nn.DotGatConv's whole message-passing block
    in one walk forward and two backward, with no E-sized tensor: the attention of an edge is rebuilt from the per-row statistics
    where it is needed (csrc/dotattn.hip)."""

    @staticmethod
    def forward(ctx, gidx, q, k, v, scale):
        # k and v that are one tensor -- or two views of the same memory -- are gathered once
        same = k is v or (k.data_ptr() == v.data_ptr() and k.stride() == v.stride())
        out, stat = sparse.backend_for(q).dot_attention_fwd(gidx.csc(), q, k, k if same else v, float(scale))
        ctx.backward_cache = gidx, float(scale), same
        ctx.save_for_backward(q, k, v, out, stat)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_out):
        gidx, scale, same = ctx.backward_cache
        q, k, v, out, stat = ctx.saved_tensors
        need = ctx.needs_input_grad
        dq, dk, dv = sparse.backend_for(q).dot_attention_bwd(gidx.csc(), gidx.csr(), q, k, k if same else v, scale, out,
                                                             d_out.contiguous(), stat, need[1], need[2], need[3])
        return None, dq, dk, dv, None


def _dot_attention_args(graph, q, k, v):
    """The graph index of a dot_attention call, or DGLError."""
    gidx = _gidx(graph)
    _want_tensor("dot_attention", "q [N_dst, H, F] and k, v [N_src, H, F]", (q, k, v), 3)
    if (q.shape[0] != gidx.num_dst or k.shape[0] != gidx.num_src or v.shape[0] != gidx.num_src or q.shape[1:] != k.shape[1:]
            or k.shape[1:] != v.shape[1:]):
        raise DGLError("dot_attention: expected q [%d, H, F] and k, v [%d, H, F], got q %s, k %s, v %s"
                       % (gidx.num_dst, gidx.num_src, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    return gidx


def _dot_attention_kernel_ok(gidx, q, k, v):
    if (not _device_kernels(q, config.DOT_ATTENTION_FUSED, "dot_attention_fwd") or k.device != q.device or v.device != q.device
            or gidx.num_edges() == 0):
        return False
    return sparse.backend_for(q).dot_attention_supported(gidx.csc(), int(q.shape[1]), int(q.shape[2]))


def dot_attention_fused(graph, q, k, v):
    """True when dot_attention(graph, q, k, v) runs the fused kernels (else it is u_dot_v -> edge_softmax -> u_mul_e/sum)."""
    try:
        return _dot_attention_kernel_ok(_dot_attention_args(graph, q, k, v), q, k, v)
    except DGLError:
        return False


def dot_attention(graph, q, k, v, scale=None):
    """Scaled dot-product attention over a graph: out[v,h,:] = sum_{e: u->v} a[e,h] v[u,h,:] with a = edge_softmax(scale * u_dot_v(k, q)).

    q: [N_dst, H, F], k, v: [N_src, H, F] (fp32; row-strided views such as column blocks of one projection are taken without a copy),
    scale: default F ** -0.5; result [N_dst, H, F], exactly 0 for destinations without in-edges.  Device operands with F in {4, 8, 16, 32,
    64} and H*F <= 256 on an int32 graph run csrc/dotattn.hip (dot_attention_fused); everything else takes
    gspmm(g, "mul", "sum", v, edge_softmax(g, gsddmm(g, "dot", k, q, "u", "v") * scale)) -- the same values through the existing operators."""
    gidx = _dot_attention_args(graph, q, k, v)
    scale = float(q.shape[2]) ** -0.5 if scale is None else float(scale)
    if not _dot_attention_kernel_ok(gidx, q, k, v):
        return gspmm(gidx, "mul", "sum", v, edge_softmax(gidx, gsddmm(gidx, "dot", k, q, "u", "v") * scale))
    return DotAttention.apply(gidx, q, k, v, scale)


class GineSum(torch.autograd.Function):
    """out[v,:] = sum_{e: u->v} s[e] relu(x[u,:] + w[e,:]) -- a `s * relu(src.x + edge.w)` UDF message reduced with fn.sum, in one walk
    of the in-CSR forward and one of the out-CSR backward (d x and d w together), with no E-sized temporary: the relu mask is rebuilt
    from x and w where it is needed (csrc/gine.hip).  Saves x, w and scale only."""

    @staticmethod
    def forward(ctx, gidx, x, w, scale):
        x, w = x.contiguous(), w.contiguous()
        scale = None if scale is None else scale.contiguous()
        out = sparse.backend_for(x).gine_fwd(gidx.csc(), x, w, scale)
        ctx.gidx, ctx.has_scale = gidx, scale is not None
        ctx.save_for_backward(*((x, w, scale) if scale is not None else (x, w)))
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_out):
        x, w = ctx.saved_tensors[:2]
        scale = ctx.saved_tensors[2] if ctx.has_scale else None
        need = ctx.needs_input_grad
        d_x, d_w = sparse.backend_for(x).gine_bwd(ctx.gidx.csr(), x, w, scale, d_out.contiguous(), need[1], need[2])
        return None, d_x, d_w, None


def _gine_args(graph, x, w, scale):
    """(graph index, scale as [E] or None) of a gine_sum call, or DGLError."""
    gidx = _gidx(graph)
    _want_tensor("gine_sum", "x [N_src, D] and w [E, D]", (x, w), 2)
    E = gidx.num_edges()
    if x.shape[0] != gidx.num_src or w.shape[0] != E or w.shape[1] != x.shape[1]:
        raise DGLError("gine_sum: expected x [%d, D] and w [%d, D], got x %s, w %s" % (gidx.num_src, E, tuple(x.shape), tuple(w.shape)))
    if scale is not None:
        if not torch.is_tensor(scale) or tuple(scale.shape) not in ((E,), (E, 1)):
            raise DGLError("gine_sum: expected scale [%d] or [%d, 1], got %s"
                           % (E, E, tuple(scale.shape) if torch.is_tensor(scale) else type(scale).__name__))
        if scale.dtype != torch.float32:
            raise DGLError("gine_sum expects float32 inputs, got %s / %s / %s" % (x.dtype, w.dtype, scale.dtype))
        if scale.requires_grad:
            raise DGLError("gine_sum: scale gets no gradient; pass it detached")
        scale = scale.reshape(E)
    return gidx, scale


def _gine_kernel_ok(gidx, x, w, scale):
    if (not _device_kernels(x, config.GINE_FUSED, "gine_fwd", "gine_bwd") or w.device != x.device
            or (scale is not None and scale.device != x.device) or gidx.num_edges() == 0 or not _aligned16(x, w)):
        return False
    return sparse.backend_for(x).gine_supported(gidx.csc(), int(x.shape[1]))


def gine_sum_fused(graph, x, w, scale=None):
    """True when gine_sum(graph, x, w, scale) runs the fused kernels (else it is gather -> add -> relu -> mul -> copy_e/sum)."""
    try:
        gidx, scale = _gine_args(graph, x, w, scale)
        return _gine_kernel_ok(gidx, x, w, scale)
    except DGLError:
        return False


def gine_sum(graph, x, w, scale=None):
    """Sum of relu messages with edge features: out[v,:] = sum_{e: u->v} scale[e] * relu(x[u,:] + w[e,:]).

    x: [N_src, D], w: [E, D] and scale: [E] | [E, 1] | None (= 1) by edge id, fp32; result [N_dst, D], exactly 0 for destinations without
    in-edges.  scale gets no gradient.  Device operands (16-byte aligned) with D % 4 == 0 and 4 <= D <= 256 on an int32 graph run csrc/gine.hip
    (gine_sum_fused) and write nothing of size E but d w; everything else takes
    gspmm(g, "copy_rhs", "sum", None, relu(gsddmm(g, "copy_lhs", x, None, "u", "v") + w) * scale) -- the same values through the existing
    operators."""
    gidx, scale = _gine_args(graph, x, w, scale)
    if gidx.num_edges() == 0:
        return _no_edges_zeros((gidx.num_dst, x.shape[1]), x, w)
    if not _gine_kernel_ok(gidx, x, w, scale):
        m = torch.relu(gsddmm(gidx, "copy_lhs", x, None, "u", "v") + w)
        if scale is not None:
            m = m * scale.unsqueeze(-1)
        return gspmm(gidx, "copy_rhs", "sum", None, m)
    return GineSum.apply(gidx, x, w, scale)


class MultiAggregate(torch.autograd.Function):
    """out[v, a, :] = aggregate a of the messages m_e = x[u] (+ w[e]) into v, a in sum | mean | var | std | max | min, all from ONE walk of
    the in-CSR; the backward forms the per-destination rows A, B (N-sized) and returns d x and d w from ONE walk of the out-CSR
    (csrc/multiagg.hip).  Saves x, w, the int32 args of max / min and the [N_dst, 2, D] (mean, var) statistics (save_for_backward: a later in-place
    write to any of them is caught); nothing of size E."""

    @staticmethod
    def forward(ctx, gidx, x, w, aggregators, eps):
        x = x.contiguous()
        w = None if w is None else w.contiguous()
        out, arg_max, arg_min, stats = sparse.backend_for(x).multi_agg_fwd(gidx.csc(), x, w, aggregators, eps)
        ctx.gidx, ctx.aggregators, ctx.eps = gidx, aggregators, eps
        ctx.save_for_backward(x, w, arg_max, arg_min, stats)  # the args and (mean, var) of this call: absent ones are None
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_out):
        x, w, arg_max, arg_min, stats = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[1], w is not None and ctx.needs_input_grad[2]
        if not (need_x or need_w):
            return None, None, None, None, None
        g = {name: d_out[:, i, :] for i, name in enumerate(ctx.aggregators)}
        deg = ctx.gidx.in_degrees().to(torch.float32).clamp(min=1).unsqueeze(-1)   # rows without in-edges are met by no edge
        A = g["sum"] if "sum" in g else None
        if "mean" in g:
            A = g["mean"] / deg if A is None else A + g["mean"] / deg
        B = None
        if stats is not None:                                                          # the mask var > 0 from the forward's stored bits
            mean, var = stats[:, 0, :], stats[:, 1, :]
            gv = g["var"] if "var" in g else None
            if "std" in g:
                gs = g["std"] / (2 * torch.sqrt(var + ctx.eps))
                gv = gs if gv is None else gv + gs
            B = (2 * torch.where(var > 0, gv, torch.zeros_like(gv)) / deg).contiguous()
            A = -(B * mean) if A is None else A - B * mean
        A = x.new_zeros(d_out.shape[0], d_out.shape[2]) if A is None else A.contiguous()
        g_max = g["max"].contiguous() if "max" in g else None
        g_min = g["min"].contiguous() if "min" in g else None
        d_x, d_w = sparse.backend_for(x).multi_agg_bwd(ctx.gidx.csr(), x, w, A, B, g_max, arg_max, g_min, arg_min, need_x, need_w)
        return None, d_x, d_w, None, None


MULTI_AGGREGATORS = ("sum", "mean", "max", "min", "var", "std")


def _multi_agg_args(graph, x, aggregators, w, eps):
    """(graph index, aggregators as a tuple, eps as a float) of a multi_aggregate call, or DGLError."""
    gidx = _gidx(graph)
    _want_tensor("multi_aggregate", "x [N_src, D] and w [E, D] or None", (x,) if w is None else (x, w), 2)
    E = gidx.num_edges()
    if x.shape[0] != gidx.num_src or (w is not None and (w.shape[0] != E or w.shape[1] != x.shape[1])):
        raise DGLError("multi_aggregate: expected x [%d, D] and w [%d, D], got x %s, w %s"
                       % (gidx.num_src, E, tuple(x.shape), None if w is None else tuple(w.shape)))
    if isinstance(aggregators, str) or not hasattr(aggregators, "__iter__"):
        raise DGLError("multi_aggregate: aggregators must be a sequence of names, got %r" % (aggregators,))
    aggregators = tuple(aggregators)
    if not aggregators:
        raise DGLError("multi_aggregate: aggregators is empty")
    for name in aggregators:
        if name not in MULTI_AGGREGATORS:
            raise DGLError("multi_aggregate: unknown aggregator %r (one of %s)" % (name, ", ".join(MULTI_AGGREGATORS)))
    if len(set(aggregators)) != len(aggregators):
        raise DGLError("multi_aggregate: repeated aggregator in %r" % (aggregators,))
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise DGLError("multi_aggregate: eps must be a number, got %r" % (eps,))
    if not (eps > 0 and eps != float("inf")):
        raise DGLError("multi_aggregate: eps must be positive and finite, got %r" % (eps,))
    return gidx, aggregators, eps


def _multi_agg_kernel_ok(gidx, x, aggregators, w):
    """Device operands in the kernels' supported set, the switch on, and not the one case the composition was measured to win -- a single
    sum or mean without w, or a single max or min without w on a small batch (config.MULTI_AGG_SINGLE_*)."""
    E = gidx.num_edges()
    if (not _device_kernels(x, config.MULTI_AGG_FUSED, "multi_agg_fwd", "multi_agg_bwd") or (w is not None and w.device != x.device)
            or E == 0 or not _aligned16(x, w)):
        return False
    # one plain aggregate without w composes to a single g-SpMM; below the measured crossover that one wins (config.py, docs/LOG_pna.md)
    if w is None and len(aggregators) == 1:
        if aggregators[0] in ("sum", "mean") and not config.MULTI_AGG_SINGLE_SUM_FUSED:
            return False
        if aggregators[0] in ("max", "min") and x.shape[1] <= config.MULTI_AGG_SINGLE_MAX_D and E < config.MULTI_AGG_SINGLE_MIN_EDGES:
            return False
    return sparse.backend_for(x).multi_agg_supported(gidx.csc(), int(x.shape[1]))


def multi_aggregate_fused(graph, x, aggregators=("mean", "max", "min", "std"), w=None, eps=1e-30):
    """True when multi_aggregate(graph, x, aggregators, w, eps) runs the fused kernels (else it is one gspmm per aggregate)."""
    try:
        gidx, aggregators, _ = _multi_agg_args(graph, x, aggregators, w, eps)
        return _multi_agg_kernel_ok(gidx, x, aggregators, w)
    except DGLError:
        return False


def _multi_aggregate_composed(gidx, x, aggregators, w, eps):
    """The same values through the existing operators: one g-SpMM per aggregate (two for var / std), over the [E, D] messages
    gsddmm(copy_lhs) + w when the edges carry features."""
    if w is None:
        def reduce(r, square=False):
            return gspmm(gidx, "copy_lhs", r, x * x if square else x, None)
    else:
        m = gsddmm(gidx, "copy_lhs", x, None, "u", "v") + w

        def reduce(r, square=False):
            return gspmm(gidx, "copy_rhs", r, None, m * m if square else m)
    got = {}
    if "var" in aggregators or "std" in aggregators:
        got["mean"] = reduce("mean")
        got["var"] = torch.relu(reduce("mean", True) - got["mean"] * got["mean"])
        if "std" in aggregators:
            some = (gidx.in_degrees() > 0).unsqueeze(-1)
            got["std"] = torch.where(some, torch.sqrt(got["var"] + eps), torch.zeros_like(got["var"]))   # a row without in-edges: 0
    for name in aggregators:
        if name not in got:
            got[name] = reduce(name)
    return torch.stack([got[name] for name in aggregators], dim=1)


def multi_aggregate(graph, x, aggregators, w=None, eps=1e-30):
    """Several aggregates of the same messages at once (Principal Neighbourhood Aggregation): with m_e = x[u,:] (+ w[e,:], w by edge id)
    and d the in-degree of v,

        sum = S1 = sum_e m_e,  mean = S1 / d,  var = relu(sum_e m_e^2 / d - mean^2),  std = sqrt(var + eps),  max,  min

    returned as [N_dst, A, D] in the order of `aggregators` (a non-empty sequence of distinct names out of sum, mean, max, min, var, std).
    x: [N_src, D], w: [E, D] | None, fp32.  A destination without in-edges gives 0 in every aggregate, std included.  max / min follow
    gspmm's rule (the first of equal extrema in storage order takes the whole gradient, a NaN never wins).  Gradients go to x and w.
    Device operands (16-byte aligned) with D % 4 == 0 and 4 <= D <= 256 on an int32 graph run csrc/multiagg.hip
    (multi_aggregate_fused): one walk forward, one backward, nothing of size E but d w; everything else -- and a single plain aggregate
    without w where that one g-SpMM was measured to win (config.MULTI_AGG_SINGLE_*) -- is composed of gspmm
    (copy_lhs, or copy_rhs over gsddmm(copy_lhs) + w) with a second mean over the squares -- the same values through the existing operators."""
    gidx, aggregators, eps = _multi_agg_args(graph, x, aggregators, w, eps)
    if gidx.num_edges() == 0:
        return _no_edges_zeros((gidx.num_dst, len(aggregators), x.shape[1]), x, w)
    if not _multi_agg_kernel_ok(gidx, x, aggregators, w):
        return _multi_aggregate_composed(gidx, x, aggregators, w, eps)
    return MultiAggregate.apply(gidx, x, w, aggregators, eps)


class HeadDot(torch.autograd.Function):
    """(out_a, out_b)[n, h] = <feat[n, h, :], attn_{a,b}[h, :]>: one pass over feat forward, one pass backward."""

    @staticmethod
    def forward(ctx, feat, attn_a, attn_b):
        feat = feat.contiguous()
        H, F = feat.shape[1], feat.shape[2]
        a2 = attn_a.contiguous().view(H, F)
        b2 = attn_b.contiguous().view(H, F) if attn_b is not None else None
        out_a, out_b = sparse.backend_for(feat).head_dot_fwd(feat, a2, b2)
        ctx.save_for_backward(feat, a2, b2)
        ctx.attn_shape = attn_a.shape
        if out_b is None:  # autograd Functions return tensors only: an empty placeholder that carries no gradient
            out_b = feat.new_empty(0)
            ctx.mark_non_differentiable(out_b)
        return out_a, out_b

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_a, d_b):
        feat, a2, b2 = ctx.saved_tensors
        if d_a is None:
            d_a = torch.zeros(feat.shape[:2], dtype=feat.dtype, device=feat.device)
        if b2 is not None and d_b is None:
            d_b = torch.zeros(feat.shape[:2], dtype=feat.dtype, device=feat.device)
        d_feat, g_a, g_b = sparse.backend_for(feat).head_dot_bwd(
            feat, a2, b2, d_a.contiguous(), d_b.contiguous() if b2 is not None else None, ctx.needs_input_grad[0])
        return d_feat, g_a.view(ctx.attn_shape), (g_b.view(ctx.attn_shape) if g_b is not None else None)


def head_dot_supported(feat):
    return feat.dim() == 3 and feat.dtype == torch.float32 and sparse.backend_for(feat).head_dot_supported(
        int(feat.shape[1]), int(feat.shape[2]))


def head_dot(feat, attn_a, attn_b=None):
    """GATConv's `(feat * attn).sum(-1)`: feat (n, H, F), attn (1, H, F) -> (n, H); with attn_b both terms in one pass."""
    if feat.dtype != torch.float32:
        raise DGLError("head_dot expects float32 features")
    out_a, out_b = HeadDot.apply(feat, attn_a, attn_b)
    return out_a if attn_b is None else (out_a, out_b)


class LinearFn(torch.autograd.Function):
    """y = x W^T + b with the library's GEMMs; the bias gradient (column sum of dY over all N rows) runs in
    mgx_column_sum -- PyTorch's generic reduction needs 19 ms for a [2.4M, 47] column sum on MI355X, 40 % of a products epoch."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ weight).view(x.shape)
        if ctx.needs_input_grad[1]:
            dw = _weight_grad(dy2, x.reshape(-1, x.shape[-1]))
        if ctx.needs_input_grad[2]:
            db = sparse.backend_for(dy2).column_sum(dy2.contiguous())
        return dx, dw, db


class BiasAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        ctx.bias_shape = bias.shape
        return x + bias

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        db = None
        if ctx.needs_input_grad[1]:
            C = 1
            for d in ctx.bias_shape:
                C *= int(d)
            db = sparse.backend_for(dy).column_sum(dy.contiguous().view(-1, C)).view(ctx.bias_shape)
        return dy, db


def bias_add(x, bias):
    """x + bias (bias broadcast over the leading dimension of x) with the bias gradient computed by mgx_column_sum."""
    C = bias.numel()
    if x.dim() >= 2 and x[0].numel() == C:
        bias = bias.view((1,) + tuple(x.shape[1:]))
    if (not bias.requires_grad or x.dtype != torch.float32 or x.device.type not in sparse._BACKENDS or x.dim() < 2
            or x[0].numel() != C or C > sparse.backend_for(x).COLUMN_SUM_MAX):
        return x + bias
    return BiasAdd.apply(x, bias)


class ReluDropout(torch.autograd.Function):
    _calls = 0  # advances the counter-based generator: a new mask per call, reproducible after torch.manual_seed

    @staticmethod
    def forward(ctx, x, p, into=None):
        # `into` wraps the destination view in a plain object: handed over as a Tensor argument it would be an autograd INPUT
        # modified in place; created here it is simply this node's output (a view of a buffer autograd does not track)
        out = None if into is None else into.t
        be = sparse.backend_for(x)
        if out is None or not be._row_strided(x):
            x = x.contiguous()
        if capture_path():
            # a HIP graph freezes launch arguments: the position in the random stream comes from a device counter that the
            # captured step itself advances, so every replay draws a new mask
            ctr = _capture_counter(x.device)
            y, mask = be.relu_dropout_fwd(x, float(p), torch.initial_seed() & (2 ** 64 - 1), 0, out=out, counter=ctr)
            ctr.add_(1)
        else:
            seed, offset = _dropout_stream_position()
            y, mask = be.relu_dropout_fwd(x, float(p), seed, offset, out=out)
        ctx.save_for_backward(mask)
        ctx.p = float(p)
        return y

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        be = sparse.backend_for(dy)
        if not dy.is_contiguous() and not be._row_strided(dy):
            dy = dy.contiguous()
        return be.relu_dropout_bwd(dy, mask, ctx.p), None, None


def _dropout_stream_position():
    """(seed, offset) of the next relu + dropout mask in the counter-based generator's stream -- taken by every eager call that draws one,
    ReluDropout and the layers with the activation in their GEMM's epilogue alike -- and the stream moved on by one call."""
    offset = (ReluDropout._calls * _STREAM_STEP) & (2 ** 63 - 1)
    ReluDropout._calls += 1
    return torch.initial_seed() & (2 ** 64 - 1), offset


_WARMING_UP_FOR_CAPTURE = 0


def capture_path():
    """True while the current stream is being captured into a HIP graph AND during the eager warm-up steps that precede a
    capture (utils.GraphedStep, graph_classification.GraphedBatchTrainer): operators that choose a different form under
    capture must choose it in the warm-up too, so that everything the captured form needs -- BLAS handles, workspaces,
    lazily built plans -- exists before the capture starts."""
    return _WARMING_UP_FOR_CAPTURE > 0 or torch.cuda.is_current_stream_capturing()


_CAPTURE_COUNTERS = {}


def _capture_counter(device):
    """One int64 counter per device, advanced by every captured relu_dropout call (created outside any capture: warm-up)."""
    c = _CAPTURE_COUNTERS.get(device)
    if c is None:
        c = _CAPTURE_COUNTERS[device] = torch.full((1,), 1 << 20, dtype=torch.int64, device=device)
    return c


class warming_up_for_capture(object):
    def __enter__(self):
        global _WARMING_UP_FOR_CAPTURE
        _WARMING_UP_FOR_CAPTURE += 1

    def __exit__(self, *exc):
        global _WARMING_UP_FOR_CAPTURE
        _WARMING_UP_FOR_CAPTURE -= 1
        return False


def relu_dropout(x, p=0.5, training=True, out=None):
    """dropout(relu(x), p) in one pass each way (float32 HIP tensors with numel % 4 == 0; anything else and evaluation mode
    take the two PyTorch ops).  Under HIP-graph capture the mask's position in the random stream is read from a device
    counter that the captured step advances, so replays draw new masks.  `out`: a [rows, cols] view with
    unit column stride, a row stride that is a multiple of 4 and a 16-byte aligned base to write the result into (a column block of a
    wider matrix); any other `out`, and the PyTorch path, ignore it.  x itself may lie anywhere: what the kernels cannot read in
    place the backend copies (sparse.dense16)."""
    if (not training or p <= 0.0 or p >= 1.0 or x.dtype != torch.float32 or x.device.type != "cuda" or x.numel() % 4
            or x.device.type not in sparse._BACKENDS
            or (capture_path() and (x.dim() != 2 or x.shape[1] % 4 or x.stride(1) != 1 or x.stride(0) % 4))):
        return _structural_zeros(torch.nn.functional.dropout(torch.relu(x), p, training))
    if out is not None and (x.dim() != 2 or x.shape[1] % 4 or out.shape != x.shape or out.stride(1) != 1 or out.stride(0) % 4
                            or out.stride(0) < out.shape[1] or out.data_ptr() % 16 or out.requires_grad):
        out = None
    return _structural_zeros(ReluDropout.apply(x, p, None if out is None else _Into(out)))


def _structural_zeros(y):
    """Tag a relu (+ dropout) output: its zeros are structural -- this node's backward multiplies whatever gradient arrives at a zero
    position by zero -- which lets a partition's halo exchange send the row as bitmap + non-zeros and take back only the gradient
    entries under that bitmap (dist.SparseHalo).  A plain attribute on the tensor object: it does not survive further ops."""
    y._mgx_structural_zeros = int(y._version)  # (an in-place write afterwards bumps the version and voids the tag: dist.structural_zeros)
    return y


def has_structural_zeros(t):
    """True when `t` carries _structural_zeros' tag and has not been written in place since."""
    tagged = getattr(t, "_mgx_structural_zeros", None)
    return tagged is not None and tagged is not False and int(tagged) == int(t._version)


class _SlotGate(object):
    """Whether a graph's forward aggregations of relu + dropout outputs take the 128-byte-slot form (csrc/spmm_slots.inc).  The form is
    exact at any density -- a row with more than 24 non-zeros is read from the dense matrix -- but only pays while such rows are rare, so
    every producer leaves its overflow count in pinned host memory (asynchronously) and the NEXT call reads it -- waiting for it if it
    should not have arrived yet, so that the decision is a function of the operands and the call sequence, not of timing: above
    config.PACKED_GATHER_MAX_OVERFLOW of the rows the dense kernels take the following 64 calls."""
    __slots__ = ("pending", "host", "dense_until", "calls", "last_fraction")

    def __init__(self):
        self.pending, self.host, self.dense_until, self.calls, self.last_fraction = None, None, 0, 0, None

    def allow(self):
        self.calls += 1
        if self.pending is not None:
            # WAIT for the previous producer's count (it was recorded right behind that kernel, at least one aggregation ago: arrived in
            # practice) rather than ask whether it happens to be there: the decision must not depend on timing, or reruns would differ
            self.pending[0].synchronize()
            self.last_fraction = float(self.host[0]) / max(self.pending[1], 1)
            self.pending = None
            if self.last_fraction > config.PACKED_GATHER_MAX_OVERFLOW:
                self.dense_until = self.calls + 64
        return self.calls > self.dense_until

    def open(self):
        """allow() without counting a call: asked by the PRODUCER of the rows (should its epilogue write the slots as well?)."""
        return self.calls >= self.dense_until

    def watch(self, overflow, n):
        if self.pending is not None:
            return
        if self.host is None:
            self.host = torch.empty(1, dtype=torch.int64).pin_memory()
        self.host.copy_(overflow, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending = (ev, int(n))


def _slot_gate(be, gidx, csc, n):
    """The gate of `gidx` when the forward aggregation of an [n, 64] relu + dropout output over `csc` may take the slot form at all."""
    if (not config.PACKED_GATHER or csc.nnz < config.PACKED_GATHER_MIN_NNZ or not hasattr(be, "rows_slots_pack") or capture_path()
            or csc.idx_bits != 32 or csc.num_cols != n or n >= (1 << 25) or csc.tile_plan(64) is not None):
        return None
    plan, short = csc.spmm_plan_for(64)
    if short and (plan is None or plan.rest is None):
        return None  # every work item is short: the lane-group kernel walks them all, nothing would read the slots
    gate = getattr(gidx, "_slot_gate", None)
    if gate is None:
        gate = gidx._slot_gate = _SlotGate()
    return gate


def _edge_tail_operands(be, csc, cat, h):
    """(block_a, edge_tail) of the layer's CONSTANT input h [N, 100] for mgx_spmm_copy_u_edge_tail, laid out on first use and kept on the
    layer's CatBuffer while h is the same unmodified tensor (the key CatBuffer.static_key already holds); None: the one-matrix form."""
    if (not config.EDGE_TAIL or cat.K != 100 or h.requires_grad or cat.static_key is None or cat.static_key[0] is not h
            or cat.static_key[1] != h._version or csc.nnz < config.EDGE_TAIL_MIN_NNZ or not hasattr(be, "edge_tail_of") or capture_path()):
        return None
    held = cat.static_tail
    if held is not None and held[0][0] is h and held[0][1] == h._version and held[0][2] is csc:
        return held[1]
    ops_ = be.edge_tail_of(csc, h)
    cat.static_tail = ((h, h._version, csc), ops_) if ops_ is not None else None
    return ops_


def _packed_rows(be, gidx, csc, h, left):
    """The 128-byte slots of `left` (== h, a [N, 64] relu + dropout output) for the forward aggregation over `csc`, or None: the dense
    rows.  The layer that produced h may have written them already (h._mgx_slots, the GEMM epilogue of sage_mean_layer_act)."""
    if left.shape[1] != 64 or not has_structural_zeros(h):
        return None
    gate = _slot_gate(be, gidx, csc, left.shape[0])
    if gate is None or not gate.allow():
        return None
    made = getattr(h, "_mgx_slots", None)
    if made is not None and made[2] == int(h._version) and made[0].shape[0] == left.shape[0]:
        slots, overflow = made[0], made[1]
    elif be.rows_slots_supported(left, csc):
        slots, overflow = be.rows_slots_pack(left)
    else:
        return None
    gate.watch(overflow, left.shape[0])
    return slots


class _Into(object):
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


class BatchNormFn(torch.autograd.Function):
    """Training-mode BatchNorm1d over the rows of x [N, C]: two column reductions + one per-column affine map each way
    (mgx_column_pair_sums / mgx_column_affine).  Returns (y, batch mean, biased batch variance)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        be = sparse.backend_for(x)
        n = x.shape[0]
        # sums relative to the first row p: E[(x-p)^2] - E[x-p]^2 has O(std) terms, so |mean| >> std does not cancel
        s, ss = be.column_pair_sums(x, shifted=True)
        m1 = s / n
        mean = x[0] + m1
        var = (ss / n - m1 * m1).clamp_(min=0.0)
        invstd = torch.rsqrt(var + eps)
        A = invstd if weight is None else weight * invstd
        Cc = -mean * A if bias is None else bias - mean * A
        y = be.column_affine(x, A.contiguous(), Cc.contiguous())
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _dmean, _dvar):
        x, weight, mean, invstd = ctx.saved_tensors
        dy = dy.contiguous()
        be = sparse.backend_for(dy)
        n = x.shape[0]
        sdy, sdyx = be.column_pair_sums(dy, x, shifted=True)  # sum dy * (x - x[0])
        sdyxhat = (sdyx - (mean - x[0]) * sdy) * invstd
        A = invstd if weight is None else weight * invstd
        B = -A * invstd * sdyxhat / n
        Cc = -A * sdy / n - B * mean
        dx = be.column_affine(dy, A.contiguous(), Cc.contiguous(), x, B.contiguous()) if ctx.needs_input_grad[0] else None
        dw = sdyxhat if weight is not None and ctx.needs_input_grad[1] else None
        db = sdy if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


def batch_norm_supported(x):
    return (x.dim() == 2 and x.dtype == torch.float32 and x.device.type in sparse._BACKENDS and x.shape[1] % 4 == 0
            and 4 <= x.shape[1] <= sparse.backend_for(x).COLUMN_SUM_MAX and x.shape[0] > 1)


def _weight_grad(dy2, x2):
    be = sparse.backend_for(dy2)
    if (x2.shape[0] >= be.XTY_MIN_ROWS and dy2.shape[1] <= be.XTY_MAX[0] and x2.shape[1] <= be.XTY_MAX[1]
            and config.LINEAR_XTY):
        # millions of rows, <= 64 x 128 outputs: streamed once; mgx_xty takes row strides, so a column slice (the [:, :D] view of
        # a line-padded aggregation) is read in place
        return be.xty(dy2 if dy2.stride(1) == 1 else dy2.contiguous(), x2 if x2.stride(1) == 1 else x2.contiguous())
    return dy2.t() @ x2


def _weight_bias_grad(dy2, x2):
    """(dy^T x, column sums of dy): the weight and the bias gradient of a dense layer from ONE pass over dy where mgx_xty_colsum applies."""
    be = sparse.backend_for(dy2)
    if (x2.shape[0] >= be.XTY_MIN_ROWS and dy2.shape[1] <= be.XTY_MAX[0] and x2.shape[1] <= be.XTY_MAX[1]
            and config.LINEAR_XTY and config.XTY_COLSUM):
        return be.xty(dy2 if dy2.stride(1) == 1 else dy2.contiguous(), x2 if x2.stride(1) == 1 else x2.contiguous(), colsum=True)
    return _weight_grad(dy2, x2), be.column_sum(dy2 if dy2.is_contiguous() else dy2.contiguous())


def _xty_masked_wanted(be, dy2, x2):
    """The conditions of _weight_bias_grad's one-pass form, for a backend that has the masked kernel (config.XTY_MASKED; MGX_XTY_MASKED=0:
    the composition relu_dropout_bwd + xty)."""
    return (config.XTY_MASKED and os.environ.get("MGX_XTY_MASKED", "1") != "0" and hasattr(be, "xty_masked") and dy2.dim() == 2
            and x2.shape[0] >= be.XTY_MIN_ROWS and dy2.shape[1] <= be.XTY_MAX[0] and x2.shape[1] <= be.XTY_MAX[1]
            and config.LINEAR_XTY and config.XTY_COLSUM)


class LinearSumFn(torch.autograd.Function):
    """y = x1 W1^T + x2 W2^T + b in two GEMMs, the second accumulating into the first's output (no separate add pass);
    gradients as LinearFn.  SAGEConv's `fc_self(h) + fc_neigh(h_neigh)` (main_dgl_product_sage.py:64)."""

    @staticmethod
    def forward(ctx, x1, w1, x2, w2, bias):
        ctx.save_for_backward(x1, w1, x2, w2)
        y = torch.nn.functional.linear(x1, w1, bias)
        return y.addmm_(x2, w2.t())

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        x1, w1, x2, w2 = ctx.saved_tensors
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        dx1 = dy @ w1 if need[0] else None
        dw1 = _weight_grad(dy, x1) if need[1] else None
        dx2 = dy @ w2 if need[2] else None
        dw2 = _weight_grad(dy, x2) if need[3] else None
        db = sparse.backend_for(dy).column_sum(dy) if need[4] else None
        return dx1, dw1, dx2, dw2, db


def linear_sum(x1, weight1, x2, weight2, bias=None):
    """x1 @ weight1.T + x2 @ weight2.T + bias for 2-D float32 HIP tensors (falls back to two F.linear calls otherwise)."""
    if (x1.dim() != 2 or x2.dim() != 2 or x1.dtype != torch.float32 or x1.device.type not in sparse._BACKENDS
            or not torch.is_grad_enabled() or (bias is not None and weight1.shape[0] > sparse.backend_for(x1).COLUMN_SUM_MAX)):
        return torch.nn.functional.linear(x1, weight1) + torch.nn.functional.linear(x2, weight2, bias)
    return LinearSumFn.apply(x1, weight1, x2, weight2, bias)


class SelectRowsFn(torch.autograd.Function):
    """x[rows] for DISTINCT rows (a training-node index): the backward writes the incoming rows into a zero matrix with
    index_copy_ -- torch's x[rows] backward sorts the index to accumulate duplicates (a radix sort, merges and a serial
    accumulation per epoch: ~0.17 ms for the 196 k training nodes of the products shape) although there are none."""

    @staticmethod
    def forward(ctx, x, rows):
        ctx.save_for_backward(rows)
        ctx.n = x.shape[0]
        return x.index_select(0, rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (rows,) = ctx.saved_tensors
        dx = torch.zeros((ctx.n,) + tuple(dy.shape[1:]), dtype=dy.dtype, device=dy.device)
        dx.index_copy_(0, rows, dy)
        return dx, None


def select_distinct_rows(x, rows):
    """x[rows] where `rows` holds no duplicates (not checked: duplicates would lose gradient)."""
    return SelectRowsFn.apply(x, rows)


def nll_sum(logp, target):
    """-sum_i logp[i, target[i]] == F.nll_loss(logp, target, reduction='sum'): one gather and a parallel sum instead of
    torch's single-workgroup reduction kernels (0.22 + 0.19 ms forward + backward for 196 k rows on MI355X)."""
    return -logp.gather(1, target.view(-1, 1)).sum()


class SageMeanLayerFn(torch.autograd.Function):
    """One mean-aggregator GraphSAGE layer on a square graph as ONE autograd node:
        y = h W_self^T + mean_{u->v}(h[u]) W_neigh^T + b          (main_dgl_product_sage.py:52-64)
    Same kernels as update_all(copy_src, mean) followed by linear_sum; what the single node adds is the backward: h feeds
    both the self GEMM and the aggregation, and autograd would add their two gradients in a separate N x D pass -- here the
    reversed aggregation ACCUMULATES into the self GEMM's gradient (mgx_spmm_csr, MGX_SPMM_ACCUMULATE)."""

    @staticmethod
    def forward(ctx, gidx, h, w_self, w_neigh, bias):
        neigh, _, _ = _raw_gspmm(gidx.csc(), "copy_lhs", "mean", h, None)
        ctx.gidx = gidx
        ctx.save_for_backward(h, w_self, neigh, w_neigh)
        y = torch.nn.functional.linear(h, w_self, bias)
        return y.addmm_(neigh, w_neigh.t())

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        h, w_self, neigh, w_neigh = ctx.saved_tensors
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        dh = None
        if need[1]:
            dh = dy @ w_self
            dn = dy @ w_neigh
            dn.mul_(ctx.gidx.csc().inv_degrees().view(-1, 1))  # d(sum / deg): one streaming pass, not a per-edge factor
            sparse.gspmm_raw(ctx.gidx.csr(), "copy_lhs", "sum", dn, None, accumulate_into=dh)
        dws = _weight_grad(dy, h) if need[2] else None
        dwn = _weight_grad(dy, neigh) if need[3] else None
        db = sparse.backend_for(dy).column_sum(dy) if need[4] else None
        return None, dh, dws, dwn, db


class CatBuffer(object):
    """An [N, 2 K] matrix whose left half holds a layer's input h and whose right half receives mean_{u->v} h[u]: the operand of
    the ONE GEMM `[h | neigh] [W_self | W_neigh]^T` that replaces SAGEConv's two.  `generation` counts the forward passes
    that wrote the right half; a backward pass checks that no later forward overwrote what it saved."""
    __slots__ = ("buf", "K", "generation", "static_key", "static_agg", "static_tail")

    def __init__(self, n, K, device):
        self.buf = torch.empty((n, 2 * K), dtype=torch.float32, device=device)
        self.K = K
        self.generation = 0
        self.static_key = None
        self.static_agg = None  # the static_key whose aggregation the right half holds (SageMeanStaticInputProjectFn)
        self.static_tail = None  # ((tensor, version, csc), block_a, edge_tail): the constant 100-column input laid out for mgx_spmm_copy_u_edge_tail

    @property
    def left(self):
        return self.buf[:, :self.K]

    @property
    def right(self):
        return self.buf[:, self.K:]

    def holds(self, h):
        return (h.dim() == 2 and h.shape == (self.buf.shape[0], self.K) and h.data_ptr() == self.buf.data_ptr()
                and h.stride(0) == self.buf.stride(0) and h.stride(1) == 1)

    def is_resident(self, h):
        """h is the SAME tensor object, unmodified (version counter), as the one the left half was last copied from.  The buffer keeps a
        reference to that tensor: a per-step temporary at a recycled address is a different object."""
        return self.static_key is not None and self.static_key[0] is h and self.static_key[1] == h._version

    def take_input(self, h):
        """Begin a forward pass over the layer input h: one that lives elsewhere -- the model's input features -- is copied into the
        left half, unless it is the resident input (config.SAGE_STATIC_CAT; never one that takes a gradient); the pass is counted."""
        if not self.holds(h) and (not self.is_resident(h) or h.requires_grad or not config.SAGE_STATIC_CAT):
            self.left.copy_(h)
            self.static_key = None if h.requires_grad else (h, h._version)
        self.generation += 1

    def check_generation(self, generation):
        """A backward pass whose forward pass left the counter at `generation` may read the buffer only while it still stands there."""
        if self.generation != generation:
            raise DGLError("SAGEConv: a later forward pass overwrote the [h | neigh] buffer this backward pass needs (two forwards "
                           "before one backward); set mi355x_graph.config.SAGE_CAT = False")


# mgx_rows_gemm (csrc/rowsgemm.hip) for the projections of a layer over a CatBuffer: tall inputs only (the library GEMM wins below,
# and the staging of B is per workgroup).  config.ROWS_GEMM = False: the library GEMM (+ the separate 1 / deg pass) everywhere.
_ROWS_GEMM_MIN = 1 << 16


def _rows_dgrad(be, dy, wcat, inv_deg, K):
    """(d h, d neigh / deg) = the two halves of dy @ wcat, the second times 1 / deg: mgx_rows_gemm with the factor in its epilogue and
    each half a compact matrix of its own (the reversed aggregation then gathers from one and accumulates into the other), else the
    GEMM and a streaming pass over that half, the halves two column blocks of one matrix."""
    if config.ROWS_GEMM and dy.is_cuda and dy.shape[0] >= _ROWS_GEMM_MIN and K % 4 == 0:
        pair = be.rows_gemm(dy, wcat, row_scale=inv_deg, scale_from=K, split_col=K)
        if pair is not None:
            return pair
    dcat = dy @ wcat
    dcat[:, K:].mul_(inv_deg.view(-1, 1))
    return dcat[:, :K], dcat[:, K:]


def _rows_linear(be, x2d, weight, bias):
    """F.linear(x2d, weight, bias) for a tall x2d through mgx_rows_gemm when it has the shape (weight: [out, in] as in nn.Linear).
    Outputs that are not a multiple of four columns wide (the 47 classes) keep the library GEMM: scalar stores, 0.49 against 0.47 ms."""
    if config.ROWS_GEMM and x2d.is_cuda and x2d.shape[0] >= _ROWS_GEMM_MIN and weight.shape[0] % 4 == 0:
        y = be.rows_gemm(x2d, weight, b_transposed=True, bias=bias)
        if y is not None:
            return y
    return torch.nn.functional.linear(x2d, weight, bias)


def _cat_project(be, cat, w_self, w_neigh, bias, act=None):
    """(y, None) for y = [h | neigh] [W_self | W_neigh]^T + bias over every row of the CatBuffer, ONE GEMM; with act = (p, into, made):
    (dropout(relu(y), p), its mask) from that GEMM's epilogue (mgx_rows_gemm_relu_dropout) -- the activation lands in `into` (the next
    layer's buffer, or None: a new matrix), the N x out pre-activation is never stored, and the mask takes the position in the random
    stream that ops.relu_dropout would take here.  made = [slots, overflow, written?] or None: the activation's rows as 128-byte
    slots too.  No fused kernel for the operand after all: the composition it stands for, same seed and offset (same bits)."""
    if act is None:
        return _rows_linear(be, cat.buf, torch.cat([w_self, w_neigh], dim=1), bias), None
    p, into, made = act
    out = None if into is None else into.t
    seed, offset = _dropout_stream_position()
    wcat = torch.cat([w_self, w_neigh], dim=1)
    fused = be.rows_gemm_relu_dropout(cat.buf, wcat, True, bias, float(p), seed, offset, out=out,
                                      slots=None if made is None else made[0], overflow=None if made is None else made[1])
    if fused is None:
        return be.relu_dropout_fwd(_rows_linear(be, cat.buf, wcat, bias), float(p), seed, offset, out=out)
    if made is not None:
        made[2] = True
    return fused


def _split_cat_grad(dw, K):
    """d[W_self | W_neigh] [out, 2K] -> (dW_self, dW_neigh)"""
    return dw[:, :K].contiguous(), dw[:, K:].contiguous()


def _cat_param_grads(be, dy, buf, K, need_w, need_b):
    """(dW_self, dW_neigh, db) of a layer over a CatBuffer from dy [N, out] and buf = [h | neigh]: weight and bias from ONE pass over dy
    where both are asked for (_weight_bias_grad), else the weight alone, else the column sums."""
    if need_w and need_b:
        dw, db = _weight_bias_grad(dy, buf)  # [out, 2K], [out]
        return _split_cat_grad(dw, K) + (db,)
    if need_w:
        return _split_cat_grad(_weight_grad(dy, buf), K) + (None,)
    return None, None, be.column_sum(dy if dy.is_contiguous() else dy.contiguous()) if need_b else None


def _cat_param_grads_masked(be, dy, mask, p, buf, K, need_dh, need_w, need_b):
    """_cat_param_grads(relu_dropout_bwd(dy, mask, p)) for a layer whose input takes no gradient (layer 1), or None: d z would be
    written once and read twice by the weight gradient's two launches and for nothing else -- the mask is applied as that kernel loads
    d y instead (mgx_xty_colsum_masked), same bits."""
    if need_dh or not (need_w and need_b) or not _xty_masked_wanted(be, dy, buf):
        return None
    masked = be.xty_masked(dy, mask, p, buf)
    return None if masked is None else _split_cat_grad(masked[0], K) + (masked[1],)


def _cat_aggregate(be, gidx, cat, h):
    """The forward aggregation of a layer over a CatBuffer: h into the left half (unless it lives there or is the resident input), its
    mean over the in-edges into the right half, every row."""
    csc = gidx.csc()
    cat.take_input(h)
    tail_ops = _edge_tail_operands(be, csc, cat, h)
    if tail_ops is not None:
        # the constant 100-column input: columns 0 .. 95 as a compact block (three cache lines per row instead of four and an eighth),
        # the last four laid out along the edge list -- once, for as long as the tensor is not written to
        be.spmm_copy_u_edge_tail(csc, "mean", tail_ops[0], tail_ops[1], cat.right)
    else:
        # a relu + dropout output (a hidden layer's input) is gathered as 128-byte slots, one cache line per edge instead of two
        be.spmm_copy_u_strided(csc, "mean", cat.left, cat.right, slots=_packed_rows(be, gidx, csc, h, cat.left))


class SageMeanCatFn(torch.autograd.Function):
    """SageMeanLayerFn over a CatBuffer: the aggregation reads the left half and writes the right half in place
    (mgx_spmm_copy_u_strided), forward and weight gradients are ONE GEMM / ONE mgx_xty against the stacked weights, and the
    backward aggregation reads the right half of d[h | neigh] and accumulates into its left half."""

    @staticmethod
    def forward(ctx, gidx, cat, h, w_self, w_neigh, bias, act=None):
        be = sparse.backend_for(h)
        _cat_aggregate(be, gidx, cat, h)
        ctx.gidx, ctx.cat, ctx.generation = gidx, cat, cat.generation
        y, mask = _cat_project(be, cat, w_self, w_neigh, bias, act)
        ctx.save_for_backward(*((w_self, w_neigh) if mask is None else (w_self, w_neigh, mask)))
        ctx.p = None if act is None else float(act[0])
        return y

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        cat = ctx.cat
        cat.check_generation(ctx.generation)
        need = ctx.needs_input_grad
        need_w = need[3] or need[4]
        be = sparse.backend_for(dy)
        K = cat.K
        dh = None
        aggregated_first = False
        if ctx.p is not None:
            w_self, w_neigh, mask = ctx.saved_tensors
            if not dy.is_contiguous() and not be._row_strided(dy):
                dy = dy.contiguous()
            gate = None
            if need[2] and dy.dim() == 2 and dy.shape[1] == 64 and K % 4 == 0 and config.ROWS_GEMM and be.rows_gemm_supported(128, K, 128):
                gate = _slot_gate(be, ctx.gidx, ctx.gidx.csr(), dy.shape[0])
                if gate is not None and not gate.allow():
                    gate = None
            if gate is not None:
                # d h = d y W_self + A^T (D^-1 d y) W_neigh: the gradient behind relu + dropout is as sparse as the activation, so the
                # reversed aggregation runs on IT -- as 128-byte slots, 1 / deg folded into the packed values -- and the projection
                # follows as one GEMM on [d y | A^T D^-1 d y], instead of projecting first and aggregating 64 dense columns
                dcat = torch.empty((dy.shape[0], 128), dtype=torch.float32, device=dy.device)
                inv = ctx.gidx.csc().inv_degrees()
                if dy.data_ptr() % 16 == 0:
                    dy, slots, overflow = be.relu_dropout_bwd_slots(dy, mask, ctx.p, dcat[:, :64], row_scale=inv)
                else:
                    dy = be.relu_dropout_bwd(dy, mask, ctx.p, out=dcat[:, :64])
                    slots, overflow = be.rows_slots_pack(dy, row_scale=inv)
                gate.watch(overflow, dy.shape[0])
                be.spmm_copy_u_strided(ctx.gidx.csr(), "sum", dy, dcat[:, 64:], slots=slots, src_scale=inv)
                dh = be.rows_gemm(dcat, torch.cat([w_self, w_neigh], dim=0))  # [N, 128] x [128, K]
                if dh is None:
                    dh = dcat @ torch.cat([w_self, w_neigh], dim=0)
                aggregated_first = True
            else:
                grads = _cat_param_grads_masked(be, dy, mask, ctx.p, cat.buf, K, need[2], need_w, need[5])
                if grads is not None:
                    return (None, None, None) + grads + (None,)
                dy = be.relu_dropout_bwd(dy, mask, ctx.p)  # the gradient of the pre-activation, as ReluDropout.backward forms it
        else:
            w_self, w_neigh = ctx.saved_tensors
        if not aggregated_first:
            dy = dy.contiguous()
        if need[2] and not aggregated_first:
            # [N, 2K] = d[h | neigh], the `neigh` half times 1 / deg (d(sum / deg)): one mgx_rows_gemm with the factor in its epilogue,
            # else the GEMM and a streaming pass over that half -- never a per-edge factor
            dh, dn = _rows_dgrad(be, dy, torch.cat([w_self, w_neigh], dim=1), ctx.gidx.csc().inv_degrees(), K)
            be.spmm_copy_u_strided(ctx.gidx.csr(), "sum", dn, dh, accumulate=True)
        dws, dwn, db = _cat_param_grads(be, dy, cat.buf, K, need_w, need[5])
        return None, None, dh, dws, dwn, db, None


def _of_row_list(cache, rows, extra, ident, build, *args):
    """What build(*args) derives from the row list `rows`, kept in `cache` under (address, length, extra) for as long as `rows` is the
    same tensor object at the same version counter (and `ident`, a second operand or None, the same object): the loss rows of a training
    run are one tensor, reused every step, and a list written in place is derived again.  A write behind autograd's back -- `.data`, a
    raw kernel -- is not seen: do not change a row list that way.  A cache that has grown past 8 entries is emptied first."""
    key = (rows.data_ptr(), int(rows.shape[0]), extra)
    held = cache.get(key)
    if held is None or held[0] is not rows or held[1] != rows._version or held[2] is not ident:
        if len(cache) > 8:
            cache.clear()
        held = cache[key] = (rows, rows._version, ident, build(*args))
    return held[3]


_ROW_BITS = {}     # per (rows, N): the bitmap of the listed nodes
_ROW_INV_DEG = {}  # per (rows, inv_deg): inv_deg[rows] -- one gather per row list, not per step
_ROW_POS = {}      # per (rows, N): int64 [N], the place of a node in `rows`, -1 outside


def _build_row_bits(rows, n, be):
    flag = torch.zeros((n, 4), dtype=torch.float32, device=rows.device)
    flag[rows] = 1.0
    return be.row_nonzero_bits(flag)


def _build_row_pos(rows, n):
    pos = torch.full((n,), -1, dtype=torch.int64, device=rows.device)
    pos[rows] = torch.arange(rows.shape[0], dtype=torch.int64, device=rows.device)
    return pos


def _row_bits(rows, n, be):
    return _of_row_list(_ROW_BITS, rows, int(n), None, _build_row_bits, rows, n, be)


def _row_inv_deg(rows, inv_deg):
    return _of_row_list(_ROW_INV_DEG, rows, inv_deg.data_ptr(), inv_deg, inv_deg.index_select, 0, rows)


def _row_pos(rows, n):
    return _of_row_list(_ROW_POS, rows, int(n), None, _build_row_pos, rows, n)


def _head_rows_forward(ctx, gidx, cat, h, w_self, w_neigh, bias, rows):
    """The forward of SageMeanCatHeadFn and SageMeanCatRowsFn: [h | mean_agg(h)][rows] x [W_self | W_neigh]^T + bias -> [R, out]: every
    row aggregated (the right half of the buffer fully written: the weight gradient and every later reader see what SageMeanCatFn
    leaves), the listed rows projected -- read in place by mgx_rows_gemm_rows where it has the shape, else gathered for the library GEMM."""
    be = sparse.backend_for(h)
    _cat_aggregate(be, gidx, cat, h)
    wcat = torch.cat([w_self, w_neigh], dim=1)
    y = be.rows_gemm(cat.buf, wcat, b_transposed=True, bias=bias, rows=rows) if config.ROWS_GEMM else None
    if y is None:
        y = torch.nn.functional.linear(cat.buf.index_select(0, rows), wcat, bias)
    ctx.gidx, ctx.cat, ctx.generation, ctx.rows = gidx, cat, cat.generation, rows
    ctx.save_for_backward(w_self, w_neigh)
    return y


def _head_dn(csr, K, rows, n, like, be):
    """The [N, K] matrix SageMeanCatHeadFn's backward scatters d neigh / deg into, zero outside `rows`: ONE matrix, kept between steps
    instead of a zero fill per step (config.SAGE_HEAD_INIT) -- on the CSR the reversed aggregation gathers it over, which lives as long
    as the graph (the CatBuffer of a hidden layer's output is a new one every forward pass; steps over one graph run one after the
    other on one stream, like everything else that shares its formats and plans).  The scatter overwrites all K columns of every listed row,
    so with the list of the last step -- the same tensor object, unwritten (version counter), as for the _ROW_* caches -- nothing needs
    clearing; with another list the rows of the previous one are cleared first (the whole matrix when that list was written to since).
    Internal to the node: the aggregation reads it, autograd never sees it.  Inside a HIP-graph capture the step gets a zero matrix
    of its own, filled in the captured step: a replay runs none of this bookkeeping, and eager steps with other lists in between
    must not leave their rows in what it reads.
    config.SAGE_HEAD_SLOTS (_head_slots_wanted): the matrix's 128-byte slots are kept beside it, for the aggregation to probe before it
    gathers a dense row (mgx_spmm_copy_u_slots_init) -- all of them packed when the matrix is created or cleared as a whole, the slots of a
    previous list's rows packed again (empty) when those rows are cleared; the step's rows are packed by the caller once the scatter has
    written them (_head_dn_slots).  A captured step has no slots."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros((n, K), dtype=like.dtype, device=like.device)
    held = csr._head_dn
    slots, stale = None, True  # stale: every slot has to be written again
    if held is None or held[0].shape != (n, K) or held[0].dtype != like.dtype or held[0].device != like.device:
        buf = torch.zeros((n, K), dtype=like.dtype, device=like.device)
    else:
        buf, prev, version, slots = held
        stale = slots is None
        if prev is rows and version == rows._version:
            pass
        elif prev._version == version:
            buf.index_fill_(0, prev, 0.0)
            if slots is not None:
                be.rows_slots_pack_rows(buf, prev, slots)  # the cleared rows' slots are empty again
        else:
            buf.zero_()
            stale = True
    if _head_slots_wanted(csr, K, be) and be.rows_slots_supported(buf, csr):
        if stale:
            slots = be.rows_slots_pack(buf)[0]  # (a kept list's rows included: the step's scatter and its pack follow)
    else:
        slots = None
    csr._head_dn = (buf, rows, rows._version, slots)
    return buf


def _head_slots_wanted(csr, K, be):
    """Does the reversed aggregation of SageMeanCatHeadFn gather d neigh / deg over `csr` as 128-byte slots (config.SAGE_HEAD_SLOTS)?"""
    return (config.SAGE_HEAD_SLOTS and config.SAGE_HEAD_INIT and os.environ.get("MGX_SAGE_HEAD_SLOTS", "1") != "0" and K == 64
            and csr.nnz >= min(config.SAGE_HEAD_SLOTS_MIN_NNZ, config.PACKED_GATHER_MIN_NNZ) and hasattr(be, "spmm_copy_u_slots_init") and hasattr(be, "rows_slots_pack_rows"))


def _head_dn_slots(csr, dn):
    """The slots kept beside `dn` when it is the matrix _head_dn keeps on `csr` (None: a captured step, the switch off, another matrix)."""
    held = csr._head_dn
    return held[3] if held is not None and held[0] is dn else None


def _head_rows_dense_backward(be, gidx, cat, w_self, w_neigh, dyr, rows, need_dh, need_w, need_b, zero_fill):
    """The dense half of the backward of _head_rows_forward from dyr [R, out], all of it on the R listed rows:
    (d_self [R, K] compact, dn [N, K] = d neigh / deg on the listed rows -- the other rows zero (zero_fill) or unwritten --, dW_self,
    dW_neigh, db).  The weight gradient reads the listed rows of the buffer in place (mgx_xty_colsum_rows)."""
    K, n = cat.K, cat.buf.shape[0]
    d_self = dn = dws = dwn = db = None
    if need_dh:
        wcat = torch.cat([w_self, w_neigh], dim=1)  # [out, 2K]
        if zero_fill and config.SAGE_HEAD_INIT:
            dn = _head_dn(gidx.csr(), K, rows, n, dyr, be)
        else:
            dn = (torch.zeros if zero_fill else torch.empty)((n, K), dtype=dyr.dtype, device=dyr.device)
        inv_r = _row_inv_deg(rows, gidx.csc().inv_degrees())
        pair = None
        if config.ROWS_GEMM and K % 4 == 0:
            pair = be.rows_gemm(dyr, wcat, row_scale=inv_r, scale_from=K, split_col=K, scatter_rows=rows, out2=dn)
        if pair is None:
            dcat = dyr @ wcat
            dn.index_copy_(0, rows, dcat[:, K:] * inv_r.view(-1, 1))
            d_self = dcat[:, :K]
        else:
            d_self = pair[0]
        slots = _head_dn_slots(gidx.csr(), dn) if zero_fill and config.SAGE_HEAD_INIT else None
        if slots is not None:
            be.rows_slots_pack_rows(dn, rows, slots)  # the listed rows hold this step's values now
    if need_w:
        # over the listed rows, but summed as the layer over all rows sums them (mgx_xty_colsum_pos): a training run then stays on the
        # bits of that layer -- sums of the listed rows alone in their own order (mgx_xty_rows) differ in the last place, and Adam on
        # gradients near zero turns that into visibly different runs after a few steps
        res = be.xty_pos(dyr, _row_pos(rows, n), cat.buf, colsum=need_b) if n >= be.XTY_MIN_ROWS and config.LINEAR_XTY and config.XTY_COLSUM else None
        if res is None:
            dy = torch.zeros((n, dyr.shape[1]), dtype=dyr.dtype, device=dyr.device).index_copy_(0, rows, dyr)
            dws, dwn, db = _cat_param_grads(be, dy, cat.buf, K, True, need_b)
        else:
            dw, db = res if need_b else (res, None)
            dws, dwn = _split_cat_grad(dw, K)
    elif need_b:
        db = be.column_sum(dyr)
    return d_self, dn, dws, dwn, db


def _head_rows_backward(ctx, dyr, zero_fill):
    """What the backward passes of SageMeanCatHeadFn and SageMeanCatRowsFn begin with: (be, need d h?) + _head_rows_dense_backward's results."""
    w_self, w_neigh = ctx.saved_tensors
    ctx.cat.check_generation(ctx.generation)
    dyr = dyr.contiguous()
    need = ctx.needs_input_grad
    be = sparse.backend_for(dyr)
    return (be, need[2]) + _head_rows_dense_backward(be, ctx.gidx, ctx.cat, w_self, w_neigh, dyr, ctx.rows, need[2], need[3] or need[4],
                                                     need[5], zero_fill)


class SageMeanCatHeadFn(torch.autograd.Function):
    """SageMeanCatFn followed by the selection of DISTINCT output rows -- the loss rows, `model(g, feats)[train_idx]` at
    main_dgl_product_sage.py:105 -- as one node that does the layer's DENSE work on those rows only (config.SAGE_HEAD_ROWS, the
    default): the projection, its input gradient and the weight / bias gradients run over the R listed rows through the row-list
    operands of mgx_rows_gemm_rows and the position map of mgx_xty_colsum_pos instead of over all N rows, of which the loss reads 8 % on ogbn-products.
    Both aggregations are untouched: every row is aggregated forward, and the reversed one gathers every source row over every edge
    from d neigh / deg, which is zero outside the rows: an [N, K] matrix the GEMM scatters into, kept zero elsewhere from step to step
    (_head_dn) -- as 128-byte slots kept beside it on a big graph with K = 64 (config.SAGE_HEAD_SLOTS, mgx_spmm_copy_u_slots_init: the
    slot of a zero row is empty and ends that edge's work, any other slot sends the walk to the dense row), else as the dense rows.  Its sums start from d self, which
    stays the compact [R, K] matrix the GEMM wrote: the aggregation takes it through the position map
    (mgx_spmm_copy_u_strided_init) and writes every row of d h once.  config.SAGE_HEAD_INIT = False, or operands that entry point declines: a zero-filled [N, K] per step, d self copied into a second one, the accumulating aggregation.
    Every sum is formed in the order the layer over all rows forms it, so the gradients are that layer's bit for bit.  No atomics,
    no host synchronisation."""

    @staticmethod
    def forward(ctx, gidx, cat, h, w_self, w_neigh, bias, rows):
        return _head_rows_forward(ctx, gidx, cat, h, w_self, w_neigh, bias, rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, dyr):
        rows = ctx.rows
        be, need_dh, d_self, dn, dws, dwn, db = _head_rows_backward(ctx, dyr, True)
        dh = None
        if need_dh:
            # d self on the rows of a zero matrix, the reversed aggregation accumulating into it: what the layer over all rows does,
            # bit for bit (its d self is zero outside the rows).  Aggregating into a new matrix and adding d self afterwards saves the
            # kernel's read of its output, but the kernel starts a row's sum from the value it accumulates into: other bits.
            # config.SAGE_HEAD_INIT: the same sums started from the compact d self through the position map
            # (mgx_spmm_copy_u_strided_init) -- no zero matrix, no copy into it, no read of it; the sequence below where it declines
            if config.SAGE_HEAD_INIT and d_self.stride(1) == 1:
                # config.SAGE_HEAD_SLOTS: ... probing the slots kept beside d neigh / deg -- one line per edge, nothing more for the 92 %
                # of the source rows that are zero, the dense row where the slot is not empty (mgx_spmm_copy_u_slots_init); the same bits
                slots = _head_dn_slots(ctx.gidx.csr(), dn)
                if slots is not None:
                    dh = be.spmm_copy_u_slots_init(ctx.gidx.csr(), "sum", dn, slots, d_self, _row_pos(rows, dn.shape[0]), torch.empty_like(dn))
            if dh is None and config.SAGE_HEAD_INIT and d_self.stride(1) == 1:
                dh = be.spmm_copy_u_strided_init(ctx.gidx.csr(), "sum", dn, d_self, _row_pos(rows, dn.shape[0]), torch.empty_like(dn))
            if dh is None:
                dh = torch.zeros_like(dn).index_copy_(0, rows, d_self)
                be.spmm_copy_u_strided(ctx.gidx.csr(), "sum", dn, dh, accumulate=True)
        return None, None, dh, dws, dwn, db, None


class SageMeanCatRowsFn(torch.autograd.Function):
    """SageMeanCatHeadFn whose reversed aggregation ALSO skips the gathers of the source rows whose gradient is zero by construction
    (mgx_spmm_copy_u_masked with a bitmap of `rows`; those rows of d neigh are never even written) -- MGX_SAGE_SPARSE_LAST=1, off by
    default and off the headline, whose five aggregations gather every row.  Same forward, same dense backward on the listed rows.  Exact."""

    @staticmethod
    def forward(ctx, gidx, cat, h, w_self, w_neigh, bias, rows):
        return _head_rows_forward(ctx, gidx, cat, h, w_self, w_neigh, bias, rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, dyr):
        rows = ctx.rows
        be, need_dh, d_self, dn, dws, dwn, db = _head_rows_backward(ctx, dyr, False)
        dh = None
        if need_dh:
            dh = be.spmm_copy_u_masked(ctx.gidx.csr(), "sum", dn, _row_bits(rows, dn.shape[0], be))
            dh.index_add_(0, rows, d_self)
        return None, None, dh, dws, dwn, db, None


def sage_mean_layer_rows(g, h, w_self, w_neigh, bias, cat, rows):
    """The last SAGE layer of a model whose loss reads `rows` only (distinct) as one node with the row selection inside, or None:
    SageMeanCatRowsFn under MGX_SAGE_SPARSE_LAST=1, else SageMeanCatHeadFn (config.SAGE_HEAD_ROWS; MGX_SAGE_HEAD_ROWS=0: neither --
    the layer over all rows followed by select_distinct_rows).  The default form is for tall graphs like the other fused layers; the
    number of rows in the list does not matter, an empty list included."""
    if (cat is None or hasattr(g, "sage_mean_layer") or rows is None
            or type(g) is not DGLGraph or not h.is_cuda or h.dim() != 2 or not _cat_eligible(g, h, cat)
            or not torch.is_grad_enabled() or h.dtype != torch.float32 or g.idtype != torch.int32 or _torch_ops() is not None
            or rows.dtype != torch.int64 or rows.dim() != 1
            or (bias is not None and w_self.shape[0] > sparse.backend_for(h).COLUMN_SUM_MAX)):
        return None
    if os.environ.get("MGX_SAGE_SPARSE_LAST", "0") == "1":
        return SageMeanCatRowsFn.apply(g._index, cat, h, w_self, w_neigh, bias, rows.contiguous())
    be = sparse.backend_for(h)
    if (not config.SAGE_HEAD_ROWS or os.environ.get("MGX_SAGE_HEAD_ROWS", "1") == "0" or not config.SAGE_FUSED_LAYER
            or h.shape[0] < _ROWS_GEMM_MIN or g.is_block or g.number_of_src_nodes() != g.number_of_dst_nodes()
            or h.shape[0] != g.number_of_src_nodes() or w_self.shape[0] > be.XTY_MAX[0] or 2 * cat.K > be.XTY_MAX[1]):
        return None
    return SageMeanCatHeadFn.apply(g._index, cat, h, w_self, w_neigh, bias, rows.contiguous())


class SageMeanProjectFirstFn(torch.autograd.Function):
    """y = h W_self^T + mean_{u->v}(h[u] W_neigh^T) + b: the projection BEFORE the aggregation -- mean and the linear map commute,
    so this is SAGEConv's `fc_self(h) + fc_neigh(mean_agg(h))` (main_dgl_reddit_sage.py:73-80) with the aggregation running at
    the OUTPUT width (upstream dgl.nn.SAGEConv does the same when in_feats > out_feats: `lin_before_mp`).  reddit's first layer
    aggregates 16 columns instead of 602.  One GEMM gives [s | z] = h [W_self | W_neigh]^T, the aggregation reads the z half and
    accumulates into the s half in place; backward: dz = A_mean^T dy (one more aggregation at the output width), then
    d[W_self | W_neigh] = [dy | dz]^T h and dh = [dy | dz] [W_self ; W_neigh]."""

    @staticmethod
    def forward(ctx, gidx, h, w_self, w_neigh, bias):
        K = w_self.shape[0]
        w = torch.cat([w_self, w_neigh], dim=0)            # [2K, in]
        sz = torch.nn.functional.linear(h, w)               # [N, 2K] = [s | z]
        sparse.backend_for(h).spmm_copy_u_strided(gidx.csc(), "mean", sz[:, K:], sz[:, :K], accumulate=True)
        y = sz[:, :K].contiguous()
        if bias is not None:
            y.add_(bias)
        ctx.gidx = gidx
        ctx.save_for_backward(h, w)
        return y

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        h, w = ctx.saved_tensors
        K = w.shape[0] // 2
        need = ctx.needs_input_grad
        be = sparse.backend_for(dy)
        dcat = torch.empty((dy.shape[0], 2 * K), dtype=dy.dtype, device=dy.device)
        dcat[:, :K] = dy
        dn = dy * ctx.gidx.csc().inv_degrees().view(-1, 1)  # d(sum / deg): one streaming pass, not a per-edge factor
        be.spmm_copy_u_strided(ctx.gidx.csr(), "sum", dn, dcat[:, K:])
        dh = dcat @ w if need[1] else None
        dws = dwn = None
        if need[2] or need[3]:
            dw = _weight_grad(dcat, h)                       # [2K, in]
            dws, dwn = dw[:K], dw[K:]
        db = be.column_sum(dy.contiguous()) if need[4] else None
        return None, dh, dws, dwn, db


STATIC_AGGREGATIONS_BUILT = [0]  # how often SageMeanStaticInputProjectFn aggregated its constant input (bench.py reports it: once per model)


class SageMeanStaticInputProjectFn(torch.autograd.Function):
    """The FIRST SAGE layer of a full-graph model, whose input x is a constant (the node features: no gradient), with the
    projection before the aggregation (MGX_SAGE_L1_PROJECT_FIRST=1; off by default, reported beside the headline):

        y = x W_self^T + mean_agg(x W_neigh^T) + b        ==  fc_self(x) + fc_neigh(mean_agg(x))   (main_dgl_product_sage.py:61-64)

    so the products layer aggregates 64 columns instead of 100 (whole 256-byte rows instead of 400-byte rows that straddle 4.125
    cache lines).  SageMeanProjectFirstFn pays for that with a second aggregation in the backward (dz = A_mean^T dy) because its
    weight gradient is [dy | dz]^T h; here x is constant, so  dW_neigh = dy^T (A_mean x)  is taken against a CONSTANT matrix that is
    aggregated once and kept in the right half of the layer's CatBuffer for as long as the left half holds the same unmodified
    tensor object (identity + version counter, exactly like the resident copy of x itself) -- the forward aggregation still runs
    every pass, over every edge, and no aggregation is added to the backward."""

    @staticmethod
    def forward(ctx, gidx, cat, x, w_self, w_neigh, bias):
        be = sparse.backend_for(x)
        K = w_self.shape[0]
        if not cat.is_resident(x) or cat.static_agg is not cat.static_key:
            cat.left.copy_(x)
            cat.static_key = (x, x._version)
            be.spmm_copy_u_strided(gidx.csc(), "mean", cat.left, cat.right)      # A_mean x: once per (tensor, version)
            STATIC_AGGREGATIONS_BUILT[0] += 1
            cat.static_agg = cat.static_key
            cat.generation += 1
        w = torch.cat([w_self, w_neigh], dim=0)                                   # [2K, in]
        b2 = None if bias is None else torch.cat([bias, torch.zeros_like(bias)])
        sz = torch.nn.functional.linear(x, w, b2)                                 # [N, 2K] = [x W_self^T + b | x W_neigh^T]
        be.spmm_copy_u_strided(gidx.csc(), "mean", sz[:, K:], sz[:, :K], accumulate=True)
        ctx.cat, ctx.generation = cat, cat.generation
        return sz[:, :K]                                                           # row-strided view: relu_dropout reads it in place

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        cat = ctx.cat
        cat.check_generation(ctx.generation)
        need = ctx.needs_input_grad
        be = sparse.backend_for(dy)
        if dy.stride(1) != 1:
            dy = dy.contiguous()
        D = cat.K
        dws = dwn = None
        if need[3] or need[4]:
            dw = _weight_grad(dy, cat.buf)                                        # [K, 2 in] = dy^T [x | A_mean x]
            dws, dwn = dw[:, :D].contiguous(), dw[:, D:].contiguous()
        db = be.column_sum(dy if dy.is_contiguous() else dy.contiguous()) if need[5] else None
        return None, None, None, dws, dwn, db


def sage_static_input_project(g, x, w_self, w_neigh, bias, cat):
    """SageMeanStaticInputProjectFn when it applies (opt-in switch, constant input, out_feats < in_feats), else None."""
    K, D = w_self.shape
    if (os.environ.get("MGX_SAGE_L1_PROJECT_FIRST", "0") != "1" or cat is None or x.requires_grad
            or not _fused_layer_operands(g, x, w_self, bias) or cat.K != D or cat.buf.shape[0] != x.shape[0]
            or K % 4 or D % 4 or K >= D or not _cat_eligible(g, x, cat) or x.shape[0] * 2 * K * 4 >= (1 << 32)):
        return None
    return SageMeanStaticInputProjectFn.apply(g._index, cat, x, w_self, w_neigh, bias)


def sage_project_first(g, h, w_self, w_neigh, bias=None):
    """SAGEConv with the projection before the aggregation, or None when that form does not apply / does not pay: a square int32
    DGLGraph, 2-D float32 HIP features, out_feats a multiple of 4, and TWO aggregations at the output width (forward and
    backward) cheaper than ONE at the input width (the input needs no gradient) resp. two (it does)."""
    K, D = w_self.shape
    if hasattr(g, "sage_project_first"):  # dist.DistGraph: the same form with the halo exchange at the output width
        return g.sage_project_first(h, w_self, w_neigh, bias)
    if (not _fused_layer_operands(g, h, w_self, bias) or K % 4 or K > 128 or not config.SAGE_PROJECT_FIRST
            or g.number_of_src_nodes() * 2 * K * 4 >= (1 << 32)):
        return None
    aggs_now = 2 if h.requires_grad else 1
    if 2 * max(K, 16) * 1.1 > aggs_now * D:  # rows narrower than 64 bytes cost as much as 64-byte rows (request bound)
        return None
    return SageMeanProjectFirstFn.apply(g._index, h, w_self, w_neigh, bias)


def sage_mean_layer(g, h, w_self, w_neigh, bias=None, cat=None):
    """Fused form of SAGEConv on a homogeneous square DGLGraph with 2-D float32 HIP features; None when the fused node does
    not apply (the caller then composes update_all + linear_sum)."""
    if hasattr(g, "sage_mean_layer"):  # dist.DistGraph: the same one-GEMM layer with the halo exchange inside
        return g.sage_mean_layer(h, w_self, w_neigh, bias, cat)
    if not _fused_layer_operands(g, h, w_self, bias) or not config.SAGE_FUSED_LAYER:
        return None
    if cat is not None and _cat_eligible(g, h, cat):
        return SageMeanCatFn.apply(g._index, cat, h, w_self, w_neigh, bias)
    return SageMeanLayerFn.apply(g._index, h, w_self, w_neigh, bias)


def sage_mean_layer_act(g, h, w_self, w_neigh, bias, cat, p, out):
    """dropout(relu(SAGEConv(g, h)), p) as ONE node whose GEMM applies the activation in its epilogue and writes `out` (the left half of
    the next layer's CatBuffer, or None for a new matrix): bit for bit ops.relu_dropout(ops.sage_mean_layer(...), out=out), one pass
    over the N x out pre-activation less each way.  None when that form does not apply (the caller composes the two)."""
    if hasattr(g, "sage_mean_layer_act"):  # dist.DistGraph: the same fused layer with the halo exchange inside
        return g.sage_mean_layer_act(h, w_self, w_neigh, bias, cat, p, out)
    if (not config.SAGE_FUSED_ACT or not config.ROWS_GEMM or cat is None or capture_path() or not (0.0 < p < 1.0)
            or not _fused_layer_operands(g, h, w_self, bias) or h.shape[0] < _ROWS_GEMM_MIN
            or not config.SAGE_FUSED_LAYER or not _cat_eligible(g, h, cat) or w_self.shape[0] % 4
            or not sparse.backend_for(h).rows_gemm_supported(2 * cat.K, w_self.shape[0], cat.buf.stride(0))
            or (out is not None and (out.shape != (h.shape[0], w_self.shape[0]) or out.stride(1) != 1 or out.stride(0) % 4
                                     or out.data_ptr() % 16 or out.requires_grad))):
        return None
    K, D = w_self.shape
    if config.SAGE_PROJECT_FIRST and K % 4 == 0 and K <= 128 and 2 * max(K, 16) * 1.1 <= (2 if h.requires_grad else 1) * D:
        return None  # sage_project_first's rule: this layer aggregates fewer columns projected first (reddit: 602 -> 16)
    if os.environ.get("MGX_SAGE_L1_PROJECT_FIRST", "0") == "1" and not h.requires_grad and K < D:
        return None  # the opt-in layer-1 form (sage_static_input_project) takes this layer
    # the NEXT layer aggregates this layer's output over the same graph: when that aggregation will gather 128-byte slots (64 columns,
    # _slot_gate), the GEMM's epilogue writes them beside the rows and the pack pass over the N x 64 activation is saved
    made = None
    be = sparse.backend_for(h)
    if K == 64 and out is not None:
        gate = _slot_gate(be, g._index, g._index.csc(), h.shape[0])
        if gate is not None and gate.open():
            made = [torch.empty((h.shape[0], 32), dtype=torch.int32, device=h.device), torch.zeros(1, dtype=torch.int64, device=h.device), False]
    y = _structural_zeros(SageMeanCatFn.apply(g._index, cat, h, w_self, w_neigh, bias, (float(p), None if out is None else _Into(out), made)))
    if made is not None and made[2]:
        y._mgx_slots = (made[0], made[1], int(y._version))
    return y


def _fused_layer_operands(g, h, w_self, bias):
    """What every fused SAGE layer form asks of its operands: a plain square int32 DGLGraph (the accumulating aggregation is exercised on
    the int32 kernels only), 2-D float32 HIP features with one row per node, gradients enabled, the dispatcher ops (MGX_TORCH_OPS) off,
    and a bias narrow enough for mgx_column_sum to form its gradient."""
    return (type(g) is DGLGraph and not g.is_block and h.dim() == 2 and h.dtype == torch.float32 and h.is_cuda
            and h.device.type in sparse._BACKENDS and torch.is_grad_enabled() and g.idtype == torch.int32
            and g.number_of_src_nodes() == g.number_of_dst_nodes() and h.shape[0] == g.number_of_src_nodes()
            and _torch_ops() is None and (bias is None or w_self.shape[0] <= sparse.backend_for(h).COLUMN_SUM_MAX))


def _cat_eligible(g, h, cat):
    K = h.shape[1]
    idx = g._index
    return (config.SAGE_CAT and cat.K == K and K % 4 == 0 and cat.buf.shape[0] == h.shape[0]
            and idx.csc().indptr.dtype == torch.int32 and h.shape[0] * 2 * K * 4 < (1 << 32))


def cat_buffer_for(g, x, K):
    """A CatBuffer for a layer whose input has K columns, or None when the one-GEMM form does not apply to this graph / width."""
    if ((type(g) is not DGLGraph and not hasattr(g, "sage_mean_layer")) or g.is_block or x.dtype != torch.float32 or not x.is_cuda or x.device.type not in sparse._BACKENDS
            or not torch.is_grad_enabled() or K % 4 or g.number_of_src_nodes() != g.number_of_dst_nodes()
            or g.number_of_src_nodes() * 2 * K * 4 >= (1 << 32) or g.idtype != torch.int32
            or not config.SAGE_CAT or not config.SAGE_FUSED_LAYER):
        return None
    return CatBuffer(g.number_of_src_nodes(), K, x.device)


def linear(x, weight, bias=None):
    """torch.nn.functional.linear whose bias gradient (column sum) and tall-skinny weight gradient (dY^T X) are computed
    by the library (float32 HIP tensors; <= 256 outputs with a bias)."""
    if (x.dtype != torch.float32 or x.device.type not in sparse._BACKENDS or not torch.is_grad_enabled()
            or (bias is not None and weight.shape[0] > sparse.backend_for(x).COLUMN_SUM_MAX)):
        return torch.nn.functional.linear(x, weight, bias)
    return LinearFn.apply(x, weight, bias)


class SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, x, offsets, total):
        out, arg = sparse.segment_reduce_raw(offsets, x, op, want_arg=op in ("max", "min"), total=total)
        ctx.backward_cache = op, x.shape[0]
        ctx.save_for_backward(arg, offsets)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        op, n = ctx.backward_cache
        arg, offsets = ctx.saved_tensors
        dy = dy.contiguous()
        if op in ("sum", "mean"):
            lens = offsets[1:] - offsets[:-1]
            if op == "mean":
                dy = dy / lens.clamp(min=1).to(dy.dtype).view((-1,) + (1,) * (dy.dim() - 1))
            seg = torch.repeat_interleave(torch.arange(lens.shape[0], device=dy.device), lens, output_size=n)
            dx = sparse.gather_rows_raw(dy, seg) if dy.is_cuda else dy[seg]
        else:
            dx = torch.zeros((n,) + tuple(dy.shape[1:]), dtype=dy.dtype, device=dy.device)
            valid = arg >= 0
            dx.scatter_add_(0, arg.clamp(min=0), dy * valid)
        return None, dx, None, None


# ----------------------------------------------------------------------------- graph readout: segment softmax / attention
def _segment_ids(offsets, n):
    lens = offsets[1:] - offsets[:-1]
    return torch.repeat_interleave(torch.arange(lens.shape[0], device=offsets.device), lens, output_size=n)


class SegmentBroadcast(torch.autograd.Function):
    """out[i] = x[segment of row i] (dgl.broadcast_nodes): a row gather forward, a segment sum backward."""

    @staticmethod
    def forward(ctx, x, offsets, n):
        seg = _segment_ids(offsets, n)
        ctx.save_for_backward(offsets)
        ctx.n = n
        return sparse.gather_rows_raw(x, seg) if x.is_cuda else x[seg]

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        offsets, = ctx.saved_tensors
        return sparse.segment_reduce_raw(offsets, dy.contiguous(), "sum", total=ctx.n)[0], None, None


def _segment_softmax_composed(offsets, z, n):
    """The softmax of every column over every segment from segment_reduce and row gathers: max, gather, exp, sum, gather, multiply.
    The edge rules of csrc/segattn.hip: a segment of -inf logits only gives zeros."""
    with torch.no_grad():
        m = sparse.segment_reduce_raw(offsets, z, "max", total=n)[0]
        m = torch.where(m == -float("inf"), torch.zeros_like(m), m)
    e = torch.exp(z - SegmentBroadcast.apply(m, offsets, n))
    s = SegmentReduce.apply("sum", e, offsets, n)
    empty = s == 0
    inv = torch.where(empty, torch.zeros_like(s), 1.0 / torch.where(empty, torch.ones_like(s), s))
    return e * SegmentBroadcast.apply(inv, offsets, n)


def _segment_attention_composed(offsets, feat, logits, query, scale, n):
    """ops.segment_attention through the operators that existed before csrc/segattn.hip: the fallback and the comparison form."""
    z = logits if query is None else (feat * SegmentBroadcast.apply(query, offsets, n)).sum(-1) * scale
    a = _segment_softmax_composed(offsets, z, n)
    return SegmentReduce.apply("sum", a.unsqueeze(-1) * feat, offsets, n)


class SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offsets):
        out = sparse.backend_for(x).segment_softmax_fwd(offsets, x.contiguous().view(x.shape[0], -1)).view(x.shape)
        ctx.save_for_backward(out, offsets)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, dy):
        out, offsets = ctx.saved_tensors
        dx = sparse.backend_for(out).segment_softmax_bwd(offsets, out.view(out.shape[0], -1), dy.contiguous().view(out.shape[0], -1))
        return dx.view(out.shape), None


class SegmentAttention(torch.autograd.Function):
    """out[g,h,:] = sum_{i in g} softmax_g(z)[i,h] feat[i,h,:] with z the gate column (logits) or scale <feat, query[g]>: the readout of
    GlobalAttentionPooling / Set2Set in one walk each way, the weights rebuilt from per-segment statistics (csrc/segattn.hip)."""

    @staticmethod
    def forward(ctx, feat, logits, query, offsets, scale):
        logits = None if logits is None else logits.contiguous()
        query = None if query is None else query.contiguous()
        out, stat = sparse.backend_for(feat).segment_attention_fwd(offsets, feat, logits, query, scale)
        ctx.scale = scale
        ctx.gate = logits is not None
        ctx.save_for_backward(feat, logits if ctx.gate else query, offsets, out, stat)
        return out

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_out):
        feat, other, offsets, out, stat = ctx.saved_tensors
        logits, query = (other, None) if ctx.gate else (None, other)
        need = ctx.needs_input_grad
        d_feat, d_logits, d_query = sparse.backend_for(feat).segment_attention_bwd(offsets, feat, logits, query, ctx.scale, out,
                                                                                   d_out.contiguous(), stat, need[0], need[1], need[2])
        return d_feat, d_logits, d_query, None, None


def _offsets_of(seglen, device):
    offsets = torch.zeros(seglen.shape[0] + 1, dtype=torch.int64, device=device)
    torch.cumsum(seglen.to(device).long(), 0, out=offsets[1:])
    return offsets


def _want_seglen(who, seglen, value, total):
    """seglen is a 1-D tensor and `total`, where it is known, is value's row count, or DGLError: the part that reads no tensor value."""
    if not torch.is_tensor(seglen) or seglen.dim() != 1:
        raise DGLError("%s: seglen must be a 1-D tensor of segment lengths" % who)
    if total is not None and int(total) != value.shape[0]:
        raise DGLError("%s: segment lengths sum to %d, value has %d rows" % (who, total, value.shape[0]))


def _segment_offsets(seglen, value, total, who):
    """(offsets on value's device, number of rows) after _want_seglen: as segment_reduce builds them -- a cumsum on the device, the row
    count from the caller or from host lengths, read back once otherwise."""
    if total is None:
        _want_seglen(who, seglen, value, int(seglen.sum()))
    return _offsets_of(seglen, value.device), int(value.shape[0])


# What the operand checks (_X_args: everything an operator rejects, DGLError) and the kernel predicates (_X_kernel_ok: what sends a valid
# call to the composed form) of the fused operators share.  X_fused is `_X_args` then `_X_kernel_ok`, False where the operator raises;
# the checks of a segment operator read no tensor value, so a predicate never waits for the device (its operator builds the offsets after).
def _want_tensor(who, name, t, dims, dtype=torch.float32):
    """`t` -- one operand or a tuple of them, named `name` in the message -- are tensors of `dims` dimensions and of `dtype`, or DGLError."""
    ts, dims = t if type(t) is tuple else (t,), dims if type(dims) is tuple else (dims,)
    for x in ts:  # (plain loops: this runs in every call of every operator)
        if not torch.is_tensor(x) or x.dim() not in dims:
            raise DGLError("%s: expected %s, got %s"
                           % (who, name, ", ".join(str(tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__ for x in ts)))
    for x in ts:
        if x.dtype != dtype:
            raise DGLError("%s expects %s input%s, got %s"
                           % (who, str(dtype).replace("torch.", ""), "s" if len(ts) > 1 else "", " / ".join(str(x.dtype) for x in ts)))


def _want_count(who, name, k):
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise DGLError("%s: %s must be an integer >= 1, got %r" % (who, name, k))


def _want_seglen_device(who, seglen, x):
    if seglen.device != x.device and seglen.device.type != "cpu":  # host lengths go with any x
        raise DGLError("%s: operands on different devices: %s vs %s" % (who, x.device, seglen.device))


def _row_ld(x):
    """The row stride of a [N, D] operand as the kernels get it: its own for a row-strided column block, D after a copy."""
    return int(x.stride(0)) if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else int(x.shape[1])


def _rows_fit(x):
    return x.shape[0] * _row_ld(x) < 2 ** 30  # 32-bit element indices in the kernels


_aligned16 = sparse.aligned16  # the kernels read 16 bytes per lane: a contiguous view at an odd storage offset is not theirs.  The backend
# wrappers would copy it (sparse.dense16); the operators that have a composition send it there instead, which reads it in place


def _device_kernels(t, switch, *methods):
    """`switch` is on and the backend of device tensor `t` has every wrapper in `methods` (not under MGX_TORCH_OPS=1); CPU backends compose."""
    if not (switch and _torch_ops() is None and t.is_cuda and t.device.type in sparse._BACKENDS):
        return False
    be = sparse.backend_for(t)
    return all(hasattr(be, m) for m in methods)


def _no_edges_zeros(shape, x, w):
    """No message: zeros, tied to x and w so that both get a zero gradient; no kernel of this library."""
    return x.new_zeros(shape) + (x[:0].sum() if w is None else x[:0].sum() + w.sum())


def segment_softmax(seglen, value, total=None):
    """Softmax of every column of `value` [N, ...] over consecutive row segments (dgl.softmax_nodes / softmax_edges).  Device tensors run
    csrc/segattn.hip (any width, one launch each way); CPU tensors -- under a registered CPU backend, as segment_reduce -- the
    composition segment max -> gather -> exp -> segment sum -> gather -> multiply."""
    if not torch.is_tensor(value) or value.dim() < 1:
        raise DGLError("segment_softmax: expected a tensor [N, ...], got %s" % (type(value).__name__,))
    if value.dtype != torch.float32:
        raise DGLError("segment_softmax expects float32 input, got %s" % (value.dtype,))
    _want_seglen("segment_softmax", seglen, value, total)
    offsets, n = _segment_offsets(seglen, value, total, "segment_softmax")
    if value.numel() == 0:
        return value.clone()
    if _device_kernels(value, True, "segment_attention_fwd"):  # csrc/segattn.hip holds both
        return SegmentSoftmax.apply(value, offsets)
    sparse.backend_for(value)  # no CPU backend: DGLError
    return _segment_softmax_composed(offsets, value, n)


def _segment_attention_args(seglen, feat, logits, query, total):
    if not torch.is_tensor(feat) or feat.dim() != 3:
        raise DGLError("segment_attention: expected feat [N, H, F], got %s" % (tuple(feat.shape) if torch.is_tensor(feat) else type(feat).__name__,))
    if (logits is None) == (query is None):
        raise DGLError("segment_attention: exactly one of logits (gate mode) and query (query mode) must be given, got %s"
                       % ("both" if logits is not None else "neither"))
    other = logits if logits is not None else query
    if not torch.is_tensor(other) or feat.dtype != torch.float32 or other.dtype != torch.float32:
        raise DGLError("segment_attention expects float32 inputs, got %s / %s"
                       % (feat.dtype, other.dtype if torch.is_tensor(other) else type(other).__name__))
    if other.device != feat.device:
        raise DGLError("segment_attention: operands on different devices: %s vs %s" % (feat.device, other.device))
    _want_seglen("segment_attention", seglen, feat, total)
    N, H, F = feat.shape
    if logits is not None and tuple(logits.shape) != (N, H):
        raise DGLError("segment_attention: expected logits [%d, %d] for feat %s, got %s" % (N, H, tuple(feat.shape), tuple(logits.shape)))
    if query is not None and tuple(query.shape) != (seglen.shape[0], H, F):
        raise DGLError("segment_attention: expected query [%d, %d, %d] for %d segments and feat %s, got %s"
                       % (seglen.shape[0], H, F, seglen.shape[0], tuple(feat.shape), tuple(query.shape)))


def _segment_attention_kernel_ok(seglen, feat):
    return (_device_kernels(feat, config.SEGMENT_ATTENTION_FUSED, "segment_attention_fwd") and feat.shape[0] > 0 and seglen.shape[0] > 0
            and sparse.backend_for(feat).segment_attention_supported(feat))


def segment_attention_fused(seglen, feat, logits=None, query=None, scale=1.0, total=None):
    """True when segment_attention(...) with these operands runs the fused pair of csrc/segattn.hip (else the composition)."""
    try:
        _segment_attention_args(seglen, feat, logits, query, total)
        return _segment_attention_kernel_ok(seglen, feat)
    except DGLError:
        return False


def segment_attention(seglen, feat, logits=None, query=None, scale=1.0, total=None):
    """Attention readout over consecutive row segments: out[g,h,:] = sum_{i in g} a[i,h] feat[i,h,:] with a the softmax over the segment
    of z[i,h] = logits[i,h] (gate mode: GlobalAttentionPooling) or z[i,h] = scale * <feat[i,h,:], query[g,h,:]> (query mode: Set2Set).

    feat [N, H, F], logits [N, H] or query [S, H, F] (fp32; feat may be a row-strided column block), result [S, H, F]: exactly 0 for an
    empty segment or one whose logits are all -inf.  `total`: the row count when the caller knows it (no read-back of device lengths).
    Device operands with F % 4 == 0, H*F <= 256 and (H == 1 or F in {4, 8, 16, 32, 64}) run csrc/segattn.hip (segment_attention_fused);
    everything else -- CPU tensors under a registered CPU backend, other shapes, config.SEGMENT_ATTENTION_FUSED = False -- is segment
    max -> gather -> exp -> segment sum -> gather -> multiply -> segment sum through segment_reduce and row gathers."""
    _segment_attention_args(seglen, feat, logits, query, total)
    offsets, n = _segment_offsets(seglen, feat, total, "segment_attention")
    scale = float(scale)
    if _segment_attention_kernel_ok(seglen, feat):
        return SegmentAttention.apply(feat, logits, query, offsets, scale)
    sparse.backend_for(feat)  # no CPU backend: DGLError
    if feat.shape[0] == 0 or seglen.shape[0] == 0:
        return feat.new_zeros((seglen.shape[0],) + tuple(feat.shape[1:]))
    return _segment_attention_composed(offsets, feat, logits, query, scale, n)


# ----------------------------------------------------------------------------- graph readout: segment top-k
class SegmentTopk(torch.autograd.Function):
    """(values, index) of the k first rows (sortby = a column) or elements of every column (sortby = None) of every segment in the order
    of a stable sort: ONE launch of csrc/segtopk.hip, which also writes the inverse map the backward -- one gather -- reads."""

    @staticmethod
    def forward(ctx, feat, offsets, k, sortby, descending):
        values, index, slot = sparse.backend_for(feat).segment_topk_fwd(offsets, feat, k, sortby, descending)
        ctx.mark_non_differentiable(index)
        ctx.save_for_backward(slot)
        ctx.D = int(feat.shape[1])
        return values, index

    @staticmethod
    @once_differentiable  # raw kernels inside: second-order gradients would silently be wrong
    def backward(ctx, d_values, _d_index):
        slot, = ctx.saved_tensors
        return sparse.backend_for(slot).segment_topk_bwd(slot, d_values, ctx.D), None, None, None, None


def _segment_topk_composed(offsets, feat, k, sortby, descending, n):
    """ops.segment_topk through torch operators, in the same order: a stable sort by key, then a stable sort by segment id, leaves every
    segment's rows in place as a block, ordered; rank j of segment s is position offsets[s] + j.  Zero padding and index -1 past a
    segment's end.  The form for CPU tensors, for k > 1024, under MGX_TORCH_OPS=1 and with config.SEGMENT_TOPK_FUSED off."""
    S, D = offsets.shape[0] - 1, int(feat.shape[1])
    columns = sortby is None
    if n == 0 or S == 0:
        return feat.new_zeros((S, k, D)), torch.full((S, k, D) if columns else (S, k), -1, dtype=torch.int64, device=feat.device)
    with torch.no_grad():
        key = feat if columns else feat[:, sortby:sortby + 1]
        key = torch.where(key != key, key.new_full((), float("nan")), key + 0.0)  # one NaN, one zero: a sort by key bits orders the same
        seg = _segment_ids(offsets, n)
        by_key = torch.sort(key, dim=0, stable=True, descending=bool(descending)).indices        # [n, D | 1]
        by_seg = torch.sort(seg[by_key], dim=0, stable=True).indices
        perm = by_key.gather(0, by_seg)                                                          # position -> row
        rank = torch.arange(k, device=feat.device)
        valid = rank.unsqueeze(0) < (offsets[1:] - offsets[:-1]).unsqueeze(1)                    # [S, k]
        pos = (offsets[:-1].unsqueeze(1) + rank.unsqueeze(0)).clamp(max=n - 1)                   # [S, k]
        row = perm[pos.view(-1)]                                                                 # [S * k, D | 1]
        index = torch.where(valid.view(-1, 1), row - offsets[:-1].repeat_interleave(k).unsqueeze(1), row.new_full((), -1))
    if columns:
        values = feat.gather(0, row)
    else:
        values = feat[row.view(-1)]
    values = torch.where(valid.view(-1, 1), values, values.new_zeros(()))
    return values.view(S, k, D), index.view((S, k, D) if columns else (S, k))


def _segment_topk_args(seglen, feat, k, sortby, total):
    """(feat as [N, D], sortby as a column >= 0 or None) of a segment_topk call, or DGLError."""
    who = "segment_topk"
    _want_tensor(who, "feat [N] or [N, D]", feat, (1, 2))
    _want_count(who, "k", k)
    feat2d = feat if feat.dim() == 2 else feat.unsqueeze(1)
    _want_seglen(who, seglen, feat2d, total)
    _want_seglen_device(who, seglen, feat)
    D = int(feat2d.shape[1])
    if D < 1:
        raise DGLError("segment_topk: feat has no columns")
    if sortby is not None:
        if isinstance(sortby, bool) or not isinstance(sortby, int) or not -D <= sortby < D:
            raise DGLError("segment_topk: sortby must be None or a column in [%d, %d), got %r" % (-D, D, sortby))
        sortby = sortby % D
    return feat2d, sortby


def _segment_topk_kernel_ok(seglen, feat2d, k, sortby):
    N, D, S = int(feat2d.shape[0]), int(feat2d.shape[1]), int(seglen.shape[0])
    return (_device_kernels(feat2d, config.SEGMENT_TOPK_FUSED, "segment_topk_fwd") and N > 0 and S > 0 and N < 2 ** 31 and S * k < 2 ** 31
            and (sortby is not None or S * D < 2 ** 31) and sparse.backend_for(feat2d).segment_topk_supported(k, D, sortby is None))


def segment_topk_fused(seglen, feat, k, sortby=None, descending=True, total=None):
    """True when segment_topk(...) with these operands runs csrc/segtopk.hip (else the composition of sorts and gathers)."""
    try:
        feat2d, sortby = _segment_topk_args(seglen, feat, k, sortby, total)
        return _segment_topk_kernel_ok(seglen, feat2d, k, sortby)
    except DGLError:
        return False


def segment_topk(seglen, feat, k, sortby=None, descending=True, total=None):
    """The k first rows of every consecutive row segment in sorted order (dgl.topk_nodes / topk_edges): (values, index).

    feat [N, D] (fp32; [N] is taken as D = 1; may be a row-strided column block), seglen [S] segment lengths.
      sortby = c (negative c counts from the last column): rows ordered by column c; values [S, k, D] are whole rows, index [S, k] int64
               the row's number inside its segment
      sortby = None: every column ordered on its own; values [S, k, D], index [S, k, D]
    The order is torch.sort(key, stable=True, descending=descending) per segment: NaN is the greatest key, -0.0 == +0.0, equal keys keep
    the lower row first in both directions; values are copies of the input bits.  A segment shorter than k is padded with zero values
    and index -1 (DGL leaves those indices unspecified; -1 is this package's choice).  Gradients flow to `feat` through `values` (each
    selected row or element receives its rank's gradient, everything else zero); `index` is not differentiable.
    `total`: the row count when the caller knows it (no read-back of device lengths).  Device operands with k <= 1024 run
    csrc/segtopk.hip, one launch each way (segment_topk_fused); everything else -- CPU tensors under a registered CPU backend, larger k,
    config.SEGMENT_TOPK_FUSED = False -- is two stable sorts and gathers in torch operators."""
    feat2d, sortby = _segment_topk_args(seglen, feat, k, sortby, total)
    offsets, n = _segment_offsets(seglen, feat2d, total, "segment_topk")
    if _segment_topk_kernel_ok(seglen, feat2d, k, sortby):
        return SegmentTopk.apply(feat2d, offsets, k, sortby, bool(descending))
    sparse.backend_for(feat)  # no CPU backend: DGLError
    return _segment_topk_composed(offsets, feat2d, k, sortby, descending, n)


# ----------------------------------------------------------------------------- point clouds: segment k nearest neighbours
_KNN_COMPOSED_ELEMS = 1 << 24  # the composition's [queries, len, D] difference tensor is built this many elements at a time


def _segment_knn_composed(offsets, x, k, return_dist):
    """ops.segment_knn through torch operators, by the same definition: per segment the direct-form distances sum_c (x_i - x_j)^2 and a
    stable sort of every query's row of them (NaN greatest, equal distances keep the lower row); index -1 and dist +inf past a
    segment's end.  One read-back of the offsets, a loop over segments.  The form for CPU tensors, for k > 64 or D > 256, under
    MGX_TORCH_OPS=1 and with config.KNN_FUSED off."""
    N, D = int(x.shape[0]), int(x.shape[1])
    index = torch.full((N, k), -1, dtype=torch.int64, device=x.device)
    dist = torch.full((N, k), float("inf"), dtype=torch.float32, device=x.device) if return_dist else None
    with torch.no_grad():
        ends = offsets.tolist()
        for beg, end in zip(ends[:-1], ends[1:]):
            n = end - beg
            if n <= 0:
                continue
            seg, m = x[beg:end], min(k, n)
            step = max(1, _KNN_COMPOSED_ELEMS // (n * D))
            for q in range(0, n, step):
                diff = seg[q:q + step].unsqueeze(1) - seg.unsqueeze(0)                          # [queries, n, D]
                d = (diff * diff).sum(-1)
                d = torch.where(d != d, d.new_full((), float("nan")), d)
                order = torch.sort(d, dim=1, stable=True)
                rows = slice(beg + q, beg + min(q + step, n))
                index[rows, :m] = order.indices[:, :m] + beg
                if return_dist:
                    dist[rows, :m] = order.values[:, :m]
    return index, dist


def _segment_rows_args(who, seglen, x, total):
    """What the point-cloud operators ask of their rows: x [N, D] fp32 with D >= 1 in segments of seglen, or DGLError."""
    _want_tensor(who, "x [N, D]", x, 2)
    _want_seglen(who, seglen, x, total)
    _want_seglen_device(who, seglen, x)
    if x.shape[1] < 1:
        raise DGLError("%s: x has no columns" % who)


def _segment_knn_args(seglen, x, k, total):
    _segment_rows_args("segment_knn", seglen, x, total)
    _want_count("segment_knn", "k", k)


def _segment_knn_kernel_ok(seglen, x, k):
    return (_device_kernels(x, config.KNN_FUSED, "segment_knn") and x.shape[0] > 0 and seglen.shape[0] < 2 ** 31 and _rows_fit(x)
            and sparse.backend_for(x).segment_knn_supported(k, int(x.shape[1])))


def segment_knn_fused(seglen, x, k, total=None, return_dist=False):
    """True when segment_knn(...) with these operands runs csrc/knn.hip (else the composition of distances and a stable sort)."""
    try:
        _segment_knn_args(seglen, x, k, total)
        return _segment_knn_kernel_ok(seglen, x, k)
    except DGLError:
        return False


def segment_knn(seglen, x, k, total=None, return_dist=False):
    """The k nearest rows of every row inside its own consecutive row segment (dgl.knn_graph / segmented_knn_graph): index int64 [N, k],
    or (index, dist [N, k]) with return_dist.

    x [N, D] (fp32; may be a row-strided column block), seglen [S] segment lengths.  d(i, j) = sum_c (x[i,c] - x[j,c])^2 in fp32, the
    direct difference form, over every j of i's segment, i included; neighbours are ordered by (d, j) ascending, so equal distances
    keep the lower row first and rank 0 of a finite point is itself or a lower-numbered duplicate; a NaN distance is the greatest
    key.  index holds global row numbers of x.  A segment shorter than k is padded with index -1 and dist +inf.  Neither output is
    differentiable: `index` is a selection, and `dist` is returned detached (no gradient flows to x through it).
    `total`: the row count when the caller knows it (no read-back of device lengths).  Device operands with k <= 64 and D <= 256 run
    csrc/knn.hip in one launch that writes no [n, n] matrix (segment_knn_fused); everything else -- CPU tensors under a registered CPU
    backend, larger k or D, config.KNN_FUSED = False -- is a stable sort of the distances per segment in torch operators."""
    _segment_knn_args(seglen, x, k, total)
    offsets, _ = _segment_offsets(seglen, x, total, "segment_knn")
    if _segment_knn_kernel_ok(seglen, x, k):
        with torch.no_grad():
            index, dist = sparse.backend_for(x).segment_knn(offsets, x.detach(), k, return_dist)
    else:
        sparse.backend_for(x)  # no CPU backend: DGLError
        index, dist = _segment_knn_composed(offsets, x.detach(), k, return_dist)
    return (index, dist) if return_dist else index


def _segment_knn_query_composed(offsets, x, q_offsets, y, k, eps, return_dist, return_weight):
    """ops.segment_knn_query through torch operators, by the same definition: per segment the direct-form distances
    sum_c (y_q - x_j)^2 of its queries to its references, built _KNN_COMPOSED_ELEMS elements at a time, and a stable sort of every
    query's row of them (NaN greatest, equal distances keep the lower row); index -1 and dist +inf past the reference segment's end;
    then the weights 1 / (d + eps) of the valid ranks over their sum.  One read-back of the two offset vectors, a loop over
    segments.  The form for CPU tensors, for k > 64 or D > 256, under MGX_TORCH_OPS=1 and with config.KNN_QUERY_FUSED off."""
    M, D = int(y.shape[0]), int(y.shape[1])
    index = torch.full((M, k), -1, dtype=torch.int64, device=y.device)
    dist = torch.full((M, k), float("inf"), dtype=torch.float32, device=y.device)
    with torch.no_grad():
        ends, q_ends = offsets.tolist(), q_offsets.tolist()
        for beg, end, q_beg, q_end in zip(ends[:-1], ends[1:], q_ends[:-1], q_ends[1:]):
            n, nq = end - beg, q_end - q_beg
            if n <= 0 or nq <= 0:
                continue
            seg, m = x[beg:end], min(k, n)
            step = max(1, _KNN_COMPOSED_ELEMS // (n * D))
            for q in range(0, nq, step):
                rows = slice(q_beg + q, q_beg + min(q + step, nq))
                diff = y[rows].unsqueeze(1) - seg.unsqueeze(0)                                  # [queries, n, D]
                d = (diff * diff).sum(-1)
                d = torch.where(d != d, d.new_full((), float("nan")), d)
                order = torch.sort(d, dim=1, stable=True)
                index[rows, :m] = order.indices[:, :m] + beg
                dist[rows, :m] = order.values[:, :m]
        weight = None
        if return_weight:
            valid = index >= 0
            inv = torch.where(valid, 1.0 / (dist + eps), dist.new_zeros(()))
            weight = torch.where(valid, inv / inv.sum(1, keepdim=True), dist.new_zeros(()))
    return index, (dist if return_dist else None), weight


def _segment_knn_query_args(ref_seglen, x, query_seglen, y, k, ref_total, query_total, eps):
    who = "segment_knn_query"
    for name, t in (("x", x), ("y", y)):  # one operand per message, and its name in the dtype one
        if not torch.is_tensor(t) or t.dim() != 2:
            raise DGLError("%s: expected %s [rows, D], got %s" % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__,))
        if t.dtype != torch.float32:
            raise DGLError("%s expects float32 input, got %s for %s" % (who, t.dtype, name))
    if x.device != y.device:
        raise DGLError("%s: operands on different devices: %s vs %s" % (who, x.device, y.device))
    if x.shape[1] != y.shape[1] or x.shape[1] < 1:
        raise DGLError("%s: x and y need the same number of columns, at least one (got %d and %d)" % (who, x.shape[1], y.shape[1]))
    _want_count(who, "k", k)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0 <= eps < float("inf"):
        raise DGLError("%s: eps must be a finite number >= 0, got %r" % (who, eps))
    for seglen, rows, total in ((ref_seglen, x, ref_total), (query_seglen, y, query_total)):
        _want_seglen(who, seglen, rows, total)
        _want_seglen_device(who, seglen, x)
    if ref_seglen.shape[0] != query_seglen.shape[0]:
        raise DGLError("%s: %d reference segments but %d query segments" % (who, ref_seglen.shape[0], query_seglen.shape[0]))


def _segment_knn_query_kernel_ok(ref_seglen, x, y, k):
    return (_device_kernels(x, config.KNN_QUERY_FUSED, "segment_knn_query") and y.shape[0] > 0 and ref_seglen.shape[0] < 2 ** 31
            and _rows_fit(x) and _rows_fit(y) and sparse.backend_for(x).segment_knn_query_supported(k, int(x.shape[1])))


def segment_knn_query_fused(ref_seglen, x, query_seglen, y, k, ref_total=None, query_total=None, return_dist=False, return_weight=False,
                            eps=1e-8):
    """True when segment_knn_query(...) with these operands runs csrc/knn.hip (else the composition of distances and a stable sort)."""
    try:
        _segment_knn_query_args(ref_seglen, x, query_seglen, y, k, ref_total, query_total, eps)
        return _segment_knn_query_kernel_ok(ref_seglen, x, y, k)
    except DGLError:
        return False


def segment_knn_query(ref_seglen, x, query_seglen, y, k, ref_total=None, query_total=None, return_dist=False, return_weight=False, eps=1e-8):
    """The k nearest reference rows of every query row, segment by segment (PyG's knn(x, y, k, batch_x, batch_y); the neighbour step of
    PointNet++'s feature propagation): index int64 [M, k], or a tuple (index[, dist][, weight]) with return_dist / return_weight.

    x [N, D] the references and y [M, D] the queries (fp32; each may be a row-strided column block); ref_seglen [S] and query_seglen [S]
    the lengths of their consecutive row segments, the same number of segments in both.  Query q of query segment s is answered from
    reference segment s alone: d(q, j) = sum_c (y[q,c] - x[j,c])^2 in fp32, the direct difference form of segment_knn; neighbours are
    ordered by (d, j) ascending, so equal distances keep the lower row first; a NaN distance is the greatest key.  index holds global
    row numbers of x.  A reference segment shorter than k is padded with index -1 and dist +inf (an empty one: every rank).
    weight [M, k] = (1 / (dist + eps)) / sum over the valid ranks of (1 / (dist + eps)), the normalised inverse squared-distance weights
    of knn_interpolate (eps = 1e-8 is the DGL PointNet++ example's constant): 0 at a padded rank, NaN at every valid rank of a query
    that has a NaN distance.  No output is differentiable.
    `ref_total` / `query_total`: the row counts when the caller knows them (no read-back of device lengths).  Device operands with
    k <= 64 and D <= 256 run csrc/knn.hip -- the kernel of segment_knn, which is the case y = x -- in one launch that writes no [M, n]
    matrix (segment_knn_query_fused); everything else -- CPU tensors under a registered CPU backend, larger k or D,
    config.KNN_QUERY_FUSED = False -- is a stable sort of the distances per segment in torch operators."""
    _segment_knn_query_args(ref_seglen, x, query_seglen, y, k, ref_total, query_total, eps)
    offsets, _ = _segment_offsets(ref_seglen, x, ref_total, "segment_knn_query")
    q_offsets, _ = _segment_offsets(query_seglen, y, query_total, "segment_knn_query")
    if _segment_knn_query_kernel_ok(ref_seglen, x, y, k):
        with torch.no_grad():
            index, dist, weight = sparse.backend_for(x).segment_knn_query(offsets, x.detach(), q_offsets, y.detach(), k, float(eps),
                                                                          return_dist, return_weight)
    else:
        sparse.backend_for(x)  # no CPU backend: DGLError
        index, dist, weight = _segment_knn_query_composed(offsets, x.detach(), q_offsets, y.detach(), k, float(eps), return_dist, return_weight)
    out = (index,) + ((dist,) if return_dist else ()) + ((weight,) if return_weight else ())
    return out if len(out) > 1 else index


# ----------------------------------------------------------------------------- point clouds: farthest point sampling and ball query
def _segment_fps_composed(offsets, x, m, start, return_dist):
    """ops.segment_fps through torch operators, by the same definition literally: per segment mind = +inf, then min(m, len) times
    record the current row, mark it selected, lower mind of the unselected rows by the direct-form distance to it (a NaN distance
    lowers nothing) and take the first unselected row of greatest mind.  One read-back of the offsets, a loop over segments and
    samples; the current row stays a device tensor.  The form for CPU tensors, shapes outside mgx_segment_fps_supported, under
    MGX_TORCH_OPS=1 and with config.FPS_FUSED off."""
    S = int(offsets.shape[0]) - 1
    index = torch.full((S, m), -1, dtype=torch.int64, device=x.device)
    dist = torch.zeros((S, m), dtype=torch.float32, device=x.device)
    with torch.no_grad():
        ends = offsets.tolist()
        for s, (beg, end) in enumerate(zip(ends[:-1], ends[1:])):
            n = end - beg
            if n <= 0:
                continue
            seg, mm = x[beg:end], min(m, n)
            mind = torch.full((n,), float("inf"), dtype=torch.float32, device=x.device)
            live = torch.ones(n, dtype=torch.bool, device=x.device)
            cur = torch.zeros(1, dtype=torch.int64, device=x.device)
            if start is not None:
                st = start[s:s + 1]
                cur = torch.where((st >= 0) & (st < n), st, cur)
            curd = mind[:1]
            for t in range(mm):
                index[s, t:t + 1] = cur + beg
                dist[s, t:t + 1] = curd
                live.index_fill_(0, cur, False)
                if t == mm - 1:
                    break
                diff = seg.index_select(0, cur) - seg
                d = (diff * diff).sum(-1)
                mind = torch.where(live & (d < mind), d, mind)
                key = torch.where(live, mind, mind.new_full((), -1.0))
                cur = torch.argmax(key).view(1)                                                 # the first maximal value: the lowest row
                curd = key.index_select(0, cur)
    return index, (dist if return_dist else None)


_BALL_COMPOSED_ELEMS = 1 << 24  # the composition's [queries, len, D] difference tensor is built this many elements at a time


def _segment_ball_query_composed(offsets, x, centers, radius2, K, pad_first):
    """ops.segment_ball_query through torch operators, by the same definition: per segment the direct-form distances of its centres to
    its rows, the mask d <= radius2 (a NaN distance is outside), a running count along the rows for the rank, the first K kept.
    One read-back of the offsets and one of which centres a segment holds, a loop over segments.  The form for CPU tensors, for
    K > 64 or D > 256, under MGX_TORCH_OPS=1 and with config.BALL_QUERY_FUSED off."""
    M, D = int(centers.shape[0]), int(x.shape[1])
    index = torch.full((M, K), -1, dtype=torch.int64, device=x.device)
    count = torch.zeros((M,), dtype=torch.int32, device=x.device)
    with torch.no_grad():
        ends = offsets.tolist()
        for beg, end in zip(ends[:-1], ends[1:]):
            n = end - beg
            if n <= 0 or M == 0:
                continue
            qs = ((centers >= beg) & (centers < end)).nonzero().flatten()
            seg, step = x[beg:end], max(1, _BALL_COMPOSED_ELEMS // (n * D))
            for q0 in range(0, int(qs.shape[0]), step):
                q = qs[q0:q0 + step]
                diff = x.index_select(0, centers.index_select(0, q)).unsqueeze(1) - seg.unsqueeze(0)      # [queries, n, D]
                inside = (diff * diff).sum(-1) <= radius2                                      # radius2 is a float32 value
                rank = torch.cumsum(inside, 1) - 1
                qi, col = (inside & (rank < K)).nonzero(as_tuple=True)
                index[q[qi], rank[qi, col]] = col + beg
                count[q] = inside.sum(1).clamp(max=K).to(torch.int32)
        if pad_first:
            empty = torch.arange(K, device=x.device).unsqueeze(0) >= count.unsqueeze(1)
            index = torch.where(empty, index[:, :1], index)                                    # count == 0: index[:, 0] is -1
    return index, count


def _segment_fps_args(seglen, x, npoints, start, total):
    """`start` as a contiguous int64 tensor [S] or None of a segment_fps call, or DGLError."""
    _segment_rows_args("segment_fps", seglen, x, total)
    _want_count("segment_fps", "npoints", npoints)
    S = int(seglen.shape[0])
    if start is not None:
        if isinstance(start, int) and not isinstance(start, bool):
            start = torch.full((S,), start, dtype=torch.int64, device=x.device)                # filled in on the device: no copy
        elif (not torch.is_tensor(start) or start.dtype != torch.int64 or start.dim() != 1 or start.shape[0] != S
              or start.device != x.device):
            raise DGLError("segment_fps: start must be None, an int or an int64 tensor [%d] on %s, got %s"
                           % (S, x.device, (start.dtype, tuple(start.shape), start.device) if torch.is_tensor(start) else repr(start)))
        else:
            start = start.contiguous()
    return start


def _fps_max_len(seglen, max_len):
    if max_len is not None:
        if isinstance(max_len, bool) or not isinstance(max_len, int) or max_len < 0:
            raise DGLError("segment_fps: max_len must be an integer >= 0, got %r" % (max_len,))
        return max_len
    return int(seglen.max()) if seglen.shape[0] else 0   # device lengths: the one read-back


def _segment_fps_kernel_ok(seglen, x, npoints, max_len):
    S = int(seglen.shape[0])
    return (_device_kernels(x, config.FPS_FUSED, "segment_fps") and S > 0 and S * npoints < 2 ** 31 and _rows_fit(x)
            and sparse.backend_for(x).segment_fps_supported(int(x.shape[1]), max_len))


def segment_fps_fused(seglen, x, npoints, start=None, total=None, max_len=None, return_dist=False):
    """True when segment_fps(...) with these operands runs csrc/fps.hip (else the same loop in torch operators)."""
    try:
        _segment_fps_args(seglen, x, npoints, start, total)
        return _segment_fps_kernel_ok(seglen, x, npoints, _fps_max_len(seglen, max_len))
    except DGLError:
        return False


def segment_fps(seglen, x, npoints, start=None, total=None, max_len=None, return_dist=False):
    """Farthest point sampling inside every consecutive row segment (dgl.geometry.farthest_point_sampler): index int64 [S, npoints],
    global row numbers of x, or (index, dist [S, npoints]) with return_dist.

    x [N, D] (fp32; may be a row-strided column block), seglen [S] segment lengths.  Per segment: mind = +inf; the first sample is
    row `start` of the segment (None: row 0 of every segment; an int; an int64 tensor [S]; a value outside the segment is taken as 0);
    every further sample is the unselected row whose distance to the nearest sample so far, mind, is greatest -- the lowest row on
    ties -- where mind is lowered by d = sum_c (x[cur,c] - x[j,c])^2 in fp32 (the direct form of segment_knn) whenever d < mind, so a
    NaN distance lowers nothing.  dist is mind of the sample when it was taken (+inf at rank 0).  The samples of a segment are
    distinct; duplicate points are taken in row order once everything else is at distance 0; a row with a NaN coordinate is taken
    right after the start.  A segment shorter than npoints is padded with index -1 and dist 0.  Neither output is differentiable.
    `total`: the row count when the caller knows it.  `max_len`: an upper bound of the segment lengths when the caller knows it; it
    chooses the kernel's shape on the host, so a device `seglen` without it costs ONE read-back (its maximum), and a segment longer
    than max_len is sampled from its first max_len rows only.  Device operands with D <= 64 and max_len <= min(16384,
    38912 // (D | 1)) -- 12 970 points for D = 3 -- run csrc/fps.hip, the whole chain in one launch (segment_fps_fused); everything
    else -- CPU tensors under a registered CPU backend, longer segments, config.FPS_FUSED = False -- is the same loop in torch operators."""
    start = _segment_fps_args(seglen, x, npoints, start, total)
    offsets, _ = _segment_offsets(seglen, x, total, "segment_fps")
    max_len = _fps_max_len(seglen, max_len)
    if _segment_fps_kernel_ok(seglen, x, npoints, max_len):
        with torch.no_grad():
            index, dist = sparse.backend_for(x).segment_fps(offsets, x.detach(), npoints, max_len, start, return_dist)
    else:
        sparse.backend_for(x)  # no CPU backend: DGLError
        index, dist = _segment_fps_composed(offsets, x.detach(), npoints, start, return_dist)
    return (index, dist) if return_dist else index


def _segment_ball_query_args(seglen, x, centers, radius, max_neighbors, pad, total):
    """radius2 = float32(radius) * float32(radius) of a segment_ball_query call, or DGLError."""
    _segment_rows_args("segment_ball_query", seglen, x, total)
    _want_count("segment_ball_query", "max_neighbors", max_neighbors)
    if not torch.is_tensor(centers) or centers.dim() != 1 or centers.dtype != torch.int64 or centers.device != x.device:
        raise DGLError("segment_ball_query: centers must be an int64 tensor [M] of rows of x on %s, got %s"
                       % (x.device, (centers.dtype, tuple(centers.shape), centers.device) if torch.is_tensor(centers) else type(centers).__name__))
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not radius >= 0:
        raise DGLError("segment_ball_query: radius must be a number >= 0, got %r" % (radius,))
    if pad not in ("first", None):
        raise DGLError("segment_ball_query: pad must be 'first' or None, got %r" % (pad,))
    r = torch.tensor(float(radius), dtype=torch.float32)
    return float(r * r)                                                                        # once, on the host


def _segment_ball_query_kernel_ok(seglen, x, centers, max_neighbors):
    return (_device_kernels(x, config.BALL_QUERY_FUSED, "segment_ball_query") and seglen.shape[0] < 2 ** 31 and _rows_fit(x)
            and centers.shape[0] < 2 ** 31 and sparse.backend_for(x).segment_ball_query_supported(max_neighbors, int(x.shape[1])))


def segment_ball_query_fused(seglen, x, centers, radius, max_neighbors, pad="first", total=None):
    """True when segment_ball_query(...) with these operands runs csrc/ballquery.hip (else the composition in torch operators)."""
    try:
        _segment_ball_query_args(seglen, x, centers, radius, max_neighbors, pad, total)
        return _segment_ball_query_kernel_ok(seglen, x, centers, max_neighbors)
    except DGLError:
        return False


def segment_ball_query(seglen, x, centers, radius, max_neighbors, pad="first", total=None):
    """The first max_neighbors rows within `radius` of every centre, inside the centre's own consecutive row segment (the PointNet++
    ball query): (index int64 [M, K], count int32 [M]).

    x [N, D] (fp32; may be a row-strided column block), seglen [S] segment lengths, centers int64 [M] global rows of x in any order
    (duplicates allowed; -1: no centre).  index[q] holds, in ascending row order, the first K rows j of the segment of centers[q] with
    d = sum_c (x[c,c'] - x[j,c'])^2 <= radius2 in fp32 (the direct form of segment_knn), radius2 = float32(radius) * float32(radius)
    computed once on the host; a NaN distance is outside the ball.  These are the FIRST rows in the ball, not the nearest.  count[q] is
    how many were found, at most K.  Ranks past count[q] hold index[q, 0] with pad = "first" (the PointNet++ convention: every query
    has exactly K entries) and -1 with pad = None; a query that found nothing -- a NaN centre, a centre -1 or outside every segment --
    holds -1 everywhere.  Neither output is differentiable.
    `total`: the row count when the caller knows it (no read-back of device lengths).  Device operands with K <= 64 and D <= 256 run
    csrc/ballquery.hip in one launch that writes no [M, n] matrix (segment_ball_query_fused); everything else -- CPU tensors under a
    registered CPU backend, larger K or D, config.BALL_QUERY_FUSED = False -- is a masked running count per segment in torch operators."""
    radius2 = _segment_ball_query_args(seglen, x, centers, radius, max_neighbors, pad, total)
    offsets, _ = _segment_offsets(seglen, x, total, "segment_ball_query")
    if _segment_ball_query_kernel_ok(seglen, x, centers, max_neighbors):
        with torch.no_grad():
            return sparse.backend_for(x).segment_ball_query(offsets, x.detach(), centers.contiguous(), radius2, max_neighbors, pad == "first")
    sparse.backend_for(x)  # no CPU backend: DGLError
    return _segment_ball_query_composed(offsets, x.detach(), centers, radius2, max_neighbors, pad == "first")


def segment_broadcast(seglen, value, total):
    """out[i] = value[segment of row i] for `total` rows (dgl.broadcast_nodes / broadcast_edges)."""
    if value.shape[0] != seglen.shape[0]:
        raise DGLError("segment_broadcast: %d segments, value has %d rows" % (seglen.shape[0], value.shape[0]))
    return SegmentBroadcast.apply(value, _offsets_of(seglen, value.device), int(total))


# ----------------------------------------------------------------------------- public API
def gspmm(g, op, reduce_op, lhs_data, rhs_data):
    """Generalized SpMM: out[v] = reduce_{(u->v)} op(lhs[u], rhs[e]).  (kernel/dgl-new.py:20)"""
    if op not in ("add", "sub", "mul", "div", "copy_lhs", "copy_rhs"):
        raise DGLError("Unsupported binary op %r for gspmm" % (op,))
    if reduce_op not in ("sum", "max", "min", "mean"):
        raise DGLError("Unsupported reduce op %r for gspmm" % (reduce_op,))
    gidx = _gidx(g)
    if op == "sub":  # same rewrites as DGL's ops/spmm.py
        op, rhs_data = "add", -rhs_data
    elif op == "div":
        op, rhs_data = "mul", 1.0 / rhs_data
    expand_l = expand_r = False
    if op != "copy_rhs":
        if lhs_data is None:
            raise DGLError("gspmm: op %r needs lhs_data" % op)
        if lhs_data.dim() == 1:
            lhs_data, expand_l = lhs_data.unsqueeze(-1), True
    if op != "copy_lhs":
        if rhs_data is None:
            raise DGLError("gspmm: op %r needs rhs_data" % op)
        if rhs_data.dim() == 1:
            rhs_data, expand_r = rhs_data.unsqueeze(-1), True
    X = None if op == "copy_rhs" else lhs_data
    Y = None if op == "copy_lhs" else rhs_data
    out = GSpMM.apply(gidx, op, reduce_op, X, Y)
    squeeze = (expand_l or X is None) and (expand_r or Y is None) and (expand_l or expand_r)
    return out.squeeze(-1) if squeeze else out


class RelWeightCache(object):
    """The [E, R] edge weights of a multi-relation g-SpMM permuted into the position order of a graph's in-CSR (forward) and out-CSR
    (reverse walk): for ogbn-proteins they are constant data, so the two permutations are paid once.  Keyed on the tensor's storage
    (data_ptr, shape, strides), its version counter and the graph index, the way CatBuffer and the slot tags are: an in-place write to
    the weights, another tensor or another graph drops both copies."""

    def __init__(self):
        self._key, self._gidx, self._held, self._perm = None, None, None, {}

    @staticmethod
    def _key_of(w):
        return (w.data_ptr(), int(w._version), tuple(w.shape), tuple(w.stride()), w.device)

    def get(self, gidx, w, side):
        """w in the order of gidx.csc() (side "in") or gidx.csr() (side "out"); [nnz, R] contiguous."""
        key = self._key_of(w)
        if key != self._key or self._gidx is not gidx:
            self._key, self._gidx, self._held, self._perm = key, gidx, w, {}  # (`_held` keeps the storage, and so its address, alive)
        if side not in self._perm:
            self._perm[side] = _permute_rel_weights(gidx.csc() if side == "in" else gidx.csr(), w)
        return self._perm[side]

    def holds(self, gidx, w, side):
        return self._gidx is gidx and self._key == self._key_of(w) and side in self._perm


def _permute_rel_weights(csr, w):
    with torch.no_grad():
        w = w.detach()
        if csr.eids is None:
            return w.contiguous()
        return sparse.backend_for(w).gather_rows(w, csr.eids)


def rel_weight_cache_for(g):
    """The RelWeightCache kept on a graph's index: every layer of a model passes the same edge weights, so they share one."""
    gidx = _gidx(g)
    cache = gidx.__dict__.get("_rel_weights")
    if cache is None:
        cache = gidx.__dict__["_rel_weights"] = RelWeightCache()
    return cache


class RelGSpMM(torch.autograd.Function):
    """out[v, r, :] = sum | mean_{e: u -> v} w[e, r] * x[u, :] in one walk of the in-CSR (csrc/spmm_rel.hip); the gradient with respect
    to x in one walk of the out-CSR.  w is constant here (rel_gspmm sends weights that need a gradient to gspmm)."""

    @staticmethod
    def forward(ctx, gidx, reduce_op, x, w, cache):
        csc = gidx.csc()
        be = sparse.backend_for(x)
        w_in = cache.get(gidx, w, "in") if cache is not None else _permute_rel_weights(csc, w)
        ctx.backward_cache = gidx, reduce_op, cache
        ctx.save_for_backward(w)
        return be.spmm_rel(csc, reduce_op, w_in, x)

    @staticmethod
    @once_differentiable
    def backward(ctx, dZ):
        gidx, reduce_op, cache = ctx.backward_cache
        w, = ctx.saved_tensors
        if not ctx.needs_input_grad[2]:
            return None, None, None, None, None
        rev = gidx.csr()  # rows = src: the reversed graph's in-CSR
        w_out = cache.get(gidx, w, "out") if cache is not None else _permute_rel_weights(rev, w)
        inv = gidx.csc().inv_degrees() if reduce_op == "mean" else None  # the 1 / deg of `mean`, per gathered row of dZ
        dX = sparse.backend_for(dZ).spmm_rel_grad(rev, w_out, dZ.contiguous(), dst_scale=inv)
        return None, None, dX, None, None


def rel_weight_matrix(g, edge_weights):
    """The [E, R] weight matrix of a relational layer from what its caller holds: the matrix itself, or the list of R [E, 1] columns the
    reference script builds (main_dgl_proteins_rgcn_for.py:159-161).  Columns that are views of one matrix -- slices feat[:, t:t+1] of
    an edge-feature matrix already on the device -- give that matrix back as a view (same storage and version counter, nothing copied);
    any other list is concatenated once and kept on the graph until one of its tensors changes."""
    if torch.is_tensor(edge_weights):
        if edge_weights.dim() != 2:
            raise DGLError("edge_weights: expected an [E, R] matrix or a list of R [E, 1] columns, got shape %s" % (tuple(edge_weights.shape),))
        return edge_weights
    cols = list(edge_weights)
    if not cols:
        raise DGLError("edge_weights: empty list")
    first, R = cols[0], len(cols)
    for c in cols:
        if not torch.is_tensor(c) or c.shape[0] != first.shape[0] or c.numel() != c.shape[0] or c.dtype != first.dtype or c.device != first.device:
            raise DGLError("edge_weights: expected R columns of one length, dtype and device")
    if R == 1:
        return first.reshape(-1, 1)
    E, step, size = int(first.shape[0]), int(first.stride(0)), first.element_size()
    store = first.untyped_storage().data_ptr()
    if (E > 0 and step >= R and not any(c.requires_grad for c in cols)
            and all(c.untyped_storage().data_ptr() == store and int(c.stride(0)) == step and c.data_ptr() == first.data_ptr() + r * size
                    for r, c in enumerate(cols))):
        return torch.as_strided(first, (E, R), (step, 1))
    if any(c.requires_grad for c in cols):
        return torch.cat([c.reshape(-1, 1) for c in cols], 1)
    gidx = _gidx(g)
    key = tuple((c.data_ptr(), int(c._version)) for c in cols)
    held = gidx.__dict__.get("_rel_weight_cat")
    if held is None or held[0] != key:
        held = gidx.__dict__["_rel_weight_cat"] = (key, cols, torch.cat([c.reshape(-1, 1) for c in cols], 1))
    return held[2]


def _rel_gspmm_args(g, x, w, reduce):
    """The graph index of a rel_gspmm call, or DGLError.  Row counts and dtypes are gspmm's to judge: the broadcast form takes them."""
    gidx = _gidx(g)
    if reduce not in ("sum", "mean"):
        raise DGLError("rel_gspmm: reduce must be 'sum' or 'mean', got %r" % (reduce,))
    if not (torch.is_tensor(x) and torch.is_tensor(w) and x.dim() == 2 and w.dim() == 2):
        raise DGLError("rel_gspmm: expected x [N_src, D] and w [E, R], got shapes %s and %s"
                       % tuple(tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in (x, w)))
    return gidx


def _rel_gspmm_kernel_ok(gidx, x, w):
    E = gidx.num_edges()
    if (not _device_kernels(x, True, "spmm_rel") or w.device != x.device or w.requires_grad or x.dtype != torch.float32
            or w.dtype != torch.float32 or capture_path() or x.shape[0] != gidx.num_src or w.shape[0] != E or E == 0):
        return False
    return sparse.backend_for(x).spmm_rel_supported(gidx.csc(), x, int(w.shape[1]))


def rel_gspmm_fused(g, x, w):
    """True when rel_gspmm(g, x, w) runs the one-pass kernels (else it is gspmm's (N, 1, D) x (E, R, 1) broadcast)."""
    try:
        return _rel_gspmm_kernel_ok(_rel_gspmm_args(g, x, w, "mean"), x, w)
    except DGLError:
        return False


def rel_gspmm(g, x, w, reduce="mean", cache=None):
    """Multi-relation g-SpMM: out[v, r, :] = reduce_{e: u -> v} w[e, r] * x[u, :] for all R relations at once.

    x: [N_src, D], w: [E, R] in edge-id order, result [N_dst, R, D]; reduce: "sum" or "mean".  This is the R update_all(fn.u_mul_e,
    fn.mean) calls of the edge-weighted relational layer (main_dgl_proteins_rgcn_for.py:50-53) in one pass over the graph.  fp32 device
    operands with 1 <= R <= 16 and D a power of two up to 128 run csrc/spmm_rel.hip (forward and the gradient with respect to x);
    weights that need a gradient, and every other operand, take gspmm(g, "mul", reduce, x[:, None, :], w[:, :, None]) -- the same values
    through the broadcast kernels.  cache: a RelWeightCache for the permuted weights (default: the one kept on the graph; False: none)."""
    gidx = _rel_gspmm_args(g, x, w, reduce)
    if not _rel_gspmm_kernel_ok(gidx, x, w):
        return gspmm(gidx, "mul", reduce, x.unsqueeze(1), w.unsqueeze(-1))
    if cache is None:
        cache = rel_weight_cache_for(gidx)
    return RelGSpMM.apply(gidx, reduce, x, w, cache if cache is not False else None)


def gsddmm(g, op, lhs_data, rhs_data, lhs_target="u", rhs_target="v"):
    """Generalized SDDMM: out[e] = op(lhs[t_l(e)], rhs[t_r(e)]).  (kernel/dgl-new.py:39)"""
    if op not in ("add", "sub", "mul", "div", "dot", "copy_lhs", "copy_rhs"):
        raise DGLError("Unsupported binary op %r for gsddmm" % (op,))
    for t in (lhs_target, rhs_target):
        if t not in ("u", "e", "v"):
            raise DGLError("Unsupported target %r; expected 'u', 'e' or 'v'" % (t,))
    gidx = _gidx(g)
    expand_l = expand_r = False
    if op != "copy_rhs" and lhs_data is not None and lhs_data.dim() == 1:
        lhs_data, expand_l = lhs_data.unsqueeze(-1), True
    if op != "copy_lhs" and rhs_data is not None and rhs_data.dim() == 1:
        rhs_data, expand_r = rhs_data.unsqueeze(-1), True
    X = None if op == "copy_rhs" else lhs_data
    Y = None if op == "copy_lhs" else rhs_data
    out = GSDDMM.apply(gidx, op, X, Y, lhs_target, rhs_target)
    squeeze = (expand_l or X is None) and (expand_r or Y is None) and (expand_l or expand_r) and op != "dot"
    return out.squeeze(-1) if squeeze else out


def edge_softmax(graph, logits, eids="__ALL__", norm_by="dst"):
    """Softmax of edge logits over the in-edges of every destination node (fused kernel)."""
    if not isinstance(eids, str):
        raise DGLError("edge_softmax on an edge subset is not supported by this backend")
    if norm_by not in ("dst", "src"):
        raise DGLError("norm_by must be 'dst' or 'src'")
    return EdgeSoftmax.apply(_gidx(graph), logits, norm_by)


def segment_reduce(seglen, value, reducer="sum", total=None):
    """dgl.ops.segment_reduce: reduce consecutive row segments of `value` (AvgPooling readout)."""
    if reducer not in ("sum", "mean", "max", "min"):
        raise DGLError("Unsupported segment reducer %r" % (reducer,))
    # value must have sum(seglen) rows: known on the host for host lengths, or passed by a caller that knows it
    # (a batched graph's node count); otherwise read back once
    if total is None and not seglen.is_cuda:
        total = int(seglen.sum())
    offsets = torch.zeros(seglen.shape[0] + 1, dtype=torch.int64, device=value.device)
    torch.cumsum(seglen.to(value.device).long(), 0, out=offsets[1:])
    return SegmentReduce.apply(reducer, value, offsets, total)


# named shortcuts (dgl.ops.copy_u_sum, ...)
def copy_u_sum(g, x):
    return gspmm(g, "copy_lhs", "sum", x, None)


def copy_u_mean(g, x):
    return gspmm(g, "copy_lhs", "mean", x, None)


def copy_e_sum(g, x):
    return gspmm(g, "copy_rhs", "sum", None, x)


def u_mul_e_sum(g, x, y):
    return gspmm(g, "mul", "sum", x, y)


def u_add_v(g, x, y):
    return gsddmm(g, "add", x, y, "u", "v")


def u_dot_v(g, x, y):
    return gsddmm(g, "dot", x, y, "u", "v")
