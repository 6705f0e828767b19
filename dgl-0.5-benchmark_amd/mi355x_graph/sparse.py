"""Raw (non-autograd) sparse primitives on torch tensors, dispatched to the HIP C ABI.

Mirrors the role of DGL's python/dgl/sparse.py (_gspmm / _gsddmm, UPSTREAM) for the call sites
kernel/dgl-new.py:20,39 and main_dgl_product_sage.py:62: shape/broadcast bookkeeping and output
allocation happen here (caller-allocates convention of the seam), the arithmetic happens in
csrc/*.hip.  Tensors on a HIP device go to `HipBackend`; there is no built-in backend for CPU
tensors -- message-passing arithmetic on CPU tensors raises DGLError.  (tests/ registers a checker
backend for multi-process gloo tests; the product never does.)
"""
import ctypes
import os
import functools

import numpy as np
import torch

from . import _lib
from ._lib import DGLError, MgxCsr, OP, REDUCE, TARGET
from . import config


# Every tile plan is bounds-checked once when it is built (the kernels follow its tables blindly: a wrong entry would be an
# out-of-bounds access on the device).  A dozen reductions with host syncs per plan; config.TILE_VALIDATE = False skips them.
PROFILE = None  # set to a list by bench.py to collect per-launch HIP-event timings of mgx_spmm_csr


class timed_call(object):
    """`with timed_call(dev, kernel=..., **meta):` around ONE C-ABI call: when bench.py has set PROFILE to a list, HIP events on the
    launch stream bracket the call and a record {kernel, meta..., start, end} is appended (the g-SpMM entry points below build
    theirs inline, with the same keys).  Costs one attribute read otherwise."""
    __slots__ = ("rec", "dev")

    def __init__(self, dev, **meta):
        self.rec, self.dev = (meta if PROFILE is not None else None), dev

    def __enter__(self):
        if self.rec is not None:
            self.rec["start"] = torch.cuda.Event(enable_timing=True)
            self.rec["end"] = torch.cuda.Event(enable_timing=True)
            self.rec["start"].record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.rec is not None and exc[0] is None and PROFILE is not None:
            self.rec["end"].record(torch.cuda.current_stream(self.dev))
            PROFILE.append(self.rec)
        return False


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _prod(shape):
    p = 1
    for s in shape:
        p *= int(s)
    return p


# ----------------------------------------------------------------------------- operand layouts
# The C entry points take raw pointers; the kernels behind many of them read 16 bytes per lane.  What a wrapper may hand such an entry
# is decided here, once (docs/LOG_operand_layouts.md lists every entry point and which of these it needs):
#   aligned16  the predicate: no operand is contiguous at an odd storage offset
#   dense16    a dense operand: contiguous, base 16-byte aligned -- the tensor itself when it already is, else a copy
#   rows16     an operand of an entry that takes a row stride: the view itself when the kernels can walk it, else dense16
def _off16(t):
    """the one statement of the rule: the base of `t` is not on a 16-byte boundary"""
    return t.data_ptr() % 16 != 0


def aligned16(*tensors):
    """False when one of `tensors` is contiguous at a base that is not 16-byte aligned (a slice of a flattened buffer, a gradient cut
    out of a `cat`): the 16-byte lanes cannot read it where it lies.  None entries pass; a strided tensor is copied by its wrapper and
    a fresh allocation is aligned."""
    return not any(t is not None and t.is_contiguous() and _off16(t) for t in tensors)


def dense16(t):
    """`t` as the kernels take a dense operand: contiguous with a 16-byte aligned base.  An aligned contiguous tensor is returned as
    it is (no copy); a strided or expanded view is made contiguous; a contiguous tensor at an odd storage offset is copied into a
    fresh allocation: the entry points refuse such a base."""
    if t is None:
        return None
    t = t.contiguous()
    return t if aligned16(t) else t.clone(memory_format=torch.contiguous_format)


def rows16(t, max_bytes=None):
    """(tensor, row stride in floats) of a [N, ...] operand as an entry point with a row-stride argument takes it: the floats of a row
    contiguous, the row stride a multiple of 4 floats and at least the row length, the base 16-byte aligned (a column block of a wider
    matrix whose first column is a multiple of 4 qualifies; max_bytes: rows * stride * 4 stays below it) -- else a dense16 copy."""
    W, want = _prod(t.shape[1:]), 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and stride != want:
            return dense16(t), W
        want *= int(size)
    ld = int(t.stride(0))
    if (t.dim() >= 2 and t.shape[0] > 0 and ld >= W and ld % 4 == 0 and not _off16(t)
            and (max_bytes is None or t.shape[0] * ld * 4 < max_bytes)):
        return t, ld
    return dense16(t), W


class CsrView(object):
    """An immutable CSR over torch tensors (in-CSR: rows = destination nodes)."""

    __slots__ = ("__weakref__", "num_rows", "num_cols", "indptr", "indices", "eids", "_c", "_deg", "_inv_deg", "_plan", "_sm_plan",
                 "_row_order", "dst_is_src_prefix", "_tile_plan", "_short", "short_hint", "_rows", "_gate", "_head_dn")

    def __init__(self, num_rows, num_cols, indptr, indices, eids):
        self.num_rows, self.num_cols = int(num_rows), int(num_cols)
        self.indptr, self.indices, self.eids = indptr, indices, eids
        self._c = None
        self._deg = None
        self._inv_deg = None
        self._plan = False  # False = not built yet; None = run without a plan
        self._sm_plan = False
        self._tile_plan = False
        self._short = {}        # lane groups per wave -> None | True | two-part SpmmPlan (see _short_choice); "split": its tables
        self.short_hint = None  # the owner's word on short rows where reading the lengths back is impossible (graph capture) or not
                                # worth it (a sampled block): True / False, or the average row length (see _short_choice)
        self._row_order = (None, None)  # (row order, kind) computed with the first plan
        self._rows = None  # row id of every stored position (the expanded indptr), built on first use by the permuted g-SDDMM walk
        self._gate = None  # ops._SlotGate of untagged 64-column operands aggregated over this CSR (ops._gspmm_over_slots)
        self._head_dn = None  # (matrix, row list, its version, its slots or None): the [N, K] operand ops.SageMeanCatHeadFn's backward gathers over this CSR, kept
                              # zero outside the list between steps (ops._head_dn)
        self.dst_is_src_prefix = False  # block graphs whose destination nodes are the first source nodes

    @property
    def nnz(self):
        return int(self.indices.shape[0])

    @property
    def device(self):
        return self.indptr.device

    @property
    def idx_bits(self):
        return 32 if self.indptr.dtype == torch.int32 else 64

    def c_struct(self):
        if self._c is None:
            self._c = MgxCsr(self.num_rows, self.num_cols, self.nnz, self.indptr.data_ptr(),
                             self.indices.data_ptr() if self.indices.numel() else None,
                             None if self.eids is None else self.eids.data_ptr(), self.idx_bits, 0)
        return self._c

    def row_of_position(self):
        """[nnz] the row of every stored entry: with `indices` and `eids` the CSR as an edge list in ITS order (sorted by row)."""
        if self._rows is None:
            ids = torch.arange(self.num_rows, dtype=self.indptr.dtype, device=self.indptr.device)
            self._rows = torch.repeat_interleave(ids, (self.indptr[1:] - self.indptr[:-1]).long(), output_size=self.nnz)
        return self._rows

    def degrees(self):
        if self._deg is None:
            if self.indptr.is_cuda:
                self._deg = backend_for(self.indptr).degrees(self)
            else:  # integer graph preparation on the host, like the reference (bit-exact either way)
                self._deg = self.indptr[1:] - self.indptr[:-1]
        return self._deg

    def inv_degrees(self):
        """1 / max(deg, 1) as fp32 -- the factor of fn.mean (main_dgl_product_sage.py:62)."""
        if self._inv_deg is None:
            self._inv_deg = backend_for(self.indptr).inv_degrees(self)
        return self._inv_deg

    def short_rows(self, width):
        """True when the summing g-SpMM of `width` columns gives the work items a LANE GROUP each (see spmm_plan_for)."""
        return self._short_choice(width) is not None

    def spmm_plan_for(self, width):
        """(plan, short) for a full-width copy_u / copy_e sum of `width` columns: the CSR's schedule and False, or -- short rows -- the
        plan to pass with MGX_SPMM_SHORT_ROWS set: the schedule itself when no item is long, else its two-part form (mgx_spmm_plan::rest)."""
        choice = self._short_choice(width)
        if choice is None:
            return self.plan(), False
        return (self.plan() if choice is True else choice), True

    def _short_choice(self, width):
        """None: a wave per work item (spmm_rowwave32_kernel).  Otherwise the SHORT work items -- at most schedule.short_item_limit(B)
        edges, B = 64 / G the items a wave walks side by side, G = lanes per feature row -- get a lane group each
        (spmm_rowgroup32_kernel): True = every item is short, pass the CSR's own schedule; a SpmmPlan = pass this two-part plan, whose
        `rest` (longer rows, chunks of split rows) keeps the wave-per-item kernel in a second launch of the same call.
        Taken when (measurements: docs/LOG_r04.md section 2)
          enough items are short  all of them, or at least schedule.MIN_SHORT_ITEMS (what the second launch has to pay for),
          short on average        the short items average fewer than 3 edges per lane group of the wave, at most 16,
          and even                sum over batches of B consecutive short items of max(length) * B <= MGX_ROWGROUP_IMBALANCE (6) x their
                                  edges: a wave lasts as long as the longest item of its batch.
        Decided once per CSR and lane-group count (two host reads); a structure rebuilt on the device inside a captured step cannot be
        read back and says so itself through `short_hint` (graph_classification.GraphedBatchTrainer: molecules, degree <= 6)."""
        lanes, G = (int(width) + 3) // 4, 1
        while G < lanes and G < 64:
            G *= 2
        nb = 64 // G
        if nb < 2 or self.idx_bits != 32 or not self.indptr.is_cuda or self.nnz == 0 or width % 4:
            return None
        if self.short_hint is not None:
            if self.short_hint is True or self.short_hint is False:
                return True if self.short_hint else None
            # a number: the average row length of a structure that lives for one step (a sampled block) -- the average rule alone,
            # from host-known sizes; rows above 32 edges are taken by the whole wave inside the kernel
            return True if float(self.short_hint) < (16.0 if nb >= 8 else 3.0 * nb) else None
        if nb not in self._short:
            if torch.cuda.is_current_stream_capturing():
                return None  # the lengths cannot be read back inside a capture: the wave-per-item kernel, nothing cached
            from . import schedule
            limit = schedule.short_item_limit(nb)
            if ("split", limit) not in self._short:
                self._short[("split", limit)] = schedule.split_short_items(self, self.plan(), limit=limit)
            split, choice = self._short[("split", limit)], None
            if split is not None:
                plan, lens, edges = split
                n_short = int(lens.shape[0])
                pad = (-n_short) % nb
                padded = torch.cat([lens, lens.new_zeros(pad)]) if pad else lens
                worst = float(padded.view(-1, nb).max(dim=1)[0].sum()) * nb  # one host read
                if edges / n_short < (16.0 if nb >= 8 else 3.0 * nb) and worst <= config.SHORT_ROWS_IMBALANCE * edges:
                    choice = True if (plan is None or plan.rest is None) else plan
            self._short[nb] = choice
        return self._short[nb]

    def plan(self):
        """Execution schedule for the summing g-SpMM (schedule.py); built on first use, device only."""
        if self._plan is False:
            from . import schedule
            self._plan = schedule.plan_for(self) if self.indptr.is_cuda else None
        return self._plan

    def _tile_base_plan(self):
        """The work items every tile plan of this CSR is cut from (hub rows split at tileplan.TILE_SPLIT edges): built once."""
        from . import schedule, tileplan
        if "base" not in self._tile_plan:
            self._tile_plan["base"] = schedule.plan_for(self, split=tileplan.TILE_SPLIT)
        return self._tile_plan["base"]

    def gat_tile_plan(self, F):
        """Tile plan for the fused GAT walks over this CSR (one head of 4 .. 16 columns, dense neighbourhoods: gat_tile.inc), else None.
        Its own plan: 4 lanes per row with the node of every position and every entry's rank among parallel edges (attn_drop keys)."""
        from . import tileplan
        if F % 4 != 0 or not 4 <= F <= 16 or os.environ.get("MGX_GAT_TILE", "1") == "0" or self.num_cols >= (1 << 24):
            return None
        if self._tile_plan is False:
            self._tile_plan = {} if tileplan.tile_plan_wanted(self) else None
        if self._tile_plan is None:
            return None
        if "gat" not in self._tile_plan:
            from . import schedule
            self.plan()
            nc, nacc, nl, tau = tileplan.gat_config()
            base = self._tile_base_plan()
            held = tileplan.build_tile_plan(self, base, nc, nacc, nl, tau, lanes_log2=2, pair_rank=True)
            if config.TILE_VALIDATE:
                tileplan.validate(held, self)
            self._tile_plan["gat"] = held
        return self._tile_plan["gat"]

    def tile_plan(self, width=64):
        """Tile plan of the LDS-staged g-SpMM (tileplan.py) for rows of `width` columns on graphs with dense neighbourhoods, else
        None; built on first use, one per kernel geometry (64- / 32- / 16-column passes)."""
        from . import tileplan
        lg = tileplan.lanes_log2_for(width)
        if self._tile_plan is False:
            self._tile_plan = {} if tileplan.tile_plan_wanted(self) else None
        if self._tile_plan is None:
            return None
        if lg not in self._tile_plan:
            from . import schedule
            self.plan()  # computes (and caches) the locality row order first
            nc, nacc, nl, tau = tileplan.config(lg)
            base = self._tile_base_plan()
            tp = tileplan.build_tile_plan(self, base, nc, nacc, nl, tau, lanes_log2=lg)
            if config.TILE_VALIDATE:
                tileplan.validate(tp, self)
            self._tile_plan[lg] = tp
        return self._tile_plan[lg]

    def softmax_plan(self):
        """Schedule of the edge-softmax / fused attention kernels: the g-SpMM plan."""
        return self.plan()

    def to(self, device):
        out = CsrView(self.num_rows, self.num_cols, self.indptr.to(device), self.indices.to(device),
                      None if self.eids is None else self.eids.to(device))
        out.short_hint = self.short_hint  # a property of the structure, not of where it lives
        return out

    def astype(self, dtype):
        if self.indptr.dtype == dtype:
            return self
        out = CsrView(self.num_rows, self.num_cols, self.indptr.to(dtype), self.indices.to(dtype),
                      None if self.eids is None else self.eids.to(dtype))
        out.short_hint = self.short_hint
        return out


# ----------------------------------------------------------------------------- broadcasting
def _is_head_bcast(shape, oshape):
    """True when `shape` == oshape[:j] + (1,)*(n-j): element k of the output uses operand element
    k // (out_len / len) -- the (N,H,F) x (E,H,1) pattern; expressed to the C ABI as a NULL table."""
    if len(shape) != len(oshape):
        return False
    j = len(shape)
    while j > 0 and shape[j - 1] == 1:
        j -= 1
    return tuple(shape[:j]) == tuple(oshape[:j])


@functools.lru_cache(maxsize=256)
def _bcast_plan(lshape, rshape):
    nd = max(len(lshape), len(rshape))
    ls = (1,) * (nd - len(lshape)) + tuple(lshape)
    rs = (1,) * (nd - len(rshape)) + tuple(rshape)
    out = []
    for a, b in zip(ls, rs):
        if a != b and a != 1 and b != 1:
            raise DGLError("Feature shapes %s and %s are not broadcastable" % (lshape, rshape))
        out.append(max(a, b))
    out = tuple(out)

    def table(shape):
        if shape == out or _is_head_bcast(shape, out):
            return None
        idx = np.indices(out).reshape(nd, -1)
        strides = np.ones(nd, np.int64)
        for d in range(nd - 2, -1, -1):
            strides[d] = strides[d + 1] * shape[d + 1]
        off = np.zeros(idx.shape[1], np.int64)
        for d in range(nd):
            if shape[d] != 1:
                off += idx[d] * strides[d]
        return off

    return out, table(ls), table(rs)


_table_cache = {}


def _device_table(arr, device):
    if arr is None:
        return None
    key = (arr.tobytes(), str(device))
    t = _table_cache.get(key)
    if t is None:
        t = torch.from_numpy(arr).to(device)
        _table_cache[key] = t
    return t


# ----------------------------------------------------------------------------- backends
def _short_variant(plan):
    """Label of a MGX_SPMM_SHORT_ROWS launch in bench.py's records: which kernels one call runs."""
    if plan is not None and plan.rest is not None:
        return "lane-group (spmm_rowgroup32_kernel, %d short items) + row (spmm_rowwave32_kernel, %d items)" % (plan.num_items, plan.rest.num_items)
    return "lane-group (spmm_rowgroup32_kernel)"


class HipBackend(object):
    """Calls the gfx950 library through its C ABI on PyTorch's current HIP stream."""

    name = "hip"

    def _check_dev(self, *tensors):
        dev = None
        for t in tensors:
            if t is None:
                continue
            if not t.is_cuda:
                raise DGLError("expected a HIP device tensor, got device %s" % t.device)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise DGLError("tensors on different devices: %s vs %s" % (dev, t.device))
        return dev

    def coo_to_csr(self, num_rows, num_cols, row, col):
        dev = self._check_dev(row, col)
        L = _lib.lib()
        nnz = row.shape[0]
        bits = 32 if row.dtype == torch.int32 else 64
        indptr = torch.empty(num_rows + 1, dtype=row.dtype, device=dev)
        indices = torch.empty(nnz, dtype=row.dtype, device=dev)
        eids = torch.empty(nnz, dtype=row.dtype, device=dev)
        with torch.cuda.device(dev):
            ws_bytes = L.mgx_coo_to_csr_workspace(num_rows, nnz, bits)
            if ws_bytes < 0:
                _lib.check(3)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            _lib.check(L.mgx_coo_to_csr(num_rows, nnz, _ptr(row), _ptr(col), bits, _ptr(indptr), _ptr(indices),
                                        _ptr(eids), _ptr(ws), ws_bytes, _stream(dev)))
        return CsrView(num_rows, num_cols, indptr, indices, eids)

    def csr_transpose(self, csr):
        dev = self._check_dev(csr.indptr, csr.indices, csr.eids)
        L = _lib.lib()
        dt = csr.indptr.dtype
        indptr = torch.empty(csr.num_cols + 1, dtype=dt, device=dev)
        indices = torch.empty(csr.nnz, dtype=dt, device=dev)
        eids = torch.empty(csr.nnz, dtype=dt, device=dev)
        with torch.cuda.device(dev):
            ws_bytes = L.mgx_csr_transpose_workspace(csr.num_cols, csr.nnz, csr.idx_bits)
            if ws_bytes < 0:
                _lib.check(3)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            _lib.check(L.mgx_csr_transpose(ctypes.byref(csr.c_struct()), _ptr(indptr), _ptr(indices), _ptr(eids), _ptr(ws), ws_bytes,
                                           _stream(dev)))
        return CsrView(csr.num_cols, csr.num_rows, indptr, indices, eids)

    def degrees(self, csr):
        dev = csr.device
        deg = torch.empty(csr.num_rows, dtype=csr.indptr.dtype, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_csr_degrees(csr.num_rows, _ptr(csr.indptr), csr.idx_bits, _ptr(deg), _stream(dev)))
        return deg

    def inv_degrees(self, csr):
        dev = csr.device
        inv = torch.empty(csr.num_rows, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_csr_inv_degrees(csr.num_rows, _ptr(csr.indptr), csr.idx_bits, _ptr(inv), _stream(dev)))
        return inv

    def spmm(self, csr, op, reduce, U, E, u_len, e_len, out_len, u_off, e_off, src_scale, dst_scale, want_arg,
             accumulate_into=None):
        dev = self._check_dev(csr.indptr, U, E, src_scale, dst_scale, accumulate_into)
        if accumulate_into is not None:
            # the C ABI takes a dense [num_rows, out_len] output: a strided view (e.g. gspmm_raw's line-padded wide result)
            # would be written at the wrong offsets -- refuse it loudly (column blocks go through spmm_copy_u_strided)
            if not accumulate_into.is_contiguous() or accumulate_into.numel() != csr.num_rows * out_len:
                raise DGLError("gspmm: accumulate_into must be a contiguous tensor of %d x %d elements (got shape %s, strides %s)"
                               % (csr.num_rows, out_len, tuple(accumulate_into.shape), tuple(accumulate_into.stride())))
            out = accumulate_into.view(csr.num_rows, out_len)
        else:
            out = torch.empty((csr.num_rows, out_len), dtype=torch.float32, device=dev)
        arg_u = arg_e = None
        if want_arg:
            if op != "copy_rhs":
                arg_u = torch.empty((csr.num_rows, out_len), dtype=csr.indptr.dtype, device=dev)
            if op != "copy_lhs":
                arg_e = torch.empty((csr.num_rows, out_len), dtype=csr.indptr.dtype, device=dev)
        if (op == "copy_lhs" and reduce in ("sum", "mean") and src_scale is None and u_off is None and e_off is None
                and u_len == out_len and out_len >= config.TILE_MIN_WIDTH and out_len % 4 == 0 and csr.idx_bits == 32
                and csr.num_cols * out_len * 4 < 2 ** 32 and U.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and not want_arg):
            tp = csr.tile_plan(out_len)
            if tp is not None:  # dense neighbourhoods: the LDS-staged tile kernel
                self.spmm_tile_copy_u(csr, tp, reduce, U.view(csr.num_cols, out_len), out, accumulate_into is not None, dst_scale)
                return out, None, None
        if (op == "copy_lhs" and reduce in ("sum", "mean") and src_scale is None and u_off is None and e_off is None
                and u_len == out_len and out_len % 4 != 0 and config.TILE_MIN_WIDTH <= 4 and csr.idx_bits == 32 and not want_arg
                and csr.num_cols * (out_len + 3) * 4 < 2 ** 32):
            padded = (out_len + 3) // 4 * 4
            tp = csr.tile_plan(padded)
            if tp is not None:  # odd widths (1, 2, 41 ...) on dense neighbourhoods: through zero-padded copies of both operands
                up = torch.zeros((csr.num_cols, padded), dtype=torch.float32, device=dev)
                up[:, :out_len] = U.view(csr.num_cols, out_len)
                res = self.spmm_tile_copy_u(csr, tp, reduce, up, None, False, dst_scale)[:, :out_len]
                if accumulate_into is not None:
                    out += res
                else:
                    out.copy_(res)
                return out, None, None
        # MGX_SPMM_SHORT_ROWS: full-width copy_u / copy_e sums over short, even work items take the lane-group-per-item kernel
        plan, short = None, False
        if reduce in ("sum", "mean"):
            if (src_scale is None and u_off is None and e_off is None
                    and ((op == "copy_lhs" and u_len == out_len) or (op == "copy_rhs" and e_len == out_len))):
                plan, short = csr.spmm_plan_for(out_len)
            else:
                plan = csr.plan()
        partial = None
        if plan is not None and plan.total_slots:
            partial = torch.empty((plan.total_slots, out_len), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:  # bench.py: HIP events on the launch stream around this launch
                rec = {"op": op, "reduce": reduce, "out_len": out_len, "n_rows": csr.num_rows, "n_cols": csr.num_cols,
                       "nnz": csr.nnz, "accumulate": accumulate_into is not None, "start": torch.cuda.Event(enable_timing=True),
                       "end": torch.cuda.Event(enable_timing=True)}
                if short:
                    rec["variant"] = _short_variant(plan)
                rec["start"].record(torch.cuda.current_stream(dev))
            _lib.check(_lib.lib().mgx_spmm_csr(
                ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()),
                OP[op], REDUCE[reduce], _ptr(U), _ptr(E), u_len, e_len, out_len,
                _ptr(u_off), _ptr(e_off), _ptr(src_scale), _ptr(dst_scale), _ptr(out), _ptr(arg_u), _ptr(arg_e),
                _ptr(partial), (1 if accumulate_into is not None else 0) | (2 if short else 0), _stream(dev)))
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out, arg_u, arg_e

    def row_nonzero_bits(self, x2d):
        """Bitmap of the rows of x2d [n, D] that hold a non-zero (uint32 words, n padded to 64 rows)."""
        dev = self._check_dev(x2d)
        n, D = x2d.shape
        bits = torch.empty(2 * ((n + 63) // 64), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_row_nonzero_bits(n, D, _ptr(x2d), _ptr(bits), _stream(dev)))
        return bits

    def spmm_copy_u_masked(self, csr, reduce, U2d, bits, dst_scale=None, accumulate_into=None):
        """copy_u / sum|mean that skips source rows whose bit is clear (exact when those rows are zero)."""
        dev = self._check_dev(csr.indptr, U2d, bits, dst_scale, accumulate_into)
        D = int(U2d.shape[1])
        if accumulate_into is not None and (not accumulate_into.is_contiguous() or accumulate_into.numel() != csr.num_rows * D):
            raise DGLError("spmm_copy_u_masked: accumulate_into must be a contiguous tensor of %d x %d elements" % (csr.num_rows, D))
        out = accumulate_into.view(csr.num_rows, D) if accumulate_into is not None else \
            torch.empty((csr.num_rows, D), dtype=torch.float32, device=dev)
        plan = csr.plan()
        partial = torch.empty((plan.num_slots, D), dtype=torch.float32, device=dev) if plan is not None and plan.num_slots else None
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:
                rec = {"op": "copy_lhs", "reduce": reduce, "out_len": D, "n_rows": csr.num_rows, "n_cols": csr.num_cols,
                       "nnz": csr.nnz, "variant": "row-sparse", "start": torch.cuda.Event(enable_timing=True),
                       "end": torch.cuda.Event(enable_timing=True)}
                rec["start"].record(torch.cuda.current_stream(dev))
            _lib.check(_lib.lib().mgx_spmm_copy_u_masked(
                ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), REDUCE[reduce], _ptr(U2d), D,
                _ptr(bits), _ptr(dst_scale), _ptr(out), _ptr(partial), 1 if accumulate_into is not None else 0, _stream(dev)))
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out

    def edge_tail_of(self, csr, x2d):
        """(block_a [n, 96] compact, 128-byte aligned; edge_tail [nnz, 4] = x2d[csr.indices, 96:100]) of a CONSTANT x2d [n, 100]: the operands
        of spmm_copy_u_edge_tail, laid out once per (CSR, matrix).  None when mgx_spmm_copy_u_edge_tail would not take them."""
        plan, short = csr.spmm_plan_for(100)
        if (x2d.dim() != 2 or x2d.shape != (csr.num_cols, 100) or x2d.dtype != torch.float32 or x2d.stride(1) != 1 or csr.idx_bits != 32
                or short or (plan is not None and plan.rest is not None) or csr.num_cols * 384 >= 2 ** 32 or csr.tile_plan(100) is not None):
            return None
        dev = self._check_dev(csr.indptr, x2d)
        block_a = torch.empty((csr.num_cols, 96), dtype=torch.float32, device=dev)   # (the allocator aligns to 512 bytes)
        block_a.copy_(x2d[:, :96])
        tail = torch.empty((csr.nnz, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_edge_tail_fill(ctypes.byref(csr.c_struct()), _ptr(x2d), int(x2d.stride(0)), _ptr(tail), _stream(dev)))
        return block_a, tail

    def spmm_copy_u_edge_tail(self, csr, reduce, block_a, tail, out2d, accumulate=False, dst_scale=None):
        """copy_u / sum|mean of the constant [num_cols, 100] matrix held as edge_tail_of() into out2d [num_rows, 100] (row-strided view allowed)."""
        dev = self._check_dev(csr.indptr, block_a, tail, out2d, dst_scale)
        if (block_a.shape != (csr.num_cols, 96) or tail.shape != (csr.nnz, 4) or not block_a.is_contiguous() or not tail.is_contiguous()
                or out2d.shape != (csr.num_rows, 100) or out2d.stride(1) != 1):
            raise DGLError("spmm_copy_u_edge_tail: operands of edge_tail_of() and a [num_rows, 100] output expected")
        plan, _ = csr.spmm_plan_for(100)
        partial = torch.empty((plan.total_slots, 100), dtype=torch.float32, device=dev) if plan is not None and plan.total_slots else None
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:
                rec = {"op": "copy_lhs", "reduce": reduce, "out_len": 100, "n_rows": csr.num_rows, "n_cols": csr.num_cols, "nnz": csr.nnz,
                       "accumulate": bool(accumulate), "variant": "row+edge tail", "strides": (96, int(out2d.stride(0))),
                       "start": torch.cuda.Event(enable_timing=True), "end": torch.cuda.Event(enable_timing=True)}
                rec["start"].record(torch.cuda.current_stream(dev))
            _lib.check(_lib.lib().mgx_spmm_copy_u_edge_tail(ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()),
                                                            REDUCE[reduce], _ptr(block_a), _ptr(tail), _ptr(dst_scale), _ptr(out2d),
                                                            int(out2d.stride(0)), _ptr(partial), 1 if accumulate else 0, _stream(dev)))
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out2d

    def rows_slots_supported(self, x2d, csr=None):
        """Can x2d [n, 64] travel as 128-byte slots (mgx_rows_slots_pack) into the g-SpMM over `csr` (mgx_spmm_copy_u_slots)?"""
        return (x2d.dim() == 2 and x2d.shape[1] == 64 and x2d.dtype == torch.float32 and x2d.stride(1) == 1 and x2d.stride(0) % 4 == 0
                and x2d.data_ptr() % 16 == 0 and x2d.shape[0] < (1 << 25) and x2d.shape[0] * int(x2d.stride(0)) * 4 < 2 ** 32
                and (csr is None or (csr.idx_bits == 32 and csr.num_cols == x2d.shape[0] and csr.tile_plan(64) is None)))

    def rows_slots_pack(self, x2d, overflow=None, row_scale=None):
        """(slots [n, 32] int32 = one 128-byte slot per row of x2d [n, 64] (times row_scale[r] when given), overflow int64[1] on the device
        += rows with more than 24 non-zeros, which the consumer reads from x2d itself): include/mi355x_graph.h, mgx_rows_slots_pack."""
        dev = self._check_dev(x2d, overflow, row_scale)
        n = int(x2d.shape[0])
        slots = torch.empty((n, 32), dtype=torch.int32, device=dev)
        if overflow is None:
            overflow = torch.zeros(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_slots_pack(n, int(x2d.shape[1]), _ptr(x2d), int(x2d.stride(0)), _ptr(row_scale), _ptr(slots),
                                                      _ptr(overflow), _stream(dev)))
        return slots, overflow

    def spmm_copy_u_strided(self, csr, reduce, U2d, out2d, accumulate=False, dst_scale=None, slots=None, src_scale=None):
        """copy_u / sum|mean reading rows of U2d [num_cols, D] and writing rows of out2d [num_rows, D] IN PLACE, both row-strided
        views (stride(1) == 1) -- column blocks of wider matrices (mgx_spmm_copy_u_strided).  `slots` = rows_slots_pack(U2d)[0]: the
        work items gather the 128-byte slots instead of the 256-byte rows (mgx_spmm_copy_u_slots); `src_scale` (with slots only): the
        row factors the slots were packed with -- out = sum_u src_scale[u] * U2d[u]."""
        dev = self._check_dev(csr.indptr, U2d, out2d, dst_scale, src_scale)
        if src_scale is not None and slots is None:
            raise DGLError("spmm_copy_u_strided: src_scale comes with slots packed with the same factors")
        D = int(U2d.shape[1])
        if (U2d.dim() != 2 or out2d.dim() != 2 or U2d.stride(1) != 1 or out2d.stride(1) != 1 or out2d.shape[1] != D
                or U2d.shape[0] != csr.num_cols or out2d.shape[0] != csr.num_rows):
            raise DGLError("spmm_copy_u_strided: expected row-strided [num_cols, D] -> [num_rows, D] views")
        if (D >= config.TILE_MIN_WIDTH and D % 4 == 0 and csr.idx_bits == 32 and csr.num_cols * int(U2d.stride(0)) * 4 < 2 ** 32
                and U2d.stride(0) % 4 == 0 and out2d.stride(0) % 4 == 0 and U2d.data_ptr() % 16 == 0 and out2d.data_ptr() % 16 == 0):
            tp = csr.tile_plan(D)
            if tp is not None:
                return self.spmm_tile_copy_u(csr, tp, reduce, U2d, out2d, accumulate, dst_scale)
        plan, short = csr.spmm_plan_for(D)
        partial = torch.empty((plan.total_slots, D), dtype=torch.float32, device=dev) if plan is not None and plan.total_slots else None
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:
                rec = {"op": "copy_lhs", "reduce": reduce, "out_len": D, "n_rows": csr.num_rows, "n_cols": csr.num_cols,
                       "nnz": csr.nnz, "accumulate": bool(accumulate), "strides": (int(U2d.stride(0)), int(out2d.stride(0))),
                       "start": torch.cuda.Event(enable_timing=True), "end": torch.cuda.Event(enable_timing=True)}
                if short:
                    rec["variant"] = _short_variant(plan)
                rec["start"].record(torch.cuda.current_stream(dev))
            if slots is not None:
                if slots.shape != (U2d.shape[0], 32) or slots.dtype != torch.int32 or not slots.is_contiguous():
                    raise DGLError("spmm_copy_u_strided: slots must be the [num_cols, 32] int32 result of rows_slots_pack")
                if rec is not None:
                    rec["variant"] = (rec.get("variant", "") + "+slots").lstrip("+")
                _lib.check(_lib.lib().mgx_spmm_copy_u_slots(
                    ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), REDUCE[reduce], _ptr(U2d), D,
                    int(U2d.stride(0)), _ptr(slots), _ptr(src_scale), _ptr(dst_scale), _ptr(out2d), int(out2d.stride(0)), _ptr(partial),
                    (1 if accumulate else 0) | (2 if short else 0), _stream(dev)))
            else:
                _lib.check(_lib.lib().mgx_spmm_copy_u_strided(
                    ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), REDUCE[reduce], _ptr(U2d), D,
                    int(U2d.stride(0)), _ptr(dst_scale), _ptr(out2d), int(out2d.stride(0)), _ptr(partial),
                    (1 if accumulate else 0) | (2 if short else 0), _stream(dev)))
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out2d

    def spmm_copy_u_strided_init(self, csr, reduce, U2d, init2d, init_pos, out2d, dst_scale=None):
        """out2d[v] = (init2d[init_pos[v]] where init_pos[v] >= 0, else +0.0) + sum_u U2d[u]: spmm_copy_u_strided(accumulate=True) into
        `zeros.index_copy_(0, rows, init2d)` bit for bit, without the zero matrix -- out2d is write-only and every row of it is written
        (mgx_spmm_copy_u_strided_init).  init_pos: int64 [num_rows], -1 or a row of init2d (ops._row_pos).  Returns out2d, or None when
        the library has no kernel for these operands (mean, a dst_scale, D % 4, an int64 graph, a CSR on the tile kernel): the caller
        keeps the zero matrix and the accumulating call."""
        dev = self._check_dev(csr.indptr, U2d, init2d, init_pos, out2d, dst_scale)
        D = int(U2d.shape[1])
        if (U2d.dim() != 2 or out2d.dim() != 2 or init2d.dim() != 2 or U2d.stride(1) != 1 or out2d.stride(1) != 1 or out2d.shape[1] != D
                or init2d.shape[1] != D or (init2d.stride(1) != 1 and init2d.shape[0] > 0) or U2d.shape[0] != csr.num_cols
                or out2d.shape[0] != csr.num_rows or init_pos.dtype != torch.int64 or init_pos.shape != (csr.num_rows,)
                or not init_pos.is_contiguous()):
            raise DGLError("spmm_copy_u_strided_init: expected row-strided [num_cols, D] -> [num_rows, D] views, a row-strided [R, D] "
                           "initial matrix and an int64 [num_rows] position map")
        if D >= config.TILE_MIN_WIDTH and D % 4 == 0 and csr.idx_bits == 32 and csr.tile_plan(D) is not None:  # (the tile kernel has no such operand)
            return None
        plan, short = csr.spmm_plan_for(D)
        partial = torch.empty((plan.total_slots, D), dtype=torch.float32, device=dev) if plan is not None and plan.total_slots else None
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:
                rec = {"op": "copy_lhs", "reduce": reduce, "out_len": D, "n_rows": csr.num_rows, "n_cols": csr.num_cols,
                       "nnz": csr.nnz, "accumulate": True, "strides": (int(U2d.stride(0)), int(out2d.stride(0))),
                       "start": torch.cuda.Event(enable_timing=True), "end": torch.cuda.Event(enable_timing=True)}
                if short:
                    rec["variant"] = _short_variant(plan)
                rec["start"].record(torch.cuda.current_stream(dev))
            st = _lib.lib().mgx_spmm_copy_u_strided_init(
                ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), REDUCE[reduce], _ptr(U2d), D,
                int(U2d.stride(0)), _ptr(dst_scale), _ptr(init2d) if init2d.shape[0] else None, int(init2d.shape[0]),
                max(int(init2d.stride(0)), D) if init2d.shape[0] else D, _ptr(init_pos), _ptr(out2d), int(out2d.stride(0)), _ptr(partial), 2 if short else 0, _stream(dev))
            if st == _lib.ERR_UNSUPPORTED:
                return None
            _lib.check(st)
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out2d

    def rows_slots_pack_rows(self, x2d, rows, slots):
        """slots[rows[i]] = the 128-byte slot of row rows[i] of x2d [n, 64], for the listed rows only (int64, distinct): byte for byte what
        rows_slots_pack writes for them; every other slot stays as it is (mgx_rows_slots_pack_rows).  Returns slots."""
        dev = self._check_dev(x2d, rows, slots)
        n = int(x2d.shape[0])
        if (x2d.dim() != 2 or x2d.stride(1) != 1 or rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous()
                or slots.shape != (n, 32) or slots.dtype != torch.int32 or not slots.is_contiguous()):
            raise DGLError("rows_slots_pack_rows: expected a row-strided [n, 64] matrix, an int64 row list and the [n, 32] int32 slots of rows_slots_pack")
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_slots_pack_rows(n, int(x2d.shape[1]), _ptr(x2d), int(x2d.stride(0)), _ptr(rows), int(rows.shape[0]),
                                                           _ptr(slots), _stream(dev)))
        return slots

    def spmm_copy_u_slots_init(self, csr, reduce, U2d, slots, init2d, init_pos, out2d, dst_scale=None):
        """spmm_copy_u_strided_init with `slots` = rows_slots_pack(U2d)[0] beside U2d: the wave-per-item work items probe the first word of
        every source row's slot (one line per edge) and gather the dense row only where the slot is not empty -- for a U2d most of whose
        rows are zero (mgx_spmm_copy_u_slots_init).  The bits of spmm_copy_u_strided_init wherever no element of U2d / init2d is -0.0.  Returns out2d,
        or None when the library has no kernel for these operands (what spmm_copy_u_strided_init declines, and D != 64)."""
        dev = self._check_dev(csr.indptr, U2d, slots, init2d, init_pos, out2d, dst_scale)
        D = int(U2d.shape[1])
        if (U2d.dim() != 2 or out2d.dim() != 2 or init2d.dim() != 2 or U2d.stride(1) != 1 or out2d.stride(1) != 1 or out2d.shape[1] != D
                or init2d.shape[1] != D or (init2d.stride(1) != 1 and init2d.shape[0] > 0) or U2d.shape[0] != csr.num_cols
                or out2d.shape[0] != csr.num_rows or init_pos.dtype != torch.int64 or init_pos.shape != (csr.num_rows,)
                or not init_pos.is_contiguous()):
            raise DGLError("spmm_copy_u_slots_init: expected row-strided [num_cols, D] -> [num_rows, D] views, a row-strided [R, D] "
                           "initial matrix and an int64 [num_rows] position map")
        if slots.shape != (U2d.shape[0], 32) or slots.dtype != torch.int32 or not slots.is_contiguous():
            raise DGLError("spmm_copy_u_slots_init: slots must be the [num_cols, 32] int32 result of rows_slots_pack")
        if D >= config.TILE_MIN_WIDTH and D % 4 == 0 and csr.idx_bits == 32 and csr.tile_plan(D) is not None:  # (the tile kernel has no such operand)
            return None
        plan, short = csr.spmm_plan_for(D)
        partial = torch.empty((plan.total_slots, D), dtype=torch.float32, device=dev) if plan is not None and plan.total_slots else None
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:
                rec = {"op": "copy_lhs", "reduce": reduce, "out_len": D, "n_rows": csr.num_rows, "n_cols": csr.num_cols,
                       "nnz": csr.nnz, "accumulate": True, "strides": (int(U2d.stride(0)), int(out2d.stride(0))),
                       "start": torch.cuda.Event(enable_timing=True), "end": torch.cuda.Event(enable_timing=True)}
                if short:
                    rec["variant"] = _short_variant(plan)
                rec["variant"] = (rec.get("variant", "") + "+slots").lstrip("+")
                rec["start"].record(torch.cuda.current_stream(dev))
            st = _lib.lib().mgx_spmm_copy_u_slots_init(
                ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), REDUCE[reduce], _ptr(U2d), D,
                int(U2d.stride(0)), _ptr(slots), _ptr(dst_scale), _ptr(init2d) if init2d.shape[0] else None, int(init2d.shape[0]),
                max(int(init2d.stride(0)), D) if init2d.shape[0] else D, _ptr(init_pos), _ptr(out2d), int(out2d.stride(0)), _ptr(partial),
                2 if short else 0, _stream(dev))
            if st == _lib.ERR_UNSUPPORTED:
                return None
            _lib.check(st)
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out2d

    def spmm_tile_copy_u(self, csr, tile_plan, reduce, U2d, out2d=None, accumulate=False, dst_scale=None):
        """copy_u / sum|mean through the LDS-staged tile kernel (mgx_spmm_tile_copy_u); U2d / out2d may be row-strided views."""
        dev = self._check_dev(csr.indptr, U2d, out2d, dst_scale)
        D = int(U2d.shape[1])
        if out2d is None:
            out2d = torch.empty((csr.num_rows, D), dtype=torch.float32, device=dev)
        if (U2d.dim() != 2 or out2d.dim() != 2 or U2d.stride(1) != 1 or out2d.stride(1) != 1 or out2d.shape[1] != D
                or U2d.shape[0] != csr.num_cols or out2d.shape[0] != csr.num_rows):
            raise DGLError("spmm_tile_copy_u: expected row-strided [num_cols, D] -> [num_rows, D] views")
        base = tile_plan.base
        partial = torch.empty((base.num_slots, D), dtype=torch.float32, device=dev) if base is not None and base.num_slots else None
        with torch.cuda.device(dev):
            rec = None
            if PROFILE is not None:
                rec = {"op": "copy_lhs", "reduce": reduce, "out_len": D, "n_rows": csr.num_rows, "n_cols": csr.num_cols,
                       "nnz": csr.nnz, "accumulate": bool(accumulate), "variant": "tile",
                       "start": torch.cuda.Event(enable_timing=True), "end": torch.cuda.Event(enable_timing=True)}
                rec["start"].record(torch.cuda.current_stream(dev))
            _lib.check(_lib.lib().mgx_spmm_tile_copy_u(
                ctypes.byref(csr.c_struct()), None if base is None else ctypes.byref(base.c_struct()), ctypes.byref(tile_plan.c_struct()),
                REDUCE[reduce], _ptr(U2d), D, int(U2d.stride(0)), _ptr(dst_scale), _ptr(out2d), int(out2d.stride(0)), _ptr(partial),
                1 if accumulate else 0, _stream(dev)))
            if rec is not None:
                rec["end"].record(torch.cuda.current_stream(dev))
                PROFILE.append(rec)
        return out2d

    @staticmethod
    def spmm_rel_supported(csr, x2d, R):
        """True when mgx_spmm_rel / mgx_spmm_rel_grad have a kernel for a [num_cols, D] operand and R relations over this CSR."""
        D = int(x2d.shape[1]) if x2d.dim() == 2 else 0
        return (x2d.dim() == 2 and x2d.is_cuda and x2d.dtype == torch.float32 and 1 <= R <= 16 and 1 <= D <= 128 and D & (D - 1) == 0
                and x2d.stride(1) == 1 and x2d.stride(0) >= D and x2d.stride(0) % min(D, 4) == 0 and x2d.data_ptr() % (4 * min(D, 4)) == 0
                and csr.indptr.is_cuda and csr.nnz > 0)

    def spmm_rel(self, csr, reduce, w_pos, x2d, src_scale=None, dst_scale=None):
        """out[v, r, :] = dst_scale[v] * sum|mean_{p in row v} w_pos[p, r] * src_scale[u_p] * x2d[u_p, :] (mgx_spmm_rel); w_pos: [nnz, R] in
        the CSR's position order; x2d may be a row-strided view.  Returns [num_rows, R, D]."""
        dev = self._check_dev(csr.indptr, w_pos, x2d, src_scale, dst_scale)
        R, D = int(w_pos.shape[1]), int(x2d.shape[1])
        if w_pos.shape[0] != csr.nnz or x2d.shape[0] != csr.num_cols or not w_pos.is_contiguous() or x2d.stride(1) != 1:
            raise DGLError("spmm_rel: expected contiguous [nnz, R] weights and a row-strided [num_cols, D] operand")
        out = torch.empty((csr.num_rows, R, D), dtype=torch.float32, device=dev)
        plan = csr.plan()
        partial = None
        if plan is not None and plan.num_slots:
            partial = torch.empty((plan.num_slots, R * D), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="spmm_rel", reduce=reduce, R=R, out_len=D, nnz=csr.nnz):
            _lib.check(_lib.lib().mgx_spmm_rel(
                ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), REDUCE[reduce], R, D, _ptr(w_pos),
                _ptr(x2d), int(x2d.stride(0)), _ptr(src_scale), _ptr(dst_scale), _ptr(out), _ptr(partial), _stream(dev)))
        return out

    def spmm_rel_grad(self, csr_t, w_pos_t, dz3d, dst_scale=None, src_scale=None):
        """dx[u, :] = src_scale[u] * sum_{p in row u} sum_r w_pos_t[p, r] * dst_scale[v_p] * dz3d[v_p, r, :] (mgx_spmm_rel_grad) over the
        TRANSPOSED CSR (rows = source nodes) with the weights in its position order; dz3d: [num_cols, R, D] in any layout (dense16)."""
        dev = self._check_dev(csr_t.indptr, w_pos_t, dz3d, src_scale, dst_scale)
        R, D = int(dz3d.shape[1]), int(dz3d.shape[2])
        if w_pos_t.shape[0] != csr_t.nnz or int(w_pos_t.shape[1]) != R or dz3d.shape[0] != csr_t.num_cols or not w_pos_t.is_contiguous():
            raise DGLError("spmm_rel_grad: expected contiguous [nnz, R] weights and a [num_cols, R, D] gradient")
        dz3d = dense16(dz3d)
        dx = torch.empty((csr_t.num_rows, D), dtype=torch.float32, device=dev)
        plan = csr_t.plan()
        partial = None
        if plan is not None and plan.num_slots:
            partial = torch.empty((plan.num_slots, D), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="spmm_rel_grad", R=R, out_len=D, nnz=csr_t.nnz):
            _lib.check(_lib.lib().mgx_spmm_rel_grad(
                ctypes.byref(csr_t.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()), R, D, _ptr(w_pos_t), _ptr(dz3d),
                _ptr(dst_scale), _ptr(src_scale), _ptr(dx), _ptr(partial), _stream(dev)))
        return dx

    def sddmm(self, graph_index, op, L, R, lhs_target, rhs_target, l_len, r_len, out_len, reduce_size, l_off, r_off):
        """graph_index supplies either COO (edge-id order) or the in-CSR."""
        nnz = graph_index.num_edges()
        dev = self._check_dev(L, R)
        out = torch.empty((nnz, out_len), dtype=torch.float32, device=dev)
        lib = _lib.lib()
        if self._sddmm_in_csr_order(graph_index, op, L, R, lhs_target, rhs_target, l_len, r_len, out_len, l_off, r_off):
            # the edge list in the in-CSR's order (sorted by destination) with the edge id as the output row: sddmm_coo32_kernel<PERM>
            csc = graph_index.csc()
            with torch.cuda.device(dev), timed_call(dev, kernel="sddmm", op=op, out_len=out_len, l_len=l_len, r_len=r_len, nnz=nnz,
                                                    n_src=graph_index.num_src, n_dst=graph_index.num_dst, targets=lhs_target + rhs_target,
                                                    walk="csr order"):
                st = lib.mgx_sddmm_coo_perm(graph_index.num_src, graph_index.num_dst, nnz, _ptr(csc.indices), _ptr(csc.row_of_position()),
                                            _ptr(csc.eids), 32, OP[op], _ptr(L), _ptr(R), TARGET[lhs_target], TARGET[rhs_target], out_len,
                                            _ptr(out), _stream(dev))
            if st != _lib.ERR_UNSUPPORTED:
                _lib.check(st)
                return out
        with torch.cuda.device(dev), timed_call(dev, kernel="sddmm", op=op, out_len=out_len, l_len=l_len, r_len=r_len, nnz=nnz,
                                                n_src=graph_index.num_src, n_dst=graph_index.num_dst, targets=lhs_target + rhs_target):
            if graph_index.has_format("coo") or not graph_index.has_format("csc"):
                src, dst = graph_index.coo()
                self._check_dev(src, L, R)
                bits = 32 if src.dtype == torch.int32 else 64
                _lib.check(lib.mgx_sddmm_coo(
                    graph_index.num_src, graph_index.num_dst, nnz, _ptr(src), _ptr(dst), bits, OP[op], _ptr(L), _ptr(R),
                    TARGET[lhs_target], TARGET[rhs_target], l_len, r_len, out_len, reduce_size, _ptr(l_off), _ptr(r_off),
                    _ptr(out), _stream(dev)))
            else:
                csr = graph_index.csc()
                self._check_dev(csr.indptr, L, R)
                plan = csr.plan()
                _lib.check(lib.mgx_sddmm_csr(
                    ctypes.byref(csr.c_struct()), None if plan is None else ctypes.byref(plan.c_struct()),
                    OP[op], _ptr(L), _ptr(R), TARGET[lhs_target], TARGET[rhs_target],
                    l_len, r_len, out_len, reduce_size, _ptr(l_off), _ptr(r_off), _ptr(out), _stream(dev)))
        return out

    SDDMM_PERM_MIN_EDGES = 1 << 20
    SDDMM_PERM_MIN_WIDTH = 32  # measured (profiles/r05_sddmm_perm.txt): D = 64 / 128 gain 17 - 27 %, D = 16 loses 20 % (a 64-byte output row
                               # is half a line: scattering it costs more than the operand misses it saves)

    @staticmethod
    def _sddmm_in_csr_order(gidx, op, L, R, lt, rt, l_len, r_len, out_len, l_off, r_off):
        """Walk the in-CSR's order with the edge id as the output row (mgx_sddmm_coo_perm) instead of the edge list's own order?
        MGX_SDDMM_WALK = coo | csr | auto (default).  auto: a big graph that holds an in-CSR whose edge ids are NOT its positions, an
        element-wise op on u / v operands as wide as the output -- and an edge list that is not already sorted by an endpoint (checked
        once per graph; a sorted list has the same locality AND streams its output, profiles/r03_sddmm_edge_order.txt)."""
        mode = os.environ.get("MGX_SDDMM_WALK", "auto")
        if (mode == "coo" or not gidx.has_format("csc") or op == "dot" or l_off is not None or r_off is not None or out_len < 4
                or (L is not None and (lt not in "uv" or l_len != out_len)) or (R is not None and (rt not in "uv" or r_len != out_len))):
            return False
        csc = gidx.csc()
        if csc.eids is None or csc.idx_bits != 32 or not csc.indptr.is_cuda:
            return False
        if mode == "csr":
            return True
        if getattr(gidx, "ephemeral", False) or csc.nnz < HipBackend.SDDMM_PERM_MIN_EDGES or out_len < HipBackend.SDDMM_PERM_MIN_WIDTH:
            return False
        if not gidx.has_format("coo"):
            return True  # no edge list to walk: the lean kernel over the CSR's order replaces the generic CSR body
        order = getattr(gidx, "_coo_sorted", None)
        if order is None:
            src, dst = gidx.coo()
            order = bool(((dst[1:] >= dst[:-1]).all() | (src[1:] >= src[:-1]).all()).item()) if dst.numel() > 1 else True
            try:
                gidx._coo_sorted = order
            except AttributeError:
                pass
        return not order

    def edge_softmax_fwd(self, csr, z2d):
        dev = self._check_dev(csr.indptr, z2d)
        a = torch.empty_like(z2d)
        plan, ws = self._softmax_plan(csr, z2d.shape[1], dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_edge_softmax_fwd(ctypes.byref(csr.c_struct()), plan, z2d.shape[1], _ptr(z2d), _ptr(a),
                                                       _ptr(ws), _stream(dev)))
        return a

    def gat_attention_fwd(self, csr, el2d, er2d, slope):
        dev = self._check_dev(csr.indptr, el2d, er2d)
        H = el2d.shape[1]
        a = torch.empty((csr.nnz, H), dtype=torch.float32, device=dev)
        plan, ws = self._softmax_plan(csr, H, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_gat_attention_fwd(ctypes.byref(csr.c_struct()), plan, H, _ptr(el2d), _ptr(er2d),
                                                        ctypes.c_float(slope), _ptr(a), _ptr(ws), _stream(dev)))
        return a

    def gat_attention_bwd(self, csr, el2d, er2d, slope, a2d, da2d):
        dev = self._check_dev(csr.indptr, el2d, er2d, a2d, da2d)
        H = el2d.shape[1]
        de = torch.empty_like(a2d)
        plan, ws = self._softmax_plan(csr, H, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_gat_attention_bwd(ctypes.byref(csr.c_struct()), plan, H, _ptr(el2d), _ptr(er2d),
                                                        ctypes.c_float(slope), _ptr(a2d), _ptr(da2d), _ptr(de), _ptr(ws),
                                                        _stream(dev)))
        return de

    @staticmethod
    def gat_fused_supported(csr, H, F):
        """Shapes mgx_gat_fused_* takes: F a power of two >= 4 with H*F <= 256, or ONE head of any width 4 < F <= 256;
        32-bit indices and byte offsets."""
        regular = F >= 4 and F % 4 == 0 and ((F // 4) & (F // 4 - 1)) == 0 and H * F <= 256
        ragged = H == 1 and 4 < F <= 256
        return ((regular or ragged) and csr.idx_bits == 32
                and max(csr.num_cols, csr.num_rows) * H * max(F * 4, 16) < 2 ** 32 and csr.nnz < 2 ** 31)

    @staticmethod
    def _plan_ptr(plan):
        return None if plan is None else ctypes.byref(plan.c_struct())

    def _plan_ws(self, workspace_fn, plans, H, F, dev):
        """Hub-row workspace of an attention call (workspace_fn: mgx_gat_fused_workspace | mgx_dot_attention_workspace): the largest need."""
        need = max([workspace_fn(self._plan_ptr(p), H, F) for p in plans] + [0])
        return torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None

    @staticmethod
    def _gat_tile_plans(csc, csr, H, F, p):
        """(tile plan of the in-CSR, of the out-CSR | None) when a layer's walks run as tile kernels, else None.  With attn_drop the
        two forms key the mask differently (edge id / (destination, source, rank among parallel edges)), so a layer takes the tile
        form for ALL three walks or for none: it needs both plans with their rank streams."""
        if H != 1:
            return None
        t_dst = csc.gat_tile_plan(F)
        if t_dst is None:
            return None
        t_src = csr.gat_tile_plan(F) if csr is not None else None
        if p > 0.0 and (t_src is None or not t_dst.stats["pair_rank_streams"] or not t_src.stats["pair_rank_streams"]):
            return None
        return t_dst, t_src

    def gat_fused_fwd(self, csc, feat3d, el2d, er2d, slope, p, seed, attn_l=None, csr=None):
        """feat3d [n_src, H, F], el2d [n_src, H], er2d [n_dst, H] -> (out [n_dst, H, F], nstat [n_dst, H, 4], form).
        csr: the out-CSR, needed to choose the tile form when p > 0 (see _gat_tile_plans).  `form` ("tile" | "row") is the
        kernel family that ran: with p > 0 it fixes how the dropout mask is keyed, and the backward must be given it back."""
        dev = self._check_dev(csc.indptr, feat3d, el2d, er2d)
        H, F = int(feat3d.shape[1]), int(feat3d.shape[2])
        feat3d, el2d, er2d = dense16(feat3d), el2d.contiguous(), er2d.contiguous()  # (el / er: 4-byte accesses, any base)
        out = torch.empty((csc.num_rows, H, F), dtype=torch.float32, device=dev)
        nstat = torch.empty((csc.num_rows, H, 4), dtype=torch.float32, device=dev)
        tiles = self._gat_tile_plans(csc, csr, H, F, p)
        if tiles is not None:  # dense neighbourhoods, one narrow head: the LDS-staged tile walk
            tp = tiles[0]
            ws = self._plan_ws(_lib.lib().mgx_gat_fused_workspace, [tp.base], H, F, dev)
            pack = self._gat_pack_ws(csc, H, F, dev)
            with torch.cuda.device(dev), timed_call(dev, kernel="gat_fwd", form="tile", H=H, F=F, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows):
                _lib.check(_lib.lib().mgx_gat_tile_fwd(ctypes.byref(csc.c_struct()), self._plan_ptr(tp.base), ctypes.byref(tp.c_struct()),
                                                       H, F, _ptr(feat3d), _ptr(el2d), _ptr(er2d), ctypes.c_float(slope), ctypes.c_float(p),
                                                       ctypes.c_uint64(seed), _ptr(out), _ptr(nstat), _ptr(ws), _ptr(pack), _stream(dev)))
            return out, nstat, "tile"
        plan = csc.plan()
        ws = self._plan_ws(_lib.lib().mgx_gat_fused_workspace, [plan], H, F, dev)
        pack = self._gat_pack_ws(csc, H, F, dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="gat_fwd", form="row", H=H, F=F, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows):
            _lib.check(_lib.lib().mgx_gat_fused_fwd(ctypes.byref(csc.c_struct()), self._plan_ptr(plan), H, F, _ptr(feat3d), _ptr(el2d),
                                                    _ptr(attn_l), _ptr(er2d), ctypes.c_float(slope), ctypes.c_float(p), ctypes.c_uint64(seed),
                                                    _ptr(out), _ptr(nstat), _ptr(ws), _ptr(pack), _stream(dev)))
        return out, nstat, "row"

    @staticmethod
    def _gat_pack_ws(csc, H, F, dev):
        if not config.GAT_PACK:
            return None
        need = _lib.lib().mgx_gat_fused_pack_workspace(csc.num_cols, csc.num_rows, H, F)
        return torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None

    def gat_fused_bwd(self, csc, csr, feat3d, el2d, slope, p, seed, out3d, d_out3d, nstat, need_src, attn_l=None, form=None):
        """-> (d_feat | None, d_el | None, d_er); nstat[..., 3] is overwritten with <out, d_out> per head.
        `form`: what gat_fused_fwd returned.  With p > 0 the backward runs that same kernel family or raises -- the two families
        key the dropout mask differently (edge id / (destination, source, rank)), so re-deriving the choice here (an environment
        switch flipped, a plan that failed to build in between) would silently apply another mask."""
        dev = self._check_dev(csc.indptr, csr.indptr, feat3d, el2d, out3d, d_out3d, nstat)
        H, F = int(feat3d.shape[1]), int(feat3d.shape[2])
        feat3d, el2d, out3d, d_out3d = dense16(feat3d), el2d.contiguous(), dense16(out3d), dense16(d_out3d)
        d_er = torch.empty((csc.num_rows, H), dtype=torch.float32, device=dev)
        d_feat = torch.empty_like(feat3d) if need_src else None
        d_el = torch.empty((csc.num_cols, H), dtype=torch.float32, device=dev) if need_src else None
        tiles = self._gat_tile_plans(csc, csr, H, F, p)
        if p > 0.0 and form == "row":
            tiles = None
        elif p > 0.0 and form == "tile" and (tiles is None or tiles[1] is None):
            raise DGLError("gat_fused backward: the forward pass drew its dropout mask with the tile kernels, but their plans are not "
                           "available any more (MGX_GAT_TILE / MGX_TILE changed between forward and backward?)")
        if tiles is not None and tiles[1] is not None:
            t_dst, t_src = tiles
            if not need_src:  # the kernel's source walk is skipped when both are NULL
                d_feat = d_el = None
            ws = self._plan_ws(_lib.lib().mgx_gat_fused_workspace, [t_dst.base, t_src.base], H, F, dev)
            pack = self._gat_pack_ws(csc, H, F, dev)
            with torch.cuda.device(dev), timed_call(dev, kernel="gat_bwd", form="tile", H=H, F=F, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows,
                                                    source_walk=bool(need_src)):
                _lib.check(_lib.lib().mgx_gat_tile_bwd(ctypes.byref(csc.c_struct()), self._plan_ptr(t_dst.base), ctypes.byref(t_dst.c_struct()),
                                                       ctypes.byref(csr.c_struct()), self._plan_ptr(t_src.base), ctypes.byref(t_src.c_struct()),
                                                       H, F, _ptr(feat3d), _ptr(el2d), ctypes.c_float(slope), ctypes.c_float(p),
                                                       ctypes.c_uint64(seed), _ptr(out3d), _ptr(d_out3d), _ptr(nstat), _ptr(d_feat),
                                                       _ptr(d_el), _ptr(d_er), _ptr(ws), _ptr(pack), _stream(dev)))
            return d_feat, d_el, d_er
        p_dst, p_src = csc.plan(), csr.plan()
        ws = self._plan_ws(_lib.lib().mgx_gat_fused_workspace, [p_dst, p_src], H, F, dev)
        pack = self._gat_pack_ws(csc, H, F, dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="gat_bwd", form="row", H=H, F=F, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows,
                                                source_walk=bool(need_src)):
            _lib.check(_lib.lib().mgx_gat_fused_bwd(ctypes.byref(csc.c_struct()), self._plan_ptr(p_dst), ctypes.byref(csr.c_struct()),
                                                    self._plan_ptr(p_src), H, F, _ptr(feat3d), _ptr(el2d), _ptr(attn_l), ctypes.c_float(slope),
                                                    ctypes.c_float(p), ctypes.c_uint64(seed), _ptr(out3d), _ptr(d_out3d), _ptr(nstat),
                                                    _ptr(d_feat), _ptr(d_el), _ptr(d_er), _ptr(ws), _ptr(pack), _stream(dev)))
        return d_feat, d_el, d_er

    # ---- scaled dot-product attention (csrc/dotattn.hip)
    @staticmethod
    def dot_attention_supported(csr, H, F):
        """Shapes mgx_dot_attention_* takes: F in {4, 8, 16, 32, 64}, H*F <= 256, 32-bit indices, at least one edge, dense operands below
        4 GiB (32-bit byte offsets)."""
        return bool(_lib.lib().mgx_dot_attention_supported(ctypes.byref(csr.c_struct()), H, F))

    @staticmethod
    def _dot_operand(x3d):
        """(tensor, row stride in floats) of a [N, H, F] operand as the kernels take it: the H*F floats of a node contiguous, the row
        stride a multiple of 4 floats, the base 16-byte aligned, rows * stride below 4 GiB (a column block of a wider projection qualifies);
        else an aligned dense copy (rows16)."""
        return rows16(x3d, max_bytes=2 ** 32)  # 32-bit byte offsets: a dense copy fits

    def dot_attention_fwd(self, csc, q3d, k3d, v3d, scale):
        """q3d [n_dst, H, F], k3d / v3d [n_src, H, F] (row-strided views are taken as they are) -> (out [n_dst, H, F],
        stat [n_dst, H, 4] = (m, 1/s, -, -))."""
        dev = self._check_dev(csc.indptr, q3d, k3d, v3d)
        H, F = int(q3d.shape[1]), int(q3d.shape[2])
        same = k3d is v3d
        (q, q_ld), (k, k_ld) = self._dot_operand(q3d), self._dot_operand(k3d)
        v, v_ld = (k, k_ld) if same else self._dot_operand(v3d)
        out = torch.empty((csc.num_rows, H, F), dtype=torch.float32, device=dev)
        stat = torch.empty((csc.num_rows, H, 4), dtype=torch.float32, device=dev)
        plan = csc.plan()
        ws = self._plan_ws(_lib.lib().mgx_dot_attention_workspace, [plan], H, F, dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="dot_attn_fwd", H=H, F=F, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows):
            _lib.check(_lib.lib().mgx_dot_attention_fwd(ctypes.byref(csc.c_struct()), self._plan_ptr(plan), H, F, _ptr(q), q_ld, _ptr(k), k_ld,
                                                        _ptr(v), v_ld, ctypes.c_float(scale), _ptr(out), _ptr(stat), _ptr(ws), _stream(dev)))
        return out, stat

    def dot_attention_bwd(self, csc, csr, q3d, k3d, v3d, scale, out3d, d_out3d, stat, need_q, need_k, need_v):
        """-> (dq | None, dk | None, dv | None), each dense; stat[..., 2] is overwritten with <out, d_out> per head."""
        dev = self._check_dev(csc.indptr, csr.indptr, q3d, k3d, v3d, out3d, d_out3d, stat)
        H, F = int(q3d.shape[1]), int(q3d.shape[2])
        if not (need_q or need_k or need_v):
            return None, None, None
        same = k3d is v3d
        (q, q_ld), (k, k_ld) = self._dot_operand(q3d), self._dot_operand(k3d)
        v, v_ld = (k, k_ld) if same else self._dot_operand(v3d)
        out3d, d_out3d = dense16(out3d), dense16(d_out3d)
        dq = torch.empty((csc.num_rows, H, F), dtype=torch.float32, device=dev) if need_q else None
        dk = torch.empty((csc.num_cols, H, F), dtype=torch.float32, device=dev) if need_k else None
        dv = torch.empty((csc.num_cols, H, F), dtype=torch.float32, device=dev) if need_v else None
        p_dst, p_src = csc.plan(), csr.plan()
        ws = self._plan_ws(_lib.lib().mgx_dot_attention_workspace, [p_dst, p_src], H, F, dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="dot_attn_bwd", H=H, F=F, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows):
            _lib.check(_lib.lib().mgx_dot_attention_bwd(ctypes.byref(csc.c_struct()), self._plan_ptr(p_dst), ctypes.byref(csr.c_struct()),
                                                        self._plan_ptr(p_src), H, F, _ptr(q), q_ld, _ptr(k), k_ld, _ptr(v), v_ld,
                                                        ctypes.c_float(scale), _ptr(out3d), _ptr(d_out3d), _ptr(stat), _ptr(dq), _ptr(dk),
                                                        _ptr(dv), _ptr(ws), _stream(dev)))
        return dq, dk, dv

    # ---- sum of relu(x_u + w_e) messages (csrc/gine.hip)
    @staticmethod
    def gine_supported(csr, D):
        """Shapes mgx_gine_* takes: D % 4 == 0, 4 <= D <= 256, 32-bit indices, at least one edge, x / w / d_w below 4 GiB each."""
        return bool(_lib.lib().mgx_gine_supported(ctypes.byref(csr.c_struct()), D))

    def _gine_ws(self, plan, D, dev):
        need = _lib.lib().mgx_gine_workspace(self._plan_ptr(plan), D)
        return torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None

    def gine_fwd(self, csc, x2d, w2d, scale1d):
        """x2d [n_src, D], w2d [E, D] and scale1d [E] | None by edge id (any layout: what the kernels cannot read in place is copied,
        dense16) -> out [n_dst, D]."""
        dev = self._check_dev(csc.indptr, x2d, w2d, scale1d)
        x2d, w2d, scale1d = dense16(x2d), dense16(w2d), None if scale1d is None else scale1d.contiguous()
        D = int(x2d.shape[1])
        out = torch.empty((csc.num_rows, D), dtype=torch.float32, device=dev)
        plan = csc.plan()
        ws = self._gine_ws(plan, D, dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="gine_fwd", D=D, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows):
            _lib.check(_lib.lib().mgx_gine_fwd(ctypes.byref(csc.c_struct()), self._plan_ptr(plan), D, _ptr(x2d), _ptr(w2d), _ptr(scale1d),
                                               _ptr(out), _ptr(ws), _stream(dev)))
        return out

    def gine_bwd(self, csr, x2d, w2d, scale1d, d_out2d, need_x, need_w):
        """csr: the out-CSR (rows = sources); operands and the gradient d_out2d [n_dst, D] in any layout (dense16)
        -> (d_x [n_src, D] | None, d_w [E, D] by edge id | None)."""
        dev = self._check_dev(csr.indptr, x2d, w2d, scale1d, d_out2d)
        D = int(x2d.shape[1])
        if not (need_x or need_w):
            return None, None
        x2d, w2d, d_out2d = dense16(x2d), dense16(w2d), dense16(d_out2d)
        scale1d = None if scale1d is None else scale1d.contiguous()
        d_x = torch.empty((csr.num_rows, D), dtype=torch.float32, device=dev) if need_x else None
        d_w = torch.empty((csr.nnz, D), dtype=torch.float32, device=dev) if need_w else None
        plan = csr.plan()
        ws = self._gine_ws(plan, D, dev) if need_x else None
        with torch.cuda.device(dev), timed_call(dev, kernel="gine_bwd", D=D, nnz=csr.nnz, n_src=csr.num_rows, n_dst=csr.num_cols):
            _lib.check(_lib.lib().mgx_gine_bwd(ctypes.byref(csr.c_struct()), self._plan_ptr(plan), D, _ptr(x2d), _ptr(w2d), _ptr(scale1d),
                                               _ptr(d_out2d), _ptr(d_x), _ptr(d_w), _ptr(ws), _stream(dev)))
        return d_x, d_w

    # ---- sum / mean / var / std / max / min of the same messages in one walk (csrc/multiagg.hip)
    @staticmethod
    def multi_agg_supported(csr, D):
        """Shapes mgx_multi_agg_* takes: those of gine_supported."""
        return bool(_lib.lib().mgx_multi_agg_supported(ctypes.byref(csr.c_struct()), D))

    def _multi_agg_ws(self, plan, D, dev):
        need = _lib.lib().mgx_multi_agg_workspace(self._plan_ptr(plan), D)
        return torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None

    def multi_agg_fwd(self, csc, x2d, w2d, aggregators, eps):
        """x2d [n_src, D], w2d [E, D] by edge id | None (any layout: what the kernels cannot read in place is copied, dense16) ->
        (out [n_dst, A, D] in the order of `aggregators`, arg_max | None, arg_min | None (int32 [n_dst, D], edge ids),
        stats [n_dst, 2, D] = (mean, var) | None)."""
        dev = self._check_dev(csc.indptr, x2d, w2d)
        x2d, w2d = dense16(x2d), dense16(w2d)
        D, A = int(x2d.shape[1]), len(aggregators)
        out = torch.empty((csc.num_rows, A, D), dtype=torch.float32, device=dev)
        block = {name: ctypes.c_void_p(out.data_ptr() + i * D * 4) for i, name in enumerate(aggregators)}
        arg_max = torch.empty((csc.num_rows, D), dtype=torch.int32, device=dev) if "max" in block else None
        arg_min = torch.empty((csc.num_rows, D), dtype=torch.int32, device=dev) if "min" in block else None
        stats = torch.empty((csc.num_rows, 2, D), dtype=torch.float32, device=dev) if ("var" in block or "std" in block) else None
        plan = csc.plan()
        ws = self._multi_agg_ws(plan, D, dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="multi_agg_fwd", D=D, nnz=csc.nnz, n_src=csc.num_cols, n_dst=csc.num_rows):
            _lib.check(_lib.lib().mgx_multi_agg_fwd(ctypes.byref(csc.c_struct()), self._plan_ptr(plan), D, _ptr(x2d), _ptr(w2d),
                                                    ctypes.c_float(eps), *[block.get(n) for n in ("sum", "mean", "var", "std", "max", "min")],
                                                    A * D, _ptr(arg_max), _ptr(arg_min), _ptr(stats), _ptr(ws), _stream(dev)))
        return out, arg_max, arg_min, stats

    def multi_agg_bwd(self, csr, x2d, w2d, A2d, B2d, g_max, arg_max, g_min, arg_min, need_x, need_w):
        """csr: the out-CSR (rows = sources); A2d, B2d | None, g_max / g_min | None [n_dst, D] (any layout, dense16) with their
        int32 args -> (d_x [n_src, D] | None, d_w [E, D] by edge id | None)."""
        dev = self._check_dev(csr.indptr, x2d, w2d, A2d, B2d, g_max, arg_max, g_min, arg_min)
        D = int(x2d.shape[1])
        if not (need_x or need_w):
            return None, None
        x2d, w2d, A2d, B2d, g_max, g_min = (dense16(t) for t in (x2d, w2d, A2d, B2d, g_max, g_min))
        d_x = torch.empty((csr.num_rows, D), dtype=torch.float32, device=dev) if need_x else None
        d_w = torch.empty((csr.nnz, D), dtype=torch.float32, device=dev) if need_w else None
        plan = csr.plan()
        ws = self._gine_ws(plan, D, dev) if need_x else None   # [slots, D] partial rows of d x
        with torch.cuda.device(dev), timed_call(dev, kernel="multi_agg_bwd", D=D, nnz=csr.nnz, n_src=csr.num_rows, n_dst=csr.num_cols):
            _lib.check(_lib.lib().mgx_multi_agg_bwd(ctypes.byref(csr.c_struct()), self._plan_ptr(plan), D, _ptr(x2d), _ptr(w2d), _ptr(A2d),
                                                    _ptr(B2d), _ptr(g_max), _ptr(arg_max), _ptr(g_min), _ptr(arg_min), _ptr(d_x), _ptr(d_w),
                                                    _ptr(ws), _stream(dev)))
        return d_x, d_w

    @staticmethod
    def head_dot_supported(H, F):
        return H * F <= 256 and (F <= 64 or F in (128, 256))

    def head_dot_fwd(self, feat3d, attn_a, attn_b):
        """feat3d [n, H, F], attn_a/attn_b [H, F] (attn_b may be None) -> (out_a [n, H], out_b [n, H] | None)."""
        dev = self._check_dev(feat3d, attn_a, attn_b)
        n, H, F = feat3d.shape
        feat3d, attn_a, attn_b = dense16(feat3d), dense16(attn_a), dense16(attn_b)  # the 16-byte lanes of F % 4 == 0 refuse any other base
        out_a = torch.empty((n, H), dtype=torch.float32, device=dev)
        out_b = torch.empty((n, H), dtype=torch.float32, device=dev) if attn_b is not None else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_head_dot_fwd(n, H, F, _ptr(feat3d), _ptr(attn_a), _ptr(attn_b), _ptr(out_a), _ptr(out_b),
                                                   _stream(dev)))
        return out_a, out_b

    def head_dot_bwd(self, feat3d, attn_a, attn_b, d_a, d_b, need_feat_grad):
        dev = self._check_dev(feat3d, attn_a, attn_b, d_a, d_b)
        n, H, F = feat3d.shape
        feat3d, attn_a, d_a = feat3d.contiguous(), attn_a.contiguous(), d_a.contiguous()  # (4-byte accesses only: any base)
        attn_b, d_b = (None, None) if attn_b is None else (attn_b.contiguous(), d_b.contiguous())
        d_feat = torch.empty_like(feat3d) if need_feat_grad else None
        g_a = torch.empty_like(attn_a)
        g_b = torch.empty_like(attn_b) if attn_b is not None else None
        ws = torch.empty(_lib.lib().mgx_head_dot_bwd_workspace(H, F) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_head_dot_bwd(n, H, F, _ptr(feat3d), _ptr(attn_a), _ptr(attn_b), _ptr(d_a), _ptr(d_b),
                                                   _ptr(d_feat), _ptr(g_a), _ptr(g_b), _ptr(ws), _stream(dev)))
        return d_feat, g_a, g_b

    @staticmethod
    def _softmax_plan(csr, H, dev):
        plan = csr.softmax_plan()
        if plan is None:
            return None, None
        ws = None
        if plan.num_slots:
            ws = torch.empty((plan.num_slots + plan.num_hubs) * 2 * H, dtype=torch.float32, device=dev)
        return ctypes.byref(plan.c_struct()), ws

    def edge_softmax_bwd(self, csr, a2d, da2d):
        dev = self._check_dev(csr.indptr, a2d, da2d)
        dz = torch.empty_like(a2d)
        plan, ws = self._softmax_plan(csr, a2d.shape[1], dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_edge_softmax_bwd(ctypes.byref(csr.c_struct()), plan, a2d.shape[1], _ptr(a2d), _ptr(da2d),
                                                       _ptr(dz), _ptr(ws), _stream(dev)))
        return dz

    def segment_reduce(self, offsets, x2d, reduce, want_arg):
        dev = self._check_dev(offsets, x2d)
        n = offsets.shape[0] - 1
        out = torch.empty((n, x2d.shape[1]), dtype=torch.float32, device=dev)
        arg = torch.empty((n, x2d.shape[1]), dtype=torch.int64, device=dev) if want_arg else None
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_reduce", reduce=reduce, segments=int(n), rows=int(x2d.shape[0]), D=int(x2d.shape[1])):
            _lib.check(_lib.lib().mgx_segment_reduce(n, _ptr(offsets), x2d.shape[1], REDUCE[reduce], _ptr(x2d), _ptr(out), _ptr(arg), _stream(dev)))
        return out, arg

    # ---- graph readout (csrc/segattn.hip): nothing here reads `offsets` on the host
    def segment_softmax_fwd(self, offsets, x2d):
        dev = self._check_dev(offsets, x2d)
        n, D = offsets.shape[0] - 1, int(x2d.shape[1])
        out = torch.empty_like(x2d)
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_softmax_fwd", segments=int(n), rows=int(x2d.shape[0]), D=D):
            _lib.check(_lib.lib().mgx_segment_softmax_fwd(n, _ptr(offsets), D, _ptr(x2d), _ptr(out), _stream(dev)))
        return out

    def segment_softmax_bwd(self, offsets, out2d, d_out2d):
        dev = self._check_dev(offsets, out2d, d_out2d)
        n, D = offsets.shape[0] - 1, int(out2d.shape[1])
        dx = torch.empty_like(out2d)
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_softmax_bwd", segments=int(n), rows=int(out2d.shape[0]), D=D):
            _lib.check(_lib.lib().mgx_segment_softmax_bwd(n, _ptr(offsets), D, _ptr(out2d), _ptr(d_out2d), _ptr(dx), _stream(dev)))
        return dx

    @staticmethod
    def _seg_operand(x3d):
        """(tensor, row stride in floats) of a [N, H, F] feature operand as the kernels take it: the H*F floats of a row contiguous, the
        row stride a multiple of 4 floats, the base 16-byte aligned (a column block of a wider matrix qualifies); else an aligned dense
        copy (rows16)."""
        return rows16(x3d)

    _dense16 = staticmethod(dense16)  # the module's rule under the name the segment-attention wrappers came with

    @classmethod
    def segment_attention_supported(cls, feat3d):
        """Shapes mgx_segment_attention_* takes: F % 4 == 0, H*F <= 256; one head: any such F, several: F in {4, 8, 16, 32, 64}."""
        H, F = int(feat3d.shape[1]), int(feat3d.shape[2])
        if H < 1 or F < 1:
            return False
        return bool(_lib.lib().mgx_segment_attention_supported(H, F, H * F))  # a stride the kernels cannot take becomes a dense copy

    def segment_attention_fwd(self, offsets, feat3d, logits2d, query3d, scale):
        """feat3d [N, H, F] (row-strided views are taken as they are), logits2d [N, H] | None, query3d [S, H, F] | None ->
        (out [S, H, F], stat [S, H, 2] = (m, 1/s))."""
        dev = self._check_dev(offsets, feat3d, logits2d, query3d)
        S, H, F = offsets.shape[0] - 1, int(feat3d.shape[1]), int(feat3d.shape[2])
        feat, ld = self._seg_operand(feat3d)
        logits2d = None if logits2d is None else logits2d.contiguous()
        query3d = self._dense16(query3d)
        out = torch.empty((S, H, F), dtype=torch.float32, device=dev)
        stat = torch.empty((S, H, 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="seg_attn_fwd", H=H, F=F, segments=int(S), rows=int(feat3d.shape[0]),
                                                mode="gate" if query3d is None else "query"):
            _lib.check(_lib.lib().mgx_segment_attention_fwd(S, _ptr(offsets), H, F, _ptr(feat), ld, _ptr(logits2d), _ptr(query3d),
                                                            ctypes.c_float(scale), _ptr(out), _ptr(stat), _stream(dev)))
        return out, stat

    def segment_attention_bwd(self, offsets, feat3d, logits2d, query3d, scale, out3d, d_out3d, stat, need_feat, need_logits, need_query):
        """-> (d_feat | None, d_logits | None, d_query | None), each dense."""
        dev = self._check_dev(offsets, feat3d, logits2d, query3d, out3d, d_out3d, stat)
        S, H, F = offsets.shape[0] - 1, int(feat3d.shape[1]), int(feat3d.shape[2])
        need_logits, need_query = need_logits and logits2d is not None, need_query and query3d is not None
        if not (need_feat or need_logits or need_query):
            return None, None, None
        feat, ld = self._seg_operand(feat3d)
        logits2d = None if logits2d is None else logits2d.contiguous()
        query3d, out3d, d_out3d = self._dense16(query3d), self._dense16(out3d), self._dense16(d_out3d)
        d_feat = torch.empty((feat3d.shape[0], H, F), dtype=torch.float32, device=dev) if need_feat else None
        d_logits = torch.empty((feat3d.shape[0], H), dtype=torch.float32, device=dev) if need_logits else None
        d_query = torch.empty((S, H, F), dtype=torch.float32, device=dev) if need_query else None
        with torch.cuda.device(dev), timed_call(dev, kernel="seg_attn_bwd", H=H, F=F, segments=int(S), rows=int(feat3d.shape[0]),
                                                mode="gate" if query3d is None else "query"):
            _lib.check(_lib.lib().mgx_segment_attention_bwd(S, _ptr(offsets), H, F, _ptr(feat), ld, _ptr(logits2d), _ptr(query3d),
                                                            ctypes.c_float(scale), _ptr(out3d), _ptr(d_out3d), _ptr(stat), _ptr(d_feat),
                                                            _ptr(d_logits), _ptr(d_query), _stream(dev)))
        return d_feat, d_logits, d_query

    # ---- segment top-k (csrc/segtopk.hip): nothing here reads `offsets` on the host either
    @classmethod
    def segment_topk_supported(cls, k, D, columns):
        """Shapes mgx_segment_topk_* takes: 1 <= k <= 1024, any D >= 1."""
        return bool(_lib.lib().mgx_segment_topk_supported(int(k), int(D), 1 if columns else 0))

    def segment_topk_fwd(self, offsets, feat2d, k, sortby, descending):
        """feat2d [N, D] (a column block of a wider matrix is taken as it is), sortby a column in [0, D) or None (every column on its
        own) -> (values [S, k, D], index int64 [S, k] | [S, k, D], slot int32 [N] | [N, D])."""
        dev = self._check_dev(offsets, feat2d)
        S, N, D = offsets.shape[0] - 1, int(feat2d.shape[0]), int(feat2d.shape[1])
        columns = sortby is None
        if not (feat2d.stride(1) == 1 and feat2d.stride(0) >= D) and N > 0:  # a stride the kernel cannot take becomes a dense copy
            feat2d = feat2d.contiguous()
        ld = int(feat2d.stride(0)) if N > 0 else D
        values = torch.empty((S, k, D), dtype=torch.float32, device=dev)
        index = torch.empty((S, k, D) if columns else (S, k), dtype=torch.int64, device=dev)
        slot = torch.empty((N, D) if columns else (N,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="seg_topk_fwd", k=int(k), D=D, segments=int(S), rows=N,
                                                mode="columns" if columns else "rows"):
            _lib.check(_lib.lib().mgx_segment_topk_fwd(S, _ptr(offsets), N, D, ld, _ptr(feat2d), int(k), 1 if columns else 0,
                                                       0 if columns else int(sortby), 1 if descending else 0, _ptr(values), _ptr(index),
                                                       _ptr(slot), _stream(dev)))
        return values, index, slot

    def segment_topk_bwd(self, slot, d_values, D):
        """slot int32 [N] | [N, D], d_values [S, k, D] -> d_feat [N, D]: a gather, every element written once."""
        dev = self._check_dev(slot, d_values)
        N = int(slot.shape[0])
        d_values = d_values.contiguous()
        d_feat = torch.empty((N, D), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="seg_topk_bwd", D=int(D), rows=N, mode="columns" if slot.dim() == 2 else "rows"):
            _lib.check(_lib.lib().mgx_segment_topk_bwd(N, int(D), 1 if slot.dim() == 2 else 0, _ptr(slot), _ptr(d_values), _ptr(d_feat),
                                                       _stream(dev)))
        return d_feat

    # ---- segment k nearest neighbours (csrc/knn.hip)
    @classmethod
    def segment_knn_supported(cls, k, D):
        """Shapes mgx_segment_knn takes: 1 <= k <= 64, 1 <= D <= 256."""
        return bool(_lib.lib().mgx_segment_knn_supported(int(k), int(D)))

    def segment_knn(self, offsets, x2d, k, return_dist):
        """x2d [N, D] (a column block of a wider matrix is taken as it is) -> (index int64 [N, k], dist [N, k] | None)."""
        dev = self._check_dev(offsets, x2d)
        S, N, D = offsets.shape[0] - 1, int(x2d.shape[0]), int(x2d.shape[1])
        if not (x2d.stride(1) == 1 and x2d.stride(0) >= D) and N > 0:  # a stride the kernel cannot take becomes a dense copy
            x2d = x2d.contiguous()
        ld = int(x2d.stride(0)) if N > 0 else D
        index = torch.empty((N, k), dtype=torch.int64, device=dev)
        dist = torch.empty((N, k), dtype=torch.float32, device=dev) if return_dist else None
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_knn", k=int(k), D=D, segments=int(S), rows=N):
            _lib.check(_lib.lib().mgx_segment_knn(S, _ptr(offsets), N, D, ld, _ptr(x2d), int(k), _ptr(index), _ptr(dist), _stream(dev)))
        return index, dist

    @classmethod
    def segment_knn_query_supported(cls, k, D):
        """Shapes mgx_segment_knn_query takes: 1 <= k <= 64, 1 <= D <= 256."""
        return bool(_lib.lib().mgx_segment_knn_query_supported(int(k), int(D)))

    def segment_knn_query(self, offsets, x2d, q_offsets, y2d, k, eps, return_dist, return_weight):
        """references x2d [N, D], queries y2d [M, D] (column blocks of wider matrices are taken as they are) ->
        (index int64 [M, k], dist [M, k] | None, weight [M, k] | None)."""
        dev = self._check_dev(offsets, x2d, q_offsets, y2d)
        S, N, M, D = offsets.shape[0] - 1, int(x2d.shape[0]), int(y2d.shape[0]), int(x2d.shape[1])
        if not (x2d.stride(1) == 1 and x2d.stride(0) >= D) and N > 0:  # a stride the kernel cannot take becomes a dense copy
            x2d = x2d.contiguous()
        if not (y2d.stride(1) == 1 and y2d.stride(0) >= D) and M > 0:
            y2d = y2d.contiguous()
        ld, ldq = int(x2d.stride(0)) if N > 0 else D, int(y2d.stride(0)) if M > 0 else D
        index = torch.empty((M, k), dtype=torch.int64, device=dev)
        dist = torch.empty((M, k), dtype=torch.float32, device=dev) if return_dist else None
        weight = torch.empty((M, k), dtype=torch.float32, device=dev) if return_weight else None
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_knn_query", k=int(k), D=D, segments=int(S), rows=N, queries=M):
            _lib.check(_lib.lib().mgx_segment_knn_query(S, _ptr(offsets), N, ld, _ptr(x2d), _ptr(q_offsets), M, ldq, _ptr(y2d), D, int(k),
                                                        ctypes.c_float(eps), _ptr(index), _ptr(dist), _ptr(weight), _stream(dev)))
        return index, dist, weight

    # ---- farthest point sampling (csrc/fps.hip) and fixed-radius ball query (csrc/ballquery.hip)
    @classmethod
    def segment_fps_supported(cls, D, max_len):
        """Shapes mgx_segment_fps takes: 1 <= D <= 64, max_len <= min(16384, 38912 // (D | 1))."""
        return bool(_lib.lib().mgx_segment_fps_supported(int(D), int(max_len)))

    def segment_fps(self, offsets, x2d, m, max_len, start, return_dist):
        """x2d [N, D] (a column block of a wider matrix is taken as it is), start int64 [S] | None -> (index int64 [S, m], dist [S, m] | None)."""
        dev = self._check_dev(offsets, x2d, start)
        S, N, D = offsets.shape[0] - 1, int(x2d.shape[0]), int(x2d.shape[1])
        if not (x2d.stride(1) == 1 and x2d.stride(0) >= D) and N > 0:  # a stride the kernel cannot take becomes a dense copy
            x2d = x2d.contiguous()
        ld = int(x2d.stride(0)) if N > 0 else D
        index = torch.empty((S, m), dtype=torch.int64, device=dev)
        dist = torch.empty((S, m), dtype=torch.float32, device=dev) if return_dist else None
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_fps", m=int(m), D=D, segments=int(S), rows=N, max_len=int(max_len)):
            _lib.check(_lib.lib().mgx_segment_fps(S, _ptr(offsets), N, D, ld, _ptr(x2d), int(m), int(max_len), _ptr(start), _ptr(index),
                                                  _ptr(dist), _stream(dev)))
        return index, dist

    @classmethod
    def segment_ball_query_supported(cls, K, D):
        """Shapes mgx_segment_ball_query takes: 1 <= K <= 64, 1 <= D <= 256."""
        return bool(_lib.lib().mgx_segment_ball_query_supported(int(K), int(D)))

    def segment_ball_query(self, offsets, x2d, centers, radius2, K, pad_first):
        """x2d [N, D], centers int64 [M] global rows (-1: none) -> (index int64 [M, K], count int32 [M])."""
        dev = self._check_dev(offsets, x2d, centers)
        S, N, D, M = offsets.shape[0] - 1, int(x2d.shape[0]), int(x2d.shape[1]), int(centers.shape[0])
        if not (x2d.stride(1) == 1 and x2d.stride(0) >= D) and N > 0:
            x2d = x2d.contiguous()
        ld = int(x2d.stride(0)) if N > 0 else D
        index = torch.empty((M, K), dtype=torch.int64, device=dev)
        count = torch.empty((M,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev), timed_call(dev, kernel="segment_ball_query", K=int(K), D=D, segments=int(S), rows=N, queries=M):
            _lib.check(_lib.lib().mgx_segment_ball_query(S, _ptr(offsets), N, D, ld, _ptr(x2d), M, _ptr(centers), ctypes.c_float(radius2),
                                                         int(K), 1 if pad_first else 0, _ptr(index), _ptr(count), _stream(dev)))
        return index, count

    @staticmethod
    def _row_strided(t):
        return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.shape[1] % 4 == 0

    def relu_dropout_fwd(self, x, p, seed, offset, out=None, counter=None):
        """`out`: a row-strided [rows, cols] view to write into (x then 2-D, possibly row-strided itself).  `counter`: a
        1-element int64 device tensor read by the launch when it RUNS instead of the host-side `offset` (HIP-graph replays).
        An x whose base is not 16-byte aligned is copied first (dense16): every kernel here reads 16 bytes per lane."""
        dev = self._check_dev(x, out, counter)
        if _off16(x):
            x = dense16(x)
        mask = torch.empty(x.numel() // 4, dtype=torch.uint8, device=dev)
        if counter is not None:
            y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=dev)
            if not (self._row_strided(x) and self._row_strided(y) and x.shape == y.shape):
                raise DGLError("relu_dropout_fwd: counter mode needs [rows, cols] operands with unit column stride, cols % 4 == 0")
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mgx_relu_dropout_fwd_counter(x.shape[0], x.shape[1], _ptr(x), x.stride(0), ctypes.c_float(p),
                                                                    ctypes.c_uint64(seed), _ptr(counter), _ptr(y), y.stride(0),
                                                                    _ptr(mask), _stream(dev)))
            return y, mask
        if out is None and x.is_contiguous():
            y = torch.empty_like(x)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mgx_relu_dropout_fwd(x.numel(), _ptr(x), ctypes.c_float(p), ctypes.c_uint64(seed),
                                                           ctypes.c_uint64(offset), _ptr(y), _ptr(mask), _stream(dev)))
            return y, mask
        y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=dev)
        if not (self._row_strided(x) and self._row_strided(y) and x.shape == y.shape):
            raise DGLError("relu_dropout_fwd: strided operands must be [rows, cols] views with unit column stride, cols % 4 == 0")
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_relu_dropout_fwd_strided(x.shape[0], x.shape[1], _ptr(x), x.stride(0), ctypes.c_float(p),
                                                                ctypes.c_uint64(seed), ctypes.c_uint64(offset), _ptr(y), y.stride(0),
                                                                _ptr(mask), _stream(dev)))
        return y, mask

    def relu_dropout_bwd(self, dy, mask, p, out=None):
        """dy: contiguous, or a row-strided [rows, cols] view (the gradient's column block); dx is dense, or `out`: a row-strided [rows, cols]
        view to write into (the left half of a wider matrix).  A dy whose base is not 16-byte aligned is copied first (dense16)."""
        dev = self._check_dev(dy, mask, out)
        if _off16(dy):
            dy = dense16(dy)
        if out is not None:
            if dy.dim() != 2 or out.shape != dy.shape or not self._row_strided(out) or not (dy.is_contiguous() or self._row_strided(dy)):
                raise DGLError("relu_dropout_bwd: `out` must be a [rows, cols] view with unit column stride of the gradient's shape")
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mgx_relu_dropout_bwd_strided(dy.shape[0], dy.shape[1], _ptr(dy), dy.stride(0), _ptr(mask),
                                                                    ctypes.c_float(p), _ptr(out), out.stride(0), _stream(dev)))
            return out
        dx = torch.empty(dy.shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if dy.is_contiguous():
                _lib.check(_lib.lib().mgx_relu_dropout_bwd(dy.numel(), _ptr(dy), _ptr(mask), ctypes.c_float(p), _ptr(dx), _stream(dev)))
            else:
                if not self._row_strided(dy):
                    raise DGLError("relu_dropout_bwd: a non-contiguous gradient must be a [rows, cols] view with unit column stride")
                _lib.check(_lib.lib().mgx_relu_dropout_bwd_strided(dy.shape[0], dy.shape[1], _ptr(dy), dy.stride(0), _ptr(mask),
                                                                    ctypes.c_float(p), _ptr(dx), dx.stride(0), _stream(dev)))
        return dx

    def relu_dropout_bwd_slots(self, dy, mask, p, out, row_scale=None):
        """relu_dropout_bwd into `out` (a row-strided [rows, 64] view) + (slots, overflow) of row_scale * result, as rows_slots_pack would
        give them -- one pass (mgx_relu_dropout_bwd_slots)."""
        dev = self._check_dev(dy, mask, out, row_scale)
        if _off16(dy):  # as relu_dropout_bwd: a gradient off a 16-byte boundary is copied, not refused
            dy = dense16(dy)
        if (dy.dim() != 2 or dy.shape[1] != 64 or out.shape != dy.shape or not self._row_strided(out) or out.data_ptr() % 16
                or not (dy.is_contiguous() or self._row_strided(dy)) or dy.data_ptr() % 16):
            raise DGLError("relu_dropout_bwd_slots: [rows, 64] operands with unit column stride, 16-byte aligned")
        n = int(dy.shape[0])
        slots = torch.empty((n, 32), dtype=torch.int32, device=dev)
        overflow = torch.zeros(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_relu_dropout_bwd_slots(n, _ptr(dy), dy.stride(0), _ptr(mask), ctypes.c_float(p), _ptr(out), out.stride(0),
                                                             _ptr(row_scale), _ptr(slots), _ptr(overflow), _stream(dev)))
        return out, slots, overflow

    def column_pair_sums(self, a2d, b2d=None, shifted=False):
        """(sum a, sum a*a) per column, or (sum a, sum a*b) when b2d is given.  `shifted`: relative to the first row p of
        the squared / second operand -- (sum (a-p), sum (a-p)^2) with p = a[0], or (sum a, sum a*(b-p)) with p = b[0]."""
        dev = self._check_dev(a2d, b2d)
        n, C = a2d.shape
        a2d, b2d = a2d.contiguous(), None if b2d is None else b2d.contiguous()  # (4-byte accesses only: any base)
        out = torch.empty((2, C), dtype=torch.float32, device=dev)
        ws = torch.empty(2 * _lib.lib().mgx_column_sum_workspace(C) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_column_pair_sums(n, C, (0 if b2d is None else 1) + (2 if shifted else 0), _ptr(a2d), _ptr(b2d), _ptr(out[0]), _ptr(out[1]),
                                                       _ptr(ws), _stream(dev)))
        return out[0], out[1]

    def column_affine(self, a2d, A, Cc, b2d=None, B=None):
        """a*A[c] + b*B[c] + Cc[c] with per-column coefficient vectors; operands in any layout (16-byte lanes: dense16)."""
        dev = self._check_dev(a2d, b2d, A, B, Cc)
        a2d, b2d, A, B, Cc = (dense16(t) for t in (a2d, b2d, A, B, Cc))
        out = torch.empty_like(a2d)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_column_affine(a2d.shape[0], a2d.shape[1], _ptr(a2d), _ptr(b2d), _ptr(A), _ptr(B), _ptr(Cc),
                                                    _ptr(out), _stream(dev)))
        return out

    COLUMN_SUM_MAX = 256
    XTY_TILE = (64, 128)      # one tile of mgx_xty
    XTY_MAX = (256, 1024)     # the grid of tiles in one launch goes up to this output shape
    XTY_MIN_ROWS = 1 << 16    # shorter reductions stay with the GEMM library

    @staticmethod
    def _row_walkable(t):
        """Can the mgx_xty* kernels walk t [n, W] by its row stride?  Unit column stride and rows that do not overlap: the wrappers pass
        max(stride(0), W), which is right for the free stride of a one-row tensor only -- an expanded view (stride 0 along the rows, what
        `row.expand(n, W)` gives) would be read W floats per row past its single row."""
        return t.stride(1) == 1 and (t.stride(0) >= t.shape[1] or t.shape[0] < 2)

    def _xty_call(self, dev, M, K, colsum, call, out=None):
        """One call of an mgx_xty* entry point: allocates out [M, K] (unless the caller hands in the tile of a larger output), sums [M]
        if colsum and the workspace of mgx_xty_workspace(M, K); call(L, out, ldc, sums, workspace, stream) -> status.
        (out, sums), or None -- nothing launched -- when the library has no kernel for the operands (ERR_UNSUPPORTED)."""
        L = _lib.lib()
        if out is None:
            out = torch.empty((M, K), dtype=torch.float32, device=dev)
        sums = torch.empty(M, dtype=torch.float32, device=dev) if colsum else None
        ws = torch.empty(max(L.mgx_xty_workspace(M, K), 4) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = call(L, _ptr(out), out.stride(0), _ptr(sums), _ptr(ws), _stream(dev))
        if st == _lib.ERR_UNSUPPORTED:
            return None
        _lib.check(st)
        return out, sums

    def _xty_rows(self, a2d, b2d, rows, colsum):
        """xty over the row list in the kernel (mgx_xty_rows / mgx_xty_colsum_rows); None when the library has no kernel for the shape."""
        dev = self._check_dev(a2d, b2d, rows)
        n, M = a2d.shape
        K = b2d.shape[1]
        tm, tk = self.XTY_TILE
        if (M > tm or K > tk or not self._row_walkable(a2d) or not self._row_walkable(b2d) or a2d.dtype != torch.float32
                or b2d.dtype != torch.float32):
            return None
        head = (n, M, K, _ptr(a2d), max(a2d.stride(0), M), _ptr(b2d), max(b2d.stride(0), K), _ptr(rows))
        if colsum:
            return self._xty_call(dev, M, K, True, lambda L, *tail: L.mgx_xty_colsum_rows(*head, *tail))
        res = self._xty_call(dev, M, K, False, lambda L, out, ldc, _, ws, stream: L.mgx_xty_rows(*head, out, ldc, ws, stream))
        return None if res is None else res[0]

    def xty_pos(self, a2d, a_pos, b2d, colsum=False):
        """a^T b over all n rows of b2d [n, K] for an a that is zero outside some rows and stored without them: a2d [R, M], a_pos int64 [n]
        = the row of a2d that stands at row r, or -1 for a zero row (entries < R: not checked).  Bit for bit xty() of a2d scattered into
        a zero [n, M] matrix (mgx_xty_colsum_pos).  None when the library has no kernel for the shape."""
        dev = self._check_dev(a2d, b2d, a_pos)
        n, K = b2d.shape
        M = a2d.shape[1]
        tm, tk = self.XTY_TILE
        if (a_pos.dtype != torch.int64 or a_pos.shape != (n,) or not a_pos.is_contiguous() or a2d.shape[0] == 0 or M > tm or K > tk or not self._row_walkable(a2d)
                or not self._row_walkable(b2d) or a2d.dtype != torch.float32 or b2d.dtype != torch.float32):
            return None
        res = self._xty_call(dev, M, K, colsum, lambda L, *tail: L.mgx_xty_colsum_pos(
            n, M, K, _ptr(a2d), max(a2d.stride(0), M), _ptr(a_pos), _ptr(b2d), max(b2d.stride(0), K), *tail))
        return res if colsum or res is None else res[0]

    def xty_masked(self, dy, mask, p, b2d):
        """(dz^T b2d [64, K], column sums of dz [64]) for dz = relu_dropout_bwd(dy, mask, p), which is never stored: the mask is applied
        to dy as the kernel loads it (mgx_xty_colsum_masked).  Bit for bit xty(relu_dropout_bwd(dy, mask, p), b2d, colsum=True).
        dy [n, 64] and b2d [n, K]: unit column stride, row strides % 4 == 0, 16-byte aligned; mask: the uint8 [n * 16] of relu_dropout_fwd.
        None -- nothing launched -- when no kernel is built for the operands (K outside the built 64, 68 .. 80, 128, 196 .. 208, 256)."""
        dev = self._check_dev(dy, mask, b2d)
        if (dy.dim() != 2 or b2d.dim() != 2 or dy.shape[1] != 64 or b2d.shape[0] != dy.shape[0] or dy.dtype != torch.float32
                or b2d.dtype != torch.float32 or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != dy.shape[0] * 16):
            return None
        n, K = b2d.shape
        if (K < 64 or K > 256 or K % 4 or not self._row_walkable(dy) or not self._row_walkable(b2d) or max(dy.stride(0), 64) % 4 or max(b2d.stride(0), K) % 4
                or dy.data_ptr() % 16 or b2d.data_ptr() % 16):
            return None
        L = _lib.lib()
        out = torch.empty((64, K), dtype=torch.float32, device=dev)
        sums = torch.empty(64, dtype=torch.float32, device=dev)
        ws = torch.empty(L.mgx_xty_masked_workspace(K) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = L.mgx_xty_colsum_masked(n, K, _ptr(dy), max(dy.stride(0), 64), _ptr(mask), ctypes.c_float(p), _ptr(b2d), max(b2d.stride(0), K),
                                         _ptr(out), out.stride(0), _ptr(sums), _ptr(ws), _stream(dev))
        if st == _lib.ERR_UNSUPPORTED:
            return None
        _lib.check(st)
        return out, sums

    def xty(self, a2d, b2d, colsum=False, rows=None):
        """a2d [n, M], b2d [n, K] -> a^T b [M, K] (the tall-skinny weight-gradient product).  colsum=True: (a^T b, column sums of a) --
        the bias gradient from the same pass over a when the shape allows (mgx_xty_colsum), else by mgx_column_sum.
        rows (int64 [n], in range -- not checked): row r of the reduction pairs a2d[r] with b2d[rows[r]], read in place by the kernel
        where one is built for the shape (same bits as on the gathered copy), else from b2d.index_select(0, rows)."""
        if rows is not None:
            if rows.dtype != torch.int64 or rows.dim() != 1 or rows.shape[0] != a2d.shape[0] or not rows.is_contiguous():
                raise DGLError("xty: rows must be a contiguous int64 vector with one entry per row of a")
            res = self._xty_rows(a2d, b2d, rows, colsum)
            if res is not None:
                return res
            b2d = b2d.index_select(0, rows)
        dev = self._check_dev(a2d, b2d)
        a2d, b2d = (t if self._row_walkable(t) else t.contiguous() for t in (a2d, b2d))
        n, M = a2d.shape
        K = b2d.shape[1]
        if M > self.XTY_MAX[0] or K > self.XTY_MAX[1]:
            raise DGLError("mgx_xty: at most %d x %d outputs, got %d x %d" % (self.XTY_MAX + (M, K)))
        out = torch.empty((M, K), dtype=torch.float32, device=dev)
        tm, tk = self.XTY_TILE
        ntiles = ((M + tm - 1) // tm) * ((K + tk - 1) // tk)

        def one(a_t, b_t, o_t, want_sums):
            """a_t^T b_t into o_t; the column sums of a_t where they were wanted and the library forms them in the same pass, else None"""
            Mt, Kt = a_t.shape[1], b_t.shape[1]
            head = (n, Mt, Kt, _ptr(a_t), max(a2d.stride(0), M), _ptr(b_t), max(b2d.stride(0), K))
            if want_sums:
                res = self._xty_call(dev, Mt, Kt, True, lambda L, *tail: L.mgx_xty_colsum(*head, *tail), out=o_t)
                if res is not None:
                    return res[1]
            if self._xty_call(dev, Mt, Kt, False, lambda L, o, ldc, _, ws, stream: L.mgx_xty(*head, o, ldc, ws, stream), out=o_t) is None:
                _lib.check(_lib.ERR_UNSUPPORTED)
            return None

        sums = None
        if ntiles == 1 or ntiles >= 4:
            # a single 64 x 128 tile, or the grid of tiles in ONE launch (operand rows shared through L2): measured
            # 256 x 512 at n = 169 k 1.07 -> 0.56 ms, 128 x 602 at n = 233 k 0.78 -> 0.57 ms (experiments/exp_wgrad_shapes.py)
            sums = one(a2d, b2d, out, colsum and ntiles == 1)
        else:
            # two or three tiles (the stacked 64 x 200 of the products layer): one launch per tile, each with the exact tile
            # shape, is faster than the grid's padded 64 x 128 tiles (n = 2.45 M: 0.93 against 1.04 ms)
            for m0 in range(0, M, tm):
                for k0 in range(0, K, tk):
                    got = one(a2d[:, m0:m0 + tm], b2d[:, k0:k0 + tk], out[m0:m0 + tm, k0:k0 + tk], colsum and M <= tm and k0 == 0)
                    sums = got if got is not None else sums
        if not colsum:
            return out
        return out, (sums if sums is not None else self.column_sum(a2d if a2d.is_contiguous() else a2d.contiguous()))

    def _rows_gemm_lists(self, a2d, b2d, b_transposed, bias, row_scale, scale_from, split_col, rows, scatter_rows, out2):
        """rows_gemm with a row list in the kernel (mgx_rows_gemm_rows); None when the library has no kernel for the shape."""
        dev = self._check_dev(a2d, b2d, bias, row_scale, rows, scatter_rows, out2)
        n = int((rows if rows is not None else scatter_rows).shape[0])
        K = a2d.shape[1]
        M = b2d.shape[0] if b_transposed else b2d.shape[1]
        if (a2d.stride(1) != 1 or b2d.stride(1) != 1 or (b2d.shape[1] if b_transposed else b2d.shape[0]) != K
                or a2d.dtype != torch.float32 or b2d.dtype != torch.float32 or (rows is not None and scatter_rows is not None)):
            return None
        out = torch.empty((n, split_col if split_col else M), dtype=torch.float32, device=dev)
        c2 = out2
        if split_col and c2 is None:
            c2 = torch.empty((n, M - split_col), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib().mgx_rows_gemm_rows(n, K, M, _ptr(a2d), a2d.stride(0), _ptr(rows), _ptr(b2d), b2d.stride(0),
                                               1 if b_transposed else 0, _ptr(bias), _ptr(row_scale), int(scale_from), _ptr(out),
                                               out.stride(0), _ptr(c2), 0 if c2 is None else c2.stride(0), int(split_col),
                                               _ptr(scatter_rows), _stream(dev))
        if st == _lib.ERR_UNSUPPORTED:
            return None
        _lib.check(st)
        return out if c2 is None else (out, c2)

    def rows_gemm(self, a2d, b2d, b_transposed=False, bias=None, row_scale=None, scale_from=0, out=None, split_col=0, rows=None,
                  scatter_rows=None, out2=None):
        """a2d [n, K] (row-strided view allowed) x B -> [n, M]; B = b2d [K, M], or [M, K] when b_transposed (nn.Linear's layout);
        + bias; columns >= scale_from times row_scale[r].  split_col > 0 (a multiple of 4): TWO compact outputs, the columns before
        and from split_col on, returned as a pair.  None when mgx_rows_gemm has no kernel for the shape (use a GEMM).
        rows (int64 [R]): the product of the rows a2d[rows] -- [R, M], compact.  scatter_rows (int64 [n], DISTINCT; with split_col and
        out2 [., M - split_col]): row r of the second output is written to out2[scatter_rows[r]] and nothing else of out2 is touched;
        the pair is (first output, out2).  row_scale is indexed by the product's rows.  Lists must be in range (not checked).  In the
        kernel where one is built for the shape (mgx_rows_gemm_rows), else index_select / index_copy_ around the plain call: same bits."""
        if rows is not None or scatter_rows is not None:
            for lst in (rows, scatter_rows):
                if lst is not None and (lst.dtype != torch.int64 or lst.dim() != 1 or not lst.is_contiguous()):
                    raise DGLError("rows_gemm: a row list is a contiguous int64 vector")
            if scatter_rows is not None and (not split_col or out2 is None or out2.dim() != 2 or out2.stride(1) != 1
                                             or out2.dtype != torch.float32 or scatter_rows.shape[0] != (a2d if rows is None else rows).shape[0]):
                raise DGLError("rows_gemm: scatter_rows needs split_col, a float32 out2 and one entry per row of the product")
            if out is None:
                res = self._rows_gemm_lists(a2d, b2d, b_transposed, bias, row_scale, scale_from, split_col, rows, scatter_rows, out2)
                if res is not None:
                    return res
            if rows is not None:
                a2d = a2d.index_select(0, rows)
            res = self.rows_gemm(a2d, b2d, b_transposed, bias, row_scale, scale_from, out, split_col)
            if res is None or scatter_rows is None:
                return res
            out2.index_copy_(0, scatter_rows, res[1])
            return res[0], out2
        dev = self._check_dev(a2d, b2d, bias, row_scale, out)
        n, K = a2d.shape
        M = b2d.shape[0] if b_transposed else b2d.shape[1]
        if (a2d.stride(1) != 1 or b2d.stride(1) != 1 or (b2d.shape[1] if b_transposed else b2d.shape[0]) != K
                or a2d.dtype != torch.float32 or b2d.dtype != torch.float32):
            return None
        out2 = None
        if split_col:
            out = torch.empty((n, split_col), dtype=torch.float32, device=dev)
            out2 = torch.empty((n, M - split_col), dtype=torch.float32, device=dev)
        elif out is None:
            out = torch.empty((n, M), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib().mgx_rows_gemm(n, K, M, _ptr(a2d), a2d.stride(0), _ptr(b2d), b2d.stride(0), 1 if b_transposed else 0,
                                          _ptr(bias), _ptr(row_scale), int(scale_from), _ptr(out), out.stride(0), _ptr(out2),
                                          0 if out2 is None else out2.stride(0), int(split_col), _stream(dev))
        if st == _lib.ERR_UNSUPPORTED:
            return None
        _lib.check(st)
        return out if out2 is None else (out, out2)

    def rows_gemm_supported(self, K, M, lda):
        return bool(_lib.lib().mgx_rows_gemm_supported(int(K), int(M), int(lda)))

    def rows_gemm_sweep_rows(self, K, M, lda, relu_dropout=False):
        """Rows one sweep of the rows_gemm grid covers on this device (0: no kernel for the shape)."""
        return int(_lib.lib().mgx_rows_gemm_sweep_rows(int(K), int(M), int(lda), 1 if relu_dropout else 0))

    def rows_gemm_relu_dropout(self, a2d, b2d, b_transposed, bias, p, seed, offset, out=None, slots=None, overflow=None):
        """dropout(relu(a2d x B + bias), p) written into `out` (a row-strided [n, M] view, or a new matrix) + the mask of
        relu_dropout_fwd -- bit for bit what rows_gemm followed by relu_dropout_fwd(seed, offset) gives, without storing the product.
        `slots` ([n, 32] int32, M == 64): the rows as 128-byte slots too -- what rows_slots_pack(result) would write --, `overflow`
        (int64[1]) += rows above 24 non-zeros.  None when mgx_rows_gemm has no kernel for the shape."""
        dev = self._check_dev(a2d, b2d, bias, out)
        n, K = a2d.shape
        M = b2d.shape[0] if b_transposed else b2d.shape[1]
        if (a2d.stride(1) != 1 or b2d.stride(1) != 1 or (b2d.shape[1] if b_transposed else b2d.shape[0]) != K or M % 4
                or a2d.dtype != torch.float32 or b2d.dtype != torch.float32 or not self.rows_gemm_supported(K, M, a2d.stride(0))):
            return None
        y = out if out is not None else torch.empty((n, M), dtype=torch.float32, device=dev)
        if not self._row_strided(y) or y.shape != (n, M) or y.data_ptr() % 16:
            return None
        mask = torch.empty(n * M // 4, dtype=torch.uint8, device=dev)
        if slots is not None and (M != 64 or slots.shape != (n, 32) or slots.dtype != torch.int32 or not slots.is_contiguous()):
            raise DGLError("rows_gemm_relu_dropout: slots are [n, 32] int32 for 64 output columns")
        with torch.cuda.device(dev):
            st = _lib.lib().mgx_rows_gemm_relu_dropout(n, K, M, _ptr(a2d), a2d.stride(0), _ptr(b2d), b2d.stride(0),
                                                       1 if b_transposed else 0, _ptr(bias), ctypes.c_float(p), ctypes.c_uint64(seed),
                                                       ctypes.c_uint64(offset), _ptr(y), y.stride(0), _ptr(mask), _ptr(slots),
                                                       _ptr(overflow) if slots is not None else None, _stream(dev))
        if st == _lib.ERR_UNSUPPORTED:  # e.g. an operand that is only dword aligned: mgx_rows_gemm_supported() never sees the pointer
            return None
        _lib.check(st)
        return y, mask

    def column_sum(self, x2d):
        dev = self._check_dev(x2d)
        n, C = x2d.shape
        x2d = x2d.contiguous()  # (4-byte accesses only: any base)
        out = torch.empty(C, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.lib().mgx_column_sum_workspace(C) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_column_sum(n, C, _ptr(x2d), _ptr(out), _ptr(ws), _stream(dev)))
        return out

    def sample_neighbors(self, csr, seeds, fanout, rng_seed):
        """seeds: graph-idtype tensor on the device.  Returns (src, eid, counts) with the picks of seed i at
        [offsets[i], offsets[i+1])."""
        dev = self._check_dev(csr.indptr, seeds)
        deg = (csr.indptr[seeds.long() + 1] - csr.indptr[seeds.long()]).long()
        counts = torch.clamp(deg, max=fanout)
        offsets = torch.zeros(seeds.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        total = int(offsets[-1].item())
        src = torch.empty(total, dtype=csr.indptr.dtype, device=dev)
        eid = torch.empty(total, dtype=csr.indptr.dtype, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_sample_neighbors(ctypes.byref(csr.c_struct()), seeds.shape[0], _ptr(seeds), int(fanout),
                                                       ctypes.c_uint64(rng_seed & (2 ** 64 - 1)), _ptr(offsets), _ptr(src),
                                                       _ptr(eid), _stream(dev)))
        return src, eid, counts

    @staticmethod
    def _sample_offsets(counts):
        """Per-seed counts -> their exclusive cumsum [n + 1]: where each seed's picks go; the last entry sizes the outputs."""
        offsets = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=counts.device)
        torch.cumsum(counts, 0, out=offsets[1:])
        return offsets

    def sample_neighbors_modes(self, csr, seeds, fanout, prob, replace, rng_seed):
        """The modes mgx_sample_neighbors does not have: `prob` (fp32, one weight per edge id, or None) and / or `replace`.
        Returns (src, eid, counts) like sample_neighbors; DGLError when an in-edge of a seed has a negative, NaN or infinite weight."""
        dev = self._check_dev(csr.indptr, seeds, prob)
        n = seeds.shape[0]
        c = ctypes.byref(csr.c_struct())
        if prob is None:
            if not replace:
                raise DGLError("sample_neighbors_modes: uniform sampling without replacement is sample_neighbors")
            deg = (csr.indptr[seeds.long() + 1] - csr.indptr[seeds.long()]).long()
            counts = (deg > 0).long() * fanout
            offsets = self._sample_offsets(counts)
            total = int(offsets[-1].item())
        else:
            positive = torch.empty(n, dtype=torch.int64, device=dev)
            invalid = torch.zeros(1, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mgx_sample_count_positive(c, n, _ptr(seeds), _ptr(prob), _ptr(positive), _ptr(invalid), _stream(dev)))
            counts = (positive > 0).long() * fanout if replace else torch.clamp(positive, max=fanout)
            offsets = self._sample_offsets(counts)
            total, bad = torch.stack([offsets[-1], invalid[0].long()]).tolist()  # output size and the weight flag in one host read
            if bad:
                raise DGLError("sample_neighbors: edge weights must be finite and non-negative")
        src = torch.empty(total, dtype=csr.indptr.dtype, device=dev)
        eid = torch.empty(total, dtype=csr.indptr.dtype, device=dev)
        if total == 0:
            return src, eid, counts
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_sample_neighbors_weighted(c, n, _ptr(seeds), int(fanout), _ptr(prob), 1 if replace else 0,
                                                                ctypes.c_uint64(rng_seed & (2 ** 64 - 1)), _ptr(offsets), _ptr(src),
                                                                _ptr(eid), _stream(dev)))
        return src, eid, counts

    def select_topk(self, csr, seeds, k, weight, ascending):
        """(src, eid, counts): the k edges of largest (ascending: smallest) weight of every seed's row, ties to the lower CSR position."""
        dev = self._check_dev(csr.indptr, seeds, weight)
        deg = (csr.indptr[seeds.long() + 1] - csr.indptr[seeds.long()]).long()
        counts = torch.clamp(deg, max=k)
        offsets = self._sample_offsets(counts)
        total = int(offsets[-1].item())
        src = torch.empty(total, dtype=csr.indptr.dtype, device=dev)
        eid = torch.empty(total, dtype=csr.indptr.dtype, device=dev)
        if total == 0:
            return src, eid, counts
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_select_topk(ctypes.byref(csr.c_struct()), seeds.shape[0], _ptr(seeds), int(k), _ptr(weight),
                                                  1 if ascending else 0, _ptr(offsets), _ptr(src), _ptr(eid), _stream(dev)))
        return src, eid, counts

    # ---- sampled blocks and induced subgraphs (csrc/relabel.hip)
    def to_block(self, num_nodes, dst_nodes, src, dst, dst_sorted, idtype):
        """dst_nodes, src, dst: contiguous int64 global ids on one device.  Returns (src_nodes int64, l_src, l_dst, indptr or None) with
        the local ids and the dst-sorted in-CSR's row pointer in `idtype`.  One host read: the number of sources and the error bits."""
        dev = self._check_dev(src, dst, dst_nodes)
        L = _lib.lib()
        num_dst, nnz = int(dst_nodes.shape[0]), int(src.shape[0])
        bits = 32 if idtype == torch.int32 else 64
        src_nodes = torch.empty(num_dst + min(nnz, num_nodes), dtype=torch.int64, device=dev)
        l_src = torch.empty(nnz, dtype=idtype, device=dev)
        l_dst = torch.empty(nnz, dtype=idtype, device=dev)
        indptr = torch.empty(num_dst + 1, dtype=idtype, device=dev) if dst_sorted else None
        with torch.cuda.device(dev):
            ws_bytes = L.mgx_to_block_workspace(num_nodes, nnz)
            if ws_bytes < 0:
                raise DGLError("to_block: negative num_nodes")
            ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device=dev)  # the last two words: {num_src, error bits}
            result = ws[-2:]
            _lib.check(L.mgx_to_block(num_nodes, num_dst, _ptr(dst_nodes), nnz, _ptr(src), _ptr(dst), 1 if dst_sorted else 0, bits,
                                      _ptr(ws), _ptr(src_nodes), _ptr(l_src), _ptr(l_dst), _ptr(indptr), _ptr(result), _stream(dev)))
        num_src, err = result.tolist()
        if err & 4:
            raise DGLError("to_block: a node id is outside [0, %d)" % num_nodes)
        if err & 1:
            raise DGLError("to_block: dst_nodes holds a node more than once")
        if err & 2:
            raise DGLError("to_block: every edge destination must be one of dst_nodes")
        if err & 8:
            raise DGLError("to_block: dst_sorted=True, but the edges are not grouped by destination in dst_nodes order")
        return src_nodes[:num_src], l_src, l_dst, indptr

    def node_subgraph(self, csc, nodes, idtype):
        """csc: the parent's in-CSR; nodes: contiguous int64 ids on its device.  Returns (l_src, l_dst in `idtype`, parent_eid int64,
        offsets int64 [n + 1], rows_by_eid): the kept edges row by row of the selection, CSR order inside a row; rows_by_eid: the edge
        ids of every selected row ascend (the rows then are in the order a stable sort of the kept edges by destination gives)."""
        dev = self._check_dev(csc.indptr, nodes)
        L = _lib.lib()
        n = int(nodes.shape[0])
        c = ctypes.byref(csc.c_struct())
        bits = 32 if idtype == torch.int32 else 64
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            ws_bytes = L.mgx_node_subgraph_workspace(csc.num_rows)
            ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)  # the last word: error bits
            result = ws[-1:]
            _lib.check(L.mgx_node_subgraph_count(c, n, _ptr(nodes), _ptr(ws), _ptr(counts), _ptr(result), _stream(dev)))
        offsets = self._sample_offsets(counts)
        total, err = torch.stack([offsets[-1], result[0]]).tolist()  # output size and the error bits in one host read
        if err & 4:
            raise DGLError("subgraph: a node id is outside [0, %d)" % csc.num_rows)
        if err & 1:
            raise DGLError("subgraph: a node is selected more than once")
        l_src = torch.empty(total, dtype=idtype, device=dev)
        l_dst = torch.empty(total, dtype=idtype, device=dev)
        parent_eid = torch.empty(total, dtype=torch.int64, device=dev)
        if total:
            with torch.cuda.device(dev):
                _lib.check(L.mgx_node_subgraph_fill(c, n, _ptr(nodes), _ptr(ws), _ptr(offsets), bits, _ptr(l_src), _ptr(l_dst),
                                                    _ptr(parent_eid), _stream(dev)))
        return l_src, l_dst, parent_eid, offsets, not (err & 16)

    # ---- link-prediction minibatches (csrc/edgefind.hip, csrc/relabel.hip)
    def edge_lookup(self, csr, row_ids, col_ids):
        """row_ids, col_ids: contiguous int64 on the CSR's device.  Returns (eid int64 [n], error bits): the lowest edge id of every
        (row, col) pair, -1 without an edge.  The caller reads the bits (4: an id out of range) with whatever else it reads."""
        dev = self._check_dev(csr.indptr, row_ids, col_ids)
        n = int(row_ids.shape[0])
        out = torch.empty(n, dtype=torch.int64, device=dev)
        result = torch.empty(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_edge_lookup(ctypes.byref(csr.c_struct()), n, _ptr(row_ids), _ptr(col_ids), _ptr(out), _ptr(result),
                                                  _stream(dev)))
        return out, result

    def negative_sample(self, csr, rows_are_sources, pos_src, k, num_dst_nodes, flags, max_tries, rng_seed):
        """pos_src: contiguous int64 on the device; csr: the CSR of the existence checks, None exactly when flags has no bit 1.
        Returns (dst int64 [n * k], -1 where every try was rejected; result int64 [2] = {failed draws, error bits})."""
        dev = self._check_dev(pos_src, None if csr is None else csr.indptr)
        n = int(pos_src.shape[0])
        out = torch.empty(n * int(k), dtype=torch.int64, device=dev)
        result = torch.empty(2, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_negative_sample(None if csr is None else ctypes.byref(csr.c_struct()), 1 if rows_are_sources else 0, n,
                                                      _ptr(pos_src), int(k), int(num_dst_nodes), int(flags), int(max_tries),
                                                      ctypes.c_uint64(rng_seed & (2 ** 64 - 1)), _ptr(out), _ptr(result), _stream(dev)))
        return out, result

    def frontier_exclude(self, offsets, src, eid, excl_sorted):
        """A frontier (offsets int64 [n + 1]; src, eid of one integer type, grouped by seed) without the edges whose id is in the
        ascending int64 list `excl_sorted`.  Returns (src, eid, counts int64 [n]); one host read: the new size."""
        dev = self._check_dev(offsets, src, eid, excl_sorted)
        L = _lib.lib()
        n = int(offsets.shape[0]) - 1
        bits = 32 if eid.dtype == torch.int32 else 64
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.mgx_frontier_exclude_count(n, _ptr(offsets), _ptr(eid), bits, int(excl_sorted.shape[0]), _ptr(excl_sorted),
                                                    _ptr(counts), _stream(dev)))
        new_offsets = self._sample_offsets(counts)
        total = int(new_offsets[-1].item())
        out_src = torch.empty(total, dtype=src.dtype, device=dev)
        out_eid = torch.empty(total, dtype=eid.dtype, device=dev)
        if total:
            with torch.cuda.device(dev):
                _lib.check(L.mgx_frontier_exclude_fill(n, _ptr(offsets), _ptr(eid), bits, int(excl_sorted.shape[0]), _ptr(excl_sorted),
                                                       _ptr(src), _ptr(new_offsets), _ptr(out_src), _ptr(out_eid), _stream(dev)))
        return out_src, out_eid, counts

    def compact_nodes(self, num_nodes, ids, idtype):
        """ids: contiguous int64 on the device.  Returns (nodes int64: the distinct ids ascending, local in `idtype`: the position of
        every entry of `ids` among them).  One host read: the number of distinct ids and the error bits."""
        dev = self._check_dev(ids)
        L = _lib.lib()
        n = int(ids.shape[0])
        nodes = torch.empty(min(n, num_nodes), dtype=torch.int64, device=dev)
        local = torch.empty(n, dtype=idtype, device=dev)
        with torch.cuda.device(dev):
            ws_bytes = L.mgx_compact_nodes_workspace(num_nodes, n)
            if ws_bytes < 0:
                raise DGLError("compact_nodes: negative num_nodes")
            ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device=dev)  # the last two words: {count, error bits}
            result = ws[-2:]
            _lib.check(L.mgx_compact_nodes(num_nodes, n, _ptr(ids), 32 if idtype == torch.int32 else 64, _ptr(ws), _ptr(nodes), _ptr(local),
                                           _ptr(result), _stream(dev)))
        count, err = result.tolist()
        if err & 4:
            raise DGLError("compact_nodes: a node id is outside [0, %d)" % num_nodes)
        return nodes[:count], local

    # ---- halo rows as bitmaps + packed values (csrc/rowpack.hip; dist.SparseHalo)
    ROWPACK_MAX_D = 256

    def rows_pack_supported(self, x2d):
        return (x2d.dim() == 2 and x2d.dtype == torch.float32 and x2d.stride(1) == 1 and x2d.shape[1] % 4 == 0
                and 4 <= x2d.shape[1] <= self.ROWPACK_MAX_D and x2d.stride(0) % 4 == 0 and x2d.data_ptr() % 16 == 0)

    def rows_pack_count(self, x2d, idx):
        """(masks [n, ceil(D / 64)] int64 bit patterns of x2d[idx[i], :] != 0, counts [n] int32); idx None = every row in order."""
        dev = self._check_dev(x2d, idx)
        n = int(x2d.shape[0] if idx is None else idx.shape[0])
        D = int(x2d.shape[1])
        masks = torch.empty((n, (D + 63) // 64), dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_pack_count(n, _ptr(idx), 0 if idx is None else (32 if idx.dtype == torch.int32 else 64), D, _ptr(x2d),
                                                      x2d.stride(0), _ptr(masks), _ptr(counts), _stream(dev)))
        return masks, counts

    def rows_mask_count(self, masks, D):
        dev = self._check_dev(masks)
        counts = torch.empty(masks.shape[0], dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_mask_count(masks.shape[0], int(D), _ptr(masks), _ptr(counts), _stream(dev)))
        return counts

    def rows_pack_values(self, x2d, idx, masks, offsets, total):
        """The values of x2d[idx[i], :] under masks[i], row i from offsets[i] on, as one [total] vector."""
        dev = self._check_dev(x2d, idx, masks, offsets)
        values = torch.empty(int(total), dtype=torch.float32, device=dev)
        n = int(masks.shape[0])
        if int(total) == 0:  # every mask empty (a layer whose boundary rows are all zero): nothing to write, and an empty tensor has no address
            return values
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_pack_values(n, _ptr(idx), 0 if idx is None else (32 if idx.dtype == torch.int32 else 64),
                                                       int(x2d.shape[1]), _ptr(x2d), x2d.stride(0), _ptr(masks), _ptr(offsets), _ptr(values),
                                                       _stream(dev)))
        return values

    def rows_unpack(self, masks, offsets, values, D, out=None):
        """Dense [n, D] rows: values under the masks, zeros elsewhere."""
        dev = self._check_dev(masks, offsets, values, out)
        n = int(masks.shape[0])
        if out is None:
            out = torch.empty((n, int(D)), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_unpack(n, int(D), _ptr(masks), _ptr(offsets), _ptr(values), _ptr(out), out.stride(0), _stream(dev)))
        return out

    def rows_unpack_add_csr(self, csr, masks, offsets, values, out):
        """out[v] += the packed rows at the positions listed in row v of `csr` (int32), in CSR order; out row-strided."""
        dev = self._check_dev(csr.indptr, masks, offsets, values, out)
        if csr.idx_bits != 32 or values.numel() >= 2 ** 32:
            raise DGLError("rows_unpack_add_csr: int32 CSR and fewer than 2^32 packed values only")
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_rows_unpack_add_csr(csr.num_rows, _ptr(csr.indptr), _ptr(csr.indices), int(out.shape[1]), _ptr(masks),
                                                          _ptr(offsets), _ptr(values), _ptr(out), out.stride(0), _stream(dev)))
        return out

    def gather_rows(self, x2d, idx):
        """out[i] = x2d[idx[i]]; x2d may be a row-strided view (stride(1) == 1) when D and the stride are multiples of 4."""
        dev = self._check_dev(x2d, idx)
        D = int(x2d.shape[1])
        out = torch.empty((idx.shape[0], D), dtype=torch.float32, device=dev)
        bits = 32 if idx.dtype == torch.int32 else 64
        with torch.cuda.device(dev):
            if (x2d.dim() == 2 and x2d.stride(1) == 1 and D % 4 == 0 and x2d.stride(0) % 4 == 0 and x2d.data_ptr() % 16 == 0 and D > 0
                    and x2d.stride(0) >= D):
                _lib.check(_lib.lib().mgx_gather_rows_strided(idx.shape[0], _ptr(idx), bits, D, _ptr(x2d), int(x2d.stride(0)), _ptr(out),
                                                              D, _stream(dev)))
            else:
                x2d = x2d.contiguous()
                _lib.check(_lib.lib().mgx_gather_rows(idx.shape[0], _ptr(idx), bits, D, _ptr(x2d), _ptr(out), _stream(dev)))
        return out

    def scatter_add_rows(self, x2d, idx, rows2d):
        dev = self._check_dev(x2d, idx, rows2d)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mgx_scatter_add_rows(idx.shape[0], _ptr(idx), 32 if idx.dtype == torch.int32 else 64,
                                                       x2d.shape[1], _ptr(rows2d), _ptr(x2d), _stream(dev)))
        return x2d


_BACKENDS = {"cuda": HipBackend()}


def register_backend(device_type, backend):
    """Hook used by tests/ only (a checker backend for CPU tensors in gloo tests)."""
    _BACKENDS[device_type] = backend


def backend_for(tensor):
    b = _BACKENDS.get(tensor.device.type)
    if b is None:
        raise DGLError(
            "message passing on %s tensors is not supported: this backend runs on MI355X (HIP) devices only; "
            "move the graph and features to a cuda/hip device" % tensor.device.type)
    return b


def coo_to_csr_host(num_rows, num_cols, row, col):
    """Stable COO->CSR for CPU index tensors (host half of the C ABI; needs no GPU)."""
    nnz = row.shape[0]
    bits = 32 if row.dtype == torch.int32 else 64
    row, col = row.contiguous(), col.contiguous()
    indptr = torch.empty(num_rows + 1, dtype=row.dtype)
    indices = torch.empty(nnz, dtype=row.dtype)
    eids = torch.empty(nnz, dtype=row.dtype)
    _lib.check(_lib.lib().mgx_coo_to_csr_host(num_rows, nnz, _ptr(row), _ptr(col), bits, _ptr(indptr), _ptr(indices), _ptr(eids)))
    return CsrView(num_rows, num_cols, indptr, indices, eids)


def csr_transpose(csr):
    """Device CSR -> its transpose (same edge ids); rows ordered by the positions in `csr`."""
    return backend_for(csr.indptr).csr_transpose(csr)


def coo_to_csr(num_rows, num_cols, row, col):
    if row.is_cuda:
        return _BACKENDS["cuda"].coo_to_csr(num_rows, num_cols, row.contiguous(), col.contiguous())
    return coo_to_csr_host(num_rows, num_cols, row, col)


# ----------------------------------------------------------------------------- raw ops
def _as_f32(t, what):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise DGLError("%s must be float32 on this backend, got %s" % (what, t.dtype))
    return t.contiguous()


_WIDE_PAD_MIN = 176  # above this width the g-SpMM runs in column passes of 128 columns (csrc/spmm.hip launch_fast_v)


def gspmm_raw(csr, op, reduce, U, E, src_scale=None, dst_scale=None, want_arg=False, accumulate_into=None, dense_out=False):
    """out[v] = reduce_{p in row v} op(U[indices[p]], E[eids[p]]).

    U: (num_cols, *ushape) or None; E: (nnz, *eshape) or None.  Returns (out, arg_u, arg_e) with out of
    shape (num_rows, *bcast(ushape, eshape)).  `out` may be a row-strided VIEW (the line-padded wide path below) unless
    `dense_out` is set -- callers that hand the result to a raw kernel (accumulate_into) ask for a dense one."""
    if op not in ("add", "mul", "copy_lhs", "copy_rhs"):
        raise DGLError("gspmm_raw: unsupported op %r (sub/div are rewritten by the caller)" % op)
    U = None if op == "copy_rhs" else _as_f32(U, "gspmm lhs feature")
    E = None if op == "copy_lhs" else _as_f32(E, "gspmm rhs feature")
    if op != "copy_rhs" and U is None:
        raise DGLError("gspmm: op %r needs node features" % op)
    if op != "copy_lhs" and E is None:
        raise DGLError("gspmm: op %r needs edge features" % op)
    if U is not None and U.shape[0] != csr.num_cols:
        raise DGLError("gspmm: expected %d source rows, got %d" % (csr.num_cols, U.shape[0]))
    if E is not None and E.shape[0] != csr.nnz:
        raise DGLError("gspmm: expected %d edge rows, got %d" % (csr.nnz, E.shape[0]))
    if (op == "copy_lhs" and reduce in ("sum", "mean") and U.dim() == 2 and U.is_cuda and accumulate_into is None
            and U.shape[1] > _WIDE_PAD_MIN and U.shape[1] % 32 and csr.nnz >= max(config.WIDE_PAD_MIN_NNZ, 64 * csr.num_cols) and config.WIDE_PAD):
        # Wide rows that are not whole 128-byte lines (reddit's 602 input features: 2408-byte rows) on a dense graph: every
        # 512-byte column pass of a gathered row straddles one more line and 16-byte lanes are misaligned.  Aggregating a copy
        # padded to whole lines and returning the [:, :D] view is faster by more than the copy costs once a row is gathered
        # ~64 times (reddit-shaped, 492 in-edges per node: D = 602 18.4 ms -> 0.3 + 14.4 ms; D = 300 9.7 -> 0.2 + 8.0 ms).
        D = U.shape[1]
        out, _, _ = gspmm_raw(csr, op, reduce, torch.nn.functional.pad(U, (0, (-D) % 32)), None, src_scale, dst_scale)
        return (out[:, :D].contiguous() if dense_out else out[:, :D]), None, None
    ushape = tuple(U.shape[1:]) if U is not None else ()
    eshape = tuple(E.shape[1:]) if E is not None else ()
    if U is not None and E is not None:
        oshape, u_tab, e_tab = _bcast_plan(ushape, eshape)
    else:
        oshape, u_tab, e_tab = (ushape if U is not None else eshape), None, None
    ref = U if U is not None else E
    dev = ref.device
    out, arg_u, arg_e = backend_for(ref).spmm(
        csr, op, reduce, U, E, _prod(ushape), _prod(eshape), _prod(oshape),
        _device_table(u_tab, dev), _device_table(e_tab, dev), src_scale, dst_scale, want_arg,
        **({"accumulate_into": accumulate_into} if accumulate_into is not None else {}))
    shape = (csr.num_rows,) + tuple(oshape)
    out = out.view(shape)
    if arg_u is not None:
        arg_u = arg_u.view(shape)
    if arg_e is not None:
        arg_e = arg_e.view(shape)
    return out, arg_u, arg_e


# nnz below which a separate pass over the gradient to flag its zero rows cannot pay


def gspmm_grad_raw(csr, dZ, dst_scale=None, accumulate_into=None, dense_out=False):
    """copy_u / sum over `csr` of a GRADIENT matrix dZ [num_cols, ...]: the backward aggregation of copy_u (dX = A^T dZ).
    Gradients of a loss taken on a subset of the nodes are zero in most rows at the last layer (ogbn-products: 92 %), so the
    rows of dZ are flagged first (one streaming pass) and the aggregation skips the all-zero ones -- same sum, fewer gathers.
    OFF by default (MGX_SPARSE_GRAD=1 enables it): measured on the products epoch the 92 %-zero launch drops only from
    2.41 to 1.65 ms (2.66 M work items of ~4 live edges each are bound by the per-item chain meta -> ids -> flags -> rows ->
    store, not by bytes) while the dense-gradient launch of the layer below pays 0.55 ms for the flagging pass and the flag
    gathers: no net gain (23.4 vs 23.5 ms).  Exact either way; kept with its test as a measured variant."""
    be = backend_for(dZ)
    flat = dZ.contiguous().view(dZ.shape[0], -1)
    if (config.SPARSE_GRAD and be.name == "hip" and csr.nnz >= config.SPARSE_GRAD_MIN_NNZ and csr.idx_bits == 32
            and flat.shape[1] % 4 == 0 and flat.shape[1] >= 4 and dZ.dtype == torch.float32 and dZ.shape[0] == csr.num_cols
            and csr.num_cols * flat.shape[1] * 4 < 2 ** 32 and flat.data_ptr() % 16 == 0):
        bits = be.row_nonzero_bits(flat)
        out = be.spmm_copy_u_masked(csr, "sum", flat, bits, dst_scale, accumulate_into)
        return out.view((csr.num_rows,) + tuple(dZ.shape[1:]))
    return gspmm_raw(csr, "copy_lhs", "sum", dZ, None, dst_scale=dst_scale, accumulate_into=accumulate_into, dense_out=dense_out)[0]


def gsddmm_raw(gidx, op, L, R, lhs_target="u", rhs_target="v"):
    """out[e] = op(L[t_l(e)], R[t_r(e)]) in edge-id order; `dot` reduces the last dim to size 1."""
    L = None if op == "copy_rhs" else _as_f32(L, "gsddmm lhs feature")
    R = None if op == "copy_lhs" else _as_f32(R, "gsddmm rhs feature")
    if op not in OP:
        raise DGLError("gsddmm: unsupported op %r" % op)
    if op != "copy_rhs" and L is None:
        raise DGLError("gsddmm: op %r needs the lhs operand" % op)
    if op != "copy_lhs" and R is None:
        raise DGLError("gsddmm: op %r needs the rhs operand" % op)
    expect = {"u": gidx.num_src, "v": gidx.num_dst, "e": gidx.num_edges()}
    for t, tgt, name in ((L, lhs_target, "lhs"), (R, rhs_target, "rhs")):
        if t is not None and t.shape[0] != expect[tgt]:
            raise DGLError("gsddmm: %s has %d rows, target %r has %d" % (name, t.shape[0], tgt, expect[tgt]))
    lshape = tuple(L.shape[1:]) if L is not None else ()
    rshape = tuple(R.shape[1:]) if R is not None else ()
    reduce_size = 1
    if op == "dot":
        if not lshape or not rshape or lshape[-1] != rshape[-1]:
            raise DGLError("gsddmm dot: last dims differ: %s vs %s" % (lshape, rshape))
        reduce_size = lshape[-1]
        oshape, l_tab, r_tab = _bcast_plan(lshape[:-1], rshape[:-1])
        out_len = _prod(oshape)
        oshape = tuple(oshape) + (1,)
    elif L is not None and R is not None:
        oshape, l_tab, r_tab = _bcast_plan(lshape, rshape)
        out_len = _prod(oshape)
    else:
        oshape, l_tab, r_tab = (lshape if L is not None else rshape), None, None
        out_len = _prod(oshape)
    ref = L if L is not None else R
    dev = ref.device
    out = backend_for(ref).sddmm(gidx, op, L, R, lhs_target, rhs_target, _prod(lshape), _prod(rshape), out_len,
                                 reduce_size, _device_table(l_tab, dev), _device_table(r_tab, dev))
    return out.view((gidx.num_edges(),) + tuple(oshape))


def edge_softmax_fwd_raw(csr, z):
    z = _as_f32(z, "edge_softmax logits")
    if z.shape[0] != csr.nnz:
        raise DGLError("edge_softmax: expected %d edge rows, got %d" % (csr.nnz, z.shape[0]))
    a = backend_for(z).edge_softmax_fwd(csr, z.view(z.shape[0], -1))
    return a.view(z.shape)


def edge_softmax_bwd_raw(csr, a, da):
    a, da = _as_f32(a, "edge_softmax out"), _as_f32(da, "edge_softmax grad")
    if a.shape[0] != csr.nnz or tuple(da.shape) != tuple(a.shape):
        raise DGLError("edge_softmax backward: expected two (%d, ...) tensors of one shape, got %s and %s"
                       % (csr.nnz, tuple(a.shape), tuple(da.shape)))
    dz = backend_for(a).edge_softmax_bwd(csr, a.view(a.shape[0], -1), da.view(da.shape[0], -1))
    return dz.view(a.shape)


def segment_reduce_raw(offsets, x, reduce="sum", want_arg=False, total=None):
    """`total`: the caller's host-side sum of the segment lengths, checked against x.shape[0] without a device sync."""
    x = _as_f32(x, "segment_reduce input")
    if total is None:
        total = int(offsets[-1].item()) if offsets.numel() else 0
    if total != x.shape[0]:
        raise DGLError("segment_reduce: segment lengths sum to %d, value has %d rows" % (total, x.shape[0]))
    out, arg = backend_for(x).segment_reduce(offsets, x.view(x.shape[0], -1), reduce, want_arg)
    shape = (offsets.shape[0] - 1,) + tuple(x.shape[1:])
    return out.view(shape), (None if arg is None else arg.view(shape))


def gather_rows_raw(x, idx):
    x = _as_f32(x, "gather_rows input")
    out = backend_for(x).gather_rows(x.view(x.shape[0], -1), idx)
    return out.view((idx.shape[0],) + tuple(x.shape[1:]))


def scatter_add_rows_raw(x, idx, rows):
    """x[idx[i]] += rows[i] in place; idx must be unique."""
    backend_for(x).scatter_add_rows(x.view(x.shape[0], -1), idx, _as_f32(rows, "rows").view(rows.shape[0], -1))
    return x
