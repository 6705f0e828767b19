"""Operand layouts for tests/test_operand_layouts.py: the ways a caller can hand an operator the SAME values.

Every layout is a pair (shape of the backing buffer, how the operand is carved out of it).  make(name, v) allocates the buffer, fills it
with a guard value (NaN for floats, GUARD_INT for integers), carves the view and writes v through it, so the view's values equal the
dense v and every element of the buffer the view does not cover still holds the guard:

    dense         a fresh contiguous tensor (the baseline)
    offset4       contiguous, one element into a flat buffer: data_ptr() % 16 == 4 for 4-byte elements
    colblock      columns [4, 4 + W) of a [n, W + 8] matrix (W = the product of the feature dims, viewed back to the feature shape): the
                  rows are W + 8 apart, the base is 16-byte aligned
    colblock_off  columns [1, 1 + W) of a [n, W'] matrix, W' the least multiple of 4 that is at least W + 1: the row stride is a multiple
                  of 4 elements, the base is 4 bytes off
    alt_rows      big[::2]
    transposed    v.transpose(0, -1).contiguous().transpose(0, -1); a 1-D operand has no such layout (LayoutError)
    expanded      one stored row, stride 0 along the rows (row.expand(n, ...)); only for values whose rows are all equal (LayoutError)

Laid.unchanged(snapshot) compares the WHOLE buffer bit for bit with a copy taken before the call: the operand is unchanged and every
guard element is still the guard (a kernel that writes with an assumed stride, or into an operand, shows here)."""
import torch

NAMES = ("dense", "offset4", "colblock", "colblock_off", "alt_rows", "transposed", "expanded")
GUARD_INT = -7


class LayoutError(ValueError):
    """The layout cannot be formed for this operand."""


def _prod(shape):
    p = 1
    for s in shape:
        p *= int(s)
    return p


def _width(shape):
    return _prod(shape[1:])


def _transposed_alloc(shape):
    if len(shape) < 2:
        raise LayoutError("a 1-D operand has no second dimension to transpose")
    return (shape[-1],) + tuple(shape[1:-1]) + (shape[0],)


_LAYOUTS = {
    "dense": (lambda s: tuple(s), lambda buf, s: buf),
    "offset4": (lambda s: (_prod(s) + 2,), lambda buf, s: buf[1:1 + _prod(s)].view(s)),
    "colblock": (lambda s: (s[0], _width(s) + 8), lambda buf, s: buf[:, 4:4 + _width(s)].view(s)),
    "colblock_off": (lambda s: (s[0], (_width(s) + 1 + 3) // 4 * 4), lambda buf, s: buf[:, 1:1 + _width(s)].view(s)),
    "alt_rows": (lambda s: (2 * s[0],) + tuple(s[1:]), lambda buf, s: buf[::2]),
    "transposed": (_transposed_alloc, lambda buf, s: buf.transpose(0, -1)),
    "expanded": (lambda s: (1,) + tuple(s[1:]), lambda buf, s: buf.expand(s)),
}


class Laid(object):
    """view: the operand; buf: its backing buffer; guard: bool mask over buf.reshape(-1) of the elements the view does not cover."""
    __slots__ = ("name", "view", "buf", "guard")

    def __init__(self, name, view, buf, guard):
        self.name, self.view, self.buf, self.guard = name, view, buf, guard

    def snapshot(self):
        return self.buf.clone()

    def unchanged(self, snap):
        """the buffer, guards included, holds the bits of `snap`"""
        a, b = self.buf.reshape(-1), snap.reshape(-1)
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        return bool(torch.equal(a, b))

    def guards_hold(self):
        g = self.buf.reshape(-1)[self.guard]
        return bool(torch.isnan(g).all()) if g.is_floating_point() else bool((g == GUARD_INT).all())


def make(name, v, device=None):
    """Laid: `v` (a dense tensor) in layout `name` on `device` (default: v's)."""
    shape, device = tuple(int(s) for s in v.shape), v.device if device is None else device
    alloc, carve = _LAYOUTS[name]
    fill = float("nan") if v.is_floating_point() else GUARD_INT
    buf = torch.full(alloc(shape), fill, dtype=v.dtype, device=device)
    view = carve(buf, shape)
    if name == "expanded":
        if shape[0] < 1 or not bool((v == v[:1]).all()):
            raise LayoutError("rows must be equal")
        buf.copy_(v[:1])
    else:
        view.copy_(v)
    ids = carve(torch.arange(buf.numel()).view(buf.shape), shape)
    guard = torch.ones(buf.numel(), dtype=torch.bool)
    guard[ids.reshape(-1)] = False
    assert tuple(view.shape) == shape and view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    return Laid(name, view, buf, guard.to(device))


def describe(t):
    return "shape %s strides %s base %% 16 = %d" % (tuple(t.shape), tuple(t.stride()), t.data_ptr() % 16)


def as_named(name, laid, shape):
    """None when laid.view has the strides and the base its layout's name promises, else what is wrong (the helpers' self-check)."""
    v, W = laid.view, _width(shape)
    n, es = shape[0], v.element_size()
    want = {
        "dense": v.is_contiguous() and v.data_ptr() % 16 == 0,
        "offset4": v.is_contiguous() and v.data_ptr() % 16 == es,
        "colblock": v.stride(0) == W + 8 and v.data_ptr() % 16 == (4 * es) % 16 and (n < 2 or not v.is_contiguous()),
        "colblock_off": v.stride(0) % 4 == 0 and v.stride(0) >= W + 1 and v.data_ptr() % 16 == es and (n < 2 or not v.is_contiguous()),
        "alt_rows": v.stride(0) == 2 * W and v.data_ptr() % 16 == 0,
        # the rows run along the LAST stored dimension (stride 1), the last dimension along the first (everything stored after it)
        "transposed": len(shape) >= 2 and v.stride(0) == 1 and v.stride(-1) == n * _prod(shape[1:-1]) and v.data_ptr() % 16 == 0,
        "expanded": v.stride(0) == 0 and laid.buf.shape[0] == 1,
    }
    return None if want[name] else describe(v)
