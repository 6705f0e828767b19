"""Host restatements of the library's two dropout streams, in numpy uint64 / uint32 with wrapping arithmetic (no torch, no device code):

  relu + dropout (csrc/elementwise.hip, the activation epilogue of csrc/rowsgemm.hip): float4 number i of the DENSE tensor draws
      r0 = splitmix64(seed ^ ((offset + i) * 2)),  r1 = splitmix64(seed ^ ((offset + i) * 2 + 1))          (all modulo 2^64)
  and keeps x, y, z, w when (uint32)r0, r0 >> 32, (uint32)r1, r1 >> 32 are >= drop_below = min(uint32(double(float32(p)) * 2^32), 2^32 - 1).
  An eager call number k sits at offset (k * 0x9E3779B97F4A7C15) & (2^63 - 1) (ops._dropout_stream_position); the counter entry
  point reads a device counter c and takes ((c * 0x9E3779B97F4A7C15) mod 2^64) & (2^63 - 1).

  attention dropout of the fused GAT row kernels (csrc/gatfused.hip): edge e, head h is kept when gat_hash(seed, e, h) >= drop_below,
  e the EDGE ID (eids[q] of CSR position q; q itself without eids); call number k uses seed = torch seed ^ (k * 0x9E3779B97F4A7C15 mod 2^64).

Seeds are NOT independent streams, by construction: the seed enters by xor with the counter, so `seed` and `seed ^ d` draw the same
numbers at counters c and c ^ d.  Seeds 0 and 1 swap the (x, y) and (z, w) halves of every float4; seeds 0 and 2 swap neighbouring
float4s at even offsets.  The tests built on this module therefore do not test cross-seed independence; changing it would change
every recorded trajectory."""
import numpy as np

STEP = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
M63 = (1 << 63) - 1
_U64 = np.uint64
_U32 = np.uint32


def splitmix64(z):
    """csrc/common.h splitmix64: one step of the generator from state z (any shape, wrapping uint64)."""
    z = np.asarray(z, dtype=_U64)
    with np.errstate(over="ignore"):
        z = z + _U64(STEP)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def drop_below(p):
    """The threshold the entry points compute from their `float p` argument."""
    thr = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if thr >= 4294967295.0 else int(thr)


def keep_scale(p):
    """1 / (1 - p) as the entry points round it: float32 arithmetic on the float32 argument."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def relu_dropout_keep(seed, offset, n4, p):
    """bool [n4, 4]: element (i, j) is the keep bit of component j (x, y, z, w) of dense float4 number i."""
    i = np.arange(n4, dtype=_U64)
    with np.errstate(over="ignore"):
        c = (_U64(int(offset) & M64) + i) * _U64(2)
        r0 = splitmix64(_U64(int(seed) & M64) ^ c)
        r1 = splitmix64(_U64(int(seed) & M64) ^ (c + _U64(1)))
    lo = _U64(0xFFFFFFFF)
    bits = np.stack([r0 & lo, r0 >> _U64(32), r1 & lo, r1 >> _U64(32)], axis=1)
    return bits >= _U64(drop_below(p))


def counter_offset(counter):
    return ((int(counter) * STEP) & M64) & M63


def call_offset(k):
    return (int(k) * STEP) & M63


def gat_hash(seed, klo, khi):
    """csrc/gatfused.hip gat_hash: uint32 mixer of (seed, two 32-bit key words); broadcasts over klo / khi."""
    seed = int(seed) & M64
    klo, khi = np.asarray(klo).astype(_U32), np.asarray(khi).astype(_U32)
    with np.errstate(over="ignore"):
        x = klo ^ _U32(seed & 0xFFFFFFFF)
        x = x ^ (x >> _U32(16))
        x = x * _U32(0x7FEB352D)
        x = x ^ (x >> _U32(15))
        x = x ^ (khi + _U32(seed >> 32))
        x = x * _U32(0x846CA68B)
        return x ^ (x >> _U32(16))


def gat_edge_keep(seed, num_edges, H, p):
    """bool [E, H]: the row kernels' attn_drop mask, keyed (edge id, head)."""
    e = np.arange(num_edges, dtype=_U32)[:, None]
    h = np.arange(H, dtype=_U32)[None, :]
    return gat_hash(seed, e, h) >= _U32(drop_below(p))


def gat_call_seed(torch_seed, k):
    return (int(torch_seed) & M64) ^ ((int(k) * STEP) & M64)


def relu_positive(x):
    """The kernels' relu test, !(x <= 0): true for positive values, +Inf and NaN."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(x) <= 0)


def mask_bytes(keep, x):
    """uint8 [n4]: the mask the kernels store for a dense float32 tensor x of 4 * n4 elements: bit j of byte i is element 4 i + j,
    set when it is kept AND passes the relu test."""
    k = keep & relu_positive(x).reshape(-1, 4)
    return (k[:, 0] * 1 + k[:, 1] * 2 + k[:, 2] * 4 + k[:, 3] * 8).astype(np.uint8)


def mask_bits(mask, shape):
    """bool `shape`: the bits of stored mask bytes, one per element."""
    m = np.asarray(mask, dtype=np.uint8)
    return np.stack([(m >> j) & 1 for j in range(4)], axis=1).astype(bool).reshape(shape)


def relu_dropout_reference(x, seed, offset, p):
    """(y, mask bytes) of relu + dropout on a dense float32 array x (numel % 4 == 0) at (seed, offset)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    keep = relu_dropout_keep(seed, offset, x.size // 4, p)
    m = mask_bytes(keep, x)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.where(mask_bits(m, x.shape), x * keep_scale(p), np.float32(0.0)).astype(np.float32)
    return y, m
