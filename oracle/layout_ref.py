"""Test infrastructure (like everything under oracle/): ONE numpy model of the sweep-order ("native") pair layout of
voronoirt_amd/csrc/vrt_device.h (pair_block_at, pair_index) and of the layout changes of vrt_layout_kernels.h that
write and read it.  tests/test_layout_host.py checks the model's own properties, tests/test_layout_domain.py holds the
kernels to it bit for bit.

The layout: a plane set holds npair = ceil(nλ / 2) wavelength PAIRS of n storage positions, 2 npair n values.  The
pairs sit in blocks: blocks of B pairs, then -- when B does not divide npair -- one block per set bit of the remainder,
widest first (26 pairs, B = 8: 8, 8, 8, 2).  Pair q of position p, in the block [k0, k0 + w) that holds q, is pair
element k0 n + p w + (q - k0); wavelength l is value 2 pair_index(l / 2, p) + l % 2.  An odd nλ leaves one pad value per
position, written as +0.

Every function moves BIT PATTERNS (unsigned views), so NaN payloads, -0 and subnormals pass through unchanged; the one
addition is in combine()."""
import numpy as np

_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}


def _block_table(npair: int, B: int):
    """(k0, w) of every pair q < npair: the first pair and the width of its block, as pair_block_at finds them"""
    if npair < 1 or B < 1 or B & (B - 1):
        raise ValueError("need npair >= 1 and B a power of two")
    k0, w = np.empty(npair, dtype=np.int64), np.empty(npair, dtype=np.int64)
    full = npair // B * B
    q = np.arange(full)
    k0[:full], w[:full] = q // B * B, B
    k, r, bit = full, npair - full, B >> 1
    while bit:                                  # the remainder: one block per set bit, widest first
        if r & bit:
            k0[k:k + bit], w[k:k + bit] = k, bit
            k += bit
        bit >>= 1
    assert k == npair
    return k0, w


def block_widths(npair: int, B: int) -> list:
    """widths of the blocks of a plane set, in storage order"""
    k0, w = _block_table(npair, B)
    starts = np.flatnonzero(np.concatenate([[True], k0[1:] != k0[:-1]]))
    return [int(x) for x in w[starts]]


def pair_index(q, p, n: int, B: int, npair: int):
    """pair element of pair q at storage position p (scalars or arrays, broadcast); IndexError for a q outside the plane"""
    k0, w = _block_table(npair, B)
    q, p = np.asarray(q, dtype=np.int64), np.asarray(p, dtype=np.int64)
    if q.size and (q.min() < 0 or q.max() >= npair):
        raise IndexError("pair outside the plane set")
    out = k0[q] * n + p * w[q] + (q - k0[q])
    return int(out) if out.ndim == 0 else out


def _value_index(n: int, nl: int, B: int, npair: int):
    """(n, nl) value indices of wavelength l < nl at position p"""
    l = np.arange(nl)
    return 2 * pair_index((l >> 1)[None, :], np.arange(n)[:, None], n, B, npair) + (l & 1)[None, :]


def to_planes(rows, order, B: int, dtype):
    """(n, nlam) caller rows (row = site) + the 0-based site of every storage position -> the flat plane set, pad = +0"""
    dtype = np.dtype(dtype)
    rows = np.ascontiguousarray(rows, dtype=dtype)
    order = np.asarray(order, dtype=np.int64)
    n, nlam = rows.shape
    npair = (nlam + 1) // 2
    out = np.zeros(2 * npair * n, dtype=_UINT[dtype])
    out[_value_index(n, nlam, B, npair)] = rows.view(_UINT[dtype])[order]
    return out.view(dtype)


def from_planes(planes, order, nlam: int, B: int):
    """the flat plane set -> (n, nlam) caller rows"""
    planes = np.ascontiguousarray(planes)
    order = np.asarray(order, dtype=np.int64)
    n, npair = order.size, (nlam + 1) // 2
    if planes.size != 2 * npair * n:
        raise ValueError("plane set of the wrong size")
    u = _UINT[planes.dtype]
    out = np.empty((n, nlam), dtype=u)
    out[order] = planes.view(u)[_value_index(n, nlam, B, npair)]
    return out.view(planes.dtype)


def combine(J_up, J_dn, order_up, order_dn, nlam: int, B: int, dtype):
    """J (n, nlam) = J_up + J_down of the two directions' plane sets (either None: a direction without angles, which
    counts as +0 planes -- 0.0 + x).  fp64: the double sum; fp32: float32(float64(a) + float64(b))."""
    dtype = np.dtype(dtype)
    if J_up is None and J_dn is None:
        raise ValueError("no direction")
    rows = [None if J is None else from_planes(np.ascontiguousarray(J, dtype=dtype), o, nlam, B).astype(np.float64)
            for J, o in ((J_up, order_up), (J_dn, order_dn))]
    zero = np.zeros_like(rows[0] if rows[0] is not None else rows[1])
    with np.errstate(invalid="ignore", over="ignore"):
        return ((zero if rows[0] is None else rows[0]) + (zero if rows[1] is None else rows[1])).astype(dtype)


def alpha_native(alpha, orders_per_angle, B: int, dtype):
    """(n_angles, n, nlam) per-angle alpha + each angle's storage order -> the native per-angle buffer (one plane set
    per angle, back to back)"""
    return np.concatenate([to_planes(a, o, B, dtype) for a, o in zip(alpha, orders_per_angle)])
