"""CPU tests of oracle/layout_ref.py, the numpy model of the sweep-order pair layout (csrc/vrt_device.h: pair_block_at,
pair_index): that it is a layout at all (a bijection), that it is the one the header describes (blocks of B pairs, then
the set bits of the remainder, widest first), and the properties the kernels rely on without checking them -- blocks of
two or more pairs start at an even pair and at an even pair element (update_units_f32<2> and k_patch_quad take two
neighbouring float pairs as one 16-byte access), and no block straddles a multiple of 32 pairs (k_to_sweep_order and
k_combine_J walk a tile of 64 wavelengths = 32 pairs block by block).  The third hand copy of the index formula,
FormalPlan.native_to_site_major, is held to the model on random data, without loading the library."""
import numpy as np
import pytest

from oracle import layout_ref as lr
from voronoirt_amd import api

BLOCKS = [1, 2, 4, 8, 16]
SITES = [1, 5, 64, 67]
NPAIRS = range(1, 131)


def _expected_widths(npair, B):
    """the header's words, written out: B repeated, then the set bits of the remainder from the widest down"""
    widths, r, bit = [B] * (npair // B), npair % B, B // 2
    while bit:
        if r & bit:
            widths.append(bit)
        bit //= 2
    return widths


@pytest.mark.parametrize("B", BLOCKS)
def test_block_widths_are_B_repeated_then_the_set_bits_of_the_remainder(B):
    for npair in NPAIRS:
        w = lr.block_widths(npair, B)
        assert w == _expected_widths(npair, B), (npair, B, w)
        assert sum(w) == npair
        tail = w[npair // B:]
        assert all(x < B and x & (x - 1) == 0 for x in tail) and tail == sorted(set(tail), reverse=True), (npair, B, w)
    assert lr.block_widths(26, 8) == [8, 8, 8, 2]


@pytest.mark.parametrize("n", SITES)
@pytest.mark.parametrize("B", BLOCKS)
def test_pair_index_is_a_bijection_with_consecutive_blocks(B, n):
    p = np.arange(n)
    for npair in NPAIRS:
        idx = lr.pair_index(np.arange(npair)[None, :], p[:, None], n, B, npair)             # (n, npair)
        assert np.array_equal(np.sort(idx.ravel()), np.arange(npair * n)), (npair, B, n)
        k = 0
        for w in lr.block_widths(npair, B):
            blk = idx[:, k:k + w]
            # the w pairs of a position are consecutive, position p + 1 follows at + w, the block starts at k n
            assert np.array_equal(blk, k * n + p[:, None] * w + np.arange(w)[None, :]), (npair, B, n, k, w)
            if w >= 2:
                assert k % 2 == 0 and not (blk[:, 0] & 1).any(), (npair, B, n, k, w)
            # the block lies inside one tile of 32 pairs
            assert k // 32 == (k + w - 1) // 32, (npair, B, k, w)
            k += w
        assert k == npair


def test_pair_index_takes_scalars_and_refuses_pairs_outside_the_plane():
    assert lr.pair_index(0, 0, 7, 8, 26) == 0
    assert lr.pair_index(25, 3, 7, 8, 26) == 24 * 7 + 3 * 2 + 1 and isinstance(lr.pair_index(25, 3, 7, 8, 26), int)
    for q in (-1, 26):
        with pytest.raises(IndexError):
            lr.pair_index(q, 0, 7, 8, 26)
    with pytest.raises(ValueError):
        lr.pair_index(0, 0, 7, 3, 26)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", BLOCKS)
def test_planes_round_trip_every_bit_and_pad_with_plus_zero(B, dtype):
    rng = np.random.default_rng(B)
    u = np.uint64 if dtype == np.float64 else np.uint32
    for n, nlam in ((5, 1), (67, 2), (67, 7), (64, 33), (5, 129), (67, 52)):
        rows = rng.integers(0, np.iinfo(u).max, (n, nlam), dtype=u, endpoint=True).view(dtype)
        order = rng.permutation(n)
        planes = lr.to_planes(rows, order, B, dtype)
        npair = (nlam + 1) // 2
        assert planes.dtype == dtype and planes.shape == (2 * npair * n,)
        back = lr.from_planes(planes, order, nlam, B)
        assert np.array_equal(back.view(u), rows.view(u)), (B, n, nlam)
        if nlam & 1:
            pad = 2 * lr.pair_index(npair - 1, np.arange(n), n, B, npair) + 1
            assert not planes.view(u)[pad].any()
            rest = np.delete(planes.view(u), pad)
        else:
            rest = planes.view(u)
        assert np.array_equal(np.sort(rest), np.sort(rows.view(u).ravel()))
        # one spot by hand: wavelength l of the site at position p
        p, l = n // 2, nlam - 1
        assert planes.view(u)[2 * lr.pair_index(l // 2, p, n, B, npair) + l % 2] == rows.view(u)[order[p], l]


def test_combine_and_alpha_native():
    rng = np.random.default_rng(1)
    n, nlam, B = 67, 7, 4
    ou, od = rng.permutation(n), rng.permutation(n)
    a, b = rng.random((n, nlam)), rng.random((n, nlam))
    a[0, 0], b[0, 0], a[1, 1], b[2, 2] = -0.0, -0.0, -0.0, np.inf
    Ju, Jd = lr.to_planes(a, ou, B, np.float64), lr.to_planes(b, od, B, np.float64)
    J = lr.combine(Ju, Jd, ou, od, nlam, B, np.float64)
    assert np.array_equal(J, a + b) and np.signbit(J[0, 0]) and not np.signbit(J[1, 1])
    up = lr.combine(Ju, None, ou, od, nlam, B, np.float64)
    assert np.array_equal(up, a) and not np.signbit(up).any()           # -0 + (+0) = +0
    assert np.array_equal(lr.combine(None, Jd, ou, od, nlam, B, np.float64), b)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    J32 = lr.combine(lr.to_planes(a32, ou, B, np.float32), lr.to_planes(b32, od, B, np.float32), ou, od, nlam, B, np.float32)
    assert J32.dtype == np.float32 and np.array_equal(J32, (a32.astype(np.float64) + b32.astype(np.float64)).astype(np.float32))
    al = rng.random((3, n, nlam))
    nat = lr.alpha_native(al, [ou, od, ou], B, np.float64)
    per = 2 * ((nlam + 1) // 2) * n
    assert nat.shape == (3 * per,)
    for k, o in enumerate((ou, od, ou)):
        assert np.array_equal(lr.from_planes(nat[k * per:(k + 1) * per], o, nlam, B), al[k])


class _Stand:
    """what FormalPlan.native_to_site_major reads of a plan: the site count and the two pair-block properties"""

    def __init__(self, n, B):
        self.sites = type("sites", (), {"n": n})
        self.native_pair_block = self.native_pair_block_f32 = B


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", BLOCKS)
def test_native_to_site_major_is_the_model(B, dtype):
    """rows in STORAGE order of each angle: from_planes with the identity order"""
    rng = np.random.default_rng(10 + B)
    for n, nlam, A in ((5, 1, 1), (67, 7, 2), (64, 52, 3), (67, 129, 2), (5, 33, 1)):
        npair = (nlam + 1) // 2
        native = rng.random(A * 2 * npair * n).astype(dtype)
        got = api.FormalPlan.native_to_site_major(_Stand(n, B), native, nlam, A)
        assert got.shape == (A, n, nlam) and got.dtype == dtype
        for a in range(A):
            want = lr.from_planes(native[a * 2 * npair * n:(a + 1) * 2 * npair * n], np.arange(n), nlam, B)
            assert np.array_equal(got[a], want), (B, n, nlam, a)
