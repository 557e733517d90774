"""Host tests of the J reduction that rides in the patch blocks of a per-layer launch (option VRT_PATCH_REDUCE_RIDE,
voronoirt_amd/csrc/vrt_patch.hip: ride_fits, ride_chunks_of, ride_slice -- the one slice map the launcher and every
per-layer kernel go through).  vrt_patch_ride_map walks the blocks of a launch's patch grid with those very functions and
reports which pair elements of the plane set [npair][n] each thread of each block reduces.

What must hold: every pair element of every range -- pair block after pair block the run of (hi - lo) << lw elements from
k0 n + (lo << lw), the layout of vrt_device.h: pair_block_of -- is reduced exactly once, nothing outside the ranges is
touched, no thread takes more than four elements, a chunk never mixes the two ranges (its angle list is the workgroup's),
and a launch whose patch grid cannot take the ranges at four chunks per block says that it keeps its reduction rows."""
import ctypes
import itertools

import numpy as np
import pytest

from voronoirt_amd import _lib

R1 = 1 << 62


def _ride(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo, hi, first=0, count=None):
    lib = _lib.load()
    dims = (ctypes.c_int64 * 4)()
    lo_a, hi_a = (ctypes.c_int32 * 2)(*lo), (ctypes.c_int32 * 2)(*hi)
    rc = lib.vrt_patch_ride_map(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo_a, hi_a, 0, 0, dims, None)
    assert rc == 0, lib.vrt_last_error()
    blocks, c0, c1, rides = (int(v) for v in dims)
    if not rides:
        return blocks, c0, c1, False, None
    count = blocks - first if count is None else count
    elems = np.full((count, 4, nt), -2, dtype=np.int64)
    rc = lib.vrt_patch_ride_map(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo_a, hi_a, first, count, dims, elems.ctypes.data_as(_lib.p_i64))
    assert rc == 0, lib.vrt_last_error()
    return blocks, c0, c1, True, elems


def _pair_blocks(npair, lgb):
    """(first pair, log2 width) of the pair blocks: full blocks, then the bits of the rest, widest first"""
    out, k0 = [], 0
    for _ in range(npair >> lgb):
        out.append((k0, lgb))
        k0 += 1 << lgb
    rest = npair - k0
    for bit in range(lgb - 1, -1, -1):
        if rest & (1 << bit):
            out.append((k0, bit))
            k0 += 1 << bit
    assert k0 == npair
    return out


def _expected(npair, lgb, n, lo, hi):
    """the plane-set indices of range [lo, hi): per pair block one contiguous run"""
    runs = [np.arange(k0 * n + (lo << lw), k0 * n + (hi << lw), dtype=np.int64) for k0, lw in _pair_blocks(npair, lgb)]
    return np.concatenate(runs) if runs else np.zeros(0, dtype=np.int64)


def _check_whole_launch(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo, hi):
    blocks, c0, c1, rides, elems = _ride(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo, hi)
    lens = [hi[r] - lo[r] for r in range(2)]
    assert (c0, c1) == tuple(-(-lens[r] * npair // nt) for r in range(2))
    assert rides == (0 < c0 + c1 <= 4 * blocks)
    if not rides:
        return blocks, False
    assert elems.shape == (blocks, 4, nt) and (elems >= -1).all()
    got = elems[elems >= 0]
    for r in range(2):
        mine = np.sort(got[(got >= R1) == bool(r)] & (R1 - 1))
        want = np.sort(_expected(npair, lgb, n, lo[r], hi[r]))
        assert mine.size == want.size and np.array_equal(mine, want), (r, mine.size, want.size)     # each once, none outside
    # a chunk (block, round) holds elements of one range only, and the rounds of a block fill up in order
    for b in range(blocks):
        used = [(elems[b, i] >= 0).any() for i in range(4)]
        assert used == sorted(used, reverse=True)
        for i in range(4):
            e = elems[b, i][elems[b, i] >= 0]
            assert e.size == 0 or (e >= R1).all() or (e < R1).all()
    return blocks, True


GRIDS = [(0, 1, 1, 0), (1, 1, 1, 0), (0, 2, 3, 0), (1, 2, 3, 0), (1, 3, 2, 1), (0, 1, 5, 1)]      # order, rows, splits, log2 siblings


@pytest.mark.parametrize("order,nrow,nsplit,lgs", GRIDS)
@pytest.mark.parametrize("npair,lgb", [(1, 0), (4, 0), (7, 1), (13, 3), (16, 3), (3, 3)])
def test_every_element_once(order, nrow, nsplit, lgs, npair, lgb):
    """both dispatch orders, one split and several, pair-block widths 1, 2 and 8 with shrinking last blocks (13 = 8 + 4 + 1,
    7 = 2 + 2 + 2 + 1, 3 in blocks of 8 = 2 + 1); element counts below the block count (some blocks get nothing), not a
    multiple of the chunk, and two ranges in one launch"""
    nt, n = 64, 5000
    for lo, hi in (((10, 0), (13, 0)),                       # 3 sites: fewer elements than blocks
                   ((0, 0), (333, 0)),                       # not a multiple of the chunk
                   ((5, 400), (205, 1001)),                  # two ranges
                   ((0, 4999), (1, 5000))):                  # the grid's first and last site
        blocks, rides = _check_whole_launch(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo, hi)
        assert blocks == 8 * nrow * (nsplit << lgs)
        total = sum(-(-(hi[r] - lo[r]) * npair // nt) for r in range(2))
        assert rides == (total <= 4 * blocks)


def test_a_launch_that_is_full_and_one_that_keeps_its_rows():
    """exactly 4 x NT x blocks elements ride; one more keeps the reduction rows"""
    nt, npair = 64, 4
    for order, nrow, nsplit, lgs in GRIDS:
        blocks = 8 * nrow * (nsplit << lgs)
        full = 4 * nt * blocks // npair                      # sites whose npair pairs fill four chunks per block exactly
        got_blocks, rides = _check_whole_launch(order, nrow, nsplit, lgs, npair, 2, nt, full + 10, (0, 0), (full, 0))
        assert got_blocks == blocks and rides
        _, c0, _, rides, elems = _ride(order, nrow, nsplit, lgs, npair, 2, nt, full + 10, (0, 0), (full, 0))
        assert c0 == 4 * blocks and (elems >= 0).all()       # every thread of every block holds four elements
        _, c0, _, rides, elems = _ride(order, nrow, nsplit, lgs, npair, 2, nt, full + 10, (0, 0), (full + 1, 0))
        assert c0 == 4 * blocks + 1 and not rides and elems is None
    # nothing to reduce: no riding either
    assert _ride(1, 2, 3, 0, 4, 2, 64, 100, (0, 0), (0, 0))[3] is False


def test_splits_with_empty_shares_and_padding_blocks_take_their_slices():
    """the map knows blocks, not items: with more splits than an item has pair steps to give (the launcher caps the splits
    at the steps, a sibling past a narrow block gets nothing) every block of the grid still has its slice"""
    order, nrow, nsplit, lgs, nt, npair, lgb, n = 1, 1, 7, 2, 128, 5, 2, 3000        # 5 pairs = 4 + 1: siblings 1-3 idle on the last block
    blocks, rides = _check_whole_launch(order, nrow, nsplit, lgs, npair, lgb, nt, n, (0, 0), (2999, 0))
    assert rides and blocks == 8 * 7 * 4
    _, _, _, _, elems = _ride(order, nrow, nsplit, lgs, npair, lgb, nt, n, (0, 0), (2999, 0))
    assert (elems[:, 0, 0] >= 0).sum() == min(blocks, -(-2999 * npair // nt))


def test_reciprocals_at_the_largest_counts():
    """the quotient by a range's length (multiply-high and one correction) at the largest element count a launch admits --
    just under 2^31 pair elements -- on the largest share-major grid (65 535 rows): the last blocks' elements, and the
    blocks around every pair-block boundary, are the ones a division gives"""
    nt, n = 1024, (1 << 28) - 1
    for length, npair, lgb in ((n, 7, 2), (3, 7, 1), (1, 13, 3), (65537, 32767, 4), (n - 5, 8, 3)):
        if length * npair > (1 << 31) - 1 - 4096:
            npair = ((1 << 31) - 1 - 4096) // length
        lo, hi = (n - length, 0), (n, 0)
        order, nrow, nsplit, lgs = 1, 13107, 5, 4            # 5 x 13107 = 65 535 rows of 128 blocks
        blocks, c0, _, rides, _ = _ride(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo, hi, 0, 0)
        assert blocks == 65535 * 128 and rides and c0 == -(-length * npair // nt)
        probe = {0, 1, blocks - 1, (c0 - 1) % blocks, c0 % blocks}
        for k0, lw in _pair_blocks(npair, lgb)[:6] + _pair_blocks(npair, lgb)[-6:]:
            f = length * k0                                   # first element of the pair block
            probe |= {(f // nt) % blocks, max(f // nt - 1, 0) % blocks}
        for b in sorted(probe):
            _, _, _, _, elems = _ride(order, nrow, nsplit, lgs, npair, lgb, nt, n, lo, hi, b, 1)
            for i in range(4):
                c = b + i * blocks
                f = c * nt + np.arange(nt, dtype=np.int64)
                ok = (c < c0) & (f < length * npair)
                q = np.where(ok, f, 0) // length              # the element's pair
                want = np.full(nt, -1, dtype=np.int64)
                for j in np.flatnonzero(ok):
                    k0, lw = next((k, w) for k, w in _pair_blocks(npair, lgb) if k <= q[j] < k + (1 << w)) if npair < 64 else _block_of(int(q[j]), npair, lgb)
                    want[j] = k0 * n + (lo[0] << lw) + (int(f[j]) - length * k0)
                assert np.array_equal(elems[0, i], want), (length, npair, b, i)


def _block_of(q, npair, lgb):
    full = npair >> lgb << lgb
    if q < full:
        return q >> lgb << lgb, lgb
    k, rest = full, npair - full
    for bit in range(lgb - 1, -1, -1):
        if rest & (1 << bit):
            if q < k + (1 << bit):
                return k, bit
            k += 1 << bit
    raise AssertionError("no such pair")


def test_arguments_are_checked():
    lib = _lib.load()
    dims = (ctypes.c_int64 * 4)()
    lo, hi = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 2)(10, 0)
    assert lib.vrt_patch_ride_map(1, 0, 2, 0, 4, 1, 64, 100, lo, hi, 0, 0, dims, None) == _lib.VRT_EINVAL      # no patch rows: such a launch keeps its rows
    assert lib.vrt_patch_ride_map(1, 2, 2, 0, 4, 1, 96, 100, lo, hi, 0, 0, dims, None) == _lib.VRT_EINVAL      # threads not a power of two
    bad = (ctypes.c_int32 * 2)(101, 0)
    assert lib.vrt_patch_ride_map(1, 2, 2, 0, 4, 1, 64, 100, lo, bad, 0, 0, dims, None) == _lib.VRT_EINVAL     # range outside the grid
    elems = np.zeros((1, 4, 64), dtype=np.int64)
    assert lib.vrt_patch_ride_map(1, 2, 2, 0, 4, 1, 64, 100, lo, hi, 32, 1, dims, elems.ctypes.data_as(_lib.p_i64)) == _lib.VRT_EINVAL   # no such block
