"""Host tests of the dispatch order of the per-layer patch launches (voronoirt_amd/csrc/vrt_patch.hip: patch_grid,
patch_block_of -- the one mapping from a block of the grid to (XCD lane, work-list row, split, sibling) that the launcher
and every per-layer kernel go through; option VRT_PATCH_ORDER).  vrt_patch_dispatch_map walks a launch's whole grid in
its linear order (x first, as the hardware dispatches it) with those very functions and reports what each block does.

Order 0 (interleaved): the workgroups of an item side by side.  Order 1 (share-major): every item's split 0, then every
item's split 1, ...: split_blocks gives the first splits the longer share, so the share must never grow along the
linear order.  In both orders a block's XCD -- its linear index mod 8 -- must be the lane whose work-list column it
reads, every (row, lane, split, sibling) must have exactly one block, and the reduction blocks must lie behind all patch
blocks, numbered in linear order, padded to whole rows."""
import ctypes
import itertools

import numpy as np
import pytest

from voronoirt_amd import _lib


def _map(order, nrow, nsplit, lgs, nred, steps, want_blocks=True):
    dims = (ctypes.c_int64 * 4)()
    lib = _lib.load()
    rc = lib.vrt_patch_dispatch_map(order, nrow, nsplit, lgs, nred, steps, dims, None)
    assert rc == 0, lib.vrt_last_error()
    gx, gy, taken, prow = (int(v) for v in dims)
    if not want_blocks:
        return gx, gy, taken, prow, None
    blocks = np.zeros((gx * gy, 6), dtype=np.int32)
    rc = lib.vrt_patch_dispatch_map(order, nrow, nsplit, lgs, nred, steps, dims, blocks.ctypes.data_as(_lib.p_i32))
    assert rc == 0, lib.vrt_last_error()
    assert (gx, gy, taken, prow) == tuple(int(v) for v in dims)
    return gx, gy, taken, prow, blocks


def _shares(nsplit, steps):
    """what split_blocks deals: the first steps % nsplit splits take one more"""
    return [steps // nsplit + (1 if s < steps % nsplit else 0) for s in range(nsplit)]


CASES = list(itertools.product((0, 1), range(1, 6), range(1, 8), (0, 1), (0, 21)))


@pytest.mark.parametrize("order,nrow,nsplit,lgs,nred", CASES)
def test_every_block_has_its_place(order, nrow, nsplit, lgs, nred):
    nred = (nred + 7) // 8 * 8                       # the launcher rounds the reduction blocks to a multiple of 8
    for steps in (nsplit, nsplit + 1, 2 * nsplit + 3, 3 * nsplit):
        gx, gy, taken, prow, blk = _map(order, nrow, nsplit, lgs, nred, steps)
        assert taken == (order if nsplit >= 2 else 0)
        assert gx % 8 == 0
        if taken == 1:
            assert (gx, prow) == (8 << lgs, nsplit * nrow)
        else:
            assert (gx, prow) == (8 * (nsplit << lgs), nrow)
        assert gy == prow + (nred + gx - 1) // gx
        npatch = prow * gx
        assert npatch == 8 * nrow * (nsplit << lgs)
        patch, red = blk[:npatch], blk[npatch:]
        # the patch blocks: all in front, each (row, lane, split, sibling) exactly once, the lane is the block's XCD
        assert not patch[:, 0].any() and red[:, 0].all()
        keys = {tuple(r) for r in patch[:, 1:5].tolist()}
        assert len(keys) == npatch
        assert keys == set(itertools.product(range(8), range(nrow), range(nsplit), range(1 << lgs)))
        assert np.array_equal(patch[:, 1], np.arange(npatch) % 8)
        # every block carries the share of its split; an item's shares add up to its steps
        share = np.array(_shares(nsplit, steps))
        assert np.array_equal(patch[:, 5], share[patch[:, 3]])
        assert share.sum() == steps and share.max() - share.min() <= 1
        if taken == 1:
            # share-major: the share never grows along the dispatch order, and inside a split the work list's own order
            assert (np.diff(patch[:, 5]) <= 0).all()
            assert (np.diff(patch[:, 3]) >= 0).all()
            lin = np.arange(npatch)
            assert np.array_equal(patch[:, 3], lin // (gx * nrow))
            assert np.array_equal(patch[:, 2], lin // gx % nrow)
            assert np.array_equal(patch[:, 4], lin % gx // 8)          # siblings of a pair block adjacent
        else:
            assert np.array_equal(patch[:, 2], np.arange(npatch) // gx)
        # the reduction blocks: behind, numbered in linear order from 0; at least nred of them, less than a row of padding
        # (a block whose number is >= nred returns at once: patch_reduce_role)
        assert np.array_equal(red[:, 1], np.arange(len(red)))
        assert nred <= len(red) < nred + gx
        assert not red[:, 2:].any()


def test_a_launch_that_only_reduces():
    """the launch behind the last solved layer: no work-list row, reduction rows alone, in either order"""
    for order in (0, 1):
        gx, gy, taken, prow, blk = _map(order, 0, 1, 0, 40, 1)
        assert (taken, prow) == (0, 0) and gx % 8 == 0 and gx * gy >= 40
        assert blk[:, 0].all() and np.array_equal(blk[:, 1], np.arange(gx * gy))


@pytest.mark.parametrize("nrow,nsplit", [(32767, 2), (16383, 4), (9362, 7), (1, 4096), (13, 4096)])
def test_the_split_of_a_row_is_exact_up_to_the_row_limit(nrow, nsplit):
    """the kernel divides a grid row by nrow with a multiply-high: exact for every row a grid can have"""
    gx, gy, taken, prow, blk = _map(1, nrow, nsplit, 0, 0, nsplit)
    assert taken == 1 and gx == 8 and gy == prow == nrow * nsplit <= 65535
    y = np.arange(gy).repeat(8)
    assert np.array_equal(blk[:, 3], y // nrow)
    assert np.array_equal(blk[:, 2], y % nrow)


def test_fallback_at_the_row_limit():
    """share-major order needs nsplit x nrow rows plus the reduction rows: past 65 535 the launch keeps the interleaved
    order instead of failing"""
    # 4 x 16383 = 65 532 rows and three rows of reduction blocks: the last grid that fits
    gx, gy, taken, prow, _ = _map(1, 16383, 4, 0, 24, 4, want_blocks=False)
    assert (taken, gx, gy, prow) == (1, 8, 65535, 65532)
    # one reduction row more: interleaved, 16 383 rows of 32 blocks and one reduction row
    gx, gy, taken, prow, _ = _map(1, 16383, 4, 0, 32, 4, want_blocks=False)
    assert (taken, gx, gy, prow) == (0, 32, 16384, 16383)
    # 4 x 16384 rows of patches alone
    gx, gy, taken, prow, _ = _map(1, 16384, 4, 0, 0, 4, want_blocks=False)
    assert (taken, gx, gy, prow) == (0, 32, 16384, 16384)
    gx, gy, taken, prow, _ = _map(1, 16384, 3, 1, 0, 3, want_blocks=False)
    assert (taken, gx, gy, prow) == (1, 16, 49152, 49152)
    # what no grid holds in either order is refused, as the launcher refuses it
    dims = (ctypes.c_int64 * 4)()
    assert _lib.load().vrt_patch_dispatch_map(1, 65535, 2, 0, 64, 2, dims, None) == _lib.VRT_EINVAL
    assert _lib.load().vrt_patch_dispatch_map(1, 4, 2, 0, 0, 1, dims, None) == _lib.VRT_EINVAL      # fewer steps than splits
    assert _lib.load().vrt_patch_dispatch_map(2, 4, 2, 0, 0, 2, dims, None) == _lib.VRT_EINVAL      # no such order
