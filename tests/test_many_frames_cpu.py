"""No GPU: the premises of tests/test_gpu_many_frames.py and the restatements of many_frames_cases.py.

The pool's premises keep the oracle alone clear of capacity effects (no frame reaches max_pts, so which records a call
keeps is never the append order's business) and make a batch skewed: empty frames, busy ones, and one with a handful of
records.  block_tables is held to the host hook of the share rule, strip_geom to the figures the row-loop test documents,
and every frame count the GPU tests use is shown to reach the second round of the loop it aims at."""
import ctypes as C

import numpy as np
import pytest

import many_frames_cases as mc

CU_COUNTS = (256, 304, 64)          # an MI355X, and two other devices' worth of workgroups for the table sizes


def _capi():
    from cudasift_amd import capi
    return capi


def _premises(wr, max_pts):
    nz = wr[wr > 0]
    assert (wr < max_pts).all(), wr                    # no capacity effects
    assert (wr == 0).any(), wr                         # empty frames
    assert wr.max() >= 200, wr                         # a busy one
    assert wr.max() >= 20 * nz.min(), wr               # skewed


def test_pool_premises():
    assert mc.POOL.shape == (7, mc.H, mc.W) and mc.TALL.shape == (7, mc.TALL_H, mc.W)
    # the textured frames are all different; the two of amplitude 0 are flat (128 everywhere)
    for p in (mc.POOL, mc.TALL):
        flat = [i for i, a in enumerate(mc.AMPS) if a == 0.0]
        assert all((p[i] == 128.0).all() for i in flat)
        assert len({p[i].tobytes() for i in range(mc.NPOOL) if i not in flat}) == mc.NPOOL - len(flat)
    num, wr, det = mc.counts_of(mc.NPOOL)
    _premises(wr, mc.MAX_PTS)
    assert (num <= wr).all() and (det <= num).all()
    # neighbours across a round's edge differ, in content and in count
    for edge in (256, 512, 768, 1024):
        a, b = (edge - 1) % mc.NPOOL, edge % mc.NPOOL
        assert a != b and wr[a] != wr[b], (edge, wr)


def test_pool_premises_8bit_scale_up():
    """The 8-bit frames doubled first hold more records than 512: that case runs at max_pts 1024."""
    kw = dict(u8=True, scale_up=True, max_pts=mc.SCALE_UP_MAX_PTS)
    num, wr, det = mc.counts_of(mc.NPOOL, **kw)
    _premises(wr, mc.SCALE_UP_MAX_PTS)
    assert wr.max() >= mc.MAX_PTS                     # ... and needs the larger capacity


def test_expected_is_cached_and_read_only():
    a, b = mc.expected(0), mc.expected(0)
    assert a[0] is b[0] and not a[0].flags.writeable and not a[2].flags.writeable


def test_canon_is_order_free():
    recs, n, cnt = mc.expected(4)
    w = mc.written(cnt)
    perm = np.random.default_rng(1).permutation(w)
    assert mc.canon(recs[:w]) == mc.canon(recs[:w][perm])
    other = recs[:w].copy()
    other["xpos"][0] = np.nextafter(other["xpos"][0], np.float32(1e9))
    assert mc.canon(recs[:w]) != mc.canon(other)


def _hook_shares(T, counts):
    pts = np.ascontiguousarray(counts, np.uint32)
    out = np.zeros(len(pts), np.int32)
    assert _capi().lib().misift_test_frame_shares(T, len(pts), pts.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("B", mc.TABLE_BATCHES)
@pytest.mark.parametrize("zero", [False, True])
def test_block_tables_against_the_share_hook(B, zero):
    det = np.zeros(B, np.int64) if zero else mc.counts_of(B)[2]
    sizes = {8 * B, B, B + 1}
    for cus in CU_COUNTS:
        sizes |= set(mc.table_sizes(cus, B))
    for T in sorted(sizes):
        tab = mc.block_tables(det, T)
        shares = _hook_shares(T, det)
        assert np.array_equal(mc.shares_of(tab, B), shares), (B, T)
        used = int(shares.sum())
        assert B <= used <= T
        # layout: frames in order, each with rows (f, 0 .. share - 1, share, 0); the rest spare
        assert np.array_equal(tab[:used, 0], np.repeat(np.arange(B), shares))
        starts = np.concatenate([[0], np.cumsum(shares)[:-1]])
        assert np.array_equal(tab[:used, 1], np.arange(used) - np.repeat(starts, shares))
        assert np.array_equal(tab[:used, 2], np.repeat(shares, shares))
        assert (tab[used:] == [-1, 0, 0, 0]).all() and (tab[:, 3] == 0).all()
        if zero:
            assert used == B and (shares == 1).all()
        elif T > 2 * B:
            assert shares.max() > shares.min()            # the batch is skewed: so are the shares


def test_table_sizes_reach_the_floor():
    """On 256 CUs the per-frame floor of 8 workgroups holds from 192 frames (orient_all) and from 256 (descr_all): every
    table batch has T = 8 * B for both launches, i.e. 7 * B rows to deal out."""
    for B in mc.TABLE_BATCHES:
        assert mc.table_sizes(256, B) == (8 * B, 8 * B)
    assert mc.grid_x(256, mc.ORIENT_BLOCKS, 191) == 9 and mc.grid_x(256, mc.ORIENT_BLOCKS, 192) == 8
    assert mc.grid_x(256, mc.POINT_BLOCKS, 255) == 9 and mc.grid_x(256, mc.POINT_BLOCKS, 256) == 8
    assert mc.grid_x(256, mc.POINT_BLOCKS, 2) == 1024 and mc.grid_x(256, mc.POINT_BLOCKS, 5) == 410


def test_strip_geom_against_the_documented_figures():
    """tests/test_gpu_pyramid_rowloop.py: 13 frames of 696 columns (three strips of 60 quads) under strip_waves 1 on 256
    CUs run 24-row segments; at the default they run 8-row ones."""
    assert mc.strip_geom(256, 1, mc.SMALL_FRAMES, 696, 150, mc.PREFILTER_LANES, 13) == (3, 24, 7)
    assert mc.strip_geom(256, mc.STRIP_WAVES_DEFAULT, mc.SMALL_FRAMES, 484, 137, mc.PREFILTER_LANES, 5)[1] == 8
    # the tall case on 256 CUs: want = 1, so the segment would be the whole 136-row frame and is clamped to 128
    assert mc.strip_geom(256, 1, mc.SMALL_FRAMES, mc.W, mc.TALL_H, mc.PREFILTER_LANES, 257) == (1, 128, 2)
    assert mc.strip_geom(256, 1, mc.SMALL_FRAMES, mc.W, mc.TALL_H, mc.PREFILTER_LANES, 256) == (1, 128, 2)
    assert mc.strip_geom(256, 1, mc.SMALL_FRAMES, mc.W, mc.TALL_H, mc.PREFILTER_LANES, 128) == (1, 72, 2)
    # ... and a segment that is the whole frame: the pool's 72 rows, and the tall frames' coarser levels
    assert mc.strip_geom(256, 1, mc.SMALL_FRAMES, mc.W, mc.H, mc.PREFILTER_LANES, 257) == (1, 72, 1)
    assert mc.strip_geom(256, 1, mc.SMALL_FRAMES, mc.W // 2, mc.TALL_H // 2, mc.STREAM_LANES, 257) == (1, 72, 1)
    # the default: 8-row segments, the largest item count
    assert mc.strip_geom(256, mc.STRIP_WAVES_DEFAULT, mc.SMALL_FRAMES, mc.W, mc.TALL_H, mc.PREFILTER_LANES, 257) == (1, 8, 17)
    for cus in CU_COUNTS:
        b = mc.smallest_batch_with(cus, 1, mc.W, mc.TALL_H, mc.PREFILTER_LANES, 128, 2)
        assert b == max(cus, mc.SHARE_ROUND + 1), (cus, b)


def test_every_gpu_case_reaches_its_second_round():
    for B in mc.TABLE_BATCHES:
        assert mc.rounds(B, mc.SHARE_ROUND) >= 2
    assert [mc.rounds(B, mc.SHARE_ROUND) for B in mc.TABLE_BATCHES] == [2, 3, 5]
    assert [mc.rounds(B, mc.COUNT_ROUND) for B in mc.PACKED_BATCHES] == [1, 2, 2]     # the full round, then beyond it
    assert sum(mc.rounds(B, mc.COUNT_ROUND) >= 2 for B in mc.PACKED_BATCHES) >= 2
    assert all(mc.rounds(B, mc.COUNT_ROUND) >= 2 for B in mc.PIPE_BATCHES)
    assert mc.rounds(mc.TALL_BATCH, mc.SHARE_ROUND) >= 2
    big = max(mc.USED_CONTEXT)
    assert mc.rounds(big, mc.COUNT_ROUND) >= 2 and min(mc.USED_CONTEXT) <= 8 < 256 < big
    assert mc.rounds(mc.USED_CONTEXT[-1], mc.COUNT_ROUND) >= 2


def test_hooks_refuse_a_missing_context():
    L = _capi().lib()
    out = np.zeros(4, np.int32)
    a, b = C.c_int(0), C.c_int(0)
    assert L.misift_test_strip_geom(None, 96, 72, 96, 257, 96, 72, 60, out.ctypes.data) != 0
    assert b"misift_test_strip_geom" in L.misift_last_error()
    assert L.misift_test_block_maps(None, C.byref(a), C.byref(b), out.ctypes.data, 1) != 0
    assert b"misift_test_block_maps" in L.misift_last_error()
