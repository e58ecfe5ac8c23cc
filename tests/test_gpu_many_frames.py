"""Extraction on batches of hundreds to a thousand frames, against the oracle.

What changes with the frame count alone, and had never run in a test (the largest batch elsewhere is 64 frames):

  frame_shares_body       the block tables of a balanced batch, built by one workgroup in rounds of 256 frames with a
                          carry from round to round — as the extra workgroup of bin_detections and, under the knob
                          bin = 0, as frame_shares_kernel; and T = 8 x frames once the per-frame floor holds
  export_counts_kernel    counts and offsets of the packed path and of the pipe, in rounds of 1024 frames with a carry
  make_geom / scan        the segment height: the 128-row clamp (126 rows in the scan) and a segment that is the whole
                          frame, once frames x strips covers the CUs
  grids with the frame on y or z, and the per-frame arrays of a context that grow with the largest call so far

The frames are many_frames_cases' pool of seven 96 x 72 frames, frame f = pool frame f % 7.  The first occurrence of a
pool frame in a call goes through util.compare_points against the oracle, with its numPts and 17 counters equal; every
later occurrence must hold the same records as the first (canonical order, byte for byte), so a 1030-frame comparison
costs a sort per frame.  Every context is a guarded one with poisoned outputs: behind a frame's written records the
poison must be intact.  The premises (what the oracle finds, that each frame count reaches the second round of its
loop) are test_many_frames_cpu.py's; where a test depends on the device's CU count it asserts its premise through the
hooks misift_test_block_maps and misift_test_strip_geom."""
import contextlib
import functools

import numpy as np
import pytest

import geometry_util as gu
import many_frames_cases as mc
from batch_util import guarded_context, num_cus
from util import compare_points

pytestmark = pytest.mark.gpu
CALL = dict(num_octaves=mc.NOCT, init_blur=mc.BLUR, thresh=mc.THRESH)
KNOB_DEFAULTS = {"bin": 1, "balance": 1, "strip_waves": mc.STRIP_WAVES_DEFAULT, "scan_waves": 32}
PACK_FILL = 0xA5


def _capi():
    from cudasift_amd import capi
    return capi


@contextlib.contextmanager
def guarded(knobs=(), **opts):
    """A guarded context with poisoned outputs, the named knobs and options; the options a path depends on are set
    whatever the environment made the defaults.  The knobs are put back before the context goes."""
    knobs = dict(knobs)
    with guarded_context(1) as c:
        c.poison_outputs = True
        c.set_options(**dict(dict(fused=1, fix_numpts=0, deterministic=0, texfrac_bits=8, reference_cap=0), **opts))
        try:
            for k, v in knobs.items():
                c.set_knob(k, v)
            yield c
        finally:
            for k in knobs:
                c.set_knob(k, KNOB_DEFAULTS[k])


@contextlib.contextmanager
def profiled(c):
    c.profile_enable(True)
    c.profile_reset()
    out = {}
    try:
        yield out
        out.update({k: v["calls"] for k, v in c.profile_read().items()})
    finally:
        c.profile_enable(False)


def check_rows(rows, B, what, max_pts=mc.MAX_PTS, **mode):
    """rows [B, max_pts] of a padded result against the oracle: see the module docstring."""
    num, wr, _ = mc.counts_of(B, max_pts=max_pts, **mode)
    raw = rows.view(np.uint8).reshape(B, max_pts, 576)
    first = {}
    for f in range(B):
        i = f % mc.NPOOL
        mine = rows[f, :wr[f]]
        if i not in first:
            ref = mc.expected(i, max_pts=max_pts, **mode)[0]
            compare_points(ref[:wr[f]], mine, "%s/f%d" % (what, f))
            first[i] = mc.canon(mine)
        else:
            assert mc.canon(mine) == first[i], "%s: frame %d differs from frame %d, the same pixels" % (what, f, i)
    for i in range(min(B, mc.NPOOL)):
        tail = raw[i::mc.NPOOL, wr[i]:]
        assert tail.min() == 0xFF, "%s: written behind the %d records of a frame of pool index %d" % (what, wr[i], i)


def check_counters(c, B, what, max_pts=mc.MAX_PTS, **mode):
    for f in range(B):
        want = mc.expected(f % mc.NPOOL, max_pts=max_pts, **mode)[2]
        got = c.get_counters(f)
        assert np.array_equal(got, want), "%s: counters of frame %d: %s, oracle %s" % (what, f, got, want)


def check_batch(c, rows, n, B, what, max_pts=mc.MAX_PTS, **mode):
    assert np.array_equal(n, mc.counts_of(B, max_pts=max_pts, **mode)[0]), what + ": numPts"
    check_counters(c, B, what, max_pts, **mode)
    check_rows(rows, B, what, max_pts, **mode)


def check_tables(c, B, what):
    """The block tables of the last call, row for row, for both launches."""
    to, td = mc.table_sizes(num_cus(), B)
    if num_cus() * mc.ORIENT_BLOCKS <= 8 * B and num_cus() * mc.POINT_BLOCKS <= 8 * B:
        assert (to, td) == (8 * B, 8 * B)                    # the per-frame floor: 7 * B rows to deal out
    got_o, got_d = c.block_maps(to + td + 64)
    assert (len(got_o), len(got_d)) == (to, td), (what, len(got_o), len(got_d), to, td)
    det = mc.counts_of(B)[2]
    for name, got, T in (("orient_all", got_o, to), ("descr_all", got_d, td)):
        want = mc.block_tables(det, T)
        bad = np.flatnonzero((got != want).any(1))
        assert len(bad) == 0, "%s: %s table of %d rows differs in %d, first row %d: %s, expected %s" % (
            what, name, T, len(bad), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


# ------------------------------------------------------------------ the block tables
@pytest.mark.parametrize("B", mc.TABLE_BATCHES)
def test_default_launch_structure(B):
    """Binned and balanced: the tables come from the extra workgroup of the bin_detections launch."""
    with guarded() as c:
        with profiled(c) as calls:
            rows, n = c.extract_batch(mc.batch(B), max_pts=mc.MAX_PTS, **CALL)
        assert c.last_call_balanced() == 1
        assert calls.get("bin_detections") == 1 and "frame_shares" not in calls, calls
        check_tables(c, B, "default/B%d" % B)
        check_batch(c, rows, n, B, "default/B%d" % B)


def test_unbinned_batch_builds_its_tables_in_a_kernel_of_their_own():
    B = 600
    with guarded({"bin": 0}) as c:
        with profiled(c) as calls:
            rows, n = c.extract_batch(mc.batch(B), max_pts=mc.MAX_PTS, **CALL)
        assert c.last_call_balanced() == 1
        assert calls.get("frame_shares") == 1 and "bin_detections" not in calls, calls
        check_tables(c, B, "bin0/B%d" % B)
        check_batch(c, rows, n, B, "bin0/B%d" % B)


def test_unbalanced_batch():
    B = 257
    with guarded({"balance": 0}) as c:
        rows, n = c.extract_batch(mc.batch(B), max_pts=mc.MAX_PTS, **CALL)
        assert c.last_call_balanced() == 0
        with pytest.raises(_capi().MisiftError, match="not balanced"):
            c.block_maps(16 * B)
        check_batch(c, rows, n, B, "balance0/B%d" % B)


# ------------------------------------------------------------------ deterministic mode
@pytest.mark.parametrize("fused,refcap,label", [(1, 0, "renumber_dups"), (0, 0, "sort_segments"), (0, 1, "refcap")])
def test_deterministic_mode(fused, refcap, label):
    """Two runs agree byte for byte without canonicalising, and equal the oracle.  The merged-octave path orders the
    staged detections and renumbers the second orientations (renumber_dups, frame on grid y); the dense kernels order the
    record array afterwards (sort_segments / sort_copy_back, frame on z and y) and, under reference_cap, run the
    refcap launches per frame — which drop nothing here: no 30 x 8 block of these frames holds 33 extrema."""
    B = 600
    what = "deterministic/fused%d/refcap%d" % (fused, refcap)
    with guarded(deterministic=1, fused=fused, reference_cap=refcap) as c:
        frames = mc.batch(B)
        with profiled(c) as calls:
            rows, n = c.extract_batch(frames, max_pts=mc.MAX_PTS, **CALL)
        assert label in calls, calls
        check_batch(c, rows, n, B, what)
        rows2, n2 = c.extract_batch(frames, max_pts=mc.MAX_PTS, **CALL)
        assert np.array_equal(n, n2)
        assert rows.tobytes() == rows2.tobytes(), what + ": two runs differ"


# ------------------------------------------------------------------ 8-bit frames, doubled first
def test_eight_bit_frames_with_scale_up():
    """misift_extract_batch_ex: scaleup, rescale_batch and the 8-bit prefilter over 257 frames.  The doubled frames
    hold up to 688 records: max_pts 1024 (test_many_frames_cpu.py states the premise)."""
    B, M = 257, mc.SCALE_UP_MAX_PTS
    with guarded() as c:
        rows, n = c.extract_batch_ex(mc.batch(B, u8=True), scale_up=True, max_pts=M, **CALL)
        assert c.last_call_balanced() == 1
        check_batch(c, rows, n, B, "scale_up_u8/B%d" % B, max_pts=M, u8=True, scale_up=True)


# ------------------------------------------------------------------ counts and offsets: the packed path and the pipe
class Source:
    """B fp32 frames resident on the device, rows padded to 128 floats, and their arena."""

    def __init__(self, c, B):
        capi = _capi()
        self.c, self.B = c, B
        self.pitch = (mc.W + 127) // 128 * 128
        host = np.zeros((B, mc.H, self.pitch), np.float32)
        host[:, :, :mc.W] = mc.batch(B)
        self.stride = mc.H * self.pitch
        self.buf = c.upload(host)
        self.scratch = capi.DevBuf(4 * capi.scratch_floats(mc.W, mc.H, mc.NOCT, False) * B)

    def filled(self, nbytes, byte):
        capi = _capi()
        buf = capi.DevBuf(nbytes)
        capi.check(capi.lib().misift_memset(self.c.h, buf.ptr, byte, nbytes), "misift_memset")
        self.c.sync()
        return buf

    def packed(self, with_pts, what):
        """One misift_extract_batch_packed_async into a packed array of 0xA5 bytes, checked against the oracle."""
        capi, c, B, M = _capi(), self.c, self.B, mc.MAX_PTS
        packed = self.filled(576 * M * B, PACK_FILL)
        cntb = self.filled(4 * (2 * B + 1), PACK_FILL)
        pts = self.filled(576 * M * B, 0xFF) if with_pts else None
        rc = c.extract_batch_packed_async_raw(self.buf.ptr, B, self.stride, mc.W, mc.H, self.pitch, self.scratch.ptr,
                                              pts.ptr if with_pts else None, cntb.ptr, cntb.ptr + 4 * B, packed.ptr,
                                              max_pts=M, **CALL)
        capi.check(rc, "misift_extract_batch_packed_async")
        c.sync()
        cb = c.download(cntb, (2 * B + 1,), np.int32)
        counts, offs = cb[:B], cb[B:]
        allp = c.download(packed, (M * B,), capi.POINT_DTYPE)
        check_packed(counts, offs, allp, B, what)
        check_counters(c, B, what)
        tail = allp[int(offs[B]):].view(np.uint8)
        assert tail.min() == PACK_FILL and tail.max() == PACK_FILL, what + ": written behind offsets[B] records"
        if with_pts:
            check_rows(c.download(pts, (B, M), capi.POINT_DTYPE), B, what + "/d_pts")


def check_packed(counts, offs, recs, B, what):
    """counts [B], offsets [B + 1] and the packed records of a batch against the oracle."""
    num = mc.counts_of(B)[0]
    bad = np.flatnonzero(counts != num)
    assert len(bad) == 0, "%s: counts differ at %d frames, first %d: %d, oracle %d" % (
        what, len(bad), bad[0], counts[bad[0]], num[bad[0]])
    want = np.concatenate([[0], np.cumsum(num)])
    bad = np.flatnonzero(offs != want)
    assert len(bad) == 0, "%s: offsets differ at %d entries, first %d: %d, expected %d" % (
        what, len(bad), bad[0], offs[bad[0]], want[bad[0]])
    assert offs[0] == 0 and np.array_equal(np.diff(offs), counts) and offs[B] == counts.sum()
    first = {}
    for f in range(B):
        i = f % mc.NPOOL
        mine = recs[offs[f]:offs[f + 1]]
        if i not in first:
            compare_points(mc.expected(i)[0][:num[f]], mine, "%s/f%d" % (what, f))
            first[i] = mc.canon(mine)
        else:
            assert mc.canon(mine) == first[i], "%s: frame %d differs from frame %d, the same pixels" % (what, f, i)


@pytest.mark.parametrize("B", mc.PACKED_BATCHES)
def test_packed_async(B):
    """1024 frames fill one round of export_counts_kernel exactly, 1025 and 1030 reach into the second.  Once with d_pts
    given and once packed-only; behind offsets[B] records the packed array keeps its 0xA5."""
    with guarded() as c:
        src = Source(c, B)
        src.packed(True, "packed/B%d" % B)
        assert c.last_call_balanced() == 1
        src.packed(False, "packed_only/B%d" % B)


def test_pipe():
    """A pipe of 1030-frame batches, depth 2: a full batch, then a ragged one of 1025, both in flight at once."""
    capi = _capi()
    big = max(mc.PIPE_BATCHES)
    frames = mc.batch(big)
    room = int(mc.counts_of(big)[0].sum()) + 8
    with guarded() as c:
        pin = capi.PinnedArray(frames.shape, np.float32)
        out = capi.PinnedArray((room,), capi.POINT_DTYPE)
        pin.array[...] = frames
        pipe = capi.Pipe(c, mc.W, mc.H, big, src_u8=False, max_pts=mc.MAX_PTS, depth=2, **CALL)
        try:
            for B in mc.PIPE_BATCHES:
                pipe.submit(pin.ptr, B)
            assert pipe.pending() == len(mc.PIPE_BATCHES)
            for B in mc.PIPE_BATCHES:
                counts, nrec = pipe.collect(out.ptr, room)
                assert len(counts) == B and nrec == counts.sum()
                offs = np.concatenate([[0], np.cumsum(counts)])
                check_packed(counts, offs, out.array[:nrec].copy(), B, "pipe/B%d" % B)
        finally:
            pipe.close()
            pin.free()
            out.free()


# ------------------------------------------------------------------ tall segments
def _tall_batch(c, strip_waves):
    """The smallest batch (beyond a round of 256) whose finest level runs 128-row segments under strip_waves 1; at the
    default the same batch runs 8-row ones."""
    cus = num_cus()
    B = mc.smallest_batch_with(cus, 1, mc.W, mc.TALL_H, mc.PREFILTER_LANES, 128, 2)
    assert B is not None and B >= mc.TALL_BATCH
    pitch = (mc.W + 127) // 128 * 128
    got = c.strip_geom(mc.W, mc.TALL_H, pitch, B, mc.W, mc.TALL_H, mc.PREFILTER_LANES)
    assert got == mc.strip_geom(cus, strip_waves, mc.SMALL_FRAMES, mc.W, mc.TALL_H, mc.PREFILTER_LANES, B), got
    if strip_waves == 1:
        assert got == (1, 128, 2), got               # fourteen turns of the nine-row loop, a ragged 8-row segment behind
        # ScaleDown of the 48 x 68 level: one segment, the whole frame
        coarse = c.strip_geom(mc.W // 2, mc.TALL_H // 2, pitch, B, mc.W // 4, mc.TALL_H // 4, mc.STREAM_LANES)
        assert coarse[1] >= mc.TALL_H // 4 and coarse[2] == 1, coarse
    else:
        assert got[1] == 8 and got[2] == (mc.TALL_H + 7) // 8, got
    return B


@functools.lru_cache(maxsize=None)
def _tall_pyramid(i, u8):
    return gu.oracle_pyramid(mc.pool(True, u8)[i], mc.NOCT, mc.BLUR)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("strip_waves", [1, mc.STRIP_WAVES_DEFAULT])
def test_tall_segments(strip_waves, u8):
    """Every pyramid level of every frame, bit for bit against the oracle's lowpass -> scaledown chain, with the finest
    level cut into a 128-row segment and an 8-row rest (strip_waves 1) and into seventeen 8-row segments (the default:
    the largest item count)."""
    with guarded({"strip_waves": strip_waves}) as c:
        B = _tall_batch(c, strip_waves)
        pyr, calls = gu.pyramids(c, mc.batch(B, tall=True, u8=u8), mc.NOCT, 1, mc.BLUR, mc.THRESH, mc.SCALE_UP_MAX_PTS)
        assert calls.get("lowpass_down") == 1 and "lowpass" not in calls and calls.get("scaledown") == mc.NOCT - 2, calls
        want = [_tall_pyramid(f % mc.NPOOL, u8) for f in range(B)]
        gu.check_pixels(pyr, want, "tall/strip_waves%d/u8=%d" % (strip_waves, u8))


def test_tall_scan_segments():
    """The DoG scan sizes its segments by the same rule (whole turns of its nine-row ring, 126 rows at the most): with
    scan_waves 1 and at least as many frames as CUs the 136-row level is scanned as 126 rows and a 10-row rest, the
    coarser levels as one segment each.  Records against the oracle."""
    M = mc.SCALE_UP_MAX_PTS                     # the tall frames hold up to 567 records
    with guarded({"strip_waves": 1, "scan_waves": 1}) as c:
        B = _tall_batch(c, 1)
        assert B >= num_cus()                   # one strip per frame: want = 1 for the scan as well
        rows, n = c.extract_batch(mc.batch(B, tall=True), max_pts=M, **CALL)
        check_batch(c, rows, n, B, "tall_scan/B%d" % B, max_pts=M, tall=True)


# ------------------------------------------------------------------ one context across frame counts
@pytest.mark.parametrize("order", [mc.USED_CONTEXT, mc.LARGE_FIRST], ids=["small_first", "large_first"])
def test_one_context_across_frame_counts(order):
    """The per-frame arrays of a context grow with the largest call so far; a smaller call afterwards runs on tables
    sized for the larger one.  Every call equals the oracle; the last one is the packed entry point."""
    with guarded() as c:
        for k, B in enumerate(order[:-1]):
            rows, n = c.extract_batch(mc.batch(B), max_pts=mc.MAX_PTS, **CALL)
            assert c.last_call_balanced() == 1
            check_tables(c, B, "used/%d/B%d" % (k, B))
            check_batch(c, rows, n, B, "used/%d/B%d" % (k, B))
        Source(c, order[-1]).packed(False, "used/packed/B%d" % order[-1])
