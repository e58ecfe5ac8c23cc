"""Extraction with frames at and over the record capacity, on every path that takes max_pts: the single call (fused and
dense), batches of six (binned and balanced, unbalanced, the gather descriptor kernel, three waves per SIMD, dense), the
small-batch kernels, 8-bit frames with scale_up, the packed entry point with and without d_pts, a candidate-list overflow
between capped frames, descr_big, deterministic mode, the host pipe, and one context whose capacity changes from call to
call.  The rule, the tables and the checker: extract_capacity_cases.py; their premises and the checker's own test:
test_extract_capacity_cpu.py.

Every output buffer has exactly the stated size, starts as 0xA5 bytes and lives in a guarded context
(batch_util.guarded_context: 64 KiB bands around every allocation, checked when the context goes and once more at the
end of the module).  The reference is the oracle's UNCAPPED run of each frame; no tolerance of this file's own.

Counters (rule 4) per path, from the code: refine_all (fused) and refine_kernel (dense) add a detection to its octave's
counter before they compare its index with max_pts, so the per-octave detection counts are the uncapped ones on every
path; they are asserted wherever misift_get_counters has the call's counters — all of the calls below but the pipe (whose
batches are collected long after they ran) and the batch with the flooded frame (that frame's counters are not an extraction's).

Deterministic mode (rule 7) per path, from the code: the fused path stages each octave's detections in a list of max_pts
entries and orders the list, so two calls agree byte for byte on every frame whose per-octave detection counts are all
<= max_pts; the dense kernels (fused = 0) append to the record array itself and order its segments afterwards, so they
agree wherever no segment inside numPts is cut (numPts uncapped <= max_pts), and where one is cut which members stay is
the append order's business: rule 2 only."""
import contextlib

import numpy as np
import pytest

import extract_capacity_cases as cc
import extract_cases as xc
from batch_util import guarded_context
from conftest import record
from extract_capacity_cases import check_counters, check_frame, check_packed_layout
from extract_cases import expected, frames6, frames6_u8, small6

pytestmark = pytest.mark.gpu
CNT_BIG = 48                      # word of a frame's counter block: keypoints deferred to descr_big
CALL = dict(num_octaves=cc.NOCT, init_blur=1.0, thresh=3.0, lowest_scale=0.0)
B6 = 6


@contextlib.contextmanager
def guarded(knobs=(), **opts):
    """A guarded context with the named knobs and options; the options a path depends on are set whatever the
    environment made the defaults (MISIFT_FUSED, MISIFT_DETERMINISTIC, MISIFT_TEXFRAC_BITS)."""
    with guarded_context(1) as c:
        for k, v in dict(knobs).items():
            c.set_knob(k, v)
        c.set_options(**dict(dict(fused=1, fix_numpts=0, deterministic=0, texfrac_bits=8), **opts))
        yield c


def repoison(c, buf):
    from cudasift_amd import capi
    capi.check(capi.lib().misift_memset(c.h, buf.ptr, cc.POISON_BYTE, buf.nbytes), "misift_memset")
    c.sync()


def poisoned(c, nbytes):
    """A device buffer of exactly nbytes, every byte the poison."""
    from cudasift_amd import capi
    buf = capi.DevBuf(nbytes)
    repoison(c, buf)
    return buf


class Source:
    """Frames resident on the device (fp32 with rows padded to 128 floats, or tightly packed 8-bit) and their arena."""

    def __init__(self, c, frames, scale_up=False):
        from cudasift_amd import capi
        frames = np.ascontiguousarray(frames)
        self.c, self.scale_up = c, scale_up
        self.B, self.h, self.w = frames.shape
        self.u8 = frames.dtype == np.uint8
        if self.u8:
            self.pitch, host = self.w, frames
        else:
            self.pitch = (self.w + 127) // 128 * 128
            host = np.zeros((self.B, self.h, self.pitch), np.float32)
            host[:, :, :self.w] = frames
        self.stride = self.h * self.pitch
        self.buf = c.upload(host)
        self.scratch = capi.DevBuf(4 * capi.scratch_floats(self.w, self.h, cc.NOCT, scale_up) * self.B)

    def single(self, f, M, pts, **kw):
        """misift_extract of frame f into pts (M rows): (rows [1, M], numPts [1])."""
        from cudasift_amd import capi
        rc, n = self.c.extract_raw(self.buf.ptr + 4 * f * self.stride, self.w, self.h, self.pitch, self.scratch.ptr, pts.ptr,
                                   max_pts=M, **dict(CALL, **kw))
        capi.check(rc, "misift_extract")
        return self.c.download(pts, (1, M), capi.POINT_DTYPE), np.array([n], np.int32)

    def batch(self, M, pts, **kw):
        """misift_extract_batch_ex of all frames into pts (B * M rows): (rows [B, M], numPts [B])."""
        from cudasift_amd import capi
        rc, n = self.c.extract_batch_raw(self.buf.ptr, self.u8, self.B, self.stride, self.w, self.h, self.pitch,
                                         self.scratch.ptr, pts.ptr, scale_up=self.scale_up, max_pts=M, **dict(CALL, **kw))
        capi.check(rc, "misift_extract_batch_ex")
        return self.c.download(pts, (self.B, M), capi.POINT_DTYPE), n

    def packed(self, M, pts, cntb, packed, **kw):
        """misift_extract_batch_packed_async (pts None: d_pts = NULL): (counts [B], offsets [B + 1])."""
        from cudasift_amd import capi
        assert not self.u8 and not self.scale_up
        rc = self.c.extract_batch_packed_async_raw(self.buf.ptr, self.B, self.stride, self.w, self.h, self.pitch,
                                                   self.scratch.ptr, pts.ptr if pts is not None else None, cntb.ptr,
                                                   cntb.ptr + 4 * self.B, packed.ptr, max_pts=M, **dict(CALL, **kw))
        capi.check(rc, "misift_extract_batch_packed_async")
        self.c.sync()
        cb = self.c.download(cntb, (2 * self.B + 1,), np.int32)
        return cb[:self.B], cb[self.B:]


_met = {}


def note(path, classes=(), kernels=None):
    """What a path met, for docs/LOG.md (through conftest.record, into the session's parity report)."""
    m = _met.setdefault(path, {"classes": set(), "kernels": set()})
    m["classes"] |= set(classes)
    if kernels is not None:
        m["kernels"] |= set(kernels)
    record("capacity/" + path, classes=sorted(m["classes"]), kernels=sorted(m["kernels"]))


def profiled_once(c, fn):
    """fn() with the profile on: (its result, the launch labels it ran)."""
    c.profile_enable(True)
    c.profile_reset()
    try:
        out = fn()
        return out, sorted(c.profile_read())
    finally:
        c.profile_enable(False)


def check_rows(path, rows, n, ref, cnt, M, fix, c=None, frames=None):
    """Rules 1 - 3 and the hole check for every frame of a padded result, rule 4 when the context is given."""
    for i, f in enumerate(range(len(rows)) if frames is None else frames):
        name = "%s/M%d/f%d" % (path, M, f)
        cls, _ = check_frame(ref[f], cnt[f], M, rows[i], fix, num_pts=n[i], name=name)
        note(path, [cls])
        if c is not None:
            check_counters(c.get_counters(i), cnt[f], M, name=name)


def padded_path(path, c, src, caps, ref, cnt, fix, frames=None, single=None, **kw):
    """Every capacity of `caps` through the batch call (single: through misift_extract on that frame), each into a
    poisoned array of exactly B * M records; then once more at 150 with the profile on, for the launch labels."""
    def call(M):
        pts = poisoned(c, 576 * M * (1 if single is not None else src.B))
        rows, n = src.single(single, M, pts, **kw) if single is not None else src.batch(M, pts, **kw)
        check_rows(path, rows, n, ref, cnt, M, fix, c, [single] if single is not None else frames)
    for M in caps:
        call(M)
    _, kernels = profiled_once(c, lambda: call(150))
    note(path, kernels=kernels)
    return kernels


# ------------------------------------------------------------------ the single call
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("fused", [1, 0])
def test_single_call(fused, fix):
    ref, _, cnt = expected(frames6())
    with guarded(fused=fused, fix_numpts=fix) as c:
        src = Source(c, frames6())
        kernels = padded_path("single/fused%d/fix%d" % (fused, fix), c, src, cc.SINGLE_CAPS, ref, cnt, fix, single=xc.SINGLE)
        assert ("descr_all" in kernels) == bool(fused) and ("descr" in kernels) == (not fused), kernels
        assert c.last_call_balanced() == 0


# ------------------------------------------------------------------ batches of six
# (id, knobs, options, balanced, a launch label the path must show, one it must not)
SIX = [
    ("default", {}, {}, 1, "descr_all", "descr"),
    ("default-fix_numpts", {}, {"fix_numpts": 1}, 1, "descr_all", "descr"),
    ("unbalanced", {"balance": 0}, {}, 0, "descr_all", "descr"),
    ("no_tile_descr", {"tile_descr": 0}, {}, 0, "descr_all", "descr"),
    ("occ3", {"descr_occ": 3}, {}, 1, "descr_all", "descr"),
    ("dense", {}, {"fused": 0}, 0, "descr", "descr_all"),
    ("dense-fix_numpts", {}, {"fused": 0, "fix_numpts": 1}, 0, "descr", "descr_all"),
]


@pytest.mark.parametrize("name,knobs,opts,balanced,has,has_not", SIX, ids=[r[0] for r in SIX])
def test_batch_of_six(name, knobs, opts, balanced, has, has_not):
    ref, _, cnt = expected(frames6())
    with guarded(knobs, **opts) as c:
        src = Source(c, frames6())
        kernels = padded_path("six/" + name, c, src, cc.BATCH_CAPS, ref, cnt, opts.get("fix_numpts", 0))
        assert c.last_call_balanced() == balanced
        assert has in kernels and has_not not in kernels, kernels
    assert set(cc.CLASSES) <= _met["six/" + name]["classes"], _met["six/" + name]["classes"]


@pytest.mark.parametrize("fix", [0, 1])
def test_batch_of_two(fix):
    """Frames 1 and 2: the small-batch kernels (plain grids, no binning, the last kernel's counter export)."""
    ref, _, cnt = expected(frames6())
    with guarded(fix_numpts=fix) as c:
        src = Source(c, frames6()[1:3])
        padded_path("two/fix%d" % fix, c, src, cc.BATCH_CAPS, ref, cnt, fix, frames=[1, 2])
        assert c.last_call_balanced() == 0


@pytest.mark.parametrize("fix", [0, 1])
def test_eight_bit_frames_with_scale_up(fix):
    """misift_extract_batch_ex, 8-bit small6() doubled first: the kept records are halved exactly once, the finest
    octave's second orientations behind numPts (fix_numpts 0) keep their unhalved coordinates — both as the uncapped
    oracle's scale_up records say, whose members the rows must be, bit for bit in position and scale."""
    ref, _, cnt = expected(small6(), scale_up=True, fix_numpts=bool(fix))
    u8 = small6().astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), small6())
    with guarded(fix_numpts=fix) as c:
        src = Source(c, u8, scale_up=True)
        padded_path("scale_up_u8/fix%d" % fix, c, src, cc.BATCH_CAPS, ref, cnt, fix)


# ------------------------------------------------------------------ the packed entry point
MATCHER_WORDS = [6, 7, 8, 9, 10, 11, 13, 14, 15]       # score ... match_error and the three spare words of a record


def packed_path(path, c, src, caps, ref, cnt, with_pts, frames=None, fused=1, counters=True, **kw):
    """Rules 1, 2, 5 and 6 for misift_extract_batch_packed_async at every capacity of `caps`.  Rule 6 in a poisoned
    d_pts: a packed record equals its row of d_pts in every word an extraction writes; the matcher's nine words are
    cleared in a packed record that descr_all wrote and are the caller's own in a row of d_pts (an extraction never
    writes them there, like the reference's), so with fused = 1 they differ by design and with fused = 0, where the packed
    record is a copy of the row, the whole 576 bytes are equal."""
    from cudasift_amd import capi
    frames = list(range(src.B)) if frames is None else frames
    fix = c.get_options().fix_numpts

    def call(M):
        packed = poisoned(c, 576 * M * src.B)
        cntb = poisoned(c, 4 * (2 * src.B + 1))
        pts = poisoned(c, 576 * M * src.B) if with_pts else None
        counts, offs = src.packed(M, pts, cntb, packed, **kw)
        all_packed = c.download(packed, (M * src.B,), capi.POINT_DTYPE)
        want = [min(int(cnt[f][2 * cc.NOCT + fix]), M) for f in frames]
        check_packed_layout(counts, offs, all_packed, want, name="%s/M%d" % (path, M))
        rows = c.download(pts, (src.B, M), capi.POINT_DTYPE) if with_pts else None
        for i, f in enumerate(frames):
            name = "%s/M%d/f%d" % (path, M, f)
            mine = all_packed[offs[i]:offs[i + 1]]
            if with_pts:
                cls, _ = check_frame(ref[f], cnt[f], M, rows[i], fix, num_pts=counts[i], name=name + "/d_pts")
                a, b = cc.words(mine), cc.words(rows[i, :counts[i]])
                assert np.array_equal(a[:, cc.EXTRACT_WORDS], b[:, cc.EXTRACT_WORDS]), name + ": packed != padded"
            if fused:                         # descr_all wrote the record: complete, the matcher's nine words cleared
                cls, _ = check_frame(ref[f], cnt[f], M, mine, fix, packed=True, name=name)
                assert not cc.words(mine)[:, MATCHER_WORDS].any(), name
            else:                             # pack_records copied the row of d_pts, the matcher's words as they were there
                assert mine.tobytes() == rows[i, :counts[i]].tobytes(), name
            note(path, [cls])
            if counters:
                check_counters(c.get_counters(i), cnt[f], M, name=name)
    for M in caps:
        call(M)
    _, kernels = profiled_once(c, lambda: call(150))
    note(path, kernels=kernels)
    return kernels


@pytest.mark.parametrize("with_pts", [1, 0], ids=["with_d_pts", "d_pts_null"])
@pytest.mark.parametrize("nframes", [6, 2])
def test_packed_entry_point(nframes, with_pts):
    ref, _, cnt = expected(frames6())
    frames = list(range(6)) if nframes == 6 else [1, 2]
    with guarded() as c:
        src = Source(c, frames6()[frames])
        kernels = packed_path("packed/%d/%s" % (nframes, "d_pts" if with_pts else "null"), c, src, cc.BATCH_CAPS, ref, cnt,
                              with_pts, frames)
        assert c.last_call_balanced() == (1 if nframes == 6 else 0)
        assert "descr_all" in kernels and "descr" not in kernels, kernels


def test_packed_entry_point_on_the_dense_kernels():
    """fused = 0: the records go to d_pts and pack_records copies numPts rows of every frame."""
    ref, _, cnt = expected(frames6())
    with guarded(fused=0) as c:
        src = Source(c, frames6())
        kernels = packed_path("packed/6/dense", c, src, cc.BATCH_CAPS, ref, cnt, 1, fused=0)
        assert "descr" in kernels and "descr_all" not in kernels, kernels


# ------------------------------------------------------------------ a flooded candidate list between capped frames
def test_candidate_overflow_between_capped_frames():
    """Six frames at thresh 0.05, frame 2 white noise that floods the fused scan's candidate list, max_pts 700: the packed
    call reports it as count -1 with a packed width of 0, and the frames on both sides — every one of them over capacity
    at this threshold — obey rule 2 against their own uncapped oracle records, in d_pts and in the packed array.  Measured
    on the MI355X: frame 0 (3130 records in the oracle) floods its list at this threshold as well, so the batch holds two
    flooded frames, one of them first in the packed array, and four capped ones."""
    from cudasift_amd import capi
    M, th = cc.OVERFLOW_CAP, cc.OVERFLOW_THRESH
    frames = frames6().copy()
    frames[2] = cc.noise_frame()
    refs = {f: expected(frames[f], thresh=th, max_pts=cc.OVERFLOW_UNCAPPED) for f in (0, 1, 3, 4, 5)}
    with guarded() as c:
        src = Source(c, frames)
        # the premise, frame by frame through misift_extract_batch_async on that frame alone: the noise frame floods its
        # list (count -1), its two neighbours do not.  (Frame 0 does as well at this threshold — a list holds w * h / 4
        # pre-candidates — and is then held to the same answer inside the batch: -1, width 0.)
        flooded = []
        for f in range(B6):
            pts1, cnt1 = poisoned(c, 576 * M), poisoned(c, 4)
            capi.check(capi.lib().misift_extract_batch_async(c.h, src.buf.ptr + 4 * f * src.stride, 1, src.stride, src.w,
                                                             src.h, src.pitch, cc.NOCT, 1.0, th, 0.0, src.scratch.ptr,
                                                             pts1.ptr, M, cnt1.ptr), "misift_extract_batch_async")
            c.sync()
            alone = int(c.download(cnt1, (1,), np.int32)[0])
            assert alone in (-1, M), (f, alone)
            flooded.append(alone == -1)
        assert flooded[2] and not flooded[1] and not flooded[3] and sum(flooded) <= 2, flooded
        packed, cntb, pts = poisoned(c, 576 * M * B6), poisoned(c, 4 * (2 * B6 + 1)), poisoned(c, 576 * M * B6)
        counts, offs = src.packed(M, pts, cntb, packed, thresh=th)
        all_packed = c.download(packed, (M * B6,), capi.POINT_DTYPE)
        rows = c.download(pts, (B6, M), capi.POINT_DTYPE)
        want = [-1 if flooded[f] else M for f in range(B6)]
        check_packed_layout(counts, offs, all_packed, want, name="overflow")
        assert offs[3] == offs[2]
        record("capacity/overflow", flooded=flooded)
        for f, (ref, n, cnt) in refs.items():
            assert n > M
            if flooded[f]:
                continue
            cls, _ = check_frame(ref, cnt, M, all_packed[offs[f]:offs[f + 1]], 0, packed=True, name="overflow/packed/f%d" % f)
            check_frame(ref, cnt, M, rows[f], 0, num_pts=counts[f], name="overflow/d_pts/f%d" % f)
            assert np.array_equal(cc.words(all_packed[offs[f]:offs[f + 1]])[:, cc.EXTRACT_WORDS],
                                  cc.words(rows[f])[:, cc.EXTRACT_WORDS]), f
            note("overflow", [cls])
        # the synchronous call redoes the flooded frames on the dense kernels, each run of them as a sub-call on its own
        # slice of d_pts: nobody is -1 now, and the noise frame obeys the rule against its own uncapped records too
        refs[2] = expected(frames[2], thresh=th, max_pts=cc.OVERFLOW_UNCAPPED)
        assert refs[2][2][9] < cc.OVERFLOW_UNCAPPED
        pts = poisoned(c, 576 * M * B6)
        (rows, n), kernels = profiled_once(c, lambda: src.batch(M, pts, thresh=th))
        assert "dog_scan" in kernels and "detect" in kernels and "descr" in kernels, kernels
        note("overflow/rerun", kernels=kernels)
        check_rows("overflow/rerun", rows, n, {f: r[0] for f, r in refs.items()}, {f: r[2] for f, r in refs.items()}, M, 0, c)


# ------------------------------------------------------------------ descr_big
def test_patch_reach_9_sends_most_keypoints_through_descr_big():
    """patch_reach = 9: every keypoint of scale > 1.0 at its level is deferred to descr_big_kernel — launched at once
    behind a batch, by the host behind a folded single call — whose capacity test is its own."""
    ref, _, cnt = expected(frames6())
    with guarded({"patch_reach": 9.0}) as c:
        src = Source(c, frames6())
        for M in cc.BIG_CAPS:
            pts = poisoned(c, 576 * M)
            rows, n = src.single(xc.SINGLE, M, pts)
            check_rows("big/single", rows, n, ref, cnt, M, 0, c, [xc.SINGLE])
            big1 = int(c.get_counter_block(0)[CNT_BIG])
            assert big1 > 0, big1
            pts = poisoned(c, 576 * M * B6)
            rows, n = src.batch(M, pts)
            check_rows("big/six", rows, n, ref, cnt, M, 0, c)
            big = [int(c.get_counter_block(f)[CNT_BIG]) for f in range(B6)]
            assert min(big) > 0, big
            record("capacity/big/M%d" % M, deferred_single=big1, deferred=big)
        assert c.descr_big_fallbacks() == len(cc.BIG_CAPS)
        _, kernels = profiled_once(c, lambda: src.single(xc.SINGLE, 150, poisoned(c, 576 * 150)))
        assert "descr_big" in kernels, kernels
        note("big/single", kernels=kernels)
        _, kernels = profiled_once(c, lambda: src.batch(150, poisoned(c, 576 * 150 * B6)))
        note("big/six", kernels=kernels)
        packed_path("big/packed", c, src, cc.BIG_CAPS, ref, cnt, 0)
        big = [int(c.get_counter_block(f)[CNT_BIG]) for f in range(B6)]
        assert min(big) > 0, big


# ------------------------------------------------------------------ deterministic mode
@pytest.mark.parametrize("fused", [1, 0])
def test_deterministic_mode(fused):
    """Rule 7 on top of rule 2 (the module docstring says which frames each path promises)."""
    ref, _, cnt = expected(frames6())
    promised = cc.LISTS_FIT if fused else cc.NOTHING_CUT
    path = "deterministic/fused%d" % fused
    with guarded(fused=fused, deterministic=1) as c:
        src = Source(c, frames6())
        for M in cc.DETERMINISTIC_CAPS:
            runs = []
            for rep in range(2):
                pts = poisoned(c, 576 * M * B6)
                rows, n = src.batch(M, pts)
                check_rows(path, rows, n, ref, cnt, M, 0, c)
                runs.append((rows, n))
            (a, na), (b, nb) = runs
            assert np.array_equal(na, nb)
            same = [f for f in range(B6) if a[f, :na[f]].tobytes() == b[f, :nb[f]].tobytes()]
            record("capacity/%s/M%d" % (path, M), identical=same, promised=list(promised[M]))
            assert set(promised[M]) <= set(same), (M, same, promised[M])
        _, kernels = profiled_once(c, lambda: src.batch(150, poisoned(c, 576 * 150 * B6)))
        note(path, kernels=kernels)


# ------------------------------------------------------------------ the pipe
def test_pipe_at_capacity():
    """Depth 2, two batches of three 8-bit frames, max_pts 150 (under every frame's coarse octaves plus a part of the
    finest): counts by rule 1, the collected records by rule 2, nrecords_out their sum, nothing written behind them."""
    from cudasift_amd import capi
    ref, _, cnt = expected(frames6())
    M, nb = cc.PIPE_CAP, 3
    with guarded() as c:
        pin = capi.PinnedArray((B6, xc.H, xc.W), np.uint8)
        pin.array[...] = frames6_u8()
        out = capi.PinnedArray((nb * M,), capi.POINT_DTYPE)
        pipe = capi.Pipe(c, xc.W, xc.H, nb, src_u8=True, max_pts=M, depth=2, **{k: v for k, v in CALL.items()})
        try:
            pipe.submit(pin.ptr, nb)
            pipe.submit(pin.ptr + nb * xc.H * xc.W, nb)
            for k in range(2):
                out.array.view(np.uint8)[...] = cc.POISON_BYTE
                counts, nrec = pipe.collect(out.ptr, nb * M)
                recs = out.array.copy()
                want = [min(int(cnt[nb * k + i][8]), M) for i in range(nb)]
                assert counts.tolist() == want and nrec == sum(want), (k, counts, nrec, want)
                offs = np.concatenate([[0], np.cumsum(counts)])
                check_packed_layout(counts, offs, recs, want, name="pipe/%d" % k)
                for i in range(nb):
                    f = nb * k + i
                    cls, _ = check_frame(ref[f], cnt[f], M, recs[offs[i]:offs[i + 1]], 0, packed=True,
                                         name="pipe/%d/f%d" % (k, f))
                    note("pipe", [cls])
            assert pipe.pending() == 0
        finally:
            pipe.close()
            pin.free()
            out.free()


# ------------------------------------------------------------------ one context, alternating capacities
def test_one_context_alternating_capacities():
    """The same frames, arena and record array at max_pts 4096, 150, 4096, 1, 4096, every call made twice in a row with
    graph replay requested (the second call has the key of the first: it is the one the library captures and replays, if
    capture succeeds): each call obeys the rules for its own capacity, nothing of a larger call's layout survives into a
    smaller one or the other way round, and the 4096 calls equal the uncapped oracle outright.  Then the same sequence
    through the packed call with d_pts = NULL."""
    from cudasift_amd import capi
    ref, nref, cnt = expected(frames6())
    big = max(cc.ALTERNATING)
    with guarded() as c:
        capi.check(capi.lib().misift_ctx_set_graph_replay(c.h, 1), "misift_ctx_set_graph_replay")
        src = Source(c, frames6())
        pts = poisoned(c, 576 * big * B6)
        for step, M in enumerate(cc.ALTERNATING):
            for rep in range(2):
                repoison(c, pts)
                rc, n = c.extract_batch_raw(src.buf.ptr, False, B6, src.stride, src.w, src.h, src.pitch, src.scratch.ptr,
                                            pts.ptr, max_pts=M, **CALL)
                capi.check(rc, "misift_extract_batch_ex")
                everything = c.download(pts, (big * B6,), capi.POINT_DTYPE)
                path = "alternating/padded"
                check_rows(path, everything[:M * B6].reshape(B6, M), n, ref, cnt, M, 0, c)
                assert (cc.words(everything[M * B6:]) == cc.POISON_U32).all(), (step, rep, M)
                if M == big:
                    assert np.array_equal(n, nref), (step, rep)
                    for f in range(B6):
                        assert np.array_equal(c.get_counters(f), cnt[f]), (step, rep, f)
        packed, cntb = poisoned(c, 576 * big * B6), poisoned(c, 4 * (2 * B6 + 1))
        for step, M in enumerate(cc.ALTERNATING):
            for rep in range(2):
                repoison(c, packed)
                repoison(c, cntb)
                counts, offs = src.packed(M, None, cntb, packed)
                everything = c.download(packed, (big * B6,), capi.POINT_DTYPE)
                want = [min(int(cnt[f][8]), M) for f in range(B6)]
                check_packed_layout(counts, offs, everything, want, name="alternating/packed/%d.%d" % (step, rep))
                for f in range(B6):
                    cls, _ = check_frame(ref[f], cnt[f], M, everything[offs[f]:offs[f + 1]], 0, packed=True,
                                         name="alternating/packed/%d.%d/M%d/f%d" % (step, rep, M, f))
                    note("alternating/packed", [cls])
                    check_counters(c.get_counters(f), cnt[f], M)


# ------------------------------------------------------------------ last: the guard bands
def test_guards_intact_at_the_end():
    """Every context above checked its bands when it went; the allocations freed since then (the record arrays and
    arenas of the last tests) were verified as they were freed, and this collects their verdict."""
    import gc
    from cudasift_amd import capi
    gc.collect()
    capi.check_guards()
