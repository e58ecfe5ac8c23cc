"""misift_find_homography_batch / misift_improve_homography_batch: FindHomography and ImproveHomography of many frames of a
device-resident batch, stream-ordered, with the counts read on the device.

Find, per entry: H (by bits) and the inlier count equal srand(seed) + misift_find_homography on that frame alone, and
orc_find_homography after the same srand.  Improve, per entry: H, num_fit and every match_error equal
misift_improve_homography on that frame; no other byte of the records changes."""
import ctypes as C

import numpy as np
import pytest

from batch_util import gated_frame as _gated, guarded_context, layout, matched_frames as _frames, orc, span
from synth import synth_frame, synth_matches

pytestmark = pytest.mark.gpu

SIZES = [0, 7, 8, 40, 777, 1500, 5000]
FIND = dict(min_score=0.85, max_ambiguity=0.95, thresh=5.0)
IMPROVE = dict(min_score=0.0, max_ambiguity=0.80, thresh=3.0)
IDENTITY = np.eye(3, dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _single_find(ctx, recs, n, seed, loops, oracle=True):
    """srand(seed) + misift_find_homography on one frame (and the oracle after the same srand)."""
    o = orc()
    if n < 8:
        return IDENTITY, 0
    d = ctx.upload(recs)
    o.srand(seed)
    H, nm = ctx.find_homography(d.ptr, n, num_loops=loops, **FIND)
    if oracle:
        o.srand(seed)
        Ho, no, _ = o.find_homography(recs.copy(), n, num_loops=loops, **FIND)
        assert no == nm and np.array_equal(_bits(Ho), _bits(H)), (n, loops, no, nm)
    return H, nm


def _run_find(ctx, frames, seeds, recs, counts, offs, stride, loops, max_pts=8192):
    from cudasift_amd import capi
    d, dc = ctx.upload(recs), ctx.upload(np.asarray(counts, np.int32))
    do = ctx.upload(offs) if offs is not None else None
    H, nm = ctx.find_homography_batch(frames, seeds, d, len(counts), dc, do, stride, max_pts=max_pts, num_loops=loops,
                                      **FIND)
    ctx.sync()
    after = ctx.download(d, (len(recs),), capi.POINT_DTYPE)
    assert after.tobytes() == recs.tobytes(), "find wrote into the records"
    return ctx.download(H, (len(frames), 3, 3), np.float32), ctx.download(nm, (len(frames),), np.int32)


def _check_find(ctx, frames_sel, seeds, recs, counts, offs, stride, loops, oracle=True):
    H, nm = _run_find(ctx, frames_sel, seeds, recs, counts, offs, stride, loops)
    for i, (f, s) in enumerate(zip(frames_sel, seeds)):
        n = max(int(counts[f]), 0)
        He, ne = _single_find(ctx, recs[span(offs, stride, f, n)].copy(), n, s, loops, oracle)
        assert nm[i] == ne and np.array_equal(_bits(H[i]), _bits(He)), (i, f, n, loops, nm[i], ne)
    return H, nm


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("loops", [50, 1000])
def test_find_bit_identical(ctx, padded, loops):
    fr = _frames(SIZES, 3)
    recs, offs, stride = layout(fr, SIZES, padded, min_stride=1, pad_error=-7.0)
    sel = [6, 0, 4, 1, 5, 3, 2]                       # not in frame order
    seeds = [11, 12, 13, 0, 2**32 - 1, 12345, 7]
    H, nm = _check_find(ctx, sel, seeds, recs, SIZES, offs, stride, loops, oracle=loops <= 1000)
    assert (nm[[0, 2, 4, 5]] > 0).all(), nm


def test_find_ragged_and_degenerate(ctx):
    """Packed, with a count -1 frame (no records), a frame with fewer than 8 valid points and a frame in no entry."""
    sizes = [1500, 40, 300, 777, 0, 64]
    counts = [1500, -1, 300, 777, 0, 64]
    fr = _frames(sizes, 5)
    fr[2]["score"] = 0.0                              # only 5 valid points left in frame 2
    fr[2]["score"][[3, 50, 100, 200, 299]] = 0.99
    fr[2]["ambiguity"] = 0.5
    recs, offs, stride = layout(fr, counts, False, min_stride=1, pad_error=-7.0)
    sel = [0, 1, 2, 3, 4]
    H, nm = _check_find(ctx, sel, [1, 2, 3, 4, 5], recs, counts, offs, stride, 1000)
    for i in (1, 2, 4):
        assert nm[i] == 0 and np.array_equal(_bits(H[i]), _bits(IDENTITY)), (i, nm[i])


def test_find_10000_loops(ctx):
    sizes = [40, 1500]
    fr = _frames(sizes, 9)
    recs, offs, stride = layout(fr, sizes, False, min_stride=1, pad_error=-7.0)
    _check_find(ctx, [0, 1], [99, 100], recs, sizes, offs, stride, 10000)


def test_process_rand_state_untouched(ctx):
    o = orc()
    fr = _frames([777, 1500], 4)
    recs, offs, stride = layout(fr, [777, 1500], False, min_stride=1, pad_error=-7.0)
    LIBC = C.CDLL(None)
    o.srand(5)
    expect = [LIBC.rand() for _ in range(64)]
    o.srand(5)
    _run_find(ctx, [0, 1], [5, 6], recs, [777, 1500], offs, stride, 1000)
    assert [LIBC.rand() for _ in range(64)] == expect


def _run_improve(ctx, sel, recs, counts, offs, stride, H0, loops):
    from cudasift_amd import capi
    d, dc = ctx.upload(recs), ctx.upload(np.asarray(counts, np.int32))
    do = ctx.upload(offs) if offs is not None else None
    dH = ctx.upload(np.ascontiguousarray(H0, np.float32))
    nf = ctx.improve_homography_batch(sel, d, len(counts), dc, dH, do, stride, num_loops=loops, **IMPROVE)
    ctx.sync()
    return (ctx.download(d, (len(recs),), capi.POINT_DTYPE), ctx.download(dH, (len(sel), 3, 3), np.float32),
            ctx.download(nf, (len(sel),), np.int32))


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("loops", [0, 5])
def test_improve_bit_identical(ctx, padded, loops):
    from cudasift_amd import capi
    sizes = [1500, 0, 777, 40, 5000, 300]
    counts = [1500, 0, 777, -1, 5000, 300]             # frame 5: in no entry
    fr = _frames(sizes, 6)
    recs, offs, stride = layout(fr, counts, padded, min_stride=1, pad_error=-7.0)
    recs["match_error"] = np.arange(len(recs), dtype=np.float32) * 0.5 - 3.0
    sel = [4, 0, 3, 1, 2]
    H0 = []
    for i, f in enumerate(sel):                        # start H: near the truth, H[8] != 1 so the division shows
        _, Ht, _ = synth_matches(8, seed=0)
        H0.append(Ht * np.float32(1.0 + 0.25 * i) + np.float32(0.001 * i))
    H0 = np.stack(H0).astype(np.float32)
    got, H, nf = _run_improve(ctx, sel, recs, counts, offs, stride, H0, loops)
    exp = recs.copy()
    for i, f in enumerate(sel):
        n = max(counts[f], 0)
        sl = span(offs, stride, f, n)
        d = ctx.upload(recs[sl].copy()) if n else ctx.zeros(576)      # a frame with no records: start pointer, 0 records
        He, ne = ctx.improve_homography(d.ptr, n, H0[i], loops, **IMPROVE)
        if n:
            exp[sl] = ctx.download(d, (n,), capi.POINT_DTYPE)
        elif loops >= 1:                               # Cholesky fails on an empty system: the zeroed solution
            assert np.array_equal(He.reshape(9)[:8], np.zeros(8, np.float32)), He
        assert nf[i] == ne and np.array_equal(_bits(H[i]), _bits(He)), (i, f, n, nf[i], ne)
    assert got.tobytes() == exp.tobytes()


def test_count_above_max_pts_guarded(ctx):
    """A frame whose device count exceeds max_pts gets -1 and the identity H, and nothing past its records is read: the
    buffer ends where the frame's real records end.  On a guarded context (temp starts as 0xFF, bands checked)."""
    sizes = [1500, 300, 777]
    fr = _frames(sizes, 8)
    recs, offs, _ = layout(fr, sizes, False, min_stride=1, pad_error=-7.0)
    counts = np.array([1500, 5000, 777], np.int32)     # frame 1 claims 5000 records; 300 exist, the buffer ends after it
    order = [0, 2, 1]
    fr2 = [fr[i] for i in order]
    recs = np.concatenate(fr2)
    offs = np.array([0, 1500 + 777, 1500, len(recs)], np.int32)
    with guarded_context(3) as g:
        H, nm = _run_find(g, [0, 1, 2], [1, 2, 3], recs, counts, offs, 0, 1000, max_pts=2000)
    assert nm[1] == -1 and np.array_equal(_bits(H[1]), _bits(IDENTITY)), nm
    for i, f in ((0, 0), (2, 2)):
        He, ne = _single_find(ctx, recs[span(offs, 0, f, int(counts[f]))].copy(), int(counts[f]), i + 1, 1000,
                              oracle=False)
        assert nm[i] == ne and np.array_equal(_bits(H[i]), _bits(He)), (i, nm[i], ne)


def _same_as_single(g, got, sel, seeds, recs, counts, offs, stride, max_pts, loops, what, oracle=True):
    """The way _check_find compares, with the frames over max_pts expected as -1 and the identity."""
    H, nm = g.download(got[0], (len(sel), 3, 3), np.float32), g.download(got[1], (len(sel),), np.int32)
    for i, (f, s) in enumerate(zip(sel, seeds)):
        n = max(int(counts[f]), 0)
        He, ne = (IDENTITY, -1) if n > max_pts else _single_find(g, recs[span(offs, stride, f, n)].copy(), n, s, loops,
                                                                 oracle)
        assert nm[i] == ne and np.array_equal(_bits(H[i]), _bits(He)), (what, i, f, n, nm[i], ne)
    return nm


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
def test_find_off_16_shapes(padded):
    """Frames of 9, 8, 7 and 40 records (one with exactly 8 valid records, one with 7), max_pts 9 and 40 (neither a
    multiple of 16; at 9 the 40-record frame is over it), 1 and 17 loops (worked over as 16 and 32): every stride of the
    temp is a rounded-up size, and every entry still equals the single call bit for bit."""
    sizes = [9, 8, 7, 40, 9]
    fr = [_gated(9, 31, 8), _gated(8, 32, 8), _gated(7, 33, 7), _gated(40, 34, 33), _gated(9, 35, 7)]
    recs, offs, stride = layout(fr, sizes, padded, min_stride=1, pad_error=-7.0)
    sel, seeds = [3, 0, 4, 2, 1], [5, 2**32 - 1, 7, 8, 0]
    with guarded_context(3) as g:
        d, dc = g.upload(recs), g.upload(np.asarray(sizes, np.int32))
        do = g.upload(offs) if offs is not None else None
        for max_pts in (9, 40):
            for loops in (1, 17):
                got = g.find_homography_batch(sel, seeds, d, len(sizes), dc, do, stride, max_pts=max_pts,
                                              num_loops=loops, **FIND)
                g.sync()
                nm = _same_as_single(g, got, sel, seeds, recs, sizes, offs, stride, max_pts, loops, (max_pts, loops))
                assert (nm[0] == -1) == (max_pts == 9) and nm[1] >= 4 and nm[4] >= 4, nm
                assert nm[2] == 0 and nm[3] == 0, nm              # 7 valid records; 7 records


def test_find_stale_temp():
    """The mirror of test_gpu_fundamental_edges.test_stale_temp with the homography search as the checked call.  The
    grow-only temp is shared: a 15-entry fundamental search at 200 loops and a brute-force match on other buffers, the
    2-entry homography search (9 and 8 records, 1 loop), a larger one (256 loops, max_pts 2048), the 2-entry one again;
    meta, hcount and sample of the small layout lie in bytes the other calls wrote in theirs.  Every buffer is uploaded
    first; the steps are then library calls only, with no synchronisation by the test until all are enqueued."""
    from batch_util import frames as match_frames
    from test_gpu_fundamental import COUNTS, MAX_PTS, SEEDS, SEL, make_batch
    big, boffs, bstride = layout(make_batch(), COUNTS, False, min_stride=2048, pad_error=-7.0)
    small_sizes = [9, 8]
    small, soffs, sstride = layout([_gated(9, 41, 8), _gated(8, 42, 8)], small_sizes, False, min_stride=1, pad_error=0.0)
    mrecs, moffs, _ = layout(match_frames([300, 280], 5, True), [300, 280], False, min_stride=0, pad_error=0.0)
    ssel, sseeds = [1, 0], [7, 2**32 - 1]
    with guarded_context(3) as g:
        d_big, d_bc, d_bo = g.upload(big), g.upload(np.asarray(COUNTS, np.int32)), g.upload(boffs)
        d_small, d_sc, d_so = g.upload(small), g.upload(np.asarray(small_sizes, np.int32)), g.upload(soffs)
        d_m, d_mc, d_mo = g.upload(mrecs), g.upload(np.array([300, 280], np.int32)), g.upload(moffs)
        dF, dFn = g.zeros(4 * 9 * len(SEL)), g.zeros(4 * len(SEL))
        outs = [(g.zeros(4 * 9 * n), g.zeros(4 * n)) for n in (2, len(SEL), 2)]
        g.sync()
        g.find_fundamental_batch(SEL, SEEDS, d_big, len(COUNTS), d_bc, d_bo, bstride, max_pts=MAX_PTS, num_loops=200,
                                 fundamental=dF, num_inliers=dFn)         # library calls only from here to the sync
        g.match_batch([(0, 1)], d_m, 2, d_mc, d_mo, 0)
        g.find_homography_batch(ssel, sseeds, d_small, 2, d_sc, d_so, sstride, max_pts=9, num_loops=1,
                                homography=outs[0][0], num_matches=outs[0][1], **FIND)
        g.find_homography_batch(SEL, SEEDS, d_big, len(COUNTS), d_bc, d_bo, bstride, max_pts=2048, num_loops=256,
                                homography=outs[1][0], num_matches=outs[1][1], **FIND)
        g.find_homography_batch(ssel, sseeds, d_small, 2, d_sc, d_so, sstride, max_pts=9, num_loops=1,
                                homography=outs[2][0], num_matches=outs[2][1], **FIND)
        g.sync()
        assert g.download(dFn, (len(SEL),), np.int32).max() >= 8     # the fundamental search ran
        for step, o in ((1, outs[0]), (3, outs[2])):
            nm = _same_as_single(g, o, ssel, sseeds, small, small_sizes, soffs, sstride, 9, 1, ("step", step))
            assert (nm >= 4).all(), nm
        nm = _same_as_single(g, outs[1], SEL, SEEDS, big, COUNTS, boffs, bstride, 2048, 256, ("step", 2),
                             oracle=False)
        assert (nm > 0).sum() >= 8, nm


def test_argument_errors(ctx):
    from cudasift_amd import capi
    L = capi.lib()
    recs = ctx.zeros(576 * 64)
    counts = ctx.upload(np.array([32, 32], np.int32))
    H = ctx.upload(np.full(18, 3.5, np.float32))
    num = ctx.upload(np.full(2, 77, np.int32))

    def find(frames, nsel=None, seeds=None, loops=100, max_pts=64, h=True, n=True):
        fr = np.ascontiguousarray(frames, np.int32)
        sd = np.ascontiguousarray(seeds if seeds is not None else [1] * len(fr), np.uint32)
        return L.misift_find_homography_batch(ctx.h, len(fr) if nsel is None else nsel, fr.ctypes.data, sd.ctypes.data,
                                              recs.ptr, 2, counts.ptr, None, 32, max_pts, loops, 0.85, 0.95, 5.0,
                                              H.ptr if h else None, num.ptr if n else None)

    def improve(frames, nsel=None, loops=5, h=True, n=True):
        fr = np.ascontiguousarray(frames, np.int32)
        return L.misift_improve_homography_batch(ctx.h, len(fr) if nsel is None else nsel, fr.ctypes.data, recs.ptr, 2,
                                                 counts.ptr, None, 32, loops, 0.0, 0.8, 3.0, H.ptr if h else None,
                                                 num.ptr if n else None)
    assert find([0], nsel=-1) == -1
    assert find([2]) == -1 and find([-1]) == -1
    assert find([0, 0]) == -1
    assert find([0], h=False) == -1 and find([0], n=False) == -1
    assert find([0], loops=0) == -1
    assert find([0], max_pts=0) == -1
    assert improve([0], nsel=-1) == -1
    assert improve([1, 2]) == -1 and improve([1, 1]) == -1
    assert improve([0], h=False) == -1 and improve([0], n=False) == -1
    assert improve([0], loops=-1) == -1
    ctx.sync()
    assert (ctx.download(H, (18,), np.float32) == 3.5).all() and (ctx.download(num, (2,), np.int32) == 77).all()
    assert find(np.zeros(0)) == 0 and improve(np.zeros(0)) == 0     # nsel == 0: nothing happens
    ctx.sync()
    assert (ctx.download(H, (18,), np.float32) == 3.5).all() and (ctx.download(num, (2,), np.int32) == 77).all()


def test_chain_behind_real_extraction(ctx):
    """misift_extract_batch_packed_async -> misift_match_batch (f, f + 1) -> find batch -> improve batch, with no host read
    in between, against the synchronous per-pair chain on the same records."""
    from cudasift_amd import capi
    o = orc()
    B, h, w, mp = 6, 480, 640, 4096
    frames = np.stack([synth_frame(f, w, h) for f in range(B)]).astype(np.float32)
    frames[1:] = np.stack([np.roll(frames[0], (2 * f, 3 * f), axis=(0, 1)) for f in range(1, B)])
    d = ctx.upload(frames)
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    pairs = [(f, f + 1) for f in range(B - 1)]
    sel = [f for f, _ in pairs]
    seeds = [100 + f for f in sel]
    ctx.match_batch(pairs, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0)
    dH, dn = ctx.find_homography_batch(sel, seeds, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp, num_loops=1000,
                                       min_score=0.0, max_ambiguity=0.80, thresh=5.0)
    dnf = ctx.improve_homography_batch(sel, packed, B, cnt.ptr, dH, cnt.ptr + 4 * B, 0, num_loops=5, **IMPROVE)
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    counts, offs = ci[:B], ci[B:]
    got = ctx.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    H = ctx.download(dH, (len(sel), 3, 3), np.float32)
    nm = ctx.download(dn, (len(sel),), np.int32)
    nf = ctx.download(dnf, (len(sel),), np.int32)
    assert (counts > 100).all(), counts
    for i, (f1, f2) in enumerate(pairs):
        n1, n2 = int(counts[f1]), int(counts[f2])
        s1, s2 = span(offs, 0, f1, n1), span(offs, 0, f2, n2)
        m = ctx.match(got[s1].copy(), n1, got[s2].copy(), n2)
        for k in ("score", "ambiguity", "match", "match_xpos", "match_ypos"):
            assert np.array_equal(m[k], got[s1][k]), (f1, k)
        dm = ctx.upload(m)
        o.srand(seeds[i])
        He, ne = ctx.find_homography(dm.ptr, n1, num_loops=1000, min_score=0.0, max_ambiguity=0.80, thresh=5.0)
        assert nm[i] == ne, (i, nm[i], ne)
        Hi, nfi = ctx.improve_homography(dm.ptr, n1, He, 5, **IMPROVE)
        after = ctx.download(dm, (n1,), capi.POINT_DTYPE)
        assert nf[i] == nfi and np.array_equal(_bits(H[i]), _bits(Hi)), (i, nf[i], nfi)
        assert after.tobytes() == got[s1].tobytes(), f1
    assert nm.max() > 50, nm

