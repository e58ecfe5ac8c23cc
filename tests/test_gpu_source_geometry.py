"""Extraction and the stage calls on the sources include/misift.h promises to accept but capi's helpers never make: a
sub-rectangle of a larger image, an odd pitch, frames with a gap or an odd stride between them, rows whose padding is
not zero, destinations that are no 128-float pitched allocation, and a scratch arena at an offset inside a pool.

Every case places the same pixels (geometry_util.crop) into a buffer of hostile values — quiet NaN for fp32, a 0 / 255
checkerboard for 8-bit — at (base, pitch, frame stride) and hands the library a pointer into it.  Then
  1. every pyramid level of every frame, read from the caller's arena through misift_test_pyramid_layout, equals the
     oracle's chain lowpass -> scaledown -> ... bit for bit (borders and clamps included),
  2. numPts (single calls: all 17 counters) and the records equal the oracle's (util.compare_points, unchanged),
  3. in canonical order the fields ExtractSift writes are byte-identical to the same context's extraction of the same
     pixels from a fresh 128-float pitched allocation,
  4. for batches of 5 and 8 frames the profile shows the launches the geometry is meant to reach,
and the source buffer still holds the bytes that were uploaded.  The whole module also runs under MISIFT_GUARD=1."""
import functools

import numpy as np
import pytest

import geometry_util as gu
from conftest import record
from test_gpu_guard import _canon
from util import compare_points

pytestmark = pytest.mark.gpu

NOCT, UP_NOCT, BLUR, THRESH, MAX_PTS = 4, 3, 1.0, 2.5, 8192
EINVAL = -1
POISON = 0x7FC0BAD1            # arenas and destinations start as this quiet NaN


def _capi():
    from cudasift_amd import capi
    return capi


def _orc():
    from oracle import pyoracle
    return pyoracle


@functools.lru_cache(maxsize=None)
def _oracle(f, w, u8, scale_up):
    """(records, numPts, counters, pyramid levels finest first) of the oracle for frame f at width w: once per (pixels,
    parameters), shared by every geometry."""
    h, noct = gu.height_for(w), UP_NOCT if scale_up else NOCT
    pix = gu.crop(f, w, h, u8).astype(np.float32)
    pts, n, cnt = _orc().extract(pix, num_octaves=noct, init_blur=BLUR, thresh=THRESH, scale_up=scale_up, max_pts=MAX_PTS)
    assert n > 100, ("the test pixels must give every frame more than 100 keypoints", f, w, u8, scale_up, n)
    lvl = _orc().lowpass(_orc().scaleup(pix) if scale_up else pix, BLUR)
    pyr = [lvl]
    for _ in range(noct - 1):
        lvl = _orc().scaledown(lvl)
        pyr.append(lvl)
    return pts, n, cnt, pyr


class _Fused:
    """ctx.set_options(fused=...) for the length of a with block."""

    def __init__(self, ctx, fused):
        self.ctx, self.fused = ctx, fused

    def __enter__(self):
        self.saved = self.ctx.get_options().fused
        self.ctx.set_options(fused=self.fused)

    def __exit__(self, *exc):
        self.ctx.set_options(fused=self.saved)


def _run(ctx, w, B, name, u8=False, scale_up=False, single=False, k=0, profile=False):
    """One extraction of frames 0 .. B-1 at width w from geometry `name`, with the arena at float offset k of its
    allocation.  Checks on the way that the source kept its bytes and that nothing was written in front of or behind
    the arena.  Returns {rc, n[B], recs[B, MAX_PTS], counters[B][17], pyr[B][level], prof}."""
    capi = _capi()
    h, noct = gu.height_for(w), UP_NOCT if scale_up else NOCT
    frames = np.stack([gu.crop(f, w, h, u8) for f in range(B)])
    base, pitch, stride = gu.geometry(name, w, h)
    host = gu.place(frames, base, pitch, stride)
    assert gu.same_bytes(gu.read_back(host, base, pitch, stride, B, h, w), frames)
    src = ctx.upload(host)
    S = capi.scratch_floats(w, h, noct, scale_up)
    arena = ctx.upload(np.full(S * B + 4, POISON, np.uint32))
    pts = ctx.zeros(576 * MAX_PTS * B)
    before = ctx.download(pts, (576 * MAX_PTS * B,), np.uint8)
    kw = dict(num_octaves=noct, init_blur=BLUR, thresh=THRESH, scale_up=scale_up, max_pts=MAX_PTS)
    if profile:
        ctx.profile_reset()
        ctx.profile_enable(True)
    try:
        if single:
            assert B == 1 and not u8
            rc, n = ctx.extract_raw(src.ptr + host.itemsize * base, w, h, pitch, arena.ptr + 4 * k, pts.ptr, **kw)
            n = np.array([n], np.int32)
        else:
            rc, n = ctx.extract_batch_raw(src.ptr + host.itemsize * base, u8, B, stride, w, h, pitch, arena.ptr + 4 * k,
                                          pts.ptr, **kw)
        ctx.sync()
        prof = ctx.profile_read() if profile else None
    finally:
        if profile:
            ctx.profile_enable(False)
    assert gu.same_bytes(ctx.download(src, host.shape, host.dtype), host), "the const source was written"
    mem = ctx.download(arena, (S * B + 4,), np.uint32)
    assert (mem[:k] == POISON).all() and (mem[k + S * B:] == POISON).all(), "a write outside the arena"
    out = dict(rc=rc, n=n, prof=prof)
    if rc != 0:
        assert (mem == POISON).all(), "a refused call wrote into the arena"
        assert gu.same_bytes(ctx.download(pts, before.shape, np.uint8), before), "a refused call wrote records"
        return out
    out["recs"] = ctx.download(pts, (B, MAX_PTS), capi.POINT_DTYPE)
    out["counters"] = [ctx.get_counters(f) for f in range(B)]
    lay = capi.pyramid_layout(w, h, noct, scale_up)
    fl = mem.view(np.float32)
    out["pyr"] = [[fl[k + f * S + off:k + f * S + off + lh * lp].reshape(lh, lp)[:, :lw] for off, lw, lh, lp in lay]
                  for f in range(B)]
    return out


_REFERENCE = {}


def _reference(ctx, w, B, u8, scale_up, single):
    """The same context's extraction of the same pixels from a 128-float pitched allocation (what capi.upload_image
    makes), with the arena at the start of its allocation: once per context and case, shared by the geometries."""
    key = (ctx.h, ctx.get_options().fused, w, B, u8, scale_up, single)
    if key not in _REFERENCE:
        _REFERENCE[key] = _run(ctx, w, B, "pitch128", u8, scale_up, single)
        assert _REFERENCE[key]["rc"] == 0
    return _REFERENCE[key]


def _check(ctx, res, w, B, u8, scale_up, single, what):
    assert res["rc"] == 0, (what, res["rc"], _capi().lib().misift_last_error())
    ref = _reference(ctx, w, B, u8, scale_up, single)
    for f in range(B):
        opts, on, ocnt, opyr = _oracle(f, w, u8, scale_up)
        # 1. every pixel of every pyramid level
        assert len(res["pyr"][f]) == len(opyr)
        for lev, (got, want) in enumerate(zip(res["pyr"][f], opyr)):
            assert got.shape == want.shape, (what, f, lev, got.shape, want.shape)
            if not gu.same_bytes(got, want):
                bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != want.view(np.uint32))
                raise AssertionError("%s: frame %d pyramid level %d differs from the oracle at %d pixels, first (y, x) = %s, "
                                     "last %s" % (what, f, lev, len(bad), bad[0].tolist(), bad[-1].tolist()))
        # 2. records against the oracle
        n = int(res["n"][f])
        assert n == on, (what, f, n, on)
        if single:
            assert np.array_equal(res["counters"][f], ocnt), (what, res["counters"][f], ocnt)
        compare_points(opts[:on], res["recs"][f, :n], "%s/f%d" % (what, f))
        # 3. records against the pitched control of the same context
        assert n == int(ref["n"][f]), (what, f, n, ref["n"][f])
        assert _canon(res["recs"][f, :n]) == _canon(ref["recs"][f, :n]), (what, f, "records differ from the pitched control")


def _check_profile(prof, w, B, name, noct, fused=True, scale_up=False):
    """4. the launches the geometry is meant to reach (batches above small_frames = 4: the strip prefilter)."""
    calls = {k: v["calls"] for k, v in prof.items()}
    h = gu.height_for(w)
    aligned = gu.source_aligned(name, w, h, B) or scale_up        # (under scale_up the prefilter reads the arena's doubled frame)
    if scale_up:
        assert calls.get("scaleup") == 1, calls
    if aligned and fused:
        assert calls.get("lowpass_down") == 1 and "lowpass" not in calls, (name, w, B, calls)
        assert calls.get("scaledown", 0) == noct - 2, (name, w, B, calls)
        # split_tail = 8: the two finest levels are scanned beside the coarse pyramid, in a launch of their own
        assert calls.get("dog_scan") == (2 if B >= 8 and noct >= 3 else 1), (name, w, B, calls)
    else:
        assert calls.get("lowpass") == 1 and "lowpass_down" not in calls, (name, w, B, calls)
        assert calls.get("scaledown", 0) == noct - 1, (name, w, B, calls)
        if fused:
            assert calls.get("dog_scan") == 1, (name, w, B, calls)
    return calls


# ------------------------------------------------------------------------------------------- extraction, fp32
@pytest.mark.parametrize("w", [320, 321, 322, 323])
@pytest.mark.parametrize("name", gu.SINGLE)
def test_single_call(ctx, name, w):
    """misift_extract (tiled prefilter, ScaleDown chain inside the scan launch)."""
    res = _run(ctx, w, 1, name, single=True)
    _check(ctx, res, w, 1, False, False, True, "single/%s/%d" % (name, w))


@pytest.mark.parametrize("w", [320, 322, 323])
@pytest.mark.parametrize("name", gu.BATCH)
@pytest.mark.parametrize("B", [3, 5, 8])
def test_batch_fp32(ctx, B, name, w):
    """misift_extract_batch_ex: B = 3 the tiled prefilter and the chain, B = 5 the strip prefilter and one ScaleDown per
    level, B = 8 the split tail where the source qualifies."""
    res = _run(ctx, w, B, name, profile=B > 4)
    what = "batch%d/%s/%d" % (B, name, w)
    _check(ctx, res, w, B, False, False, False, what)
    if B > 4:
        record("geometry/" + what, launches=_check_profile(res["prof"], w, B, name, NOCT))


# ------------------------------------------------------------------------------------------- 8-bit sources
@pytest.mark.parametrize("w", [320, 321, 323])
@pytest.mark.parametrize("B,name", [(1, g) for g in gu.SINGLE] + [(5, g) for g in gu.BATCH])
def test_batch_u8(ctx, B, name, w):
    res = _run(ctx, w, B, name, u8=True, profile=B > 4)
    what = "u8_batch%d/%s/%d" % (B, name, w)
    _check(ctx, res, w, B, True, False, False, what)
    if B > 4:
        record("geometry/" + what, launches=_check_profile(res["prof"], w, B, name, NOCT))


# ------------------------------------------------------------------------------------------- scale_up
@pytest.mark.parametrize("name", ["roi", "roi+1", "oddpitch"])
@pytest.mark.parametrize("u8,B", [(False, 1), (True, 5)])
def test_scale_up(ctx, u8, B, name):
    res = _run(ctx, 322, B, name, u8=u8, scale_up=True, single=not u8, profile=B > 4)
    what = "up_u8%d_batch%d/%s" % (u8, B, name)
    _check(ctx, res, 322, B, u8, True, not u8, what)
    if B > 4:
        record("geometry/" + what, launches=_check_profile(res["prof"], 322, B, name, UP_NOCT, scale_up=True))


# ------------------------------------------------------------------------------------------- dense kernels
@pytest.mark.parametrize("w", [320, 323])
@pytest.mark.parametrize("name", ["roi+1", "oddpitch", "padded"])
@pytest.mark.parametrize("B", [1, 5])
def test_dense_kernels(ctx, B, name, w):
    """fused = 0: LowPass, one ScaleDown per level, LaplaceMulti / FindPointsMulti per octave."""
    with _Fused(ctx, 0):
        res = _run(ctx, w, B, name, single=B == 1, profile=B > 4)
        what = "dense_batch%d/%s/%d" % (B, name, w)
        _check(ctx, res, w, B, False, False, B == 1, what)
    if B > 4:
        calls = _check_profile(res["prof"], w, B, name, NOCT, fused=False)
        assert calls.get("laplace") == NOCT and "dog_scan" not in calls, calls
        record("geometry/" + what, launches=calls)


# ------------------------------------------------------------------------------------------- packed, asynchronous
def _packed(ctx, w, B, name):
    capi = _capi()
    h = gu.height_for(w)
    frames = np.stack([gu.crop(f, w, h) for f in range(B)])
    base, pitch, stride = gu.geometry(name, w, h)
    host = gu.place(frames, base, pitch, stride)
    src = ctx.upload(host)
    arena = capi.DevBuf(4 * capi.scratch_floats(w, h, NOCT, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * MAX_PTS * B)
    rc = ctx.extract_batch_packed_async_raw(src.ptr + 4 * base, B, stride, w, h, pitch, arena.ptr, None, cnt.ptr,
                                            cnt.ptr + 4 * B, packed.ptr, num_octaves=NOCT, init_blur=BLUR, thresh=THRESH,
                                            max_pts=MAX_PTS)
    capi.check(rc, "misift_extract_batch_packed_async")
    ctx.sync()
    assert gu.same_bytes(ctx.download(src, host.shape, host.dtype), host), "the const source was written"
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    return ci[:B].copy(), ci[B:].copy(), ctx.download(packed, (int(ci[2 * B]),), capi.POINT_DTYPE)


@pytest.mark.parametrize("w", [320, 323])
@pytest.mark.parametrize("name", ["roi+1", "oddstride+1", "oddstride+2"])
def test_packed_async(ctx, name, w):
    B = 5
    counts, offs, recs = _packed(ctx, w, B, name)
    rcounts, roffs, rrecs = _packed(ctx, w, B, "pitch128")
    want = [_oracle(f, w, False, False) for f in range(B)]
    assert counts.tolist() == [o[1] for o in want]
    assert np.array_equal(counts, rcounts) and np.array_equal(offs, roffs)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), counts)
    for f in range(B):
        mine = recs[offs[f]:offs[f + 1]]
        compare_points(want[f][0][:want[f][1]], mine, "packed/%s/%d/f%d" % (name, w, f))
        assert _canon(mine) == _canon(rrecs[roffs[f]:roffs[f + 1]]), (name, w, f)


# ------------------------------------------------------------------------------------------- arena at an offset
# Every kernel that forms an address from the scratch pointer either takes an alignment flag (lowpass, scaledown,
# lowpass_down, the tiled prefilter's pair stores, laplace, detect, the merged scan) or works on single floats (the
# ScaleDown chain, refine_all, the window loads of the orientation and descriptor kernels), so an arena at any float
# offset runs: on the generic kernels, with the same results.
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("w", [320, 323])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("mode", ["fp32", "scale_up", "dense"])
def test_offset_scratch(ctx, mode, B, w, k):
    up = mode == "scale_up"
    with _Fused(ctx, 0 if mode == "dense" else ctx.get_options().fused):
        res = _run(ctx, w, B, "tight", scale_up=up, single=B == 1, k=k)
        _check(ctx, res, w, B, False, up, B == 1, "offset_scratch+%d/%s/batch%d/%d" % (k, mode, B, w))


# ------------------------------------------------------------------------------------------- stage calls
STAGE_SHAPES = [(321, 67), (320, 66)]


@functools.lru_cache(maxsize=None)
def _stage_pixels(w, h):
    rng = np.random.default_rng(w * 1009 + h)
    return _orc().lowpass((rng.random((h, w), dtype=np.float32) * 255.0).astype(np.float32), 0.7)


@functools.lru_cache(maxsize=None)
def _stage_oracle(stage, w, h):
    img = _stage_pixels(w, h)
    if stage == "lowpass":
        return _orc().lowpass(img, 1.3)[None]
    if stage == "scaledown":
        return _orc().scaledown(img)[None]
    if stage == "scaleup":
        return _orc().scaleup(img)[None]
    if stage == "laplace":
        return _orc().laplace(img, 4, 2)
    raise KeyError(stage)


def _stage_source(ctx, w, h, name):
    base, pitch, stride = gu.geometry(name, w, h)
    host = gu.place(_stage_pixels(w, h)[None], base, pitch, stride)
    return host, ctx.upload(host), base, pitch


def _dest(ctx, k, dpitch, plane, nplanes, oh, ow):
    """A poisoned destination whose output rectangle(s) start k floats in; 64 floats of slack behind the last row."""
    n = gu.buffer_elems(k, dpitch, plane, nplanes, oh, ow, slack=64)
    return ctx.upload(np.full(n, POISON, np.uint32)), n


def _dest_check(ctx, dst, n, k, dpitch, plane, want, what):
    nplanes, oh, ow = want.shape
    got = ctx.download(dst, (n,), np.uint32)
    rect = gu.read_back(got, k, dpitch, plane, nplanes, oh, ow).view(np.float32)
    if not gu.same_bytes(rect, want):
        bad = np.argwhere(rect.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d output pixels differ from the oracle, first (plane, y, x) = %s, last %s"
                             % (what, len(bad), bad[0].tolist(), bad[-1].tolist()))
    rest = gu.outside(got, k, dpitch, plane, nplanes, oh, ow)
    assert (rest == POISON).all(), "%s: %d floats outside the output rectangle were written" % (what, int((rest != POISON).sum()))


def _dest_untouched(ctx, dst, n, what):
    assert (ctx.download(dst, (n,), np.uint32) == POISON).all(), "%s: a refused call wrote to its destination" % what


@pytest.mark.parametrize("w,h", STAGE_SHAPES)
@pytest.mark.parametrize("name", gu.SINGLE)
@pytest.mark.parametrize("stage", ["lowpass", "scaledown", "scaleup"])
def test_stage_calls(ctx, stage, name, w, h):
    L = _capi().lib()
    host, src, base, pitch = _stage_source(ctx, w, h, name)
    want = _stage_oracle(stage, w, h)
    _, oh, ow = want.shape
    pitches = (ow, ow + 2) if stage == "scaleup" else (ow, ow + 1)
    for dpitch in pitches:
        for k in range(4):
            what = "%s/%s/%dx%d/dpitch%d/k%d" % (stage, name, w, h, dpitch, k)
            dst, n = _dest(ctx, k, dpitch, 0, 1, oh, ow)
            if stage == "lowpass":
                rc = L.misift_lowpass(ctx.h, src.ptr + 4 * base, w, h, pitch, dst.ptr + 4 * k, dpitch, 1.3)
            elif stage == "scaledown":
                rc = L.misift_scaledown(ctx.h, src.ptr + 4 * base, w, h, pitch, dst.ptr + 4 * k, dpitch)
            else:
                rc = L.misift_scaleup(ctx.h, src.ptr + 4 * base, w, h, pitch, dst.ptr + 4 * k, dpitch)
            assert rc == 0, (what, rc, L.misift_last_error())
            _dest_check(ctx, dst, n, k, dpitch, 0, want, what)
    if stage == "scaleup":                   # an odd dpitch is refused and nothing is written
        dst, n = _dest(ctx, 0, ow + 1, 0, 1, oh, ow)
        assert L.misift_scaleup(ctx.h, src.ptr + 4 * base, w, h, pitch, dst.ptr, ow + 1) == EINVAL
        ctx.sync()
        _dest_untouched(ctx, dst, n, "scaleup/odd dpitch")
    assert gu.same_bytes(ctx.download(src, host.shape, host.dtype), host), "the const source was written"


@pytest.mark.parametrize("w,h", STAGE_SHAPES)
@pytest.mark.parametrize("name", gu.SINGLE)
def test_stage_laplace(ctx, name, w, h):
    """misift_laplace: 7 DoG planes with the SOURCE's pitch, plane stride height * pitch, at a destination offset."""
    L = _capi().lib()
    host, src, base, pitch = _stage_source(ctx, w, h, name)
    want = _stage_oracle("laplace", w, h)
    for k in range(4):
        what = "laplace/%s/%dx%d/k%d" % (name, w, h, k)
        dst, n = _dest(ctx, k, pitch, h * pitch, 7, h, w)
        rc = L.misift_laplace(ctx.h, src.ptr + 4 * base, w, h, pitch, 4, 2, dst.ptr + 4 * k)
        assert rc == 0, (what, rc, L.misift_last_error())
        _dest_check(ctx, dst, n, k, pitch, h * pitch, want, what)
    assert gu.same_bytes(ctx.download(src, host.shape, host.dtype), host), "the const source was written"


@pytest.mark.parametrize("w,h", STAGE_SHAPES)
@pytest.mark.parametrize("name", gu.SINGLE)
def test_stage_lowpass_scaledown(ctx, name, w, h):
    """The fused stage call needs 16-byte aligned rows of source and destination and 8-byte aligned rows of the decimated
    destination (include/misift.h): everything else is MISIFT_EINVAL with nothing written; where it runs it equals the
    oracle's — and so the two separate calls' — pixels, and writes nothing but them."""
    L = _capi().lib()
    host, src, base, pitch = _stage_source(ctx, w, h, name)
    lp = _stage_oracle("lowpass", w, h)
    dn = _orc().scaledown(lp[0])[None]
    w2, h2 = w // 2, h // 2
    ran = 0
    for dpitch, dpitch2 in ((w, w2), (w + 1, w2 + 1), ((w + 3) // 4 * 4, (w2 + 1) // 2 * 2), ((w + 3) // 4 * 4 + 4, w2 + 2 + w2 % 2)):
        for k in range(4):
            for k2 in (0, 1, 2):
                what = "lowpass_scaledown/%s/%dx%d/dpitch%d,%d/k%d,%d" % (name, w, h, dpitch, dpitch2, k, k2)
                dst, n = _dest(ctx, k, dpitch, 0, 1, h, w)
                dst2, n2 = _dest(ctx, k2, dpitch2, 0, 1, h2, w2)
                rc = L.misift_lowpass_scaledown(ctx.h, src.ptr + 4 * base, w, h, pitch, dst.ptr + 4 * k, dpitch, 1.3,
                                                dst2.ptr + 4 * k2, dpitch2)
                ctx.sync()
                supported = (gu.source_aligned(name, w, h) and k == 0 and dpitch % 4 == 0 and k2 % 2 == 0
                             and dpitch2 % 2 == 0)
                if supported:
                    assert rc == 0, (what, rc, L.misift_last_error())
                    _dest_check(ctx, dst, n, k, dpitch, 0, lp, what)
                    _dest_check(ctx, dst2, n2, k2, dpitch2, 0, dn, what + " (decimated)")
                    ran += 1
                else:
                    assert rc == EINVAL, (what, rc)
                    _dest_untouched(ctx, dst, n, what)
                    _dest_untouched(ctx, dst2, n2, what)
    assert (ran > 0) == (name in ("roi", "padded") or (name == "tight" and w % 4 == 0)), (name, w, ran)
    assert gu.same_bytes(ctx.download(src, host.shape, host.dtype), host), "the const source was written"
