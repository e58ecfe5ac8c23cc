"""Whole extraction calls off the default corner of their argument surface: texfrac_bits 23 / 0 (the Q8 = false
instantiations of every per-keypoint kernel a call launches), descr_occ 3, init_blur 0 / 0.5 / 2 through every prefilter,
lowest_scale on the batch path (and doubled by scale_up), and the state a context carries from one call to the next (the
cached tap tables, the graph key).  Inputs, oracle results and the case table: extract_cases.py; their premises:
test_extract_options_cpu.py.  Every comparison is compare_points with no outlier budget, plus numPts (and the 17 counters
of a single call)."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extract_cases as xc
from conftest import record
from extract_cases import expected, frames6, frames6_u8, gpu_args, small6
from util import compare_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_BIG = 48                      # word of a frame's counter block: keypoints deferred to descr_big
PITCH_U8 = 484                    # bytes per row of a padded 8-bit frame
PITCH_F32 = 512                   # floats per row of a resident fp32 frame (what capi.extract_batch makes of 483)


def _canon(recs):
    k = [recs[f].view(np.uint32) for f in ("orientation", "scale", "ypos", "xpos")]
    return recs[np.lexsort(k)].tobytes()


@contextlib.contextmanager
def options(c, **kw):
    saved = c.get_options()
    c.set_options(**kw)
    try:
        yield c
    finally:
        c.set_options(**{k: getattr(saved, k) for k in kw})


@contextlib.contextmanager
def fresh(knobs=(), **opts):
    from cudasift_amd import capi
    c = capi.Context(0)
    try:
        for k, v in dict(knobs).items():
            c.set_knob(k, v)
        if opts:
            c.set_options(**opts)
        yield c
    finally:
        c.close()


@contextlib.contextmanager
def profiled(c):
    c.profile_enable(True)
    c.profile_reset()
    try:
        yield c
    finally:
        c.profile_enable(False)


def check_batch(c, frames, name, ex=False, **kw):
    """frames through extract_batch (extract_batch_ex: 8-bit sources, scale_up) with the context's options as they are,
    against the oracle's records for the keywords kw.  Returns (points, numPts)."""
    ref, nref, _ = expected(frames, **kw)
    _, call = gpu_args(**kw)
    got, n = (c.extract_batch_ex if ex or frames.dtype == np.uint8 else c.extract_batch)(frames, **call)
    assert np.array_equal(n, nref), (name, n, nref)
    for f in range(len(frames)):
        compare_points(ref[f, :nref[f]], got[f, :n[f]], "options/%s/f%d" % (name, f), record)
    return got, n


def check_batch_u8_pitched(c, name, **kw):
    """frames6 as 8-bit frames with rows of PITCH_U8 bytes: dword-aligned rows, which the strip form of the fused prefilter
    asks of an 8-bit source (tightly packed rows of 483 bytes take launch_lowpass and a ScaleDown of its own)."""
    ref, nref, _ = expected(frames6(), **kw)
    _, call = gpu_args(**kw)
    host = np.zeros((6, xc.H, PITCH_U8), np.uint8)
    host[:, :, :xc.W] = frames6_u8()
    src = c.upload(host)
    pts = c.zeros(576 * call["max_pts"] * 6)
    rc, n = c.extract_batch_raw(src.ptr, True, 6, xc.H * PITCH_U8, xc.W, xc.H, PITCH_U8, None, pts.ptr, **call)
    assert rc == 0, (name, rc)
    assert np.array_equal(n, nref), (name, n, nref)
    from cudasift_amd import capi
    got = c.download(pts, (6, call["max_pts"]), capi.POINT_DTYPE)
    for f in range(6):
        compare_points(ref[f, :nref[f]], got[f, :n[f]], "options/%s/f%d" % (name, f), record)


def check_single(c, img, name, **kw):
    ref, nref, cref = expected(img, **kw)
    _, call = gpu_args(**kw)
    got, n, cnt = c.extract(img, **call)
    assert n == nref and np.array_equal(cnt, cref), (name, n, nref, cnt, cref)
    compare_points(ref[:nref], got[:n], "options/%s" % name, record)
    return got, n


def deferred(c, nframes):
    return [int(c.get_counter_block(f)[CNT_BIG]) for f in range(nframes)]


# ------------------------------------------------------------------ a. exact weights through every per-keypoint kernel
# (id, knobs, texfrac_bits, balanced): the 6-frame batch must report last_call_balanced() == balanced.
# What a row can and cannot show of its path.  balance = 0 is read back directly.  tile_orient = 1 and tile_descr = 0 are
# told from the default only through last_call_balanced() == 0 on six frames, which holds because prepare_block_maps builds
# no block tables under either knob: if it ever does, these two rows need another witness.  descr_occ has no read-back at
# all: the launch label is "descr_all" for <Q, 3, B> and <Q, 4, B> alike, so the occ3 rows rest on set_knob having taken
# the knob (test_a_misspelt_knob_is_refused: a name it does not know is an error, not a no-op) and on launch_descr_all's
# switch; they hold the records to the oracle whichever instantiation ran.
ROWS = [
    ("default", {}, 23, 1),                                       # orient_all_gather<false,true>, descr_all<false,4,true>
    ("unbalanced", {"balance": 0}, 23, 0),                        # orient_all_gather<false,false>, descr_all<false,4,false>
    ("occ3", {"descr_occ": 3}, 23, 1),                            # descr_all<false,3,true>
    ("occ3-unbalanced", {"descr_occ": 3, "balance": 0}, 23, 0),   # descr_all<false,3,false>
    ("occ3-bits8", {"descr_occ": 3}, 8, 1),                       # descr_all<true,3,true>
    ("occ3-unbalanced-bits8", {"descr_occ": 3, "balance": 0}, 8, 0),
    ("tile_orient", {"tile_orient": 1}, 23, 0),                   # orient_all_kernel<false> (no block tables with it)
    ("no_tile_descr", {"tile_descr": 0}, 23, 0),                  # descr_all_gather_kernel<false>
]


@pytest.mark.parametrize("name,knobs,bits,balanced", ROWS, ids=[r[0] for r in ROWS])
def test_batch_reaches_the_kernel_of_its_row(name, knobs, bits, balanced):
    with fresh(knobs, texfrac_bits=bits) as c, profiled(c):
        check_batch(c, frames6(), "a/" + name, fracbits=bits)
        prof = c.profile_read()
        assert c.last_call_balanced() == balanced
        assert prof["orient_all"]["calls"] == 1 and prof["descr_all"]["calls"] == 1 and "orient_descr" not in prof, prof
        assert c.descr_big_fallbacks() == 0 and sum(deferred(c, 6)) == 0
        assert c.get_options().texfrac_bits == bits


def test_a_misspelt_knob_is_refused():
    """The rows above select their kernels by name: every name is one the library lists, and one it does not know fails
    instead of leaving the default path in place."""
    from cudasift_amd import capi
    names = capi.knob_names()
    assert all(k in names for r in ROWS for k in r[1]) and "patch_reach" in names, names
    with fresh() as c:
        with pytest.raises(capi.MisiftError, match="unknown knob"):
            c.set_knob("descr_occ_", 3)
        c.set_knob("descr_occ", 3)


def test_zero_fraction_bits_take_the_exact_weight_kernels():
    """texfrac_bits = 0 is accepted and means what 23 means: the same bytes from the same context."""
    with fresh(texfrac_bits=23) as c:
        a, an = check_batch(c, frames6(), "a/bits23", fracbits=23)
        s, sn = check_single(c, frames6()[xc.SINGLE], "a/bits23/single", fracbits=23)
        c.set_options(texfrac_bits=0)
        assert c.get_options().texfrac_bits == 0
        b, bn = check_batch(c, frames6(), "a/bits0", fracbits=0)
        t, tn = check_single(c, frames6()[xc.SINGLE], "a/bits0/single", fracbits=0)
    assert np.array_equal(an, bn) and sn == tn
    for f in range(6):
        assert _canon(a[f, :an[f]]) == _canon(b[f, :bn[f]]), f
    assert _canon(s[:sn]) == _canon(t[:tn])


def test_small_batch_and_single_call_with_exact_weights():
    """A batch of three and a single call: plain grids, descr_all's folded tail (no descr_big launch: nothing deferred)."""
    with fresh(texfrac_bits=23) as c, profiled(c):
        check_batch(c, frames6()[:3], "a/three", fracbits=23)
        assert c.last_call_balanced() == 0 and sum(deferred(c, 3)) == 0
        check_single(c, frames6()[xc.SINGLE], "a/single", fracbits=23)
        prof = c.profile_read()
        assert c.last_call_balanced() == 0 and deferred(c, 1) == [0]
        assert prof["orient_all"]["calls"] == 2 and prof["descr_all"]["calls"] == 2, prof
        assert "descr_big" not in prof and "orient_descr" not in prof and c.descr_big_fallbacks() == 0


def test_descr_big_with_exact_weights():
    """patch_reach = 9 sends every keypoint of scale > 1.0 at its level to descr_big_kernel<false>: launched at once
    behind a batch, and by the host behind a folded single call once it has seen deferred keypoints in the counters."""
    with fresh({"patch_reach": 9.0}, texfrac_bits=23) as c, profiled(c):
        _, n = check_batch(c, frames6(), "a/big", fracbits=23)
        big = deferred(c, 6)
        assert all(b > 0.3 * k for b, k in zip(big, n)), (big, n)              # the rare path is the busy one here
        assert c.descr_big_fallbacks() == 0 and "descr_big" not in c.profile_read()      # part of the descr_all launch scope
        _, n1 = check_single(c, frames6()[xc.SINGLE], "a/big/single", fracbits=23)
        big1 = deferred(c, 1)[0]
        assert big1 > 0.3 * n1, (big1, n1)
        assert c.descr_big_fallbacks() == 1 and c.profile_read()["descr_big"]["calls"] == 1
        record("options/a/big", deferred=big, keypoints=n.tolist(), deferred_single=big1)


def test_eight_bit_source_with_exact_weights(ctx):
    with options(ctx, texfrac_bits=23):
        check_batch(ctx, frames6_u8(), "a/u8", fracbits=23)
        assert ctx.last_call_balanced() == 1


# ------------------------------------------------------------------ b. off-default blur through every prefilter
BLUR_CASES = [(0.0, 8), (0.5, 8), (2.0, 8), (0.5, 23)]


@pytest.mark.parametrize("blur,bits", BLUR_CASES)
def test_blur_through_every_prefilter(ctx, blur, bits):
    kw = dict(init_blur=blur, fracbits=bits)
    tag = "b/blur%.1f/bits%d" % (blur, bits)
    one = frames6()[xc.SINGLE]
    with options(ctx, texfrac_bits=bits), profiled(ctx):
        check_batch(ctx, frames6(), tag + "/six", **kw)                   # launch_lowpass_down (strips)
        check_batch(ctx, frames6()[:2], tag + "/two", **kw)               # launch_lowpass_down_tile
        check_single(ctx, one, tag + "/single", **kw)
        check_batch_u8_pitched(ctx, tag + "/u8_pitched", **kw)            # launch_lowpass_down from 8-bit rows
        prof = ctx.profile_read()
        assert prof["lowpass_down"]["calls"] == 4 and "lowpass" not in prof, prof
        check_batch(ctx, frames6_u8(), tag + "/u8", **kw)                 # packed 8-bit rows: launch_lowpass + ScaleDown
        prof = ctx.profile_read()
        assert prof["lowpass_down"]["calls"] == 4 and prof["lowpass"]["calls"] == 1, prof
        ctx.profile_reset()
        check_single(ctx, one, tag + "/one_octave", num_octaves=1, **kw)  # no ScaleDown: the plain launch_lowpass
        prof = ctx.profile_read()
        assert prof["lowpass"]["calls"] == 1 and "lowpass_down" not in prof, prof
    with fresh(fused=0, texfrac_bits=bits) as c, profiled(c):             # launch_lowpass and the dense kernels
        check_batch(c, frames6(), tag + "/dense", **kw)
        check_single(c, one, tag + "/dense_single", **kw)
        prof = c.profile_read()
        assert prof["lowpass"]["calls"] == 2 and "lowpass_down" not in prof and "descr_all" not in prof, prof
        assert prof["laplace"]["calls"] == 8 and prof["orient"]["calls"] == 8 and prof["descr"]["calls"] == 8, prof


def test_blur_through_the_packed_entry_point(ctx):
    """misift_extract_batch_packed_async with init_blur = 0.5: counts, offsets and records (d_pts = NULL when fused)."""
    from cudasift_amd import capi
    c, B, mp = ctx, 6, xc.ARGS["max_pts"]
    ref, nref, _ = expected(frames6(), init_blur=0.5)
    host = np.zeros((B, xc.H, PITCH_F32), np.float32)                    # 16-byte aligned rows: the strip prefilter
    host[:, :, :xc.W] = frames6()
    d = c.upload(host)
    scratch = capi.DevBuf(4 * capi.scratch_floats(xc.W, xc.H, 4, False) * B)
    cntb = c.zeros(4 * (2 * B + 1))
    packed = c.upload(np.full(576 * mp * B, 0xA5, np.uint8))
    dpts = None if c.get_options().fused else c.zeros(576 * mp * B)
    rc = c.extract_batch_packed_async_raw(d.ptr, B, xc.H * PITCH_F32, xc.W, xc.H, PITCH_F32, scratch.ptr,
                                          dpts.ptr if dpts is not None else None, cntb.ptr, cntb.ptr + 4 * B, packed.ptr,
                                          num_octaves=4, init_blur=0.5, thresh=3.0, lowest_scale=0.0, max_pts=mp)
    capi.check(rc, "misift_extract_batch_packed_async")
    c.sync()
    cb = c.download(cntb, (2 * B + 1,), np.int32)
    counts, offs = cb[:B], cb[B:]
    assert np.array_equal(counts, nref), (counts, nref)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), counts), (offs, counts)
    recs = c.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    for f in range(B):
        compare_points(ref[f, :nref[f]], recs[offs[f]:offs[f + 1]], "options/b/packed/f%d" % f, record)


# ------------------------------------------------------------------ c. scale floor on the batch path
@pytest.mark.parametrize("bits", [8, 23])
@pytest.mark.parametrize("floor", [xc.FLOOR_PARTIAL, xc.FLOOR_OCTAVES])
def test_scale_floor_on_the_batch_path(ctx, floor, bits):
    kw = dict(lowest_scale=floor, fracbits=bits)
    with options(ctx, texfrac_bits=bits):
        check_batch(ctx, frames6(), "c/floor%.1f/bits%d/six" % (floor, bits), **kw)
        assert ctx.last_call_balanced() == 1
        check_batch(ctx, frames6()[:3], "c/floor%.1f/bits%d/three" % (floor, bits), **kw)
        assert ctx.last_call_balanced() == 0


@pytest.mark.parametrize("bits", [8, 23])
def test_scale_floor_doubled_by_scale_up(ctx, bits):
    with options(ctx, texfrac_bits=bits):
        check_batch(ctx, small6(), "c/scale_up/bits%d" % bits, ex=True, lowest_scale=xc.FLOOR_PARTIAL, scale_up=True,
                    fracbits=bits)


# ------------------------------------------------------------------ d. nothing stale between calls
CONF = {"A": dict(), "B": dict(init_blur=0.5, fracbits=23), "C": dict(init_blur=2.0, num_octaves=3)}
SEQUENCE = "ABCABA"


class Resident:
    """Frames, arena and record array that stay where they are from call to call: a repeated call has the same key."""

    def __init__(self, c, frames):
        from cudasift_amd import capi
        self.c, self.frames = c, frames
        self.B = len(frames)
        self.mp = xc.ARGS["max_pts"]
        host = np.zeros((self.B, xc.H, PITCH_F32), np.float32)
        host[:, :, :xc.W] = frames
        self.d = c.upload(host)
        self.scratch = capi.DevBuf(4 * capi.scratch_floats(xc.W, xc.H, 4, False) * self.B)
        self.pts = c.zeros(576 * self.mp * self.B)

    def run(self, single, **kw):
        """-> (points [B, max_pts], numPts [B], counters of frame 0 after a single call)."""
        from cudasift_amd import capi
        c = self.c
        bits, call = gpu_args(**kw)
        c.set_options(texfrac_bits=bits)
        capi.check(capi.lib().misift_memset(c.h, self.pts.ptr, 0, self.pts.nbytes), "misift_memset")
        c.sync()
        if single:
            rc, n = c.extract_raw(self.d.ptr, xc.W, xc.H, PITCH_F32, self.scratch.ptr, self.pts.ptr, **call)
            n = np.array([n], np.int32)
        else:
            rc, n = c.extract_batch_raw(self.d.ptr, False, self.B, xc.H * PITCH_F32, xc.W, xc.H, PITCH_F32, self.scratch.ptr,
                                        self.pts.ptr, **call)
        capi.check(rc, "misift_extract*")
        return c.download(self.pts, (self.B, self.mp), capi.POINT_DTYPE), n, c.get_counters(0) if single else None


@pytest.mark.parametrize("graph", [0, 1], ids=["plain", "graph_replay"])
def test_nothing_stale_between_calls(graph):
    """One context, configurations A B C A B A (init_blur, texfrac_bits and num_octaves all change between neighbours), as
    a 6-frame batch and as a single call: every result is the oracle's for its own arguments, every repeat the same bytes
    as the first time.  With graph replay on, each configuration is called twice in a row: the second call has the key of the
    first and is the one the library replays — if capture succeeded.  enqueue_via_graph goes back to ordinary launches (and
    switches replay off) when capture or instantiation fails, and nothing the library exports tells the two apart, so this
    variant shows that no state goes stale with replay requested, not that hipGraphLaunch ran (test_gpu_parity.py's
    replay test has the same limit)."""
    from cudasift_amd import capi
    with fresh() as c:
        if graph:
            capi.check(capi.lib().misift_ctx_set_graph_replay(c.h, 1), "misift_ctx_set_graph_replay")
        for single in (False, True):
            frames = frames6()[xc.SINGLE:xc.SINGLE + 1] if single else frames6()
            res = Resident(c, frames)
            first = {}
            for step, conf in enumerate(SEQUENCE):
                kw = CONF[conf]
                for rep in range(1 + graph):
                    name = "options/d/%s/%s/%d%s.%d" % ("graph" if graph else "plain", "single" if single else "six", step,
                                                      conf, rep)
                    got, n, cnt = res.run(single, **kw)
                    if single:
                        ref, nref, cref = expected(frames[0], **kw)
                        assert n[0] == nref and np.array_equal(cnt, cref), (name, n, nref, cnt, cref)
                        ref, nref = ref[None], np.array([nref])
                    else:
                        ref, nref, _ = expected(frames, **kw)
                        assert np.array_equal(n, nref), (name, n, nref)
                    canon = []
                    for f in range(len(frames)):
                        compare_points(ref[f, :nref[f]], got[f, :n[f]], "%s/f%d" % (name, f), record)
                        canon.append(_canon(got[f, :n[f]]))
                    assert first.setdefault(conf, canon) == canon, name


# ------------------------------------------------------------------ e. the fused orientation + descriptor launch
CHILD = r"""
import json, sys, hashlib
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
from cudasift_amd import capi
from synth import synth_frame
import extract_cases as xc
ctx = capi.Context(0)
assert ctx.get_options().texfrac_bits == 23
out = []
for img, kw in ((xc.frames6()[1], xc.ARGS), (synth_frame(6, 1920, 1080), dict(num_octaves=5, thresh=3.0))):
    pts, n, cnt = ctx.extract(img, **kw)
    k = [pts[:n][f].view(np.uint32) for f in ("orientation", "scale", "ypos", "xpos")]
    out.append({"n": int(n), "cnt": cnt.tolist(), "sha": hashlib.sha256(pts[:n][np.lexsort(k)].tobytes()).hexdigest()})
print("RESULT " + json.dumps({"frames": out, "fallbacks": ctx.chain_fallbacks(), "fuse_fallbacks": ctx.fuse_fallbacks()}))
"""


def _child(env_extra):
    env = dict(os.environ, MISIFT_TUNABLES="1", MISIFT_TEXFRAC_BITS="23", **env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env_extra, r.stdout[-1500:], r.stderr[-1500:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_fused_orientation_and_descriptor_launch_with_exact_weights():
    """orient_descr_fused_kernel<false, 3>: one launch for a single call's orientations and descriptors (it waits inside
    the launch, hence the child process under a time limit).  Same records as the two launches, the oracle's counters."""
    from synth import synth_frame
    fused = _child({"MISIFT_FUSE_ORIENT": "1"})
    plain = _child({})
    assert fused["fuse_fallbacks"] == 0 and plain["fuse_fallbacks"] == 0, (fused, plain)
    assert fused["frames"] == plain["frames"]
    refs = (expected(frames6()[1], fracbits=23), expected(synth_frame(6, 1920, 1080), fracbits=23, num_octaves=5,
                                                           max_pts=32768))
    for got, (_, nref, cref) in zip(fused["frames"], refs):
        assert got["n"] == nref and got["cnt"] == cref.tolist(), (got["n"], nref, got["cnt"], cref)
    record("options/e/fused_exact_weights", keypoints=[f["n"] for f in fused["frames"]])
