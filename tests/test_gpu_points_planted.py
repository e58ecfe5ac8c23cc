"""The production per-keypoint kernels — bin_detections, orient_all (gather and LDS-window forms), renumber_dups,
descr_all (LDS window), descr_all_gather, descr_big, the balanced block tables — on PLANTED detections
(Context.describe_detections / misift_test_describe_detections), against the oracle's answer to the same detections.

The cases and what each is aimed at: points_cases.py; that they reach it: test_points_cases_cpu.py.  Every comparison is
util.compare_points unchanged (orientation and scale bit-identical, every descriptor element within DESC_ATOL, no
outliers, no NaN) plus the 17 counters, numPts, the segment a record lies in, and the untouched rest of the record array.
Every context here is guarded (64 KiB bands around every device allocation, output arrays start as 0xFF bytes)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import points_cases as pc
from batch_util import guarded_context
from conftest import record
from util import compare_points

pytestmark = pytest.mark.gpu
M = 4096                          # records per frame: roomy for every case
CNT_BIG = 48                      # word of a frame's counter block: keypoints deferred to descr_big
DEFAULTS = dict(bin=1, balance=1, tile_descr=1, tile_orient=0, descr_occ=4, fold_tail=1, fuse_orient=0, bin_min_frames=4,
                small_frames=4, patch_reach=17.9)


@contextlib.contextmanager
def guarded(knobs=(), **opts):
    """A fresh guarded context with the library's default launch structure (whatever the environment of a variant run
    made of it), then the named knobs and options."""
    with guarded_context(1) as c:
        c.poison_outputs = True
        for k, v in dict(DEFAULTS, **dict(knobs)).items():
            c.set_knob(k, v)
        c.set_options(**dict(dict(fused=1, fix_numpts=0, deterministic=0, texfrac_bits=8), **opts))
        yield c


@pytest.fixture(scope="module")
def dctx():
    """The default context of this module: one for all single-frame tests, so a call also follows other shapes' calls."""
    with guarded() as c:
        yield c


def run(c, cases, max_pts=M, scale_up=False):
    return c.describe_detections([k["levels"] for k in cases], [k["dets"] for k in cases], max_pts, scale_up)


def check_frame(name, case, got, n, cnt, max_pts=M, **kw):
    """One frame of a call against the oracle: numPts, all 17 counters, every written record, nothing else written."""
    ref, nref, cref, _ = pc.expected(case, max_pts, **kw)
    assert n == nref, (name, n, nref)
    assert np.array_equal(cnt, cref), (name, cnt, cref)
    tot = pc.written(cref, case["geom"][2], max_pts)
    assert np.array_equal(got["subsampling"][:tot], ref["subsampling"][:tot]), name        # every record in its octave's segment
    st = compare_points(ref[:tot], got[:tot], name, record) if tot else None
    assert (got[tot:].view(np.uint8) == 0xFF).all(), name                                 # the rest keeps its poison
    return st


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_every_case_class(dctx, name):
    """One frame through the single-call shape: no binning, descr_all exports the counters and descr_big is launched only
    when the host finds a deferred keypoint in them."""
    case = pc.case(name)
    before = dctx.descr_big_fallbacks()
    pts, n, cnt = run(dctx, [case])
    assert dctx.last_call_balanced() == 0
    check_frame("planted/" + name, case, pts[0], n[0], cnt[0])
    nbig = pc.count_big(case, M)
    assert int(dctx.get_counter_block(0)[CNT_BIG]) == nbig, name
    assert dctx.descr_big_fallbacks() - before == (1 if nbig else 0), name


@pytest.mark.parametrize("knobs", [{}, {"bin": 0}, {"balance": 0}, {"tile_descr": 0}, {"tile_orient": 1}, {"descr_occ": 3}],
                         ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()) or "default")
def test_five_frames_in_one_call(knobs):
    """Different cases per frame and one frame without a detection: binned and balanced by default, then each launch
    structure switched on its own."""
    frames = pc.multi_frames()
    with guarded(knobs) as c:
        pts, n, cnt = run(c, frames)
        balanced = knobs.get("balance", 1) and knobs.get("tile_descr", 1) and not knobs.get("tile_orient", 0)
        assert c.last_call_balanced() == (1 if balanced else 0), knobs
        tag = ",".join("%s=%s" % kv for kv in knobs.items()) or "default"
        for f, case in enumerate(frames):
            check_frame("planted/five[%s]/f%d_%s" % (tag, f, case["name"]), case, pts[f], n[f], cnt[f])
            if knobs.get("tile_descr", 1):
                assert int(c.get_counter_block(f)[CNT_BIG]) == pc.count_big(case, M), (knobs, f)
        assert n[pc.MULTI.index(None)] == 0 and not cnt[pc.MULTI.index(None)].any()


@pytest.mark.parametrize("bits", [8, 23])
def test_texture_weight_bits(bits):
    with guarded(texfrac_bits=bits) as c:
        for name in ("thresholds", "small", "reach"):
            case = pc.case(name)
            pts, n, cnt = run(c, [case])
            check_frame("planted/texfrac%d/%s" % (bits, name), case, pts[0], n[0], cnt[0], fracbits=bits)
        frames = pc.multi_frames()
        pts, n, cnt = run(c, frames)
        for f, case in enumerate(frames):
            check_frame("planted/texfrac%d/five_f%d" % (bits, f), case, pts[f], n[f], cnt[f], fracbits=bits)


@pytest.mark.parametrize("fix", [0, 1])
def test_scale_up_with_and_without_fix_numpts(fix):
    """out_scale = 0.5: every record is halved but the finest octave's second orientations, which lie behind numPts
    (Appendix B #1) — unless fix_numpts puts them inside."""
    with guarded(fix_numpts=fix) as c:
        for name in ("dups", "small", "border"):
            case = pc.case(name)
            noct = case["geom"][2]
            pts, n, cnt = run(c, [case], scale_up=True)
            check_frame("planted/scaleup_fix%d/%s" % (fix, name), case, pts[0], n[0], cnt[0], scale_up=True, fix_numpts=bool(fix))
            assert n[0] == int(cnt[0][2 * noct + fix])
        assert int(cnt[0][2 * noct + 1]) > int(cnt[0][2 * noct])             # the last case has second orientations there
        frames = pc.multi_frames()
        pts, n, cnt = run(c, frames, scale_up=True)
        for f, case in enumerate(frames):
            check_frame("planted/scaleup_fix%d/five_f%d" % (fix, f), case, pts[f], n[f], cnt[f], scale_up=True,
                        fix_numpts=bool(fix))


def test_deterministic_mode_repeats_byte_for_byte():
    with guarded(deterministic=1) as c:
        for cases in ([pc.case("interior")], [pc.case("dups")], pc.multi_frames()):
            a, an, ac = run(c, cases)
            b, bn, bc = run(c, cases)
            assert np.array_equal(an, bn) and np.array_equal(ac, bc)
            assert a.tobytes() == b.tobytes()
            for f, case in enumerate(cases):
                check_frame("planted/deterministic/%d_f%d_%s" % (len(cases), f, case["name"]), case, a[f], an[f], ac[f])


def test_capacity_inside_octave_two():
    """max_pts cuts inside octave 2's detections, in deterministic mode and with the records supplied in the order that
    mode gives the staging area (points_cases.tile_order), so that WHICH records survive is defined on both sides: the
    records below capacity match; counters below the capacity match and the others are at or over it (the rule of
    test_extract_options_and_edge_cases: over capacity the duplicate counts depend on what was kept)."""
    case = pc.tile_order(pc.case("interior"))
    cap = 200
    ref, nref, cref, _ = pc.expected(case, cap)
    assert int(cref[3]) < cap < int(cref[4]) and nref == cap
    with guarded(deterministic=1) as c:
        a, an, ac = run(c, [case], max_pts=cap)
        b, bn, bc = run(c, [case], max_pts=cap)
        assert a.tobytes() == b.tobytes() and np.array_equal(ac, bc)
        assert an[0] == nref == cap
        below = cref < cap
        assert np.array_equal(ac[0][below], cref[below]) and (ac[0][~below] >= cap).all(), (ac[0], cref)
        # the per-octave detection counts are the uncapped ones
        assert [int(c.get_counter_block(0)[32 + o]) for o in (1, 2, 3)] == [len(d) for d in case["dets"]]
        assert np.array_equal(a[0]["subsampling"], ref["subsampling"])
        compare_points(ref[:cap], a[0][:cap], "planted/capacity", record)
        # the same records, position by position (deterministic order = the supplied order)
        for f in ("xpos", "ypos", "sharpness", "orientation"):
            assert np.array_equal(a[0][f], ref[f]), f


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_per_octave_kernels_on_the_same_points(dctx, name):
    """orient_kernel / descr_kernel — the MISIFT_FUSED=0 path and the overflow re-run — octave by octave on the same
    planted points and the same levels."""
    from cudasift_amd import capi
    from oracle import pyoracle as orc
    case = pc.case(name)
    noct = case["geom"][2]
    for o in range(1, noct + 1):
        level, d = case["levels"][o - 1], case["dets"][o - 1]
        n = len(d)
        if n == 0:
            continue
        sub = float(2 ** (noct - o))
        pts = np.zeros(2 * n, capi.POINT_DTYPE)
        for j, f in enumerate(("xpos", "ypos", "scale", "sharpness", "edgeness")):
            pts[f][:n] = d[:, j]
        pts["subsampling"] = sub
        ref = pts.copy()
        end = orc.orientations(level, ref, 0, n, len(ref))
        orc.descriptors(level, ref, 0, end, sub)
        got, cnt = dctx.orient_and_describe(level, pts, 0, n, 1, subsampling=sub)
        assert int(cnt[2]) == n and int(cnt[3]) == end, (name, o, cnt[:4], end)
        compare_points(ref[:end], got[:end], "planted/per_octave/%s_o%d" % (name, o), record)


def test_argument_errors_enqueue_nothing(dctx):
    from cudasift_amd import capi
    L = capi.lib()
    case = pc.case("counts")
    w, h, noct = case["geom"]
    lv = [np.ascontiguousarray(a) for a in case["levels"]]
    ptrs = (C.c_void_p * noct)(*[a.ctypes.data for a in lv])
    holed = (C.c_void_p * noct)(lv[0].ctypes.data, None, lv[2].ctypes.data)
    counts = np.array([len(d) for d in case["dets"]], np.int32)
    negative = np.array([3, -1, 3], np.int32)
    flat = np.ascontiguousarray(np.concatenate(case["dets"]))
    n = np.full(1, -7, np.int32)
    cap = 512
    buf = capi.DevBuf(576 * cap)
    capi.check(L.misift_memset(dctx.h, buf.ptr, 0xA5, buf.nbytes), "misift_memset")
    dctx.sync()
    good = dict(ctx=dctx.h, nframes=1, w=w, h=h, noct=noct, up=0, levels=ptrs, dets=flat.ctypes.data, counts=counts.ctypes.data,
                pts=buf.ptr, cap=cap, n=n.ctypes.data)
    bad = [dict(ctx=None), dict(nframes=0), dict(nframes=-1), dict(w=0), dict(h=0), dict(w=16384), dict(noct=0), dict(noct=8),
           dict(w=3, h=3), dict(levels=None), dict(levels=holed), dict(dets=None), dict(counts=None),
           dict(counts=negative.ctypes.data), dict(pts=None), dict(cap=0), dict(n=None)]
    for change in bad:
        a = dict(good, **change)
        rc = L.misift_test_describe_detections(a["ctx"], a["nframes"], a["w"], a["h"], a["noct"], a["up"], a["levels"], a["dets"],
                                               a["counts"], a["pts"], a["cap"], a["n"])
        assert rc == -1, (change, rc)                          # MISIFT_EINVAL
        assert n[0] == -7, change
    dctx.sync()
    assert (dctx.download(buf, (buf.nbytes,), np.uint8) == 0xA5).all()
    # ... and the same arguments unchanged are a valid call
    a = good
    rc = L.misift_test_describe_detections(a["ctx"], a["nframes"], a["w"], a["h"], a["noct"], a["up"], a["levels"], a["dets"],
                                           a["counts"], a["pts"], a["cap"], a["n"])
    assert rc == 0 and n[0] == pc.expected(case, cap)[1]


def test_guard_bands_intact_after_the_module(dctx):
    """Last in the file: every context above checked its bands as it went; the module's own context is still alive."""
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
