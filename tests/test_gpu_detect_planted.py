"""The production detector — dog_scan_all_kernel and refine_all_kernel — on PLANTED pyramid levels
(Context.detect_levels / misift_test_detect_levels), against the oracle's answer to the same levels.

The cases and what each is aimed at: detect_cases.py; that they reach it: test_detect_cases_cpu.py.  Per frame and octave:
the candidate codes the scan wrote are the model's set (the necessary in-row test on the oracle's planes), the staged
detections are the oracle's (paired exactly by util.associate, five fields within RTOL, the rule of test_gpu_parity.py's
_cmp_detections) and the counters say so.  Bit equality of the five fields is measured and recorded, not asserted.
Every case runs as one scan launch and as split-tail mode's two.  The module's context is guarded."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
from batch_util import guarded_context
from conftest import record
from util import RTOL, associate

pytestmark = pytest.mark.gpu
CNT_CAND, CNT_CANDOVF, CNT_PTOVF, CNT_DET = 20, 28, 29, 32
FIELDS = ("xpos", "ypos", "scale", "sharpness", "edgeness")
RUNS = dict(dc.all_runs())
LATTICES = ("lattice_r1", "lattice_r5", "lattice_q1", "lattice_q5")


@pytest.fixture(scope="module")
def dctx():
    """One guarded context for the whole module, so every call also follows calls of other shapes and batch sizes."""
    with guarded_context(1) as c:
        c.set_knob("small_frames", dc.SMALL_FRAMES)
        c.set_options(fused=1)
        yield c


def run(c, case, two):
    return c.detect_levels(case["frames"], case["thresh"], case["lowest_scale"], case["max_pts"], two_ranges=two)


def records(d, sub):
    """[n, 5] floats as SiftPoint records (what associate and the oracle speak)."""
    from cudasift_amd import capi
    r = np.zeros(len(d), capi.POINT_DTYPE)
    for j, f in enumerate(FIELDS):
        r[f] = d[:, j]
    r["subsampling"] = sub
    return r


def cmp_detections(ref, got, name):
    """_cmp_detections of test_gpu_parity.py; also returns the largest absolute difference per field over the pairs."""
    A, B = ref.copy(), got.copy()
    A["orientation"] = 0
    B["orientation"] = 0
    ia, ib, oa, ob = associate(A, B)
    st = {"n_oracle": len(A), "n_hip": len(B), "paired": len(ia), "paired_exact": associate.last_exact,
          "only_oracle": len(oa), "only_hip": len(ob)}
    diff = {}
    for f in FIELDS:
        x, y = A[f][ia].astype(np.float64), B[f][ib].astype(np.float64)
        st[f + "_relerr"] = float((np.abs(x - y) / np.maximum(np.abs(x), 1.0)).max()) if len(ia) else 0.0
        diff[f] = float(np.abs(x - y).max()) if len(ia) else 0.0
        st[f + "_bits_differ"] = int((A[f][ia].view(np.uint32) != B[f][ib].view(np.uint32)).sum()) if len(ia) else 0
    assert len(A) == len(B) and not oa and not ob, (name, st)
    assert st["paired_exact"] == len(A), (name, st)
    for f in FIELDS:
        assert st[f + "_relerr"] <= RTOL, (name, st)
    return st, diff


def check(name, case, out, two):
    """One call against the model and the oracle: candidate sets, counters, detections."""
    exp = dc.expected(name)
    w, h, noct = case["geom"]
    tag = "detect_planted/%s/%s" % (name, "two_ranges" if two else "one_range")
    worst = {f: 0.0 for f in FIELDS}
    bits = {f: 0 for f in FIELDS}
    total = 0
    for f, row in enumerate(exp):
        cnt = out["counters"][f]
        ovf = 0
        for k, e in enumerate(row):
            o = k + 1
            where = (name, two, f, o)
            cap = int(out["cand_caps"][k])
            ncand = int(cnt[CNT_CAND + o])
            assert ncand == len(e["codes"]), (where, ncand, len(e["codes"]))
            assert int(out["cand_counts"][f, k]) == min(ncand, cap), where
            got = np.sort(out["cand"][f, k, :min(ncand, cap)])
            if ncand <= cap:
                if not np.array_equal(got, e["codes"]):
                    extra, missing = np.setdiff1d(got, e["codes"]), np.setdiff1d(e["codes"], got)
                    raise AssertionError((where, "only on device", [tuple(int(v[0]) for v in dc.decode([c])) for c in extra[:8]],
                                          "only in model", [tuple(int(v[0]) for v in dc.decode([c])) for c in missing[:8]]))
            else:                                          # a full list holds `cap` different codes of the model's
                assert len(np.unique(got)) == cap and np.isin(got, e["codes"]).all(), where
                ovf += ncand - cap
            if not case["detections"]:
                continue
            assert int(cnt[CNT_DET + o]) == e["n"], (where, int(cnt[CNT_DET + o]), e["n"])
            assert int(out["det_counts"][f, k]) == e["n"], where
            sub = float(2 ** (noct - o))
            st, diff = cmp_detections(e["pts"], records(out["dets"][f, k, :e["n"]], sub), where)
            total += e["n"]
            for fld in FIELDS:
                worst[fld] = max(worst[fld], diff[fld])
                bits[fld] += st[fld + "_bits_differ"]
        assert int(cnt[CNT_CANDOVF]) == ovf, (name, two, f, int(cnt[CNT_CANDOVF]), ovf)
        assert int(cnt[CNT_PTOVF]) == 0 or not case["detections"], (name, two, f)
    record(tag, detections=total, seg_rows=out["seg_rows"], **{"maxabs_" + k: v for k, v in worst.items()}, **{"bits_differ_" + k: v for k, v in bits.items()})
    return out


def seam_check(name, case, out):
    """From the segment length the scan used on THIS machine: per level that has a seam, detections on either side of one."""
    w, h, noct = case["geom"]
    exp = dc.expected(name)
    for k, (lw, lh) in enumerate(dc.level_sizes(w, h, noct)):
        seg = int(out["seg_rows"][k])
        assert seg >= 1 and int(out["nstrips"][k]) == (lw + dc.STRIP - 1) // dc.STRIP, (name, k, seg)
        seams = [r for r in range(seg, lh, seg) if 2 <= r - 1 and r <= lh - 3]
        if not seams:
            continue
        for f in range(len(case["frames"])):
            if len(case["frames"]) > 1 and f == 1:
                continue
            ys = set(np.rint(out["dets"][f, k, :exp[f][k]["n"], 1]).astype(int))
            assert any(r - 1 in ys and r in ys for r in seams), (name, f, k, seg)
            if k == noct - 1:
                xs = set(np.rint(out["dets"][f, k, :exp[f][k]["n"], 0]).astype(int))
                assert {dc.STRIP - 1, dc.STRIP, 2 * dc.STRIP - 1, 2 * dc.STRIP} <= xs, (name, f)


@pytest.mark.parametrize("two", [False, True], ids=["one_range", "two_ranges"])
@pytest.mark.parametrize("name", list(RUNS))
def test_planted_levels(dctx, name, two):
    case = RUNS[name]
    out = check(name, case, run(dctx, case, two), two)
    if name in LATTICES:
        seam_check(name, case, out)
    if name == "overflow":
        assert int(out["counters"][0][CNT_CANDOVF]) > 0
        assert int(out["counters"][0][CNT_CAND + 3]) > int(out["cand_caps"][2])


def test_segment_rule_differs_across_small_frames(dctx):
    """A frame and small_frames + 1 frames of one geometry cut the finest level differently: both rules ran above."""
    a = run(dctx, RUNS["lattice_r1"], False)
    b = run(dctx, RUNS["lattice_r5"], False)
    assert a["seg_rows"][-1] != b["seg_rows"][-1] or a["seg_rows"][-2] != b["seg_rows"][-2], (a["seg_rows"], b["seg_rows"])
    assert (b["seg_rows"] % 9 == 0).all() and (b["seg_rows"] >= 18).all()          # a batch: whole turns of the row ring


def test_scale_up_doubles_the_scale_floor(dctx):
    """An up-sampled call doubles lowest_scale: half the floor with scale_up is the floor itself, at the ulp on either side."""
    for name in ("floor_eq", "floor_above"):
        case = RUNS[name]
        out = dctx.detect_levels(case["frames"], case["thresh"], case["lowest_scale"] / 2, case["max_pts"], scale_up=True)
        exp = dc.expected(name)[0]
        assert [int(v) for v in out["det_counts"][0]] == [e["n"] for e in exp], name
        for k, e in enumerate(exp):
            cmp_detections(e["pts"], records(out["dets"][0, k, :e["n"]], float(2 ** (case["geom"][2] - k - 1))), (name, "scale_up", k))


def test_repeats_with_another_shape_in_between(dctx):
    def sets(out, case):
        s = []
        for f in range(len(case["frames"])):
            for k in range(case["geom"][2]):
                s.append(np.sort(out["cand"][f, k, :out["cand_counts"][f, k]]).tobytes())
                d = out["dets"][f, k, :out["det_counts"][f, k]]
                s.append(d[np.lexsort(d.T[::-1])].tobytes())
        return s
    for name, other in (("lattice_r5", "tiny4"), ("subpixel", "lattice_q1"), ("queue", "ties")):
        case = RUNS[name]
        first = sets(run(dctx, case, False), case)
        run(dctx, RUNS[other], True)
        assert sets(run(dctx, case, False), case) == first, name
        assert sets(run(dctx, case, True), case) == first, name


@pytest.mark.parametrize("name", [n for n in RUNS if RUNS[n]["detections"]])
def test_per_level_kernels_on_the_same_levels(dctx, name):
    """dog_scan_kernel + refine_kernel<true> (Context.dog_findpoints) and detect_kernel + refine_kernel<false> on the
    oracle's planes (Context.findpoints) — the dense kernels production falls back to — level by level."""
    case = RUNS[name]
    w, h, noct = case["geom"]
    exp = dc.expected(name)
    for f, frame in enumerate(case["frames"]):
        for k, level in enumerate(frame):
            o, e = k + 1, exp[f][k]
            if min(level.shape) < 16:                          # the two stage entries take levels from 16 x 16 on
                assert name == "tiny4" and k == 0
                continue
            sub = float(2 ** (noct - o))
            floor = float(np.float32(case["lowest_scale"]) / np.float32(sub))
            got, n = dctx.dog_findpoints(level, noct, o, case["thresh"], sub, floor, max_pts=case["max_pts"])
            cmp_detections(e["pts"], got[:n], (name, "dog_findpoints", f, o))
            got, n = dctx.findpoints(dc.planes_of(level, noct, o), case["thresh"], sub, floor, max_pts=case["max_pts"], octave=o)
            cmp_detections(e["pts"], got[:n], (name, "findpoints", f, o))


def test_argument_errors_enqueue_nothing(dctx):
    from cudasift_amd import capi
    L = capi.lib()
    case = RUNS["lattice_r1"]
    w, h, noct = case["geom"]
    lv = [np.ascontiguousarray(a) for a in case["frames"][0]]
    ptrs = (C.c_void_p * noct)(*[a.ctypes.data for a in lv])
    holed = (C.c_void_p * noct)(lv[0].ctypes.data, None, lv[2].ctypes.data)
    cap, slots = 1024, dc.cand_cap(w, h)
    bufs = dict(cand=np.full((noct, slots), 0xA5A5A5A5, np.uint32), ccnt=np.full(noct, -7, np.int32),
                dets=np.full((noct, cap, 5), -7.0, np.float32), dcnt=np.full(noct, -7, np.int32),
                cnt=np.full(64, 0xA5A5A5A5, np.uint32), geom=np.full(2 * noct, -7, np.int32))
    before = {k: v.copy() for k, v in bufs.items()}
    dctx.sync()
    block = dctx.get_counter_block(0).copy()
    good = dict(ctx=dctx.h, nframes=1, w=w, h=h, noct=noct, thresh=2.0, floor=0.0, up=0, levels=ptrs, cap=cap, two=0,
                cand=bufs["cand"].ctypes.data, slots=slots, ccnt=bufs["ccnt"].ctypes.data, dets=bufs["dets"].ctypes.data,
                dcnt=bufs["dcnt"].ctypes.data, cnt=bufs["cnt"].ctypes.data, geom=bufs["geom"].ctypes.data)

    def call(a):
        return L.misift_test_detect_levels(a["ctx"], a["nframes"], a["w"], a["h"], a["noct"], a["thresh"], a["floor"], a["up"],
                                           a["levels"], a["cap"], a["two"], a["cand"], a["slots"], a["ccnt"], a["dets"], a["dcnt"],
                                           a["cnt"], a["geom"])
    bad = [dict(ctx=None), dict(nframes=0), dict(nframes=-1), dict(w=0), dict(h=0), dict(w=16384), dict(noct=0), dict(noct=8),
           dict(w=3, h=3), dict(w=15, noct=1), dict(w=63, h=65, noct=4), dict(w=67, h=63, noct=4),      # tiny calls
           dict(levels=None), dict(levels=holed), dict(cap=0), dict(two=2), dict(two=-1), dict(two=1, noct=2),
           dict(cand=None), dict(slots=slots - 1), dict(slots=0), dict(ccnt=None), dict(dets=None), dict(dcnt=None),
           dict(cnt=None), dict(geom=None)]
    for change in bad:
        rc = call(dict(good, **change))
        assert rc == -1, (change, rc)                          # MISIFT_EINVAL
        for k, v in bufs.items():
            assert np.array_equal(v, before[k]), (change, k)
    dctx.sync()
    assert np.array_equal(dctx.get_counter_block(0), block)    # not even the counter blocks were cleared
    # ... and the same arguments unchanged are a valid call
    assert call(good) == 0
    e = dc.expected("lattice_r1")[0]
    assert [int(v) for v in bufs["dcnt"]] == [min(r["n"], cap) for r in e]
    assert [int(v) for v in bufs["ccnt"]] == [len(r["codes"]) for r in e]


def test_guard_bands_intact_after_the_module(dctx):
    """Last in the file: the module's context is still alive, with every buffer the calls above used."""
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
