"""misift_refine_cameras_batch on the device: every linked camera refined against the triangulated track points.

Every comparison is byte equality with refine_cases.expected_refine (pinned in test_refine_cpu.py to the library's host
hook and to float64, where the premises of the cases are asserted too): d_cam_out, d_cam_obs, d_cam_rms, d_cam_steps,
d_cam_status and d_summary, and every byte of the offsets, the observations, the export summary, the points, their
status, the cameras and d_cam_pair, which the call must not write.  The scenes are planted directly; no images are
needed.  The outputs have exactly the stated capacity and are poisoned first; all allocations of the module are guarded.
The shapes are the ones at which the kernel can go wrong: no slot, one, either side of one row of the 256 lane slots and
the wrap, T and O from the device below, beyond and under their capacities, 1, 2, 3, 64 and 65 images, images around
min_obs and with no observation, all members of an image in one lane slot."""
import numpy as np
import pytest

import posegraph_cases as G
import pose_cases as PC
import refine_cases as RC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
INPUTS = (("track_offsets", np.int32), ("obs", TC.OBS_DTYPE), ("export_summary", np.int32), ("points", f32),
          ("point_status", np.int32), ("cam", f32), ("cam_pair", np.int32))
INTS = ("cam_obs", "cam_steps", "cam_status", "summary")


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _sizes(case):
    n = case["nimages"]
    return dict(cam_out=12 * n, cam_obs=n, cam_rms=2 * n, cam_steps=n, cam_status=n, summary=8)


def _inputs(case):
    """The inputs at exactly the sizes the call states."""
    mt, mo = case["max_tracks"], case["max_obs"]
    ins = dict(track_offsets=np.ascontiguousarray(case["track_offsets"][:mt + 1], np.int32),
               obs=np.ascontiguousarray(case["obs"][:mo]), export_summary=np.ascontiguousarray(case["export_summary"]),
               points=np.ascontiguousarray(case["points"], f32).reshape(-1, 4),
               point_status=np.ascontiguousarray(case["point_status"], np.int32),
               cam=np.ascontiguousarray(case["cam"], f32), cam_pair=np.ascontiguousarray(case["cam_pair"], np.int32))
    assert len(ins["track_offsets"]) == mt + 1 and len(ins["obs"]) == mo and len(ins["cam"]) == case["nimages"]
    assert len(ins["points"]) == mt == len(ins["point_status"])
    return ins


def _refine(ctx, case, in_place=False):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays.  The inputs must come back
    as they went in (but for d_cam when it is d_cam_out)."""
    ins = _inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in _sizes(case).items()}
    if in_place:
        outs["cam_out"] = dev["cam"]
    ctx.refine_cameras_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                             dev["points"], dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"],
                             case["intrinsics"], hold=case["hold"], min_obs=case["min_obs"], num_loops=case["num_loops"],
                             max_error=case["max_error"], orthonormalise=case["orthonormalise"], **outs)
    ctx.sync()
    for k, dt in INPUTS:
        if not (in_place and k == "cam"):
            assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (n,), np.uint32) for k, n in _sizes(case).items()}


def _compare(got, case, what):
    e = RC.expected_refine(case)
    for k in RC.OUTPUTS:
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in INTS else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))
    return e


def _status(e):
    return e["cam_status"].view(np.int32).tolist()


@pytest.mark.parametrize("O", [0, 1, 255, 256, 257, 513])
def test_every_slot_count(g, O):
    """O slots in all: an empty lane slot, exactly one row of lane slots, one more, and the wrap into a third row."""
    case = RC.spread_case(O)
    assert RC.counts(case)[1] == O and case["max_obs"] == max(O, 1)
    e = _compare(_refine(g, case), case, "O = %d" % O)
    assert (e["summary"].view(np.int32)[1] > 0) == (O >= 255)


@pytest.mark.parametrize("T,O", [(63, 513), (171, 200), (300, 10 ** 9), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 513), (171, -5),
                                 (171, 256), (-2 ** 31, -2 ** 31)])
def test_counts_from_the_device(g, T, O):
    """T and O below their capacities cut the tracks and the slots; beyond them they are clamped; below 0 they are 0.  A
    track that ends beyond O is not valid."""
    base = RC.spread_case(513)
    assert (base["max_tracks"], base["max_obs"]) == (171, 513)
    case = RC.with_counts(base, T, O)
    e = _compare(_refine(g, case), case, "T = %d, O = %d" % (T, O))
    assert e["summary"].view(np.int32)[0] == min(max(T, 0), 171)


@pytest.mark.parametrize("nimages", [1, 2, 3, 64, 65])
def test_every_image_count(g, nimages):
    case = RC.scene(RC.runs(8 * nimages, nimages, 66), nimages, 66, orthonormalise=1)["case"]
    e = _compare(_refine(g, case), case, "%d images" % nimages)
    s = e["summary"].view(np.int32)
    assert s[5] == 1 and s[1] + s[3] == nimages - 1 and (nimages < 3 or s[1] >= nimages // 2)


def test_images_around_min_obs_and_one_with_no_observation(g):
    case = RC.member_counts_case()
    e = _compare(_refine(g, case), case, "around min_obs")
    assert e["cam_obs"].view(np.int32).tolist() == [0, 5, 6, 7, 0, 40]
    assert _status(e) == [RC.HELD, RC.FEW_OBS, RC.OK, RC.OK, RC.FEW_OBS, RC.OK]


def test_all_members_of_an_image_in_one_lane_slot(g):
    case = RC.one_lane_case()
    key, _ = RC.candidate_keys(case)
    assert (np.nonzero(key == 1)[0] % 256 == 5).all() and (key == 1).sum() == 8
    e = _compare(_refine(g, case), case, "one lane slot")
    assert _status(e) == [RC.HELD, RC.OK, RC.OK, RC.OK] and e["cam_steps"].view(np.int32)[1] > 0


@pytest.mark.parametrize("max_error,num_loops,orth", [(RC.INF, 0, 0), (RC.INF, 1, 1), (8.0, 5, 0), (RC.INF, 5, 1),
                                                      (8.0, 0, 1)])
def test_gate_loops_and_orthonormalise(g, max_error, num_loops, orth):
    """The spread scene and the hostile one (the root, a held and an unset image, a NaN and an inf in a camera, points of
    status 1 to 4 and non-finite ones, frames outside the images, non-finite positions, points behind a camera) under
    every setting; two runs give the same bytes."""
    for name, base in (("spread", RC.spread_case(513)), ("hostile", RC.hostile_case())):
        case = RC.variant(base, max_error=max_error, num_loops=num_loops, orthonormalise=orth)
        got = _refine(g, case)
        e = _compare(got, case, name)
        s = e["summary"].view(np.int32)
        assert (s[6] > 0) == (num_loops > 0) and s[1] > 0
        if num_loops == 0 and orth == 0:
            assert got["cam_out"].tobytes() == np.ascontiguousarray(case["cam"], f32).tobytes()
        if name == "hostile":
            assert s[5] == 2 and s[7] == 3
            again = _refine(g, case)
            for k in RC.OUTPUTS:
                assert got[k].tobytes() == again[k].tobytes(), k


def test_a_rejected_step_and_a_member_behind_a_trial_camera(g):
    case = RC.rejected_step_case()
    e = _compare(_refine(g, case), case, "rejected step")
    assert e["images"][1]["trace"] == ["kept", "worse"]
    case = RC.behind_trial_case()
    e = _compare(_refine(g, case), case, "behind a trial camera")
    assert e["images"][1]["trace"] == ["behind"] and _status(e)[1] == RC.OK


def test_bad_offsets(g):
    """Offsets that are negative, decrease, overlap or pass O address nothing; the largest valid track owns a slot."""
    case = RC.bad_offsets_case()
    _compare(_refine(g, case), case, "bad offsets")


def test_in_place(g):
    for case in (RC.variant(RC.spread_case(513), orthonormalise=1), RC.hostile_case()):
        got = _refine(g, case, in_place=True)
        _compare(got, case, "d_cam_out == d_cam")


def test_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = RC.spread_case(257)
    ins = _inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in _sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n = case["nimages"]
    hold = np.array([1, 2], np.int32)
    good = dict(ctx=g.h, max_tracks=case["max_tracks"], max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, points=dev["points"].ptr,
                point_status=dev["point_status"].ptr, nimages=n, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr,
                intrinsics=K.ctypes.data, nhold=0, hold=None, min_obs=6, num_loops=5, max_error=np.inf, orthonormalise=0,
                **{k: outs[k].ptr for k in RC.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_refine_cameras_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-7), dict(nimages=0),
           dict(nimages=-1), dict(min_obs=2), dict(min_obs=0), dict(min_obs=-3), dict(num_loops=-1),
           dict(max_error=np.nan), dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=-np.inf),
           dict(orthonormalise=2), dict(orthonormalise=-1), dict(nhold=-1), dict(nhold=2, hold=None),
           dict(obs=dev["obs"].ptr + 4), dict(obs=dev["obs"].ptr + 8),
           dict(cam_out=dev["cam"].ptr + 4), dict(cam_out=dev["cam"].ptr + 48 * n - 4), dict(cam_out=dev["cam"].ptr - 4)]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "points", "point_status", "cam", "cam_pair",
                                "intrinsics") + RC.OUTPUTS]
    lists = []                                                   # kept alive until the calls are made
    for h in ([-1, 1], [1, n], [2 ** 31 - 1, 0]):
        lists.append(np.array(h, np.int32))
        bad.append(dict(nhold=2, hold=lists[-1].ctypes.data))
    for at in (0, 1, 4 * n - 4, 4 * n - 3):
        for v in (0.0, -1500.0, np.nan, np.inf, -np.inf):        # fx, fy of the first and the last image
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for at in (2, 3, 4 * n - 1):
        for v in (np.nan, np.inf, -np.inf):                      # cx, cy
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in _sizes(case).items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, dt in INPUTS:
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # the same arguments, unbroken; then with a hold list
    assert call() == MISIFT_OK
    g.sync()
    _compare({k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}, case, "unbroken")
    assert call(nhold=2, hold=hold.ctypes.data) == MISIFT_OK
    g.sync()
    e = _compare({k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()},
                 RC.variant(case, hold=(1, 2)), "held")
    assert _status(e)[:3] == [RC.HELD] * 3


def test_export_triangulate_refine_triangulate(g):
    """The chain on the 8-camera scene of posegraph_cases, nothing read in between: the cameras of find -> improve ->
    recover_pose -> link_poses, the observation lists of link_tracks -> export_tracks, then triangulate -> refine ->
    triangulate.  Both calls are byte-equal to their restatements fed the device's own buffers."""
    from cudasift_amd import capi
    sc = G.planted_scene()
    pc, S = sc["case"], sc["S"]
    n, npairs, nimg = S["n"], len(sc["pairs"]), pc["nimages"]
    sel = list(range(npairs))
    d, dc = g.upload(np.concatenate(sc["raw"])), g.upload(np.full(npairs, n, np.int32))
    dfit, dpose, dfront, dxyz = (_poisoned(g, k) for k in (npairs, 12 * npairs, npairs, 4 * n * npairs))
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=S["thresh"])
    dF, _ = g.find_fundamental_batch(sel, sc["seeds"], d, npairs, dc, None, n, max_pts=n, num_loops=S["find_loops"],
                                     **gates)
    g.improve_fundamental_batch(sel, d, npairs, dc, dF, None, n, num_fit=dfit, num_loops=S["improve_loops"], **gates)
    g.recover_pose_batch(sel, np.tile(sc["K8"], (npairs, 1)), d, npairs, dc, dF, None, n, pose=dpose, num_front=dfront,
                         xyz=dxyz, **gates)
    _, _, _, dcam, dcam_pair, _ = g.link_poses_batch(pc["pairs"], nimg, d, dc, n, dpose, dfront, dxyz, pc["links"],
                                                     pc["seed_pair"], pc["root_image"], pc["walk"],
                                                     min_common=pc["min_common"], min_score=GATES[0],
                                                     max_ambiguity=GATES[1], max_error=pc["max_error"])
    recs = np.zeros(nimg * n, capi.POINT_DTYPE)
    for i in range(nimg - 1):
        assert tuple(sc["pairs"][i]) == (i, i + 1)
        recs[i * n:(i + 1) * n] = sc["raw"][i]
    last = sc["raw"][nimg - 2]
    for k, mk in (("xpos", "match_xpos"), ("ypos", "match_ypos")):
        recs[k][(nimg - 1) * n + last["match"]] = last[mk]
    total = nimg * n
    d_recs, d_cnt = g.upload(recs), g.upload(np.full(nimg, n, np.int32))
    lab = g.link_tracks_batch(pc["pairs"], d, dc, n, nimg, d_cnt, None, n, max_records=total, min_score=GATES[0],
                              max_ambiguity=GATES[1], max_error=pc["max_error"])
    mt, mo = total // 3 + 1, total
    doff, _, dobs, _, dsum = g.export_tracks_batch(d_recs, nimg, d_cnt, None, n, max_records=total, track=lab[0],
                                                   track_len=lab[1], track_frames=lab[2], min_len=3, consistent_only=1,
                                                   max_tracks=mt, max_obs=mo, record_obs=None)
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    seed = pc["pairs"][pc["seed_pair"]]
    hold = [i for i in seed if i != pc["root_image"]]
    tri1 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    outs = {k: _poisoned(g, m) for k, m in _sizes(dict(nimages=nimg)).items()}
    g.refine_cameras_batch(mt, mo, doff, dobs, dsum, tri1[0], tri1[2], nimg, dcam, dcam_pair, K, hold=hold, min_obs=6,
                           num_loops=5, max_error=RC.INF, orthonormalise=1, **outs)
    tri2 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, outs["cam_out"], dcam_pair, K, min_views=2,
                                      num_loops=5)
    g.sync()
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=g.download(doff, (mt + 1,), np.int32),
                obs=g.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, cam_pair=g.download(dcam_pair, (nimg,), np.int32), intrinsics=K)
    T = int(base["export_summary"][2])

    def tri_outputs(t):
        return dict(points=g.download(t[0], (4 * mt,), np.uint32), point_views=g.download(t[1], (mt,), np.uint32),
                    point_status=g.download(t[2], (mt,), np.uint32), obs_error=g.download(t[3], (mo,), np.uint32),
                    summary=g.download(t[4], (8,), np.uint32))

    def pooled(t):
        p, st = t["points"].view(f32).reshape(-1, 4)[:T], t["point_status"].view(np.int32)[:T]
        v = t["point_views"].view(np.int32)[:T][st == 0]
        return float(np.sqrt((p[st == 0, 3].astype(np.float64) ** 2 * v).sum() / v.sum()))

    got1, got2 = tri_outputs(tri1), tri_outputs(tri2)
    cam1 = g.download(dcam, (nimg, 12), f32)
    case = dict(base, cam=cam1, points=got1["points"].view(f32).reshape(-1, 4),
                point_status=got1["point_status"].view(np.int32), hold=tuple(hold), min_obs=6, num_loops=5,
                max_error=RC.INF, orthonormalise=1)
    e = _compare({k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}, case, "chain, refine")
    for got, cam in ((got1, cam1), (got2, e["cam_out"].view(f32).reshape(-1, 12))):
        tc = dict(base, cam=cam, min_views=2, num_loops=5, memo={})
        with np.errstate(all="ignore"):
            x = TC.expected_triangulate(tc)
        for k in ("points", "point_views", "point_status", "obs_error", "summary"):
            written = x[k] != POISON_WORD                        # what the call leaves alone was zeroed here, not poisoned
            assert (got[k][written] == x[k][written]).all(), k
    s = e["summary"].view(np.int32)
    rms = e["cam_rms"].view(f32).reshape(-1, 2)
    print("chain: T %d summary %s rms before %s after %s; pooled %.4g -> %.4g px" % (
        T, s.tolist(), rms[:, 0], rms[:, 1], pooled(got1), pooled(got2)))
    assert s[0] == T >= 100 and s[5] == 2 and s[1] == nimg - 2 and s[7] == 0


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
