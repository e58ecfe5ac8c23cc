"""misift_resect_cameras_batch on the device: the camera of each selected image by batch RANSAC over six-point solves.

Every comparison is byte equality with resect_cases.expected_resect (pinned in test_resect_cpu.py to the library's host
hooks and to float64, where the premises of the cases are asserted too): d_res_cam, d_res_cand, d_res_inliers,
d_res_status and d_summary, d_cam and d_cam_pair as the call leaves them, and every byte of the offsets, the
observations, the export summary, the points and their status, which the call must not write.  The scenes are planted
directly; no images are needed.  The outputs have exactly the stated size and are poisoned first; all allocations of the
module are guarded.  The shapes are the ones at which the kernels can go wrong: candidates either side of six and of one
and two count chunks, max_cand off the multiple of 16 and one below n, hypotheses either side of a block, T and O from
the device below, beyond and under their capacities, hostile offsets, frames, points and observations."""
import numpy as np
import pytest

import posegraph_cases as G
import pose_cases as PC
import refine_cases as RC
import resect_cases as C
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
INPUTS = (("track_offsets", np.int32), ("obs", TC.OBS_DTYPE), ("export_summary", np.int32), ("points", f32),
          ("point_status", np.int32))
INTS = ("res_cand", "res_inliers", "res_status", "summary")


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _sizes(case):
    n = len(case["images"])
    return dict(res_cam=12 * n, res_cand=n, res_inliers=n, res_status=n, summary=8)


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


def _call(ctx, case, dev, outs):
    ctx.resect_cameras_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                             dev["points"], dev["point_status"], case["nimages"], case["intrinsics"], case["images"],
                             case["seeds"], case["max_cand"], num_loops=case["num_loops"], thresh=case["thresh"],
                             min_inliers=case["min_inliers"], only_unset=case["only_unset"], install=case["install"],
                             cam=dev["cam"], cam_pair=dev["cam_pair"], **outs)


def _resect(ctx, case):
    """The call on poisoned outputs of exactly the stated sizes; returns them, d_cam and d_cam_pair as uint32 arrays.  The
    other inputs must come back as they went in, and what lies behind an output of no entry must stay poisoned."""
    ins = _inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in _sizes(case).items()}
    _call(ctx, case, dev, outs)
    ctx.sync()
    for k, dt in INPUTS:
        assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    got = {k: ctx.download(outs[k], (n,), np.uint32) if n else np.zeros(0, np.uint32)
           for k, n in _sizes(case).items()}
    for k, n in _sizes(case).items():
        if n == 0:
            assert ctx.download(outs[k], (1,), np.uint32)[0] == POISON_WORD, k
    got["cam"] = ctx.download(dev["cam"], (12 * case["nimages"],), np.uint32)
    got["cam_pair"] = ctx.download(dev["cam_pair"], (case["nimages"],), np.uint32)
    return got


def _compare(got, case, what):
    e = C.expected_resect(case)
    for k in C.OUTPUTS + ("cam", "cam_pair"):
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in INTS + ("cam_pair",) else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))
    return e


@pytest.mark.parametrize("name", C.GPU_CASES)
def test_case(g, name):
    """Every case of resect_cases.gpu_cases (what each is built to hit is asserted in test_resect_cpu.py)."""
    case = C.gpu_cases()[name]
    e = _compare(_resect(g, case), case, name)
    print(name, "status", [x["status"] for x in e["entries"]], "candidates", [x["cand"] for x in e["entries"]],
          "inliers", [x["inliers"] for x in e["entries"]])


def test_temp_left_dirty_and_two_runs(g):
    """Behind a call of another kind that leaves the temp memory dirty (refine: owners and keys of another scene), and
    again behind a resection with other strides: the same bytes."""
    other = RC.spread_case(513)
    ins = {k: g.upload(np.ascontiguousarray(v)) for k, v in (("o", other["track_offsets"]), ("b", other["obs"]),
                                                             ("s", other["export_summary"]), ("p", other["points"]),
                                                             ("t", other["point_status"]), ("c", other["cam"]),
                                                             ("q", other["cam_pair"]))}
    g.refine_cameras_batch(other["max_tracks"], other["max_obs"], ins["o"], ins["b"], ins["s"], ins["p"], ins["t"],
                           other["nimages"], ins["c"], ins["q"], other["intrinsics"])
    cases = C.gpu_cases()
    first = _resect(g, cases["hostile"])
    _compare(first, cases["hostile"], "behind refine")
    _compare(_resect(g, cases["candidates 513 1025"]), cases["candidates 513 1025"], "other strides")
    again = _resect(g, cases["hostile"])
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k


def test_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = C.gpu_cases()["only_unset, install 1"]
    ins = _inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in _sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n = case["nimages"]
    images, seeds = np.ascontiguousarray(case["images"], np.int32), np.ascontiguousarray(case["seeds"], np.uint32)
    good = dict(ctx=g.h, max_tracks=case["max_tracks"], max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, points=dev["points"].ptr,
                point_status=dev["point_status"].ptr, nimages=n, intrinsics=K.ctypes.data, nsel=len(images),
                images=images.ctypes.data, seeds=seeds.ctypes.data, max_cand=case["max_cand"],
                num_loops=case["num_loops"], thresh=case["thresh"], min_inliers=case["min_inliers"], only_unset=1,
                install=1, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr, **{k: outs[k].ptr for k in C.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_resect_cameras_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-7), dict(nimages=0),
           dict(nimages=-1), dict(nsel=-1), dict(images=None), dict(seeds=None), dict(max_cand=5), dict(max_cand=0),
           dict(max_cand=-1), dict(num_loops=0), dict(num_loops=-1), dict(thresh=np.nan), dict(thresh=0.0),
           dict(thresh=-1.0), dict(thresh=-np.inf), dict(min_inliers=5), dict(min_inliers=0), dict(min_inliers=-6),
           dict(only_unset=2), dict(only_unset=-1), dict(install=2), dict(install=-1),
           dict(obs=dev["obs"].ptr + 4), dict(obs=dev["obs"].ptr + 8),
           dict(cam=None), dict(cam_pair=None), dict(cam_pair=None, install=0), dict(cam_pair=None, only_unset=0),
           # one launch holds 2^31 - 1 workgroups: 3 entries x 2^25 hypothesis blocks x 24 chunks do not fit
           dict(nsel=3, num_loops=2 ** 31 - 16, max_cand=12000, max_obs=12000), dict(num_loops=2 ** 31 - 15),
           dict(num_loops=2 ** 31 - 1)]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "points", "point_status", "intrinsics") +
            C.OUTPUTS]
    lists = []                                                   # kept alive until the calls are made
    for h in ([-1, 1, 2, 3], [1, n, 0, 2], [2 ** 31 - 1, 0, 1, 2], [0, 1, 2, 0], [3, 3, 1, 2]):
        lists.append(np.array(h, np.int32))
        bad.append(dict(images=lists[-1].ctypes.data))
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
    for k, dt in INPUTS + (("cam", f32), ("cam_pair", np.int32)):
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # without only_unset and install the cameras are not looked at: NULL is fine; then the same arguments, unbroken
    assert call(cam=None, cam_pair=None, only_unset=0, install=0) == MISIFT_OK
    assert call(nsel=0, images=None, seeds=None) == MISIFT_OK
    assert call() == MISIFT_OK
    g.sync()
    got = {k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}
    got["cam"] = g.download(dev["cam"], (12 * n,), np.uint32)
    got["cam_pair"] = g.download(dev["cam_pair"], (n,), np.uint32)
    _compare(got, case, "unbroken")


def test_export_triangulate_resect_triangulate_refine(g):
    """The chain on the 8-camera scene of posegraph_cases with pair (4, 5) made unusable (no record in front), so that
    link_poses leaves images 5, 6 and 7 without a camera: export -> triangulate -> resect(only_unset, install) ->
    triangulate -> refine, nothing read in between.  After the resection those images have d_cam_pair == -3, the second
    triangulation uses their views, refine gives them status 0 where it gave 4 before, and every stage is byte-equal to
    its restatement fed the device's own buffers."""
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
    g.sync()
    front = g.download(dfront, (npairs,), np.int32)
    assert tuple(sc["pairs"][4]) == (4, 5) and front[4] > 0
    front[4] = 0                                                 # the unusable pair
    dfront = g.upload(front)
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
    hold = [i for i in pc["pairs"][pc["seed_pair"]] if i != pc["root_image"]]
    images, seeds = np.arange(nimg, dtype=np.int32)[::-1].copy(), np.arange(nimg, dtype=np.uint32) + 500
    rargs = dict(max_cand=n, num_loops=256, thresh=4.0, min_inliers=12, only_unset=1, install=1)
    tri1 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    ref1 = g.refine_cameras_batch(mt, mo, doff, dobs, dsum, tri1[0], tri1[2], nimg, dcam, dcam_pair, K, hold=hold,
                                  min_obs=6, num_loops=5, max_error=4.0, orthonormalise=1)
    g.sync()
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=g.download(doff, (mt + 1,), np.int32),
                obs=g.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, intrinsics=K)
    cam_linked, pair_linked = g.download(dcam, (nimg, 12), f32), g.download(dcam_pair, (nimg,), np.int32)
    status1 = g.download(ref1[4], (nimg,), np.int32)
    outs = {k: _poisoned(g, m) for k, m in _sizes(dict(images=images)).items()}
    g.resect_cameras_batch(mt, mo, doff, dobs, dsum, tri1[0], tri1[2], nimg, K, images, seeds, cam=dcam,
                           cam_pair=dcam_pair, **rargs, **outs)
    tri2 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    ref_outs = {k: _poisoned(g, m) for k, m in dict(cam_out=12 * nimg, cam_obs=nimg, cam_rms=2 * nimg, cam_steps=nimg,
                                                    cam_status=nimg, summary=8).items()}
    g.refine_cameras_batch(mt, mo, doff, dobs, dsum, tri2[0], tri2[2], nimg, dcam, dcam_pair, K, hold=hold, min_obs=6,
                           num_loops=5, max_error=4.0, orthonormalise=1, **ref_outs)
    g.sync()
    T = int(base["export_summary"][2])

    def tri_outputs(t):
        return dict(points=g.download(t[0], (4 * mt,), np.uint32), point_views=g.download(t[1], (mt,), np.uint32),
                    point_status=g.download(t[2], (mt,), np.uint32), obs_error=g.download(t[3], (mo,), np.uint32),
                    summary=g.download(t[4], (8,), np.uint32))

    got1, got2 = tri_outputs(tri1), tri_outputs(tri2)
    assert pair_linked.tolist()[5:] == [C.UNSET] * 3 and (pair_linked[:5] != C.UNSET).all()
    assert status1.tolist()[5:] == [RC.NO_CAMERA] * 3
    # the resection against its restatement
    case = C.resect_case(dict(base, cam=cam_linked, cam_pair=pair_linked, points=got1["points"].view(f32).reshape(-1, 4),
                              point_status=got1["point_status"].view(np.int32)), images, seeds=seeds, **rargs)
    got = {k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}
    got["cam"], got["cam_pair"] = g.download(dcam, (12 * nimg,), np.uint32), g.download(dcam_pair, (nimg,), np.uint32)
    e = _compare(got, case, "chain, resect")
    status = [x["status"] for x in e["entries"]]
    print("chain: T %d, resect status %s candidates %s inliers %s" % (
        T, status, [x["cand"] for x in e["entries"]], [x["inliers"] for x in e["entries"]]))
    assert status == [C.OK] * 3 + [C.SKIPPED] * 5                # images 7, 6, 5, then the linked ones
    pair2 = got["cam_pair"].view(np.int32)
    assert pair2.tolist() == pair_linked.tolist()[:5] + [C.RESECTED] * 3
    cam2 = got["cam"].view(f32).reshape(-1, 12)
    assert cam2[:5].tobytes() == cam_linked[:5].tobytes()
    # both triangulations against theirs
    for gt, cam, pair in ((got1, cam_linked, pair_linked), (got2, cam2, pair2)):
        tc = dict(base, cam=cam, cam_pair=pair, min_views=2, num_loops=5, memo={})
        with np.errstate(all="ignore"):
            x = TC.expected_triangulate(tc)
        for k in ("points", "point_views", "point_status", "obs_error", "summary"):
            written = x[k] != POISON_WORD
            assert (gt[k][written] == x[k][written]).all(), k
    v1, v2 = got1["point_views"].view(np.int32)[:T], got2["point_views"].view(np.int32)[:T]
    behind = np.array([(base["obs"]["frame"][base["track_offsets"][t]:base["track_offsets"][t + 1]] >= 5).sum()
                       for t in range(T)])
    assert (v2 == v1 + behind).all() and behind.sum() > 0
    # refine behind it
    rcase = dict(base, cam=cam2, cam_pair=pair2, points=got2["points"].view(f32).reshape(-1, 4),
                 point_status=got2["point_status"].view(np.int32), hold=tuple(hold), min_obs=6, num_loops=5,
                 max_error=4.0, orthonormalise=1)
    er = RC.expected_refine(rcase)
    for k in RC.OUTPUTS:
        assert g.download(ref_outs[k], (len(er[k]),), np.uint32).tobytes() == er[k].tobytes(), k
    assert er["cam_status"].view(np.int32).tolist()[5:] == [RC.OK] * 3
    print("chain: views %d -> %d, refine status %s" % (v1.sum(), v2.sum(), er["cam_status"].view(np.int32).tolist()))


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
