"""misift_triangulate_tracks_batch on the device: one world point per exported track under the linked cameras.

Every comparison is byte equality with triangulate_cases.expected_triangulate (pinned in test_triangulate_cpu.py to the
library's host hook and to float64, where the premises of the cases are asserted too): d_points, d_point_views,
d_point_status, d_obs_error and d_summary, entries the call must leave alone included, and every byte of the offsets, the
observations, the export summary, the cameras and d_cam_pair, which the call must not write.  The tracks are planted
directly; no images are needed.  The outputs have exactly the stated capacity and are poisoned first; all allocations of
the module are guarded.  The shapes are the ones at which the kernel can go wrong: no track, one, either side of a
wavefront and of the 256-lane workgroup, T from the device below, beyond and under max_tracks, tracks of 1, 2, 3, 7 and
301 observations, and images on either side of what the kernel stages on chip."""
import numpy as np
import pytest

import posegraph_cases as G
import pose_cases as PC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
OUTPUTS = ("points", "point_views", "point_status", "obs_error", "summary")
INPUTS = (("track_offsets", np.int32), ("obs", TC.OBS_DTYPE), ("export_summary", np.int32), ("cam", f32),
          ("cam_pair", np.int32))
assert POISON_WORD == TC.POISON_WORD


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _sizes(case):
    mt, mo = case["max_tracks"], case["max_obs"]
    return dict(points=4 * mt, point_views=mt, point_status=mt, obs_error=mo, summary=8)


def _inputs(case):
    """The inputs at exactly the sizes the call states."""
    mt, mo = case["max_tracks"], case["max_obs"]
    ins = dict(track_offsets=np.ascontiguousarray(case["track_offsets"][:mt + 1], np.int32),
               obs=np.ascontiguousarray(case["obs"][:mo]), export_summary=np.ascontiguousarray(case["export_summary"]),
               cam=np.ascontiguousarray(case["cam"], f32), cam_pair=np.ascontiguousarray(case["cam_pair"], np.int32))
    assert len(ins["track_offsets"]) == mt + 1 and len(ins["obs"]) == mo and len(ins["cam"]) == case["nimages"]
    return ins


def _triangulate(ctx, case, obs_error=True):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays (obs_error None when it is
    left out).  The inputs must come back as they went in."""
    ins = _inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in _sizes(case).items() if obs_error or k != "obs_error"}
    ctx.triangulate_tracks_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"],
                                 dev["export_summary"], case["nimages"], dev["cam"], dev["cam_pair"], case["intrinsics"],
                                 min_views=case["min_views"], num_loops=case["num_loops"],
                                 **dict(outs, obs_error=outs.get("obs_error")))
    ctx.sync()
    for k, dt in INPUTS:
        assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    got = {k: ctx.download(outs[k], (n,), np.uint32) for k, n in _sizes(case).items() if k in outs}
    got.setdefault("obs_error", None)
    return got


def _compare(got, case, what):
    with np.errstate(all="ignore"):
        e = TC.expected_triangulate(case, obs_error=got["obs_error"] is not None)
    for k in OUTPUTS:
        if e[k] is None:
            assert got[k] is None
            continue
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in ("point_views", "point_status", "summary") else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))
    return e


@pytest.mark.parametrize("T", [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_track_count(g, T):
    """max_tracks = T: the last workgroup is cut at every offset, and 257 is one more than a workgroup's worth.  The pool
    holds tracks of 1, 2, 3 and 7 observations and, as track 5, one of 301."""
    pool = TC.pool_case()
    case = TC.with_T(pool, T, max(T, 1))
    e = _compare(_triangulate(g, case), case, "T = %d" % T)
    s = e["summary"].view(np.int32)
    assert s[0] == T and s[1] + s[3] == T
    if T > 5:
        assert pool["track_offsets"][6] - pool["track_offsets"][5] == 301


@pytest.mark.parametrize("T,want", [(63, 63), (200, 200), (300, 258), (2 ** 31 - 1, 258), (-1, 0), (-2 ** 31, 0)])
def test_track_count_from_the_device(g, T, want):
    """T below max_tracks leaves the entries behind it alone; beyond it, it is clamped; below 0 it is 0."""
    case = TC.with_T(TC.pool_case(), T)
    e = _compare(_triangulate(g, case), case, "T = %d of 258" % T)
    assert e["summary"].view(np.int32)[0] == want and (e["point_status"][want:] == POISON_WORD).all()


@pytest.mark.parametrize("num_loops,min_views,obs_error", [(5, 2, True), (0, 2, True), (1, 3, False), (5, 3, True)])
def test_hostile_tracks_loops_and_views(g, num_loops, min_views, obs_error):
    """Frames outside the images, unset and non-finite cameras, non-finite positions, a point behind a camera, identical
    cameras, a point on a camera centre, a frame seen twice; then the pool; d_obs_error NULL in one of the settings."""
    for name, case in (("hostile", TC.hostile_case(num_loops, min_views)), ("pool", TC.pool_case(num_loops, min_views))):
        got = _triangulate(g, case, obs_error)
        e = _compare(got, case, name)
        s = e["summary"].view(np.int32)
        assert (s[6] > 0) == (num_loops > 0) and s[1] > 0 and s[3] > 0
        if name == "hostile":
            assert s[4] > 0 and s[5] > 0                         # singular and behind, both met
            again = _triangulate(g, case, obs_error)             # two runs, the same bytes
            for k in OUTPUTS:
                assert (got[k] is None and again[k] is None) or got[k].tobytes() == again[k].tobytes(), k


def test_bad_offsets(g):
    """Offsets that decrease, pass max_obs or are negative give status 4 and address nothing."""
    case = TC.bad_offsets_case()
    e = _compare(_triangulate(g, case), case, "bad offsets")
    assert e["summary"].view(np.int32)[7] == len(case["bad"]) == 7


def test_either_side_of_the_staging_capacity(g):
    cap = TC.capacity()
    for nimages in (cap, cap + 1):
        case = TC.capacity_case(nimages)
        e = _compare(_triangulate(g, case), case, "%d images" % nimages)
        assert e["summary"].view(np.int32)[1] == 70 and case["obs"]["frame"].max() == nimages - 1


def test_chain_far_from_the_origin(g):
    case = TC.chain_case()["case"]
    e = _compare(_triangulate(g, case), case, "chain of 64")
    assert e["summary"].view(np.int32).tolist()[:3] == [244, 244, 976]


def test_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = TC.planted(0.05, 0.5, ntracks=12, ncams=6, seed=56)["case"]
    ins = _inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in _sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    good = dict(ctx=g.h, max_tracks=case["max_tracks"], max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, nimages=case["nimages"],
                cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr, intrinsics=K.ctypes.data, min_views=2, num_loops=5,
                **{k: outs[k].ptr for k in OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_triangulate_tracks_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-7), dict(nimages=0),
           dict(nimages=-1), dict(min_views=1), dict(min_views=0), dict(min_views=-2), dict(num_loops=-1),
           dict(obs=dev["obs"].ptr + 4), dict(obs=dev["obs"].ptr + 8)]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "cam", "cam_pair", "intrinsics", "points",
                                "point_views", "point_status", "summary")]
    lists = []                                                   # kept alive until the calls are made
    for at in (0, 1, 4 * case["nimages"] - 4, 4 * case["nimages"] - 3):
        for v in (0.0, -1500.0, np.nan, np.inf, -np.inf):        # fx, fy of the first and the last image
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for at in (2, 3, 4 * case["nimages"] - 1):
        for v in (np.nan, np.inf, -np.inf):                      # cx, cy
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, n in _sizes(case).items():
        assert (g.download(outs[k], (n,), np.uint32) == POISON_WORD).all(), k
    # the same arguments, unbroken; then without d_obs_error, which may be NULL
    assert call() == MISIFT_OK
    g.sync()
    _compare({k: g.download(outs[k], (n,), np.uint32) for k, n in _sizes(case).items()}, case, "unbroken")
    again = {k: _poisoned(g, n) for k, n in _sizes(case).items()}
    assert call(**{k: again[k].ptr for k in OUTPUTS if k != "obs_error"}, obs_error=None) == MISIFT_OK
    g.sync()
    got = {k: g.download(again[k], (n,), np.uint32) for k, n in _sizes(case).items()}
    assert (got["obs_error"] == POISON_WORD).all()
    _compare(dict(got, obs_error=None), case, "without d_obs_error")


def test_find_improve_recover_link_and_link_export_triangulate(g):
    """Both chains on the 8-camera scene of posegraph_cases, nothing read in between: find -> improve -> recover_pose ->
    link_poses for the cameras, link_tracks -> export_tracks for the observation lists, then this call.  The answer is
    byte-equal to the restatement fed the device's own offsets, observations, summary and cameras."""
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
    # the record batch: image i's records are the set-1 records of pair (i, i + 1); the last image's positions are the
    # set-2 positions of the rows that point into it
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
    max_tracks, max_obs = total // 3 + 1, total
    doff, _, dobs, _, dsum = g.export_tracks_batch(d_recs, nimg, d_cnt, None, n, max_records=total, track=lab[0],
                                                   track_len=lab[1], track_frames=lab[2], min_len=3, consistent_only=1,
                                                   max_tracks=max_tracks, max_obs=max_obs, record_obs=None)
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    outs = {k: _poisoned(g, m) for k, m in dict(points=4 * max_tracks, point_views=max_tracks, point_status=max_tracks,
                                                obs_error=max_obs, summary=8).items()}
    g.triangulate_tracks_batch(max_tracks, max_obs, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5,
                               **outs)
    g.sync()
    case = dict(max_tracks=max_tracks, max_obs=max_obs, track_offsets=g.download(doff, (max_tracks + 1,), np.int32),
                obs=g.download(dobs, (max_obs,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, cam=g.download(dcam, (nimg, 12), f32), cam_pair=g.download(dcam_pair, (nimg,), np.int32),
                intrinsics=K, min_views=2, num_loops=5)
    assert case["cam"].tobytes() == G.expected_link_poses(pc)["cam"].tobytes()
    got = {k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}
    e = _compare(got, case, "chain")
    s = e["summary"].view(np.int32)
    T = int(case["export_summary"][2])
    rms = e["points"].view(f32).reshape(-1, 4)[:T][e["point_status"][:T] == TC.OK, 3]
    print("chain: T %d summary %s rms median %.3g max %.3g px" % (T, s.tolist(), np.median(rms), rms.max()))
    assert s[0] == T >= 100 and s[1] >= T // 2 and s[7] == 0 and (case["cam_pair"] != G.UNSET).all()


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
