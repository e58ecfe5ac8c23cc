"""misift_correspond_tracks_batch, misift_align_points_batch and misift_transform_scene_batch on the device.

Every comparison is byte equality with the restatement of align_cases.py (pinned in test_align_cpu.py to the library's
host hooks and to float64, where the premises of the cases are asserted too).  The outputs have exactly the stated sizes
and are poisoned first, what a call must not write must stay poisoned, the inputs must come back as they went in, and
all allocations of the module are guarded.  The shapes are the ones at which the kernels can go wrong: candidates either
side of three and of one and two count chunks, a src_cap off the multiple of 16, hypotheses either side of a block, n
from the device below, at and beyond the capacity, hostile maps, coordinates and statuses, more members than slots."""
import numpy as np
import pytest

import align_cases as C
import posegraph_cases as G
import pose_cases as PC
import resect_cases as RS
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


# ---- misift_align_points_batch

def _align_sizes(case):
    n = len(case["ranges"])
    out = dict(sim=16 * n, align_cand=n, align_inliers=n, align_status=n, summary=8)
    if case["want_inlier"]:
        out["inlier"] = len(case["map"])
    return out


def _align_inputs(case):
    ins = dict(src=np.ascontiguousarray(case["src"], f32), dst=np.ascontiguousarray(case["dst"], f32),
               map=np.ascontiguousarray(case["map"], np.int32))
    for k in ("src_status", "dst_status", "count"):
        if case.get(k) is not None:
            ins[k] = np.ascontiguousarray(case[k], np.int32)
    return ins


def _align(ctx, case):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays.  The inputs must come back
    as they went in, and what lies behind an output of no entry must stay poisoned."""
    ins = _align_inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    sizes = _align_sizes(case)
    outs = {k: _poisoned(ctx, n) for k, n in sizes.items()}
    ctx.align_points_batch(dev["src"], dev["dst"], dev["map"], case["ranges"], case["seeds"],
                           src_status=dev.get("src_status"), dst_status=dev.get("dst_status"), count=dev.get("count"),
                           count_stride=case["count_stride"], num_loops=case["num_loops"], thresh=case["thresh"],
                           min_inliers=case["min_inliers"], refit_loops=case["refit_loops"], **outs)
    ctx.sync()
    for k, v in ins.items():
        assert ctx.download(dev[k], v.shape, v.dtype).tobytes() == v.tobytes(), (k, "was written")
    got = {k: ctx.download(outs[k], (n,), np.uint32) if n else np.zeros(0, np.uint32) for k, n in sizes.items()}
    for k, n in sizes.items():
        if n == 0:
            assert ctx.download(outs[k], (1,), np.uint32)[0] == POISON_WORD, k
    return got


def _compare_align(got, case, what):
    e = C.expected_align(case)
    for k in got:
        bad = np.nonzero(got[k] != e[k])[0]
        view = f32 if k == "sim" else np.int32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))
    return e


@pytest.mark.parametrize("name", C.GPU_CASES)
def test_align_case(g, name):
    """Every case of align_cases.gpu_cases (what each is built to hit is asserted in test_align_cpu.py)."""
    case = C.gpu_cases()[name]
    e = _compare_align(_align(g, case), case, name)
    print(name, "status", [x["status"] for x in e["entries"]], "candidates", [x["cand"] for x in e["entries"]],
          "inliers", [x["inliers"] for x in e["entries"]], "kept", [x["kept"] for x in e["entries"]])


def _resect(ctx, case):
    dev = {k: ctx.upload(np.ascontiguousarray(case[k])) for k in ("track_offsets", "obs", "export_summary", "points",
                                                                  "point_status")}
    ctx.resect_cameras_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                             dev["points"], dev["point_status"], case["nimages"], case["intrinsics"], case["images"],
                             case["seeds"], case["max_cand"], num_loops=case["num_loops"], thresh=case["thresh"],
                             min_inliers=case["min_inliers"])


def test_shared_temp_and_two_runs(g):
    """Behind a resection that takes more temp memory than the alignment and leaves it dirty, behind one that takes less,
    and run twice: the same bytes."""
    cases, rs = C.gpu_cases(), RS.gpu_cases()
    _resect(g, rs["candidates 513 1025"])                        # the larger
    first = _align(g, cases["hostile"])
    _compare_align(first, cases["hostile"], "behind a larger resect")
    _resect(g, rs["no candidates"])                              # the smaller
    _compare_align(_align(g, cases["candidates 513 1025"]), cases["candidates 513 1025"], "behind a smaller resect")
    again = _align(g, cases["hostile"])
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k


def test_align_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = C.gpu_cases()["four entries"]
    ins = _align_inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    sizes = _align_sizes(case)
    outs = {k: _poisoned(g, n) for k, n in sizes.items()}
    ranges, seeds = np.ascontiguousarray(case["ranges"], np.int32), np.ascontiguousarray(case["seeds"], np.uint32)
    cnt = g.upload(np.full(len(ranges), 10 ** 6, np.int32))
    good = dict(ctx=g.h, src=dev["src"].ptr, src_status=dev["src_status"].ptr, dst=dev["dst"].ptr,
                dst_status=dev["dst_status"].ptr, map=dev["map"].ptr, nsel=len(ranges), ranges=ranges.ctypes.data,
                seeds=seeds.ctypes.data, count=cnt.ptr, count_stride=1, num_loops=case["num_loops"],
                thresh=case["thresh"], min_inliers=case["min_inliers"], refit_loops=case["refit_loops"],
                sim=outs["sim"].ptr, align_cand=outs["align_cand"].ptr, align_inliers=outs["align_inliers"].ptr,
                align_status=outs["align_status"].ptr, inlier=outs["inlier"].ptr, summary=outs["summary"].ptr)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_align_points_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(nsel=-1), dict(ranges=None), dict(seeds=None), dict(num_loops=0), dict(num_loops=-1),
           dict(thresh=np.nan), dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=-np.inf), dict(min_inliers=2),
           dict(min_inliers=0), dict(min_inliers=-3), dict(refit_loops=-1), dict(count_stride=-1),
           dict(num_loops=2 ** 31 - 15), dict(num_loops=2 ** 31 - 1)]
    bad += [{k: None} for k in ("src", "dst", "map", "sim", "align_cand", "align_inliers", "align_status", "summary")]
    lists = []                                                   # kept alive until the calls are made
    for e, col, v in ((0, 0, -1), (1, 1, 0), (2, 1, -5), (3, 2, -1), (0, 3, 0), (1, 3, -2), (2, 0, 2 ** 31 - 1),
                      (3, 2, 2 ** 31 - 1), (0, 1, 2 ** 31 - 15)):
        r = ranges.copy()
        r[e, col] = v
        lists.append(r)
        bad.append(dict(ranges=r.ctypes.data))
    r = ranges.copy()                                            # d_inlier given and two source ranges overlapping
    r[1, 0] = r[0, 0] + r[0, 1] - 1
    lists.append(r)
    bad.append(dict(ranges=r.ctypes.data))
    # one launch holds 2^31 - 1 workgroups: 4 entries x 2^25 hypothesis blocks x 20 chunks do not fit
    r = ranges.copy()
    r[0, 1] = 10000
    r[1:, 0] += 10000
    lists.append(r)
    bad.append(dict(ranges=r.ctypes.data, num_loops=2 ** 31 - 16))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in sizes.items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, v in ins.items():
        assert g.download(dev[k], v.shape, v.dtype).tobytes() == v.tobytes(), (k, "was written")
    # NULL where NULL is allowed; overlapping source ranges without d_inlier; nsel 0; then the same arguments, unbroken
    lists.append(r := ranges.copy())
    r[1, :2] = r[0, :2]
    scratch = {k: _poisoned(g, n) for k, n in sizes.items()}
    alt = {k: scratch[k].ptr for k in ("sim", "align_cand", "align_inliers", "align_status", "summary")}
    assert call(ranges=r.ctypes.data, inlier=None, **alt) == MISIFT_OK
    assert call(src_status=None, dst_status=None, count=None, inlier=None, **alt) == MISIFT_OK
    assert call(nsel=0, ranges=None, seeds=None, **alt, inlier=scratch["inlier"].ptr) == MISIFT_OK
    g.sync()
    assert (g.download(scratch["summary"], (8,), np.uint32) == 0).all()
    assert (g.download(scratch["inlier"], (sizes["inlier"],), np.uint32) == POISON_WORD).all()
    assert call() == MISIFT_OK
    g.sync()
    got = {k: g.download(outs[k], (m,), np.uint32) for k, m in sizes.items()}
    _compare_align(got, case, "unbroken")


# ---- misift_correspond_tracks_batch

SCENE_KEYS = ("record_obs", "track_offsets", "export_summary")


def _correspond(ctx, case, dev=None):
    A, B = case["a"], case["b"]
    ins = {s + k: np.ascontiguousarray(x[k], np.int32) for s, x in (("a_", A), ("b_", B)) for k in SCENE_KEYS}
    assert len(ins["a_track_offsets"]) == A["max_tracks"] + 1 and len(ins["b_track_offsets"]) == B["max_tracks"] + 1
    assert len(ins["a_record_obs"]) == A["max_records"] and len(ins["b_record_obs"]) == B["max_records"]
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = dict(track_map=_poisoned(ctx, A["max_tracks"]), summary=_poisoned(ctx, 8))
    ctx.correspond_tracks_batch(A["max_records"], dev["a_record_obs"], A["max_tracks"], A["max_obs"],
                                dev["a_track_offsets"], dev["a_export_summary"], B["max_records"], dev["b_record_obs"],
                                B["max_tracks"], B["max_obs"], dev["b_track_offsets"], dev["b_export_summary"],
                                shift=case["shift"], **outs)
    ctx.sync()
    for k, v in ins.items():
        assert ctx.download(dev[k], v.shape, v.dtype).tobytes() == v.tobytes(), (k, "was written")
    return dict(map=ctx.download(outs["track_map"], (A["max_tracks"],), np.uint32),
                summary=ctx.download(outs["summary"], (8,), np.uint32))


@pytest.mark.parametrize("name", C.CORRESPOND_CASES)
def test_correspond_case(g, name):
    case = C.correspond_cases()[name]
    got, e = _correspond(g, case), C.expected_correspond(case)
    for k in ("map", "summary"):
        bad = np.nonzero(got[k] != e[k])[0]
        assert len(bad) == 0, (name, k, bad[:8], got[k][bad[:4]].view(np.int32), e[k][bad[:4]].view(np.int32))
    print(name, "summary", e["summary"].view(np.int32)[:5].tolist())


def test_correspond_argument_errors(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = C.correspond_cases()["conflict"]
    A, B = case["a"], case["b"]
    dev = {s + k: g.upload(np.ascontiguousarray(x[k], np.int32)) for s, x in (("a_", A), ("b_", B)) for k in SCENE_KEYS}
    out_map, out_sum = _poisoned(g, A["max_tracks"]), _poisoned(g, 8)
    good = dict(ctx=g.h, shift=0, mra=A["max_records"], roa=dev["a_record_obs"].ptr, mta=A["max_tracks"],
                moa=A["max_obs"], offa=dev["a_track_offsets"].ptr, suma=dev["a_export_summary"].ptr,
                mrb=B["max_records"], rob=dev["b_record_obs"].ptr, mtb=B["max_tracks"], mob=B["max_obs"],
                offb=dev["b_track_offsets"].ptr, sumb=dev["b_export_summary"].ptr, map=out_map.ptr, summary=out_sum.ptr)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_correspond_tracks_batch(*[a[k] for k in good])

    bad = [{k: None} for k in ("ctx", "roa", "offa", "suma", "rob", "offb", "sumb", "map", "summary")]
    bad += [{k: v} for k in ("mra", "mta", "moa", "mrb", "mtb", "mob") for v in (0, -1)]
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    assert (g.download(out_map, (A["max_tracks"],), np.uint32) == POISON_WORD).all()
    assert (g.download(out_sum, (8,), np.uint32) == POISON_WORD).all()
    for shift in (2 ** 31 - 1, -2 ** 31):                        # no record of A is one of B: no tie, no error
        assert call(shift=shift) == MISIFT_OK
        g.sync()
        assert g.download(out_sum, (8,), np.int32).tolist() == [3, 3, 0, 0, 0, 0, 0, 0]
        assert g.download(out_map, (A["max_tracks"],), np.int32)[:3].tolist() == [-1, -1, -1]


# ---- misift_transform_scene_batch

def _transform(ctx, case, in_place):
    ins = dict(sim=np.ascontiguousarray(case["sim"], f32), sim_status=np.array([case["sim_status"]], np.int32),
               export_summary=np.ascontiguousarray(case["export_summary"], np.int32),
               points=np.ascontiguousarray(case["points"], f32), point_status=np.ascontiguousarray(case["point_status"]),
               cam=np.ascontiguousarray(case["cam"], f32), cam_pair=np.ascontiguousarray(case["cam_pair"], np.int32))
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    if in_place:
        outs = dict(points_out=dev["points"], cam_out=dev["cam"])
    else:
        outs = dict(points_out=_poisoned(ctx, 4 * case["max_tracks"]), cam_out=_poisoned(ctx, 12 * case["nimages"]))
    ctx.transform_scene_batch(dev["sim"], case["max_tracks"], dev["export_summary"], dev["points"], dev["point_status"],
                              case["nimages"], dev["cam"], dev["cam_pair"],
                              sim_status=None if case.get("no_status") else dev["sim_status"], **outs)
    ctx.sync()
    for k, v in ins.items():
        if not (in_place and k in ("points", "cam")):
            assert ctx.download(dev[k], v.shape, v.dtype).tobytes() == v.tobytes(), (k, "was written")
    return dict(points_out=ctx.download(outs["points_out"], (4 * case["max_tracks"],), np.uint32),
                cam_out=ctx.download(outs["cam_out"], (12 * case["nimages"],), np.uint32))


@pytest.mark.parametrize("in_place", (False, True), ids=("out of place", "in place"))
@pytest.mark.parametrize("status", (0, 2, None), ids=("status 0", "status 2", "no status"))
def test_transform(g, in_place, status):
    """Unset and root cameras, failed points, NaN in a set and in an unset camera, tracks behind T, NaN payloads in the
    fourth word; under a status word of 0, of 2 (everything copied) and without one."""
    case = C.transform_case(sim_status=0 if status is None else status)
    case["no_status"] = status is None
    got, e = _transform(g, case, in_place), C.expected_transform(case)
    for k in e:
        bad = np.nonzero(got[k] != e[k])[0]
        assert len(bad) == 0, (k, bad[:8], got[k][bad[:4]].view(f32), e[k][bad[:4]].view(f32))
    if status == 2:
        assert got["points_out"].tobytes() == case["points"].tobytes() and got["cam_out"].tobytes() == case["cam"].tobytes()


def test_transform_argument_errors(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = C.transform_case()
    dev = dict(sim=g.upload(case["sim"]), st=g.upload(np.zeros(1, np.int32)), es=g.upload(case["export_summary"]),
               pts=g.upload(case["points"]), ps=g.upload(case["point_status"]), cam=g.upload(case["cam"]),
               pair=g.upload(case["cam_pair"]))
    po, co = _poisoned(g, 4 * case["max_tracks"]), _poisoned(g, 12 * case["nimages"])
    good = dict(ctx=g.h, sim=dev["sim"].ptr, st=dev["st"].ptr, mt=case["max_tracks"], es=dev["es"].ptr, pts=dev["pts"].ptr,
                ps=dev["ps"].ptr, n=case["nimages"], cam=dev["cam"].ptr, pair=dev["pair"].ptr, po=po.ptr, co=co.ptr)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_transform_scene_batch(*[a[k] for k in good])

    bad = [{k: None} for k in ("ctx", "sim", "es", "pts", "ps", "cam", "pair", "po", "co")]
    bad += [dict(mt=0), dict(mt=-1), dict(n=0), dict(n=-1), dict(po=dev["pts"].ptr + 16), dict(co=dev["cam"].ptr + 48)]
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    assert (g.download(po, (4 * case["max_tracks"],), np.uint32) == POISON_WORD).all()
    assert (g.download(co, (12 * case["nimages"],), np.uint32) == POISON_WORD).all()
    assert g.download(dev["pts"], case["points"].shape, f32).tobytes() == case["points"].tobytes()
    assert call(st=None) == MISIFT_OK


# ---- the chain

def test_correspond_align_transform_triangulate(g):
    """Two overlapping exports of one record batch on the 8-camera scene of posegraph_cases: A links the tracks over all
    pairs, B without the matches of pair 0, so B's tracks do not hold image 0 and are numbered on their own.  A is
    triangulated under the linked cameras, B under those cameras moved into another gauge (a planted similarity
    transform).  Then correspond -> align (n from A's export summary on the device) -> transform -> triangulate under the
    transformed cameras, nothing read in between; every step is byte-equal to its restatement fed the device's own
    buffers, the transform found is the planted one, and A's transformed points are B's."""
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
    counts_b = np.full(npairs, n, np.int32)
    counts_b[0] = 0                                              # B: no match of pair 0
    mt, mo = total // 3 + 1, total
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    scenes = []
    for row_counts in (dc, g.upload(counts_b)):
        lab = g.link_tracks_batch(pc["pairs"], d, row_counts, n, nimg, d_cnt, None, n, max_records=total,
                                  min_score=GATES[0], max_ambiguity=GATES[1], max_error=pc["max_error"])
        rec_obs = g.upload(np.full(total, -1, np.int32))         # the precondition of correspond
        doff, _, dobs, _, dsum = g.export_tracks_batch(d_recs, nimg, d_cnt, None, n, max_records=total, track=lab[0],
                                                       track_len=lab[1], track_frames=lab[2], min_len=3,
                                                       consistent_only=1, max_tracks=mt, max_obs=mo, record_obs=rec_obs)
        scenes.append(dict(off=doff, obs=dobs, sum=dsum, rec=rec_obs))
    A, B = scenes
    g.sync()
    cam_a, pair = g.download(dcam, (nimg, 12), f32), g.download(dcam_pair, (nimg,), np.int32)
    assert (pair != C.UNSET).all()
    planted = C.transform_case()["sim"]
    cam_b = C.one_nan(C.transform_cameras(planted, cam_a))
    dcam_b = g.upload(cam_b)
    tri_a = g.triangulate_tracks_batch(mt, mo, A["off"], A["obs"], A["sum"], nimg, dcam, dcam_pair, K, min_views=2,
                                       num_loops=5)
    tri_b = g.triangulate_tracks_batch(mt, mo, B["off"], B["obs"], B["sum"], nimg, dcam_b, dcam_pair, K, min_views=2,
                                       num_loops=5)
    # the four new steps, nothing read in between
    outs = dict(track_map=_poisoned(g, mt), csum=_poisoned(g, 8), sim=_poisoned(g, 16), cand=_poisoned(g, 1),
                inl=_poisoned(g, 1), st=_poisoned(g, 1), asum=_poisoned(g, 8), inlier=_poisoned(g, mt),
                pts=_poisoned(g, 4 * mt), cam=_poisoned(g, 12 * nimg))
    g.correspond_tracks_batch(total, A["rec"], mt, mo, A["off"], A["sum"], total, B["rec"], mt, mo, B["off"], B["sum"],
                              track_map=outs["track_map"], summary=outs["csum"])
    aargs = dict(num_loops=128, thresh=0.05, min_inliers=12, refit_loops=3)
    ranges, seeds = np.array([[0, mt, 0, mt]], np.int32), np.array([77], np.uint32)
    g.align_points_batch(tri_a[0], tri_b[0], outs["track_map"], ranges, seeds, src_status=tri_a[2], dst_status=tri_b[2],
                         count=A["sum"].ptr + 8,
                         count_stride=8, sim=outs["sim"], align_cand=outs["cand"], align_inliers=outs["inl"],
                         align_status=outs["st"], inlier=outs["inlier"], summary=outs["asum"], **aargs)
    g.transform_scene_batch(outs["sim"], mt, A["sum"], tri_a[0], tri_a[2], nimg, dcam, dcam_pair, sim_status=outs["st"],
                            points_out=outs["pts"], cam_out=outs["cam"])
    tri_t = g.triangulate_tracks_batch(mt, mo, A["off"], A["obs"], A["sum"], nimg, outs["cam"], dcam_pair, K,
                                       min_views=2, num_loops=5)
    g.sync()

    def scene_host(s):
        return dict(max_records=total, record_obs=g.download(s["rec"], (total,), np.int32), max_tracks=mt, max_obs=mo,
                    track_offsets=g.download(s["off"], (mt + 1,), np.int32),
                    export_summary=g.download(s["sum"], (8,), np.int32))

    ha, hb = scene_host(A), scene_host(B)
    TA, TB = int(ha["export_summary"][2]), int(hb["export_summary"][2])
    # correspond
    ec = C.expected_correspond(dict(a=ha, b=hb, shift=0))
    got_map = g.download(outs["track_map"], (mt,), np.uint32)
    assert got_map.tobytes() == ec["map"].tobytes()
    assert g.download(outs["csum"], (8,), np.uint32).tobytes() == ec["summary"].tobytes()
    cs = ec["summary"].view(np.int32)
    print("chain: T_A %d T_B %d ties %d mapped %d conflicts %d" % tuple(cs[:5]))
    assert 0 < TB and cs[3] >= 50 and cs[4] == 0
    # align
    pts_a, pts_b = g.download(tri_a[0], (mt, 4), f32), g.download(tri_b[0], (mt, 4), f32)
    st_a, st_b = g.download(tri_a[2], (mt,), np.int32), g.download(tri_b[2], (mt,), np.int32)
    acase = dict(src=pts_a, dst=pts_b, map=got_map.view(np.int32), ranges=ranges, seeds=seeds, src_status=st_a,
                 dst_status=st_b, count=ha["export_summary"][2:], count_stride=8, want_inlier=True, **aargs)
    ea = C.expected_align(acase)
    got = dict(sim=g.download(outs["sim"], (16,), np.uint32), align_cand=g.download(outs["cand"], (1,), np.uint32),
               align_inliers=g.download(outs["inl"], (1,), np.uint32), align_status=g.download(outs["st"], (1,), np.uint32),
               summary=g.download(outs["asum"], (8,), np.uint32), inlier=g.download(outs["inlier"], (mt,), np.uint32))
    for k in got:
        assert got[k].tobytes() == ea[k].tobytes(), k
    x = ea["entries"][0]
    sim = got["sim"].view(f32)
    print("chain: align status %d candidates %d inliers %d kept %d rms %.4g s %.6g" % (
        x["status"], x["cand"], x["inliers"], x["kept"], sim[13], sim[12]))
    assert x["status"] == C.OK and x["inliers"] >= 50
    assert np.abs(sim[:9] - planted[:9]).max() < 1e-2 and abs(sim[12] - planted[12]) < 1e-2 * planted[12]
    assert np.abs(sim[9:12] - planted[9:12]).max() < 5e-2
    # transform
    tcase = dict(sim=sim, sim_status=0, max_tracks=mt, export_summary=ha["export_summary"], points=pts_a,
                 point_status=st_a, nimages=nimg, cam=cam_a, cam_pair=pair)
    et = C.expected_transform(tcase)
    got_pts, got_cam = g.download(outs["pts"], (4 * mt,), np.uint32), g.download(outs["cam"], (12 * nimg,), np.uint32)
    assert got_pts.tobytes() == et["points_out"].tobytes() and got_cam.tobytes() == et["cam_out"].tobytes()
    mapped = np.nonzero((got_map.view(np.int32)[:TA] >= 0) & (got["inlier"].view(np.int32)[:TA] == 1))[0]
    moved = got_pts.view(f32).reshape(-1, 4)[mapped, :3]
    assert np.abs(moved - pts_b[got_map.view(np.int32)[mapped], :3]).max() < aargs["thresh"]
    # triangulate under the transformed cameras
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=ha["track_offsets"], obs=g.download(A["obs"], (mo,), TC.OBS_DTYPE),
                export_summary=ha["export_summary"], nimages=nimg, intrinsics=K, cam=got_cam.view(f32).reshape(-1, 12),
                cam_pair=pair, min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        xt = TC.expected_triangulate(base)
    gt = dict(points=g.download(tri_t[0], (4 * mt,), np.uint32), point_views=g.download(tri_t[1], (mt,), np.uint32),
              point_status=g.download(tri_t[2], (mt,), np.uint32), obs_error=g.download(tri_t[3], (mo,), np.uint32),
              summary=g.download(tri_t[4], (8,), np.uint32))
    for k in gt:
        written = xt[k] != POISON_WORD
        assert (gt[k][written] == xt[k][written]).all(), k
    ok = (gt["point_status"].view(np.int32)[:TA] == 0) & (st_a[:TA] == 0)
    again = gt["points"].view(f32).reshape(-1, 4)[:TA][ok, :3]
    assert np.abs(again - got_pts.view(f32).reshape(-1, 4)[:TA][ok, :3]).max() < 0.05


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
