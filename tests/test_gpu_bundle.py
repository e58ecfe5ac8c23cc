"""misift_adjust_bundle_batch on the device: cameras and track points adjusted jointly.

Every comparison is byte equality with bundle_cases.expected_bundle (pinned in test_bundle_cpu.py to the library's host
hook, to float64 and to dense linear algebra, where the premises of the cases are asserted too): all nine outputs, and
every byte of the offsets, the observations, the export summary, the points, their status, the cameras and d_cam_pair,
which the call must not write.  The scenes are planted directly; no images are needed.  The outputs have exactly the
stated capacity and are poisoned first; all allocations of the module are guarded.  The shapes are the ones at which the
kernels can go wrong: no free camera, one, 4 to 257 images for the cross-image rule, images around min_obs and either
side of one row of the position rule and its wrap, 0 to 257 tracks, tracks of 2 to 301 views, T and O from the device
below, beyond and under their capacities."""
import numpy as np
import pytest

import bundle_cases as BC
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


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


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


def _adjust(ctx, case, in_place=False):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays.  The inputs must come back
    as they went in (but for d_cam and d_points when they are the outputs)."""
    assert TC.POISON_WORD == POISON_WORD
    ins = _inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in BC.sizes(case).items()}
    if in_place:
        outs["cam_out"], outs["points_out"] = dev["cam"], dev["points"]
    ctx.adjust_bundle_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                            dev["points"], dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"],
                            case["intrinsics"], hold=case["hold"], min_views=case["min_views"], min_obs=case["min_obs"],
                            num_loops=case["num_loops"], cg_iters=case["cg_iters"], max_error=case["max_error"],
                            lambda0=case["lambda0"], orthonormalise=case["orthonormalise"], **outs)
    ctx.sync()
    for k, dt in INPUTS:
        if not (in_place and k in ("cam", "points")):
            assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (n,), np.uint32) for k, n in BC.sizes(case).items()}


def _check(ctx, case, what, in_place=False):
    e = BC.expected_bundle(case)
    got = _adjust(ctx, case, in_place)
    if in_place:                                                 # beyond T the input stays, which is no poison
        T = e["res"]["problem"].T
        e = dict(e, points_out=e["points_out"].copy())
        e["points_out"][4 * T:] = np.ascontiguousarray(case["points"], f32).view(np.uint32).reshape(-1)[4 * T:]
    BC.compare(got, e, what)
    return e


def _summary(e):
    return e["summary"].view(np.int32)


@pytest.mark.parametrize("nimages,ntracks,loops,cg", BC.IMAGE_SHAPES)
def test_every_image_count(g, nimages, ntracks, loops, cg):
    """Root plus held and no free camera (the points move alone), one free camera, and 4 to 257 images for the cross-image
    rule, from tracks of two and three views."""
    case = BC.image_count_case(nimages, ntracks, loops, cg)
    e = _check(g, case, "%d images" % nimages)
    s = _summary(e)
    assert s[5] == min(nimages, 2) and s[1] + s[3] == nimages - s[5] and s[1] >= (nimages - 2) // 2 and s[6] >= 1
    if nimages == 2:
        assert all(h[3] == 0 for h in e["res"]["history"])


def test_members_per_image_around_min_obs_and_the_rows_of_the_position_rule(g):
    case, want = BC.member_counts_case(num_loops=2, cg_iters=3)
    e = _check(g, case, "members per image")
    assert e["cam_obs"].view(np.int32)[2:].tolist() == want == [5, 6, 7, 255, 256, 257, 513]
    assert e["cam_status"].view(np.int32)[2:].tolist() == [BC.FEW_OBS] + [BC.ADJUSTED] * 6


@pytest.mark.parametrize("ntracks", BC.TRACK_COUNTS)
def test_every_track_count(g, ntracks):
    case = BC.track_count_case(ntracks)
    e = _check(g, case, "%d tracks" % ntracks)
    assert _summary(e)[0] == ntracks and _summary(e)[4] == ntracks


@pytest.mark.parametrize("min_views", [2, 3])
def test_tracks_of_2_3_7_and_301_views(g, min_views):
    case = BC.views_case(num_loops=2, cg_iters=4, min_views=min_views)
    e = _check(g, case, "min_views %d" % min_views)
    P = e["res"]["problem"]
    assert sorted(set(P.tcount[:P.T].tolist())) == [2, 3, 7, 301]
    assert _summary(e)[4] == (91 if min_views == 2 else 61)


@pytest.mark.parametrize("T,O", BC.DEVICE_COUNTS)
def test_counts_from_the_device(g, T, O):
    """T and O below their capacities cut the tracks and the slots; beyond them they are clamped; below 0 they are 0.  A
    track that ends beyond O is not valid."""
    case = BC.device_counts_case(T, O)
    e = _check(g, case, "T = %d, O = %d" % (T, O))
    assert _summary(e)[0] == min(max(T, 0), 171)


@pytest.mark.parametrize("num_loops,cg_iters,lambda0,max_error,orth", BC.SETTINGS)
def test_loops_iterations_damping_gate_and_orthonormalise(g, num_loops, cg_iters, lambda0, max_error, orth):
    """The hostile scene (the root, a held and an unset image, a NaN and an inf in a camera, points of status 1 to 4, a
    NaN and an inf in a point, frames outside the images, non-finite positions, points behind a camera) and a planted one
    under every setting; two runs give the same bytes."""
    for name, case in BC.settings_cases(num_loops, cg_iters, lambda0, max_error, orth):
        e = _check(g, case, name)
        s = _summary(e)
        assert len(e["res"]["history"]) == num_loops and s[1] > 0
        if lambda0 > 1e38:
            assert e["res"]["trace"] == ["singular"] * num_loops and s[6] == 0
        if num_loops == 0 and orth == 0:
            assert e["cam_out"].tobytes() == np.ascontiguousarray(case["cam"], f32).tobytes()
            assert e["cost"][0] == e["cost"][1]
        if name == "hostile":
            assert s[5] == 2 and s[7] == 3
            again = _adjust(g, case)
            BC.compare(again, e, "hostile, again")


def test_a_rejected_step_a_member_behind_and_cg_ending_early(g):
    e = _check(g, BC.behind_trial_case(), "behind a trial camera")
    assert e["res"]["trace"][0] == "kept" and "behind" in e["res"]["trace"]
    e = _check(g, BC.planted(60, 3, 3, cg_iters=40, num_loops=3)["case"], "cg ends early")
    assert 0 < max(h[3] for h in e["res"]["history"]) < 40
    e = _check(g, BC.rejected_then_kept_case(), "rejected then kept")
    assert e["res"]["trace"][2:4] == ["worse", "kept"]


def test_bad_offsets(g):
    """Offsets that are negative, decrease, overlap or pass O address nothing; the largest valid track owns a slot."""
    _check(g, BC.bundle_case(RC.bad_offsets_case(), hold=(1,)), "bad offsets")


def test_both_outputs_in_place(g):
    for case in (BC.planted(40, 4, 1, orthonormalise=1)["case"], BC.hostile_case(num_loops=3, cg_iters=5)):
        _check(g, case, "in place", in_place=True)


def test_one_context_after_a_refine_with_more_and_with_less_temp(g):
    """The temp of the context is shared: the call after a refine that left it larger (8 bytes x 100 000 slots against
    100 bytes x 119 slots), and in a fresh context after one that left it smaller."""
    case = BC.planted(40, 4, 1)["case"]
    small = RC.spread_case(257)
    big = RC.variant(small, max_obs=100000, obs=np.concatenate([small["obs"], np.zeros(100000 - 257, TC.OBS_DTYPE)]))

    def refine(ctx, rc):
        dev = {k: ctx.upload(v) for k, v in _inputs(rc).items()}
        ctx.refine_cameras_batch(rc["max_tracks"], rc["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                                 dev["points"], dev["point_status"], rc["nimages"], dev["cam"], dev["cam_pair"],
                                 rc["intrinsics"], hold=rc["hold"], min_obs=rc["min_obs"], num_loops=1,
                                 max_error=rc["max_error"], orthonormalise=0)

    refine(g, big)
    _check(g, case, "after a larger temp")
    with guarded_context(1) as fresh:
        refine(fresh, RC.spread_case(1))
        _check(fresh, case, "after a smaller temp")


def test_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = BC.planted(40, 4, 1)["case"]
    ins = _inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in BC.sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n, mt = case["nimages"], case["max_tracks"]
    hold = np.array([1], np.int32)
    good = dict(ctx=g.h, max_tracks=mt, max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, points=dev["points"].ptr,
                point_status=dev["point_status"].ptr, nimages=n, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr,
                intrinsics=K.ctypes.data, nhold=1, hold=hold.ctypes.data, min_views=2, min_obs=6, num_loops=5,
                cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0, **{k: outs[k].ptr for k in BC.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_adjust_bundle_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-7), dict(nimages=0),
           dict(nimages=-1), dict(min_views=1), dict(min_views=-2), dict(min_obs=2), dict(min_obs=0), dict(min_obs=-3),
           dict(num_loops=-1), dict(cg_iters=-1), dict(max_error=np.nan), dict(max_error=0.0), dict(max_error=-1.0),
           dict(max_error=-np.inf), dict(lambda0=0.0), dict(lambda0=-1e-3), dict(lambda0=np.nan), dict(lambda0=np.inf),
           dict(lambda0=-np.inf), dict(orthonormalise=2), dict(orthonormalise=-1), dict(nhold=-1), dict(nhold=2, hold=None),
           dict(obs=dev["obs"].ptr + 4), dict(obs=dev["obs"].ptr + 8),
           dict(cam_out=dev["cam"].ptr + 4), dict(cam_out=dev["cam"].ptr + 48 * n - 4), dict(cam_out=dev["cam"].ptr - 4),
           dict(points_out=dev["points"].ptr + 4), dict(points_out=dev["points"].ptr + 16 * mt - 4),
           dict(points_out=dev["points"].ptr - 4)]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "points", "point_status", "cam", "cam_pair",
                                "intrinsics") + BC.OUTPUTS]
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
    for k, m in BC.sizes(case).items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, dt in INPUTS:
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # the same arguments, unbroken; then without a history and without a loop
    assert call() == MISIFT_OK
    g.sync()
    BC.compare({k: g.download(outs[k], (m,), np.uint32) for k, m in BC.sizes(case).items()}, BC.expected_bundle(case),
               "unbroken")
    assert call(history=None, num_loops=0) == MISIFT_OK
    g.sync()


def test_export_triangulate_resect_triangulate_refine_adjust_triangulate(g):
    """The chain on the 8-camera scene of posegraph_cases with pair (4, 5) made unusable, so that link_poses leaves images
    5, 6 and 7 without a camera (test_gpu_resect.py holds the stages up to refine to their restatements): export ->
    triangulate -> resect(only_unset, install) -> triangulate -> refine -> adjust -> triangulate, nothing read in between.
    The adjustment and the triangulation behind it are byte-equal to their restatements fed the device's own buffers; the
    resected images are adjusted with the linked ones."""
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
    tri1 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    g.resect_cameras_batch(mt, mo, doff, dobs, dsum, tri1[0], tri1[2], nimg, K, images, seeds, max_cand=n, num_loops=256,
                           thresh=4.0, min_inliers=12, only_unset=1, install=1, cam=dcam, cam_pair=dcam_pair)
    tri2 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    ref = g.refine_cameras_batch(mt, mo, doff, dobs, dsum, tri2[0], tri2[2], nimg, dcam, dcam_pair, K, hold=hold,
                                 min_obs=6, num_loops=5, max_error=4.0, orthonormalise=1)
    args = dict(min_views=2, min_obs=6, num_loops=5, cg_iters=10, max_error=4.0, lambda0=1e-3, orthonormalise=0)
    sizes = BC.sizes(dict(nimages=nimg, max_tracks=mt, num_loops=5))
    outs = {k: _poisoned(g, m) for k, m in sizes.items()}
    g.adjust_bundle_batch(mt, mo, doff, dobs, dsum, tri2[0], tri2[2], nimg, ref[0], dcam_pair, K, hold=hold, **args,
                          **outs)
    tri3 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, outs["cam_out"], dcam_pair, K, min_views=2,
                                      num_loops=5)
    g.sync()
    pair = g.download(dcam_pair, (nimg,), np.int32)
    assert pair.tolist()[5:] == [-3] * 3
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=g.download(doff, (mt + 1,), np.int32),
                obs=g.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, intrinsics=K, cam_pair=pair)
    case = dict(base, cam=g.download(ref[0], (nimg, 12), f32), points=g.download(tri2[0], (mt, 4), f32),
                point_status=g.download(tri2[2], (mt,), np.int32), hold=tuple(hold), **args)
    e = BC.expected_bundle(case)
    BC.compare({k: g.download(outs[k], (m,), np.uint32) for k, m in sizes.items()}, e, "chain, adjust")
    s = _summary(e)
    assert e["cam_status"].view(np.int32).tolist() == [BC.HELD] * 2 + [BC.ADJUSTED] * 6 and s[6] >= 1 and s[4] >= 100
    tc = dict(base, cam=e["cam_out"].view(f32).reshape(-1, 12), min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        x = TC.expected_triangulate(tc)
    got3 = dict(points=g.download(tri3[0], (4 * mt,), np.uint32), point_views=g.download(tri3[1], (mt,), np.uint32),
                point_status=g.download(tri3[2], (mt,), np.uint32), obs_error=g.download(tri3[3], (mo,), np.uint32),
                summary=g.download(tri3[4], (8,), np.uint32))
    for k in got3:
        written = x[k] != POISON_WORD                            # what the call leaves alone was zeroed here, not poisoned
        assert (got3[k][written] == x[k][written]).all(), k
    cost = e["cost"].view(f32)
    print("chain: T %d summary %s cost %.6g -> %.6g, steps %s" % (s[0], s.tolist(), cost[0], cost[1], e["res"]["trace"]))
    assert cost[1] < cost[0]


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
