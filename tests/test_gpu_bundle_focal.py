"""misift_adjust_bundle_focal_batch on the device: cameras, track points and one focal scale per camera group adjusted
jointly.

Every comparison is byte equality with bundle_focal_cases.expected_focal (pinned in test_bundle_focal_cpu.py to the
library's host hook, to float64 and to dense linear algebra, where the premises of the cases are asserted too), or,
without a grouped image, with the restatement of the robust call and with the robust call itself on the device: all twelve
outputs at exactly their stated sizes, poisoned first, and every byte of the inputs, which the call must not write.  The
harness is that of test_gpu_bundle_robust.py.  The shapes are the smallest at which the new kernels can go wrong: no free
camera, one, 8, 65 and 257 images in one group (the cross-image rule wraps), 0 to 257 tracks (the cross-track rule of the
Schur scalar wraps), images of 255 to 513 members, a track of 301 views, tracks in two groups and in none, 1, 2 and 8
groups, groups without an image and without a member, T and O from the device below, beyond and under their capacities."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_focal_cases as BF
import bundle_robust_cases as BR
import filter_cases as FC
import posegraph_cases as G
import pose_cases as PC
import refine_cases as RC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_bundle_focal_cpu import CASE_NAMES
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
INPUTS = (("track_offsets", np.int32), ("obs", TC.OBS_DTYPE), ("export_summary", np.int32), ("points", f32),
          ("point_status", np.int32), ("cam", f32), ("cam_pair", np.int32))


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


@pytest.fixture(scope="module")
def cases():
    return BF.cpu_cases()


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _adjust(ctx, case, in_place=False, weights=True, robust=False):
    """The call (robust: misift_adjust_bundle_robust_batch on the same case) on poisoned outputs of exactly the stated
    sizes; returns them as uint32 arrays.  The inputs must come back as they went in (but for d_cam and d_points when they
    are the outputs)."""
    assert TC.POISON_WORD == POISON_WORD == BF.POISON_WORD
    ins = FC.inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in BF.sizes(case).items()}
    if in_place:
        outs["cam_out"], outs["points_out"] = dev["cam"], dev["points"]
    args = (case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
            dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"], case["intrinsics"])
    kw = dict(hold=case["hold"], min_views=case["min_views"], min_obs=case["min_obs"], num_loops=case["num_loops"],
              cg_iters=case["cg_iters"], max_error=case["max_error"], lambda0=case["lambda0"],
              orthonormalise=case["orthonormalise"], loss=case["loss"], loss_scale=case["loss_scale"],
              obs_weight=outs["obs_weight"] if weights else None, **{k: outs[k] for k in BC.OUTPUTS})
    if robust:
        ctx.adjust_bundle_robust_batch(*args, **kw)
    else:
        ctx.adjust_bundle_focal_batch(*args, case["group"], ngroups=case["ngroups"], intrinsics_out=outs["intrinsics_out"],
                                      focal=outs["focal"], **kw)
    ctx.sync()
    for k, dt in INPUTS:
        if not (in_place and k in ("cam", "points")):
            assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (n,), np.uint32) for k, n in BF.sizes(case).items()}


def _check(ctx, case, what, in_place=False, weights=True):
    e = BF.expected_focal(case)
    keys = [k for k in BF.OUTPUTS if weights or k != "obs_weight"]
    BF.compare_all(_adjust(ctx, case, in_place, weights), BR.in_place(e, case) if in_place else e, what, keys)
    return e


def _focal(e):
    """(scales, members, statuses) of the expected d_focal."""
    w = e["focal"][:3 * (len(e["focal"]) // 3)].reshape(-1, 3)
    return w[:, 0].copy().view(f32), w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case(g, cases, name):
    """The cases of bundle_focal_cases.cpu_cases (what each is built to hit is asserted in test_bundle_focal_cpu.py): two
    images with no free camera, three, eight; 1, 2 and 8 groups; groups without an image and without a member; some
    images and all images without a group, ngroups 0; tracks in two groups and in none; the 301-view track; images of 255
    to 513 members; the hostile scene; no loop, cg_iters 0 and 1, a lambda0 that fails every step; steps turned away for
    a member behind, for a worse cost and for a trial scale that is not > 0; the three losses."""
    _check(g, cases[name], name)


@pytest.mark.parametrize("shape", BF.IMAGE_SHAPES, ids=lambda a: "%d" % a[0])
def test_image_counts(g, shape):
    e = _check(g, BF.image_count_case(*shape), "%d images" % shape[0])
    s, (scale, members, status) = e["summary"].view(np.int32), _focal(e)
    assert s[5] == 2 and s[1] + s[3] == shape[0] - 2 and s[6] >= 1
    assert members[0] == s[2] and status[0] == BF.REFINED and scale[0] != 1.0


@pytest.mark.parametrize("ntracks", BF.TRACK_COUNTS)
def test_track_counts(g, ntracks):
    e = _check(g, BF.track_count_case(ntracks), "%d tracks" % ntracks)
    assert e["summary"].view(np.int32)[0] == ntracks == e["summary"].view(np.int32)[4]
    assert _focal(e)[2][0] == (BF.REFINED if ntracks else BF.NO_MEMBER)


@pytest.mark.parametrize("T,O", BF.DEVICE_COUNTS)
def test_counts_from_the_device(g, T, O):
    _check(g, BF.device_counts_case(T, O), "T %d O %d" % (T, O))


@pytest.mark.parametrize("loss,scale", BF.LOSSES, ids=("none", "huber", "geman-mcclure"))
@pytest.mark.parametrize("num_loops,cg_iters", ((0, 10), (1, 0), (1, 1), (5, 10)))
def test_loops_iterations_and_losses(g, num_loops, cg_iters, loss, scale):
    base = BC.planted(40, 4, 1, num_loops=num_loops, cg_iters=cg_iters)["case"]
    e = _check(g, BF.alternating(base, (0.95, 1.05), loss=loss, loss_scale=scale), "loops %d cg %d" % (num_loops, cg_iters))
    if num_loops == 0:
        assert e["intrinsics_out"].tobytes() == np.ascontiguousarray(e["res"]["problem"].K, f32).tobytes()
        assert (_focal(e)[0] == 1.0).all() and (_focal(e)[2] == BF.NOT_REFINED).all()


def test_without_a_grouped_image_it_is_the_robust_call(g):
    """The first identity on the device: all images -1, and ngroups 0, against the robust call itself and (loss 0) the
    restatement of the plain call, byte for byte; d_intrinsics_out is the input bit for bit."""
    for loss, c in BF.LOSSES:
        for name, base in (("4 images", BC.planted(40, 4, 1)["case"]), ("hostile", BC.hostile_case(num_loops=3, cg_iters=5))):
            for group, G in (([-1] * base["nimages"], 2), ([], 0)):
                case = BF.focal(base, group, G, loss=loss, loss_scale=c)
                got, rob = _adjust(g, case), _adjust(g, case, robust=True)
                for k in BR.OUTPUTS:
                    assert got[k].tobytes() == rob[k].tobytes(), (name, G, loss, k)
                assert got["intrinsics_out"].tobytes() == np.ascontiguousarray(case["intrinsics"], f32).tobytes()
                BF.compare_all(got, BF.expected_focal(case), name)
                if loss == BF.NONE:
                    BR.compare_all(got, BR.expected_plain_with_weights(base), name + ", the plain restatement", BR.OUTPUTS)


def test_outputs_in_place_without_weights_and_twice(g, cases):
    for name in ("two groups", "hostile"):
        _check(g, cases[name], name + ", in place", in_place=True)
        _check(g, cases[name], name + ", no d_obs_weight", weights=False)
        first, again = _adjust(g, cases[name]), _adjust(g, cases[name])
        for k in BF.OUTPUTS:
            assert first[k].tobytes() == again[k].tobytes(), (name, k)


def test_one_context_after_a_refine_with_more_and_with_less_temp(g):
    case = BF.two_group_track_case()
    small = RC.spread_case(257)
    big = RC.variant(small, max_obs=100000, obs=np.concatenate([small["obs"], np.zeros(100000 - 257, TC.OBS_DTYPE)]))

    def refine(ctx, rc):
        dev = {k: ctx.upload(v) for k, v in FC.inputs(rc).items()}
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
    case = BF.two_group_track_case()
    ins = FC.inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in BF.sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n, mt = case["nimages"], case["max_tracks"]
    hold, group = np.array([1], np.int32), np.ascontiguousarray(case["group"], np.int32)
    good = dict(ctx=g.h, max_tracks=mt, max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, points=dev["points"].ptr,
                point_status=dev["point_status"].ptr, nimages=n, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr,
                intrinsics=K.ctypes.data, nhold=1, hold=hold.ctypes.data, min_views=2, min_obs=6, num_loops=5,
                cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0, loss=BF.HUBER, loss_scale=2.0, ngroups=2,
                group=group.ctypes.data, **{k: outs[k].ptr for k in BF.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_adjust_bundle_focal_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_obs=0), dict(nimages=0), dict(min_views=1), dict(min_obs=2),
           dict(num_loops=-1), dict(cg_iters=-1), dict(max_error=np.nan), dict(max_error=0.0), dict(lambda0=0.0),
           dict(lambda0=np.nan), dict(lambda0=np.inf), dict(orthonormalise=2), dict(nhold=-1), dict(nhold=2, hold=None),
           dict(obs=dev["obs"].ptr + 4), dict(cam_out=dev["cam"].ptr + 4), dict(points_out=dev["points"].ptr + 4),
           dict(loss=3), dict(loss=-1), dict(loss_scale=0.0), dict(loss_scale=np.nan), dict(loss_scale=np.inf),
           dict(ngroups=-1), dict(ngroups=BF.MAX_GROUPS + 1), dict(group=None), dict(ngroups=1), dict(focal=None),
           dict(intrinsics_out=None), dict(intrinsics_out=None, ngroups=0, group=None)]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "points", "point_status", "cam", "cam_pair",
                                "intrinsics") + BC.OUTPUTS]
    lists = []                                                   # kept alive until the calls are made
    for h in ([-1, 1], [1, n]):
        lists.append(np.array(h, np.int32))
        bad.append(dict(nhold=2, hold=lists[-1].ctypes.data))
    for at, v in ((0, -2), (n - 1, 2), (1, 2 ** 31 - 1), (2, -2 ** 31)):
        lists.append(group.copy())
        lists[-1][at] = v
        bad.append(dict(group=lists[-1].ctypes.data))
    for at, v in ((0, 0.0), (1, np.nan), (4 * n - 3, np.inf), (2, np.nan), (4 * n - 1, np.inf)):
        lists.append(K.copy())
        lists[-1].reshape(-1)[at] = v
        bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in BF.sizes(case).items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, dt in INPUTS:
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # the same arguments, unbroken; then without the optional ones
    assert call() == MISIFT_OK
    g.sync()
    BF.compare_all({k: g.download(outs[k], (m,), np.uint32) for k, m in BF.sizes(case).items()},
                   BF.expected_focal(dict(case, loss=BF.HUBER, loss_scale=2.0)), "unbroken")
    assert call(history=None, num_loops=0, obs_weight=None) == MISIFT_OK
    assert call(ngroups=0, group=None, focal=None) == MISIFT_OK
    g.sync()


def test_export_triangulate_focal_adjust_then_triangulate_and_filter_under_the_refined_intrinsics(g):
    """The chain on the 8-camera scene of posegraph_cases, as test_gpu_bundle.py runs it: find -> improve -> recover_pose
    -> link_poses and link_tracks -> export -> triangulate -> focal adjust, the track chain given fx, fy 10 % long for the
    one camera that took all images, nothing read in between; then d_intrinsics_out read back (16 * nimages bytes) and
    triangulate and filter under it.  Every step from the adjustment on is byte-equal to its restatement fed the device's
    own buffers (test_gpu_resect.py holds the stages before it to theirs)."""
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
    fscale = 1.1
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    K[:, :2] *= f32(fscale)                                      # what the track chain is told: 10 % long
    hold = [i for i in pc["pairs"][pc["seed_pair"]] if i != pc["root_image"]]
    scene = (mt, mo, doff, dobs, dsum)
    tri1 = g.triangulate_tracks_batch(*scene, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    args = dict(min_views=2, min_obs=6, num_loops=5, cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0,
                loss=BF.HUBER, loss_scale=2.0)
    group = np.zeros(nimg, np.int32)
    sizes = BF.sizes(dict(nimages=nimg, max_tracks=mt, max_obs=mo, num_loops=5, ngroups=1))
    outs = {k: _poisoned(g, m) for k, m in sizes.items()}
    g.adjust_bundle_focal_batch(*scene, tri1[0], tri1[2], nimg, dcam, dcam_pair, K, group, ngroups=1, hold=hold, **args,
                                **outs)
    g.sync()
    K2 = g.download(outs["intrinsics_out"], (nimg, 4), f32)      # the one read: the other calls take host intrinsics
    tri2 = g.triangulate_tracks_batch(*scene, nimg, outs["cam_out"], dcam_pair, K2, min_views=2, num_loops=5)
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=g.download(doff, (mt + 1,), np.int32),
                obs=g.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, cam_pair=g.download(dcam_pair, (nimg,), np.int32))
    fsz = FC.sizes(base)
    fouts = {k: _poisoned(g, m) for k, m in fsz.items()}
    g.filter_tracks_batch(*scene, tri2[0], tri2[2], nimg, outs["cam_out"], dcam_pair, K2, max_error=3.0, max_cos=np.inf,
                          min_views=2, unique_frames=1, **fouts)
    g.sync()
    case = BF.focal(dict(base, intrinsics=K, cam=g.download(dcam, (nimg, 12), f32),
                         points=g.download(tri1[0], (mt, 4), f32), point_status=g.download(tri1[2], (mt,), np.int32),
                         hold=tuple(hold), **args), group, 1)
    e = BF.expected_focal(case)
    BF.compare_all({k: g.download(outs[k], (m,), np.uint32) for k, m in sizes.items()}, e, "chain, adjust")
    assert K2.view(np.uint32).reshape(-1).tolist() == e["intrinsics_out"].tolist()
    (scale, members, status), cost, s = _focal(e), e["cost"].view(f32), e["summary"].view(np.int32)
    print("chain: summary %s cost %.6g -> %.6g, steps %s, scale %.6f (planted %.6f)" % (
        s.tolist(), cost[0], cost[1], e["res"]["trace"], scale[0], 1 / fscale))
    assert status[0] == BF.REFINED and members[0] == s[2] and s[4] >= 100 and cost[1] < cost[0]
    assert abs(scale[0] * fscale - 1) < abs(fscale - 1)          # closer to the planted focal than it was given
    tc = dict(base, intrinsics=K2, cam=e["cam_out"].view(f32).reshape(-1, 12), min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        x = TC.expected_triangulate(tc)
    got = dict(points=g.download(tri2[0], (4 * mt,), np.uint32), point_views=g.download(tri2[1], (mt,), np.uint32),
               point_status=g.download(tri2[2], (mt,), np.uint32), obs_error=g.download(tri2[3], (mo,), np.uint32),
               summary=g.download(tri2[4], (8,), np.uint32))
    for k in got:
        written = x[k] != POISON_WORD                            # what the call leaves alone was zeroed here, not poisoned
        assert (got[k][written] == x[k][written]).all(), k
    fcase = FC.filter_case(dict(tc, points=got["points"].view(f32).reshape(-1, 4),
                                point_status=got["point_status"].view(np.int32)), max_error=3.0)
    FC.compare({k: g.download(fouts[k], (m,), np.uint32) for k, m in fsz.items()}, FC.expected_filter(fcase),
               "chain, filter")


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
