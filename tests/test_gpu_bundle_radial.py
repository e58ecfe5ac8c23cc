"""misift_adjust_bundle_radial_batch and misift_undistort_obs_batch on the device: cameras, track points, one focal scale
and one radial coefficient per camera group adjusted jointly, and the observation list undistorted under the result.

Every comparison is byte equality with bundle_radial_cases.expected_radial / expected_undistort (pinned in
test_bundle_radial_cpu.py to the library's host hooks, to float64 and to dense linear algebra, where the premises of the
cases are asserted too), or, with nothing radial, with misift_adjust_bundle_focal_batch itself on the device: all
thirteen outputs at exactly their stated sizes, poisoned first, and every byte of the inputs, which the call must not
write.  The harness is that of test_gpu_bundle_focal.py.  The shapes are the smallest at which the new kernels can go
wrong: no free camera, one, 8, 65 and 257 images in one group (the cross-image rule wraps), 0 to 257 tracks (the
cross-track rule of S_kk wraps), images of 255 to 513 members, a track of 301 views, tracks in two groups and in none, 1, 2
and 8 groups with radial mixed 0 / 1, a held coefficient that is not zero, groups without an image and without a member,
hostile observations, T and O from the device below, beyond and under their capacities."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_focal_cases as BF
import bundle_radial_cases as BD
import bundle_robust_cases as BR
import filter_cases as FC
import posegraph_cases as G
import pose_cases as PC
import refine_cases as RC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_bundle_radial_cpu import CASE_NAMES, UNDISTORT_COUNTS, _words
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
    return BD.cpu_cases()


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _adjust(ctx, case, in_place=False, weights=True, focal=False):
    """The call (focal: misift_adjust_bundle_focal_batch on the same case) on poisoned outputs of exactly the stated
    sizes; returns them as uint32 arrays.  The inputs must come back as they went in (but for d_cam and d_points when they
    are the outputs)."""
    assert TC.POISON_WORD == POISON_WORD == BD.POISON_WORD
    ins = FC.inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    sizes = BF.sizes(case) if focal else BD.sizes(case)
    outs = {k: _poisoned(ctx, n) for k, n in sizes.items()}
    if in_place:
        outs["cam_out"], outs["points_out"] = dev["cam"], dev["points"]
    args = (case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
            dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"], case["intrinsics"], case["group"])
    kw = dict(ngroups=case["ngroups"], hold=case["hold"], min_views=case["min_views"], min_obs=case["min_obs"],
              num_loops=case["num_loops"], cg_iters=case["cg_iters"], max_error=case["max_error"], lambda0=case["lambda0"],
              orthonormalise=case["orthonormalise"], loss=case["loss"], loss_scale=case["loss_scale"],
              obs_weight=outs["obs_weight"] if weights else None, intrinsics_out=outs["intrinsics_out"],
              focal=outs["focal"], **{k: outs[k] for k in BC.OUTPUTS})
    if focal:
        ctx.adjust_bundle_focal_batch(*args, **kw)
    else:
        ctx.adjust_bundle_radial_batch(*args, radial=case.get("radial"), k0=case.get("k0"), radial_out=outs["radial_out"],
                                       **kw)
    ctx.sync()
    for k, dt in INPUTS:
        if not (in_place and k in ("cam", "points")):
            assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (n,), np.uint32) for k, n in sizes.items()}


def _check(ctx, case, what, in_place=False, weights=True):
    e = BD.expected_radial(case)
    keys = [k for k in BD.OUTPUTS if weights or k != "obs_weight"]
    BD.compare_all(_adjust(ctx, case, in_place, weights), BR.in_place(e, case) if in_place else e, what, keys)
    return e


def _radial(e):
    """(coefficients, members, statuses) of the expected d_radial."""
    w = e["radial_out"][:3 * (len(e["radial_out"]) // 3)].reshape(-1, 3)
    return w[:, 0].copy().view(f32), w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case(g, cases, name):
    """The cases of bundle_radial_cases.cpu_cases (what each is built to hit is asserted in test_bundle_radial_cpu.py):
    two images with no free camera, three, eight; 1, 2, 4 and 8 groups with radial mixed 0 / 1; a held coefficient that is
    not zero; groups without an image and without a member; some and all images without a group, ngroups 0; tracks in
    two groups and in none; the 301-view track; images of 255 to 513 members; the hostile scene and the hostile
    observations (at the principal point, at 1e20, at 3e38, NaN); no loop, cg_iters 0 and 1, a lambda0 that fails every step;
    steps turned away for a member behind a trial camera ("behind, rejected then kept": kept, three times behind, kept)
    and for a worse cost ("empty groups"), and kept after; steps turned away because the trial coefficient overflows
    while the trial scale stays positive, and kept after ("k not finite"); the three losses."""
    _check(g, cases[name], name)


@pytest.mark.parametrize("shape", BD.IMAGE_SHAPES, ids=lambda a: "%d" % a[0])
def test_image_counts(g, shape):
    e = _check(g, BD.image_count_case(*shape), "%d images" % shape[0])
    s, (k, members, status) = e["summary"].view(np.int32), _radial(e)
    assert s[5] == 2 and s[1] + s[3] == shape[0] - 2 and s[6] >= 1
    assert members[0] == s[2] and status[0] == BD.REFINED and k[0] != 0.0


@pytest.mark.parametrize("ntracks", BD.TRACK_COUNTS)
def test_track_counts(g, ntracks):
    e = _check(g, BD.track_count_case(ntracks), "%d tracks" % ntracks)
    assert e["summary"].view(np.int32)[0] == ntracks
    assert _radial(e)[2][0] == (BD.REFINED if ntracks else BD.NO_MEMBER)


@pytest.mark.parametrize("T,O", BD.DEVICE_COUNTS)
def test_counts_from_the_device(g, T, O):
    _check(g, BD.device_counts_case(T, O), "T %d O %d" % (T, O))


@pytest.mark.parametrize("loss,scale", BD.LOSSES, ids=("none", "huber", "geman-mcclure"))
@pytest.mark.parametrize("num_loops,cg_iters", ((0, 10), (1, 0), (1, 1), (5, 10)))
def test_loops_iterations_and_losses(g, num_loops, cg_iters, loss, scale):
    base = BC.planted(40, 4, 1, num_loops=num_loops, cg_iters=cg_iters)["case"]
    e = _check(g, BD.alternating(base, loss=loss, loss_scale=scale), "loops %d cg %d" % (num_loops, cg_iters))
    if num_loops == 0:
        assert (_radial(e)[0] == 0.0).all() and (_radial(e)[2] == BD.NOT_REFINED).all()


@pytest.mark.parametrize("name", ("ngroups 0", "all -1", "nothing radial", "no lists"))
def test_with_nothing_radial_it_is_the_focal_call(g, cases, name):
    """The identity on the device, against misift_adjust_bundle_focal_batch itself: the twelve shared outputs byte for
    byte."""
    for case in (cases[name], dict(cases[name], loss=BD.HUBER, loss_scale=2.0)):
        got, foc = _adjust(g, case), _adjust(g, case, focal=True)
        for k in BF.OUTPUTS:
            assert got[k].tobytes() == foc[k].tobytes(), (name, k)
        BD.compare_all(got, BD.expected_radial(case), name)


def test_outputs_in_place_without_weights_and_twice(g, cases):
    for name in ("two groups", "hostile"):
        _check(g, cases[name], name + ", in place", in_place=True)
        _check(g, cases[name], name + ", no d_obs_weight", weights=False)
        first, again = _adjust(g, cases[name]), _adjust(g, cases[name])
        for k in BD.OUTPUTS:
            assert first[k].tobytes() == again[k].tobytes(), (name, k)


def test_one_context_after_a_refine_with_more_and_with_less_temp(g, cases):
    case = cases["two groups"]
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


def test_argument_errors_enqueue_nothing(g, cases):
    from cudasift_amd import capi
    L = capi.lib()
    case = cases["two groups"]
    ins = FC.inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in BD.sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n, mt = case["nimages"], case["max_tracks"]
    hold = np.array([1], np.int32)
    group, flags, k0 = BD.host_lists(case)
    good = dict(ctx=g.h, max_tracks=mt, max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, points=dev["points"].ptr,
                point_status=dev["point_status"].ptr, nimages=n, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr,
                intrinsics=K.ctypes.data, nhold=1, hold=hold.ctypes.data, min_views=2, min_obs=6, num_loops=5,
                cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0, loss=BD.HUBER, loss_scale=2.0, ngroups=2,
                group=group.ctypes.data, radial=flags.ctypes.data, k0=k0.ctypes.data,
                **{k: outs[k].ptr for k in BD.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_adjust_bundle_radial_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_obs=0), dict(nimages=0), dict(min_views=1), dict(min_obs=2),
           dict(num_loops=-1), dict(cg_iters=-1), dict(max_error=np.nan), dict(max_error=0.0), dict(lambda0=0.0),
           dict(lambda0=np.nan), dict(lambda0=np.inf), dict(orthonormalise=2), dict(nhold=-1), dict(nhold=2, hold=None),
           dict(obs=dev["obs"].ptr + 4), dict(cam_out=dev["cam"].ptr + 4), dict(points_out=dev["points"].ptr + 4),
           dict(loss=3), dict(loss=-1), dict(loss_scale=0.0), dict(loss_scale=np.nan), dict(loss_scale=np.inf),
           dict(ngroups=-1), dict(ngroups=BD.MAX_GROUPS + 1), dict(group=None), dict(ngroups=1), dict(focal=None),
           dict(intrinsics_out=None), dict(intrinsics_out=None, ngroups=0, group=None), dict(radial=None), dict(k0=None),
           dict(radial_out=None)]
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
    for fl in ([2, 1], [1, -1], [2 ** 31 - 1, 0]):
        lists.append(np.array(fl, np.int32))
        bad.append(dict(radial=lists[-1].ctypes.data))
    for kk in ([np.nan, 0.0], [0.0, np.inf], [-np.inf, 0.0]):
        lists.append(np.array(kk, f32))
        bad.append(dict(k0=lists[-1].ctypes.data))
    for at, v in ((0, 0.0), (1, np.nan), (4 * n - 3, np.inf), (2, np.nan), (4 * n - 1, np.inf)):
        lists.append(K.copy())
        lists[-1].reshape(-1)[at] = v
        bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in BD.sizes(case).items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, dt in INPUTS:
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # the same arguments, unbroken; then without the optional ones
    assert call() == MISIFT_OK
    g.sync()
    BD.compare_all({k: g.download(outs[k], (m,), np.uint32) for k, m in BD.sizes(case).items()},
                   BD.expected_radial(dict(case, loss=BD.HUBER, loss_scale=2.0)), "unbroken")
    assert call(history=None, num_loops=0, obs_weight=None) == MISIFT_OK
    assert call(radial=None, k0=None) == MISIFT_OK
    assert call(ngroups=0, group=None, focal=None, radial=None, k0=None, radial_out=None) == MISIFT_OK
    g.sync()


# ---- misift_undistort_obs_batch

def _undistort(ctx, case, words, in_place=False):
    src = np.ascontiguousarray(case["obs"][:case["max_obs"]])
    d_obs, d_sum = ctx.upload(src), ctx.upload(np.ascontiguousarray(case["export_summary"], np.int32))
    d_words = ctx.upload(np.ascontiguousarray(words, np.uint32))
    d_out = d_obs if in_place else _poisoned(ctx, 4 * len(src))
    ctx.undistort_obs_batch(case["max_obs"], d_obs, d_sum, case["nimages"], case["intrinsics"], case["group"], d_words,
                            ngroups=case["ngroups"], obs_out=d_out)
    ctx.sync()
    if not in_place:
        assert ctx.download(d_obs, src.shape, TC.OBS_DTYPE).tobytes() == src.tobytes(), "d_obs was written"
    assert ctx.download(d_words, (len(words),), np.uint32).tobytes() == np.ascontiguousarray(words, np.uint32).tobytes()
    return ctx.download(d_out, src.shape, TC.OBS_DTYPE)


@pytest.mark.parametrize("O", UNDISTORT_COUNTS)
def test_undistort_obs(g, O):
    """O of 0, 1, 63, 64, 65 and 257, beyond max_obs and negative; frames -1 and nimages; an image in no group; a NaN; both
    out of place (slots from O on stay poisoned) and in place."""
    case = BD.undistort_case(O)
    words = _words([0.07, -0.11, 0.0], BD.HELD)
    for in_place in (False, True):
        got = _undistort(g, case, words, in_place)
        assert got.tobytes() == BD.expected_undistort(case, case["obs"], words, in_place).tobytes(), (O, in_place)


def test_undistort_obs_argument_errors(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = BD.undistort_case(257)
    src = np.ascontiguousarray(case["obs"][:case["max_obs"]])
    d_obs, d_sum = g.upload(src), g.upload(np.ascontiguousarray(case["export_summary"], np.int32))
    d_words, d_out = g.upload(_words([0.07, -0.11, 0.0])), _poisoned(g, 4 * len(src) + 8)
    K = np.ascontiguousarray(case["intrinsics"], f32)
    group = np.ascontiguousarray(case["group"], np.int32)
    n = case["nimages"]
    good = dict(ctx=g.h, max_obs=case["max_obs"], obs=d_obs.ptr, export_summary=d_sum.ptr, nimages=n,
                intrinsics=K.ctypes.data, ngroups=3, group=group.ctypes.data, radial=d_words.ptr, obs_out=d_out.ptr)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_undistort_obs_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_obs=0), dict(nimages=0), dict(obs=None), dict(export_summary=None),
           dict(intrinsics=None), dict(obs_out=None), dict(group=None), dict(radial=None), dict(ngroups=-1),
           dict(ngroups=BD.MAX_GROUPS + 1), dict(ngroups=2), dict(obs=d_obs.ptr + 4), dict(obs_out=d_out.ptr + 4),
           dict(obs_out=d_obs.ptr + 16), dict(obs=d_out.ptr + 32)]
    lists = []
    for at, v in ((0, -2), (n - 1, 3)):
        lists.append(group.copy())
        lists[-1][at] = v
        bad.append(dict(group=lists[-1].ctypes.data))
    for at, v in ((0, 0.0), (1, np.nan), (2, np.inf)):
        lists.append(K.copy())
        lists[-1].reshape(-1)[at] = v
        bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    assert (g.download(d_out, (4 * len(src) + 8,), np.uint32) == POISON_WORD).all()
    assert call() == MISIFT_OK and call(ngroups=0, group=None, radial=None) == MISIFT_OK
    g.sync()


def test_export_triangulate_refine_radial_adjust_undistort_then_triangulate_and_adjust(g):
    """The chain on the 8-camera scene of posegraph_cases with a planted lens: find -> improve -> recover_pose ->
    link_poses and link_tracks on the records as matched, export of the records as the lens shows them (every position
    displaced so that the model with the planted coefficient undoes it) -> triangulate -> refine -> radial adjust ->
    undistort_obs -> triangulate -> adjust on the undistorted list under d_intrinsics_out; only d_intrinsics_out is read
    in between.  Every step from the first triangulation on is byte-equal to its restatement fed the device's own
    buffers; the export is held to its restatement in its own file."""
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
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    kplant = BD.corner_k(dict(intrinsics=K), -0.04)
    lens = np.zeros(total, TC.OBS_DTYPE)                          # the records' positions as the lens shows them
    lens["xpos"], lens["ypos"] = recs["xpos"], recs["ypos"]
    lens["frame"] = np.repeat(np.arange(nimg), n)
    lens = BD.distort_obs(dict(obs=lens, nimages=nimg, intrinsics=K, group=np.zeros(nimg, np.int32)), [kplant])["obs"]
    shown = recs.copy()
    shown["xpos"], shown["ypos"] = lens["xpos"], lens["ypos"]
    d_recs, d_cnt = g.upload(recs), g.upload(np.full(nimg, n, np.int32))
    lab = g.link_tracks_batch(pc["pairs"], d, dc, n, nimg, d_cnt, None, n, max_records=total, min_score=GATES[0],
                              max_ambiguity=GATES[1], max_error=pc["max_error"])
    mt, mo = total // 3 + 1, total
    doff, _, dobs, _, dsum = g.export_tracks_batch(g.upload(shown), nimg, d_cnt, None, n, max_records=total, track=lab[0],
                                                   track_len=lab[1], track_frames=lab[2], min_len=3, consistent_only=1,
                                                   max_tracks=mt, max_obs=mo, record_obs=None)
    hold = [i for i in pc["pairs"][pc["seed_pair"]] if i != pc["root_image"]]
    scene = (mt, mo, doff, dobs, dsum)
    tri1 = g.triangulate_tracks_batch(*scene, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    rsz = dict(cam_out=12 * nimg, cam_obs=nimg, cam_rms=2 * nimg, cam_steps=nimg, cam_status=nimg, summary=8)
    routs = {k: _poisoned(g, m) for k, m in rsz.items()}
    g.refine_cameras_batch(*scene, tri1[0], tri1[2], nimg, dcam, dcam_pair, K, hold=hold, min_obs=6, num_loops=3,
                           max_error=np.inf, orthonormalise=0, **routs)
    args = dict(min_views=2, min_obs=6, num_loops=8, cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0,
                loss=BD.HUBER, loss_scale=2.0)
    group = np.zeros(nimg, np.int32)
    sizes = BD.sizes(dict(nimages=nimg, max_tracks=mt, max_obs=mo, num_loops=8, ngroups=1))
    outs = {k: _poisoned(g, m) for k, m in sizes.items()}
    g.adjust_bundle_radial_batch(*scene, tri1[0], tri1[2], nimg, routs["cam_out"], dcam_pair, K, group, ngroups=1,
                                 radial=[1], k0=[0.0], hold=hold, **args, **outs)
    dobs2 = g.undistort_obs_batch(mo, dobs, dsum, nimg, K, group, outs["radial_out"], ngroups=1,
                                  obs_out=_poisoned(g, 4 * mo))
    g.sync()
    K2 = g.download(outs["intrinsics_out"], (nimg, 4), f32)      # the one read: the other calls take host intrinsics
    scene2 = (mt, mo, doff, dobs2, dsum)
    tri2 = g.triangulate_tracks_batch(*scene2, nimg, outs["cam_out"], dcam_pair, K2, min_views=2, num_loops=5)
    psz = BC.sizes(dict(nimages=nimg, max_tracks=mt, num_loops=2))
    pouts = {k: _poisoned(g, m) for k, m in psz.items()}
    g.adjust_bundle_batch(*scene2, tri2[0], tri2[2], nimg, outs["cam_out"], dcam_pair, K2, hold=hold, min_views=2,
                          min_obs=6, num_loops=2, cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0, **pouts)
    g.sync()
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=g.download(doff, (mt + 1,), np.int32),
                obs=g.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, cam_pair=g.download(dcam_pair, (nimg,), np.int32))
    pts1, st1 = g.download(tri1[0], (mt, 4), f32), g.download(tri1[2], (mt,), np.int32)

    def triangulated(tri, tcase, what):
        with np.errstate(all="ignore"):
            x = TC.expected_triangulate(tcase)
        got = dict(points=g.download(tri[0], (4 * mt,), np.uint32), point_views=g.download(tri[1], (mt,), np.uint32),
                   point_status=g.download(tri[2], (mt,), np.uint32), obs_error=g.download(tri[3], (mo,), np.uint32),
                   summary=g.download(tri[4], (8,), np.uint32))
        for kk in got:
            written = x[kk] != POISON_WORD                       # what the call leaves alone was zeroed here, not poisoned
            assert (got[kk][written] == x[kk][written]).all(), (what, kk)
        return got

    # the first triangulation, on the list as the lens shows it (test_gpu_tracks_export.py holds the export before it)
    triangulated(tri1, dict(base, intrinsics=K, cam=g.download(dcam, (nimg, 12), f32), min_views=2, num_loops=5, memo={}),
                 "chain, triangulate")
    # refine
    rcase = dict(base, intrinsics=K, cam=g.download(dcam, (nimg, 12), f32), points=pts1, point_status=st1,
                 hold=tuple(hold), min_obs=6, num_loops=3, max_error=np.inf, orthonormalise=0)
    er = RC.expected_refine(rcase)
    for k, m in rsz.items():
        assert g.download(routs[k], (m,), np.uint32).tolist() == er[k].reshape(-1).tolist(), ("chain, refine", k)
    # the radial adjustment
    case = BD.radial(BF.focal(dict(base, intrinsics=K, cam=er["cam_out"].view(f32).reshape(-1, 12), points=pts1,
                                   point_status=st1, hold=tuple(hold), **args), group, 1), [1], [0.0])
    e = BD.expected_radial(case)
    BD.compare_all({k: g.download(outs[k], (m,), np.uint32) for k, m in sizes.items()}, e, "chain, adjust")
    (k, members, status), cost, s = _radial(e), e["cost"].view(f32), e["summary"].view(np.int32)
    print("chain: summary %s cost %.6g -> %.6g, steps %s, k %.6f (planted %.6f), scale %.6f" % (
        s.tolist(), cost[0], cost[1], e["res"]["trace"], k[0], kplant, e["res"]["scale"][0]))
    assert status[0] == BD.REFINED and members[0] == s[2] and s[4] >= 100 and cost[1] < cost[0]
    # how close k comes to the planted lens is held in test_bundle_radial_cpu.py; from this chain's rough start eight
    # steps only have to find its sign
    assert k[0] < 0 and kplant < 0
    # undistort
    got2 = g.download(dobs2, (mo,), TC.OBS_DTYPE)
    assert got2.tobytes() == BD.expected_undistort(case, base["obs"], e["radial_out"]).tobytes()
    # triangulate and the plain adjustment on the undistorted list
    base2 = dict(base, obs=got2)
    tc = dict(base2, intrinsics=K2, cam=e["cam_out"].view(f32).reshape(-1, 12), min_views=2, num_loops=5, memo={})
    got = triangulated(tri2, tc, "chain, triangulate on the undistorted list")
    pcase = dict(base2, intrinsics=K2, cam=tc["cam"], points=got["points"].view(f32).reshape(-1, 4),
                 point_status=got["point_status"].view(np.int32), hold=tuple(hold), min_views=2, min_obs=6, num_loops=2,
                 cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0)
    BC.compare({kk: g.download(pouts[kk], (m,), np.uint32) for kk, m in psz.items()}, BC.expected_bundle(pcase),
               "chain, plain adjust")


PROFILE_ENTRIES = ("bundle_setup", "bundle_track", "bundle_image", "bundle_scalar", "bundle_trial", "bundle_out")


@pytest.mark.parametrize("loss,scale", BD.LOSSES[:2], ids=("none", "huber"))
@pytest.mark.parametrize("model", ("plain", "focal", "radial"))
def test_profile_entries_and_calls(g, model, loss, scale):
    """The launch structure tools/bundle_time.py reads: with the profile on, a call reports exactly six entries, setup
    and out once, the per-track, per-image and scalar launches num_loops * (2 + cg_iters) times each, the trial state
    num_loops times; the same for the plain call, the focal call with every image in one group and the radial call with
    that group's coefficient an unknown.  Without a loop only setup and out appear."""
    assert loss in (BD.NONE, BD.HUBER)
    for num_loops, cg_iters in ((2, 3), (0, 3)):
        base = BC.planted(40, 4, 1, num_loops=num_loops, cg_iters=cg_iters)["case"]
        case = {"plain": lambda: BF.focal(base, np.full(base["nimages"], -1), 0, loss=loss, loss_scale=scale),
                "focal": lambda: BF.one_group(base, loss=loss, loss_scale=scale),
                "radial": lambda: BD.one_group(base, loss=loss, loss_scale=scale)}[model]()
        dev = {k: g.upload(v) for k, v in FC.inputs(case).items()}
        args = (case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                dev["points"], dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"], case["intrinsics"])
        kw = dict(hold=case["hold"], min_views=case["min_views"], min_obs=case["min_obs"], num_loops=num_loops,
                  cg_iters=cg_iters, max_error=case["max_error"], lambda0=case["lambda0"],
                  orthonormalise=case["orthonormalise"])
        lossy = dict(loss=loss, loss_scale=scale, obs_weight=None)
        g.sync()
        g.profile_enable(True)
        g.profile_reset()
        try:
            if model == "plain" and loss == BD.NONE:
                g.adjust_bundle_batch(*args, **kw)
            elif model == "plain":
                g.adjust_bundle_robust_batch(*args, **kw, **lossy)
            elif model == "focal":
                g.adjust_bundle_focal_batch(*args, case["group"], ngroups=1, **kw, **lossy)
            else:
                assert list(case["radial"]) == [1]
                g.adjust_bundle_radial_batch(*args, case["group"], ngroups=1, radial=case["radial"], k0=case["k0"],
                                             **kw, **lossy)
            g.sync()
            read = g.profile_read()
        finally:
            g.profile_enable(False)
        per_step = num_loops * (2 + cg_iters)
        want = dict(bundle_setup=1, bundle_track=per_step, bundle_image=per_step, bundle_scalar=per_step,
                    bundle_trial=num_loops, bundle_out=1)
        got = {k: v["calls"] for k, v in read.items()}
        print(model, loss, num_loops, cg_iters, got)
        assert got == {k: n for k, n in want.items() if n}, (model, num_loops, got)
        assert set(got) <= set(PROFILE_ENTRIES)


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
