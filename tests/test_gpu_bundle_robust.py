"""misift_adjust_bundle_robust_batch on the device: cameras and track points adjusted jointly under a Huber or a
Geman-McClure loss.

Every comparison is byte equality with bundle_robust_cases.expected_bundle (pinned in test_bundle_robust_cpu.py to the
library's host hook and to float64, where the premises of the cases are asserted too), or, with loss 0, with the
restatement of the plain call (bundle_cases.expected_bundle) and with the plain call itself: all ten outputs, and every
byte of the inputs, which the call must not write.  The harness is that of test_gpu_bundle.py: outputs of exactly the
stated capacity, poisoned first, every allocation of the module guarded.  The shapes are the smallest at which the kernels
can still go wrong: no free camera, one, 8 and 257 images, 0, 1 and 65 tracks, a track of 301 views, images around
min_obs and either side of one row of the position rule and its wrap, T and O from the device below, beyond and under
their capacities."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_robust_cases as BR
import filter_cases as FC
import refine_cases as RC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
INPUTS = (("track_offsets", np.int32), ("obs", TC.OBS_DTYPE), ("export_summary", np.int32), ("points", f32),
          ("point_status", np.int32), ("cam", f32), ("cam_pair", np.int32))
LOSS_IDS = ("huber", "geman-mcclure")


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


@pytest.fixture(scope="module")
def cases():
    return BR.cpu_cases()


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _adjust(ctx, case, in_place=False, weights=True, plain=False):
    """The call (plain: misift_adjust_bundle_batch) on poisoned outputs of exactly the stated sizes; returns them as
    uint32 arrays, obs_weight as it was poisoned when the call does not get it.  The inputs must come back as they went
    in (but for d_cam and d_points when they are the outputs)."""
    assert TC.POISON_WORD == POISON_WORD == BR.POISON_WORD
    ins = FC.inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in BR.sizes(case).items()}
    if in_place:
        outs["cam_out"], outs["points_out"] = dev["cam"], dev["points"]
    args = (case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
            dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"], case["intrinsics"])
    kw = dict(hold=case["hold"], min_views=case["min_views"], min_obs=case["min_obs"], num_loops=case["num_loops"],
              cg_iters=case["cg_iters"], max_error=case["max_error"], lambda0=case["lambda0"],
              orthonormalise=case["orthonormalise"])
    passed = {k: outs[k] for k in BC.OUTPUTS}
    if plain:
        ctx.adjust_bundle_batch(*args, **kw, **passed)
    else:
        ctx.adjust_bundle_robust_batch(*args, **kw, loss=case["loss"], loss_scale=case["loss_scale"],
                                       obs_weight=outs["obs_weight"] if weights else None, **passed)
    ctx.sync()
    for k, dt in INPUTS:
        if not (in_place and k in ("cam", "points")):
            assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (n,), np.uint32) for k, n in BR.sizes(case).items()}


def _check(ctx, case, what, in_place=False):
    e = BR.expected_bundle(case)
    BR.compare_all(_adjust(ctx, case, in_place), BR.in_place(e, case) if in_place else e, what)
    return e


@pytest.mark.parametrize("name", ("tie, c down", "tie", "tie, c up", "inliers") + tuple(
    "%s, %s" % (name, tag) for tag in LOSS_IDS
    for name in ("outliers only", "overflow", "rejected then kept", "behind", "outlier scene")))
def test_every_new_case(g, cases, name):
    """The cases of bundle_robust_cases.cpu_cases (what each is built to hit is asserted in test_bundle_robust_cpu.py)."""
    e = _check(g, cases[name], name)
    if name.startswith("overflow"):
        assert e["summary"].view(np.int32)[6] == 0 and not np.isfinite(e["cost"].view(f32)).any()


@pytest.mark.parametrize("loss,scale", BR.LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("shape", [a for a in BC.IMAGE_SHAPES if a[0] in (2, 3, 8, 257)], ids=lambda a: "%d" % a[0])
def test_image_counts(g, shape, loss, scale):
    e = _check(g, BR.robust(BC.image_count_case(*shape), loss, scale), "%d images, loss %d" % (shape[0], loss))
    s = e["summary"].view(np.int32)
    assert s[5] == 2 and s[1] + s[3] == shape[0] - 2 and s[6] >= 1


@pytest.mark.parametrize("loss,scale", BR.LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("ntracks", (0, 1, 65))
def test_track_counts(g, ntracks, loss, scale):
    e = _check(g, BR.robust(BC.track_count_case(ntracks), loss, scale), "%d tracks, loss %d" % (ntracks, loss))
    assert e["summary"].view(np.int32)[0] == ntracks == e["summary"].view(np.int32)[4]


@pytest.mark.parametrize("loss,scale", BR.LOSSES, ids=LOSS_IDS)
def test_a_track_of_301_views_and_members_around_min_obs_and_the_row_wrap(g, loss, scale):
    e = _check(g, BR.robust(BC.views_case(num_loops=2, cg_iters=4), loss, scale), "views, loss %d" % loss)
    P = e["res"]["problem"]
    assert sorted(set(P.tcount[:P.T].tolist())) == [2, 3, 7, 301]
    case, want = BC.member_counts_case(num_loops=2, cg_iters=3)
    e = _check(g, BR.robust(case, loss, scale), "members per image, loss %d" % loss)
    assert e["cam_obs"].view(np.int32)[2:].tolist() == want == [5, 6, 7, 255, 256, 257, 513]


def _plain_cases():
    return (("4 images", BC.planted(40, 4, 1)["case"]), ("hostile", BC.hostile_case(num_loops=3, cg_iters=5)),
            ("views", BC.views_case(num_loops=2, cg_iters=4)), ("rejected then kept", BC.rejected_then_kept_case()))


def test_loss_0_is_the_plain_call(g):
    """The first identity: loss 0 through the new call against the restatement of the plain call, and against the plain
    call itself on the device, byte for byte; every member's weight is 1, loss_scale is not read."""
    for name, case in _plain_cases():
        e = BR.expected_plain_with_weights(case)
        plain = _adjust(g, BR.robust(case, BR.NONE, 0.0), plain=True)
        BC.compare(plain, e, name + ", the plain call")
        for c in (0.0, np.nan):
            got = _adjust(g, BR.robust(case, BR.NONE, c))
            BR.compare_all(got, e, name + ", loss 0")
            for k in BC.OUTPUTS:
                assert got[k].tobytes() == plain[k].tobytes(), (name, k)


def test_huber_with_every_member_an_inlier_is_the_plain_call(g, cases):
    """The second identity, on the device."""
    case = cases["inliers"]
    got, plain = _adjust(g, case), _adjust(g, case, plain=True)
    for k in BC.OUTPUTS:
        assert got[k].tobytes() == plain[k].tobytes(), k
    BR.compare_all(got, BR.expected_plain_with_weights(case), "inliers")
    w = got["obs_weight"].view(f32)[:RC.counts(case)[1]]
    assert set(np.unique(w).tolist()) <= {-1.0, 1.0} and (w == 1).sum() > 100


def test_without_weights_in_place_and_twice(g, cases):
    for name in ("outlier scene, huber", "outlier scene, geman-mcclure", "behind, huber"):
        case = cases[name]
        e = BR.expected_bundle(case)
        first, again, without = _adjust(g, case), _adjust(g, case), _adjust(g, case, weights=False)
        BR.compare_all(first, e, name)
        for k in BR.OUTPUTS:
            assert first[k].tobytes() == again[k].tobytes(), (name, k)
        BR.compare_all(without, e, name + ", no d_obs_weight", keys=BC.OUTPUTS)
        assert (without["obs_weight"] == POISON_WORD).all()
        _check(g, case, name + ", in place", in_place=True)
    for loss, scale in BR.LOSSES:
        _check(g, BR.robust(BC.hostile_case(num_loops=3, cg_iters=5), loss, scale), "hostile, in place", in_place=True)


@pytest.mark.parametrize("T,O", BC.DEVICE_COUNTS)
def test_counts_from_the_device(g, T, O):
    """T and O below their capacities cut the tracks and the slots; beyond them they are clamped; below 0 they are 0.
    d_obs_weight stays as it was at and beyond O."""
    for loss, scale in BR.LOSSES:
        case = BR.robust(BC.device_counts_case(T, O), loss, scale)
        e = _check(g, case, "T = %d, O = %d, loss %d" % (T, O, loss))
        Oc = min(max(O, 0), 513)
        assert e["summary"].view(np.int32)[0] == min(max(T, 0), 171)
        assert (e["obs_weight"][Oc:] == POISON_WORD).all() and (e["obs_weight"][:Oc] != POISON_WORD).all()


def test_one_context_after_a_refine_with_more_and_with_less_temp(g):
    """The temp of the context is shared: the call after a refine that left it larger, and in a fresh context after one
    that left it smaller."""
    case = BR.robust(BC.planted(40, 4, 1)["case"], BR.GEMAN_MCCLURE, 4.0)
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
    case = BR.robust(BC.planted(40, 4, 1)["case"], BR.HUBER, 2.0)
    ins = FC.inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(g, n) for k, n in BR.sizes(case).items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n, mt = case["nimages"], case["max_tracks"]
    hold = np.array([1], np.int32)
    good = dict(ctx=g.h, max_tracks=mt, max_obs=case["max_obs"], track_offsets=dev["track_offsets"].ptr,
                obs=dev["obs"].ptr, export_summary=dev["export_summary"].ptr, points=dev["points"].ptr,
                point_status=dev["point_status"].ptr, nimages=n, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr,
                intrinsics=K.ctypes.data, nhold=1, hold=hold.ctypes.data, min_views=2, min_obs=6, num_loops=5,
                cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0, loss=BR.HUBER, loss_scale=2.0,
                **{k: outs[k].ptr for k in BR.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_adjust_bundle_robust_batch(*[a[k] for k in good])

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
    # what the robust call adds
    bad += [dict(loss=-1), dict(loss=3), dict(loss=2 ** 31 - 1), dict(loss=-2 ** 31)]
    bad += [dict(loss=loss, loss_scale=c) for loss in (BR.HUBER, BR.GEMAN_MCCLURE)
            for c in (0.0, -0.0, -2.0, np.nan, np.inf, -np.inf)]
    lists = []                                                   # kept alive until the calls are made
    for h in ([-1, 1], [1, n], [2 ** 31 - 1, 0]):
        lists.append(np.array(h, np.int32))
        bad.append(dict(nhold=2, hold=lists[-1].ctypes.data))
    for at, v in ((0, 0.0), (1, np.nan), (4 * n - 4, np.inf), (4 * n - 3, -1500.0), (2, np.nan), (4 * n - 1, np.inf)):
        lists.append(K.copy())
        lists[-1].reshape(-1)[at] = v
        bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in BR.sizes(case).items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, dt in INPUTS:
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # the same arguments, unbroken; then without the weights, without a history and without a loop
    assert call() == MISIFT_OK
    g.sync()
    full = dict(case, hold=(1,), min_views=2, min_obs=6, num_loops=5, cg_iters=10, max_error=np.inf, lambda0=1e-3,
                orthonormalise=0)
    BR.compare_all({k: g.download(outs[k], (m,), np.uint32) for k, m in BR.sizes(case).items()}, BR.expected_bundle(full),
                   "unbroken")
    assert call(obs_weight=None) == MISIFT_OK and call(history=None, num_loops=0) == MISIFT_OK
    assert call(loss=BR.NONE, loss_scale=np.nan) == MISIFT_OK
    g.sync()


def test_adjust_robust_filter_triangulate(g):
    """The chain on the small outlier scene, nothing read in between: one robust adjust, the filter on its cameras and
    points, triangulate on the filter's lists.  Each step against its restatement fed the device's own buffers."""
    case, _ = BR.outlier_case(BR.GEMAN_MCCLURE, 4.0, num_loops=4)
    mt, mo, nimg, K = case["max_tracks"], case["max_obs"], case["nimages"], case["intrinsics"]
    fargs = dict(max_error=6.0, max_cos=0.99999, min_views=2, unique_frames=1)
    ins = FC.inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    adj = {k: _poisoned(g, m) for k, m in BR.sizes(case).items()}
    g.adjust_bundle_robust_batch(mt, mo, dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
                                 dev["point_status"], nimg, dev["cam"], dev["cam_pair"], K, hold=case["hold"],
                                 min_views=case["min_views"], min_obs=case["min_obs"], num_loops=case["num_loops"],
                                 cg_iters=case["cg_iters"], max_error=case["max_error"], lambda0=case["lambda0"],
                                 orthonormalise=case["orthonormalise"], loss=case["loss"], loss_scale=case["loss_scale"],
                                 **adj)
    flt = {k: _poisoned(g, m) for k, m in FC.sizes(case).items()}
    g.filter_tracks_batch(mt, mo, dev["track_offsets"], dev["obs"], dev["export_summary"], adj["points_out"],
                          dev["point_status"], nimg, adj["cam_out"], dev["cam_pair"], K, **fargs, **flt)
    tri = g.triangulate_tracks_batch(mt, mo, flt["track_offsets_out"], flt["obs_out"], flt["export_summary_out"], nimg,
                                     adj["cam_out"], dev["cam_pair"], K, min_views=2, num_loops=5)
    g.sync()
    got = {k: g.download(adj[k], (m,), np.uint32) for k, m in BR.sizes(case).items()}
    gotf = {k: g.download(flt[k], (m,), np.uint32) for k, m in FC.sizes(case).items()}
    e = BR.expected_bundle(case)
    BR.compare_all(got, e, "chain, robust adjust")
    casef = dict(case, cam=got["cam_out"].view(f32).reshape(-1, 12), points=got["points_out"].view(f32).reshape(-1, 4),
                 **fargs)
    ef = FC.expected_filter(casef)
    FC.compare(gotf, ef, "chain, filter")
    tc = dict(FC.filtered_case(casef, gotf), min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        x = TC.expected_triangulate(tc)
    got3 = dict(points=g.download(tri[0], (4 * mt,), np.uint32), point_views=g.download(tri[1], (mt,), np.uint32),
                point_status=g.download(tri[2], (mt,), np.uint32), obs_error=g.download(tri[3], (mo,), np.uint32),
                summary=g.download(tri[4], (8,), np.uint32))
    for k in got3:
        written = x[k] != POISON_WORD                            # what the call leaves alone was zeroed here, not poisoned
        assert (got3[k][written] == x[k][written]).all(), k
    s = ef["summary"].view(np.int32)
    w = got["obs_weight"].view(f32)[:RC.counts(case)[1]]
    print("chain: T %d -> %d, O -> %d, gated %d; members below weight 0.5: %d of %d" % (
        RC.counts(case)[0], s[0], s[1], s[3], int(((w >= 0) & (w < 0.5)).sum()), int((w >= 0).sum())))
    assert s[0] > 0 and s[3] > 0 and e["summary"].view(np.int32)[6] >= 1


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0
