"""misift_adjust_bundle_robust_batch without a GPU: bundle_robust_cases.adjust, the numpy float32 restatement of the
definition in include/misift.h, is pinned from both sides, as test_bundle_cpu.py pins the plain call: the library's
host-only hook misift_test_adjust_bundle_robust, compiled from the functions the kernels run (bundle_core.hpp), must give
the same bytes on every case; and in float64 the same restatement is held to the gradient of the robust cost by central
differences, to dense linear algebra on the weighted normal equations, and to planted scenes with displaced
observations.  test_gpu_bundle_robust.py then holds the device to the restatement byte for byte."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_robust_cases as BR
import filter_cases as FC
import refine_cases as RC
import test_bundle_cpu as TB
import test_filter_cpu as TF
from test_fundamental_cpu import f32

f64 = np.float64
EINVAL = -1


def test_library_exports_the_call_the_hook_and_the_binding():
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_adjust_bundle_robust_batch", "misift_test_adjust_bundle_robust"):
        assert name in capi.SIGNATURES, name
        assert hasattr(L, name), name
    old, new = capi.SIGNATURES["misift_adjust_bundle_batch"][1], capi.SIGNATURES["misift_adjust_bundle_robust_batch"][1]
    assert len(new) == len(old) + 3 and new[:21] == old[:21] and new[23:31] == old[21:29] and new[32] == old[29]
    old, new = capi.SIGNATURES["misift_test_adjust_bundle"][1], capi.SIGNATURES["misift_test_adjust_bundle_robust"][1]
    assert len(new) == len(old) + 3 and new[:20] == old[:20] and new[22:30] == old[20:28] and new[31] == old[28]
    assert callable(capi.Context.adjust_bundle_robust_batch)
    assert (capi.LOSS_NONE, capi.LOSS_HUBER, capi.LOSS_GEMAN_MCCLURE) == (0, 1, 2) == (BR.NONE, BR.HUBER, BR.GEMAN_MCCLURE)
    assert L.misift_adjust_bundle_robust_batch(None, 1, 1, None, None, None, None, None, 1, None, None, None, 0, None, 2,
                                               3, 0, 0, 1.0, 1e-3, 0, 1, 2.0, None, None, None, None, None, None, None,
                                               None, None, None) == EINVAL


_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update(BR.cpu_cases())
    return _CASES


CASE_NAMES = ("tie, c down", "tie", "tie, c up", "inliers") + tuple(
    "%s, %s" % (name, tag) for tag in ("huber", "geman-mcclure")
    for name in ("outliers only", "overflow", "rejected then kept", "behind", "outlier scene"))


def test_case_names():
    assert set(_cases()) == set(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_the_hook(name):
    case = _cases()[name]
    e = BR.expected_bundle(case)
    BR.compare_all(BR.hook_bundle_robust(case), e, name)
    if name in ("inliers", "outlier scene, geman-mcclure"):
        BR.compare_all(BR.hook_bundle_robust(case, in_place=True), BR.in_place(e, case), name + ", in place")
        got = BR.hook_bundle_robust(case, weights=False)            # NULL obs_weight: the nine as they were
        BR.compare_all(got, e, name + ", no weights", keys=BC.OUTPUTS)
        assert (got["obs_weight"] == BR.POISON_WORD).all()


@pytest.mark.parametrize("name", TB.CASE_NAMES)
def test_the_cases_of_the_plain_call_under_every_loss(name):
    """bundle_cases.cpu_cases under Huber at 2 px and Geman-McClure at 4 px; and with loss 0 the new hook gives the bytes
    of the old hook (and of the old restatement), every member's weight 1, whatever loss_scale says."""
    case = BC.cpu_cases()[name]
    for loss, c in BR.LOSSES:
        rc = BR.robust(case, loss, c)
        BR.compare_all(BR.hook_bundle_robust(rc), BR.expected_bundle(rc), "%s, loss %d" % (name, loss))
    old = BC.hook_bundle(case)
    e = BR.expected_plain_with_weights(case)
    for c in (2.0, 0.0, -1.0, np.nan):                               # not read with loss 0
        got = BR.hook_bundle_robust(BR.robust(case, BR.NONE, c))
        BC.compare(got, old, name + ", loss 0 against the old hook")
        BR.compare_all(got, e, name + ", loss 0 against the old restatement")
    BR.compare_all(BR.hook_bundle_robust(BR.robust(case, BR.NONE, 0.0)), BR.expected_bundle(BR.robust(case, BR.NONE, 0.0)),
                   name + ", loss 0 against the new restatement")


def test_the_shapes_of_the_device_tests_through_the_hook():
    """Every further case test_gpu_bundle_robust.py compares on the device."""
    cases = [("%d images" % a[0], BC.image_count_case(*a)) for a in BC.IMAGE_SHAPES if a[0] in (2, 3, 8, 257)]
    cases += [("%d tracks" % n, BC.track_count_case(n)) for n in (0, 1, 65)]
    cases += [("T %d O %d" % a, BC.device_counts_case(*a)) for a in BC.DEVICE_COUNTS]
    cases += [("views", BC.views_case(num_loops=2, cg_iters=4)), ("members", BC.member_counts_case(num_loops=2,
                                                                                                  cg_iters=3)[0])]
    for name, case in cases:
        for loss, c in BR.LOSSES:
            rc = BR.robust(case, loss, c)
            BR.compare_all(BR.hook_bundle_robust(rc), BR.expected_bundle(rc), "%s, loss %d" % (name, loss))


def test_every_argument_error_of_the_hook():
    from cudasift_amd import capi
    L = capi.lib()
    case = BR.robust(BC.planted(40, 4, 1)["case"], BR.HUBER, 2.0)
    a = BR.hook_args(case)
    out = {k: np.full(m, BR.POISON_WORD, np.uint32) for k, m in BR.sizes(case).items()}
    hold = np.array([1], np.int32)
    good = dict(max_tracks=case["max_tracks"], max_obs=case["max_obs"], track_offsets=a["offs"].ctypes.data,
                obs=a["obs"].ctypes.data, export_summary=a["summ"].ctypes.data, points=a["pts"].ctypes.data,
                point_status=a["st"].ctypes.data, nimages=case["nimages"], cam=a["cam"].ctypes.data,
                cam_pair=a["pair"].ctypes.data, intrinsics=a["K"].ctypes.data, nhold=1, hold=hold.ctypes.data,
                min_views=2, min_obs=6, num_loops=5, cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=0,
                loss=BR.HUBER, loss_scale=2.0, **{k: out[k].ctypes.data for k in BR.OUTPUTS})

    def call(**kw):
        b = dict(good, **kw)
        return L.misift_test_adjust_bundle_robust(*[b[k] for k in good])

    n = case["nimages"]
    lists = [np.array(h, np.int32) for h in ([-1, 1], [1, n], [2 ** 31 - 1, 0])]
    bad = [dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-7), dict(nimages=0), dict(nimages=-1),
           dict(min_views=1), dict(min_views=-2), dict(min_obs=2), dict(min_obs=0), dict(min_obs=-3), dict(num_loops=-1),
           dict(cg_iters=-1), dict(max_error=np.nan), dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=-np.inf),
           dict(lambda0=0.0), dict(lambda0=-1e-3), dict(lambda0=np.nan), dict(lambda0=np.inf), dict(lambda0=-np.inf),
           dict(orthonormalise=2), dict(orthonormalise=-1), dict(nhold=-1), dict(nhold=2, hold=None)]
    bad += [dict(nhold=2, hold=h.ctypes.data) for h in lists]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "points", "point_status", "cam", "cam_pair",
                                "intrinsics") + BC.OUTPUTS]
    # what the robust call adds
    bad += [dict(loss=-1), dict(loss=3), dict(loss=2 ** 31 - 1), dict(loss=-2 ** 31)]
    bad += [dict(loss=loss, loss_scale=c) for loss in (BR.HUBER, BR.GEMAN_MCCLURE)
            for c in (0.0, -0.0, -2.0, np.nan, np.inf, -np.inf)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    for k in out:
        assert (out[k] == BR.POISON_WORD).all(), k
    for c in (0.0, -2.0, np.nan, np.inf):                            # with loss 0 the scale is not read
        assert call(loss=BR.NONE, loss_scale=c) == 0, c
    assert call(obs_weight=None) == 0 and call(history=None, num_loops=0) == 0 and call() == 0
    BR.compare_all(out, BR.expected_bundle(dict(case, num_loops=5, cg_iters=10, min_obs=6, min_views=2, lambda0=1e-3,
                                                orthonormalise=0, max_error=np.inf, hold=(1,))), "unbroken")


# ---- the premises of the cases

def test_what_the_cases_are_built_to_hit():
    c = _cases()
    tie = BR.huber_tie_cases()
    m, s = tie["member"], tie["s"]
    sides = []
    for case in tie["cases"]:
        cc, c2 = BR.scale_of(case, f32)
        s0, _ = BR.member_s(case)
        assert s0[m] == s
        sides.append(bool(s <= c2))
        w = BR.loss_terms(s0[m:m + 1], BR.HUBER, cc, c2, f32)[1][0]
        assert (w == 1) if sides[-1] else (w <= 1)
    cc, c2 = BR.scale_of(tie["cases"][1], f32)
    assert c2 == s and np.sqrt(s) == cc                              # the tie exists
    assert sides == [False, True, True]                              # an outlier below it, an inlier on it and above
    # the shares of outliers: every member under the starting state (Huber at 1e-3 px is next to an L1 cost, which
    # brings single residuals to nothing, so not every one under the final state), some under the scene's final state
    for tag in ("huber", "geman-mcclure"):
        case = c["outliers only, " + tag]
        s0, _ = BR.member_s(case)
        cc, c2 = BR.scale_of(case, f32)
        w = BR.adjust(case)["w"]
        assert (s0 > c2).all() and (BR.loss_terms(s0, case["loss"], cc, c2, f32)[1] < 1).all() and len(w) > 100, tag
        assert (w < 1).mean() > 0.8, tag
        r = BR.adjust(c["outlier scene, " + tag])
        share = float((r["w"] < 0.5).mean())
        print("outlier scene, %s: %.3f of the members below weight 0.5, steps %s" % (tag, share, r["trace"]))
        assert 0.02 < share < 0.5 and "kept" in r["trace"]
    assert "behind" in BR.adjust(c["behind, huber"])["trace"]
    r = BR.adjust(c["inliers"])
    assert r["visited"]["inliers"] and (r["w"] == 1).all() and r["kept"] >= 1
    assert not BR.adjust(c["tie"])["visited"]["inliers"]
    # the overflow: s = +inf, Huber weight 0 and cost +inf, Geman-McClure cost NaN; no step is kept
    r = BR.adjust(c["overflow, huber"])
    assert np.isinf(r["s"]).sum() == 1 and r["w"][np.isinf(r["s"])] == 0 and np.isposinf(r["cost"]).all()
    assert r["kept"] == 0 and r["trace"] == ["worse"] * 3
    r = BR.adjust(c["overflow, geman-mcclure"])
    assert np.isinf(r["s"]).sum() == 1 and np.isnan(r["e"][np.isinf(r["s"])]).all() and np.isnan(r["cost"]).all()
    assert r["kept"] == 0 and r["w"][np.isinf(r["s"])] == 0
    e = BR.expected_bundle(c["overflow, geman-mcclure"])
    assert (e["cost"] == 0x7fc00000).all() and (e["history"][0::4] == 0x7fc00000).all()


def test_the_second_identity():
    """Huber with every member's s <= c2 at every state visited is the plain call, byte for byte, and every weight 1."""
    case = _cases()["inliers"]
    got = BR.hook_bundle_robust(case)
    BC.compare(got, BC.hook_bundle(case), "inliers against the old hook")
    BR.compare_all(got, BR.expected_plain_with_weights(case), "inliers against the old restatement")
    P = BC.Problem(case, f32)
    w = got["obs_weight"].view(f32)[:P.O]
    assert (w[P.slot] == 1).all() and (np.delete(w, P.slot) == -1).all() and len(P.slot) > 100


# ---- the definition, independently of the restatement, in float64

def _sum_rho(P, cams, pts, loss, c, c2):
    total = 0.0
    for m in range(len(P.slot)):
        p = TB._project(cams[P.img[m]], P.K[P.img[m]], pts[P.trk[m]])
        s = (P.x[m] - p[0]) ** 2 + (P.y[m] - p[1]) ** 2
        if loss == BR.HUBER:
            total += s if s <= c2 else 2 * c * np.sqrt(s) - c2
        else:
            total += s * c2 / (c2 + s)
    return total


@pytest.mark.parametrize("loss,scale", BR.LOSSES)
def test_the_weighted_gradient_against_central_differences(loss, scale):
    """gc of a camera and gp of a point, the sums of w (Ju ru + Jv rv) formed from the scaled values, are minus half the
    gradient of the sum of rho along the Cayley update and along the point.  Central differences with h = 1e-6 in float64
    on a cost of some 1e3 to 1e4 px^2: the rounding is 2.2e-16 x cost / h = 2e-6 and the truncation h^2 times a third
    derivative, against entries of 1e2 to 1e5; 1e-6 of the largest entry plus 1e-4 absolute bounds both.  The scene has
    no member at the kink of Huber within h of it."""
    case = BR.noisy_scene(40, 4, 71, loss, scale)[0]
    P = BC.Problem(case, f64)
    c, c2 = BR.scale_of(case, f64)
    s = BR.lm_step(P, P.cams0, P.pts0, f64(1e-3), 0, f64, loss, c, c2)
    l, w = s["lin"], s["w"]
    assert (w < 1).any() and (np.abs(l - np.sqrt(w)[:, None] * s["lin0"]) <= 1e-12 * np.abs(l)).all()
    if loss == BR.HUBER:
        assert (w == 1).any()
    h, worst, largest = 1e-6, 0.0, 0.0
    for i in P.free:
        m = P.of_image[i]
        g = (l[m, :6] * l[m, 18:19] + l[m, 6:12] * l[m, 19:20]).sum(0)
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            hi, lo = P.cams0.copy(), P.cams0.copy()
            hi[i], lo[i] = RC.update(P.cams0[i], d, f64), RC.update(P.cams0[i], -d, f64)
            fd = (_sum_rho(P, hi, P.pts0, loss, c, c2) - _sum_rho(P, lo, P.pts0, loss, c, c2)) / (2 * h)
            worst, largest = max(worst, abs(g[j] + fd / 2)), max(largest, abs(g[j]))
    for t in np.nonzero(P.active)[0][::5]:
        m = np.nonzero(P.trk == t)[0]
        g = (l[m, 12:15] * l[m, 18:19] + l[m, 15:18] * l[m, 19:20]).sum(0)
        for j in range(3):
            hi, lo = P.pts0.copy(), P.pts0.copy()
            hi[t, j] += h
            lo[t, j] -= h
            fd = (_sum_rho(P, P.cams0, hi, loss, c, c2) - _sum_rho(P, P.cams0, lo, loss, c, c2)) / (2 * h)
            worst, largest = max(worst, abs(g[j] + fd / 2)), max(largest, abs(g[j]))
    print("loss %d: worst |g + grad / 2| %.3g against entries up to %.3g" % (loss, worst, largest))
    assert worst <= 1e-6 * largest + 1e-4


@pytest.mark.parametrize("loss,scale", BR.LOSSES)
def test_the_step_solves_the_full_weighted_damped_normal_equations(loss, scale):
    """test_bundle_cpu's dense system built from the scaled rows is J^T W J and J^T W r; with cg_iters = 6 x free cameras
    the step is its solution.  The bound is that test's: 1e3 x cond x 2.2e-16 of the step."""
    case = BR.noisy_scene(120, 4, 94, loss, scale)[0]
    P = BC.Problem(case, f64)
    c, c2 = BR.scale_of(case, f64)
    nf = len(P.free)
    lam = f64(1e-3)
    s = BR.lm_step(P, P.cams0, P.pts0, lam, 6 * nf, f64, loss, c, c2)
    assert (s["w"] < 1).any()
    x, delta, cond = TB._dense_step(P, s, float(lam))
    ex = np.abs(s["x"] - x).max() / np.abs(x).max()
    ed = np.abs(s["delta"] - delta).max() / np.abs(delta).max()
    print("loss %d, %d free cameras: cond %.3g, |x - dense| %.3g, |delta - dense| %.3g (relative)" % (loss, nf, cond, ex,
                                                                                                     ed))
    assert not s["fail"] and nf == 2 and max(ex, ed) <= 1e3 * cond * 2.2e-16


@pytest.mark.parametrize("loss,scale", BR.LOSSES)
def test_kept_steps_never_raise_the_robust_cost(loss, scale):
    r = BR.adjust(BR.noisy_scene(90, 6, 72, loss, scale)[0], f64)
    cost = r["cost"][0]
    for c2, _, kept, _ in r["history"]:
        if kept:
            assert c2 < cost
            cost = c2
        else:
            assert not c2 < cost
    assert cost == r["cost"][1] and r["kept"] >= 2
    rho = BR.loss_terms(r["s"], loss, *BR.scale_of(r["problem"].case, f64), f64)[0]
    assert abs(rho.sum() - cost) <= 1e-9 * cost                      # the cost is the sum of rho of the final state


# ---- planted scenes with displaced observations

SCENES = ((60, 4, 71), (90, 6, 72), (120, 8, 73))
# max |fp32 - float64| over the cameras and over the points of the final state, and of the pooled rms in px over the
# members that were not displaced, the same restatement in both formats (0.5 px noise, 5 % of the observations displaced
# by 30 px, 6 steps of 10 CG iterations), the worst of SCENES, per loss
MEASURED = {(BR.HUBER, "cam"): 2.20e-6, (BR.HUBER, "point"): 1.77e-5, (BR.HUBER, "rms"): 1.40e-6,
            (BR.GEMAN_MCCLURE, "cam"): 9.48e-6, (BR.GEMAN_MCCLURE, "point"): 4.33e-5, (BR.GEMAN_MCCLURE, "rms"): 6.11e-6}


def _clean_pooled(res, hit):
    P = res["problem"]
    s = np.asarray(res["s"], f64)[~hit[P.slot]]
    return float(np.sqrt(s.mean()))


@pytest.mark.parametrize("loss,scale", BR.LOSSES)
def test_planted_scenes_with_outliers_against_float64(loss, scale):
    worst = dict(cam=0.0, point=0.0, rms=0.0)
    for ntracks, nimages, seed in SCENES:
        case, hit = BR.noisy_scene(ntracks, nimages, seed, loss, scale)
        r32, r64 = BR.adjust(case), BR.adjust(case, f64)
        P = r32["problem"]
        act = np.nonzero(P.active)[0]
        worst["cam"] = max(worst["cam"], float(np.abs(r32["cams"][P.free].astype(f64) - r64["cams"][P.free]).max()))
        worst["point"] = max(worst["point"], float(np.abs(r32["pts"][act].astype(f64) - r64["pts"][act]).max()))
        worst["rms"] = max(worst["rms"], abs(_clean_pooled(r32, hit) - _clean_pooled(r64, hit)))
        assert hit[P.slot].sum() >= 5 and r32["kept"] >= 3 and r32["trace"] == r64["trace"]
    print("planted with outliers, loss %d, |fp32 - fp64|: %s" % (loss, {k: "%.3g" % v for k, v in worst.items()}))
    for k in worst:
        assert worst[k] <= 2 * MEASURED[(loss, k)], (k, worst[k])


# the scene and the selection of test_filter_cpu.test_adjust_filter_adjust_against_adjust_adjust (152 tracks over 6
# images, 0.5 px of noise, 5 % of the observations displaced by 30 px, 8 tracks merged with another point's): the pooled
# rms in px over the planted-clean observations of the tracks that test's filter keeps, after ONE call of 6 steps under
# each loss.  test_filter_cpu.MEASURED has 4.6235 for adjust -> adjust and 0.8214 for adjust -> filter -> adjust, which
# removes 10.7 % of the clean observations; a loss removes none
MEASURED_SCENE = {"loss 0": 4.6235, "huber, 2 px": 0.8377, "geman-mcclure, 4 px": 0.5800}


def test_one_robust_call_against_the_plain_call_on_the_outlier_scene():
    sc = FC.outlier_scene(ntracks=160, nimages=6, seed=103, merged=8, drift=(0.004, 0.01), point_noise=0.01,
                          max_error=10.0)
    case = sc["case"]
    T, O = RC.counts(case)
    mt = case["max_tracks"]
    kw = dict(hold=(1,), min_views=2, min_obs=6, cg_iters=10, lambda0=1e-3, orthonormalise=0, max_error=RC.INF)
    e = BC.expected_bundle(dict(case, num_loops=3, **kw))           # that test's first adjust, for its filter's selection
    pts = e["points_out"].view(f32).reshape(mt, 4).copy()
    pts[T:] = 0
    first = dict(case, cam=e["cam_out"].view(f32).reshape(-1, 12).copy(), points=pts)
    f = FC.expected_filter(dict(first, **{k: case[k] for k in FC.ARGS}))
    track, owner = f["track_map"].view(np.int32)[:T], f["res"]["slots"]["owner"]
    sel = np.nonzero(sc["clean"] & (owner >= 0) & (track[np.maximum(owner, 0)] >= 0))[0]
    got = {}
    for name, loss, c in (("loss 0", BR.NONE, 0.0), ("huber, 2 px", BR.HUBER, 2.0),
                          ("geman-mcclure, 4 px", BR.GEMAN_MCCLURE, 4.0)):
        x = BR.expected_bundle(BR.robust(dict(case, num_loops=6, **kw), loss, c))
        P = x["res"]["problem"]
        assert np.isin(sel, P.slot).all()                            # nothing removed: every one of them is a member
        got[name] = TF._clean_rms(case, x["cam_out"].view(f32), x["points_out"].view(f32), sel, owner[sel])
    print("measured: %s over %d clean observations (test_filter_cpu has %.4f for adjust -> adjust)" % (
        {k: round(v, 4) for k, v in got.items()}, len(sel), TF.MEASURED["adjust, adjust"]))
    assert got["huber, 2 px"] < got["loss 0"] and got["geman-mcclure, 4 px"] < got["loss 0"]
