"""misift_adjust_bundle_batch without a GPU: bundle_cases.adjust, the numpy float32 restatement of the definition in
include/misift.h, is pinned from both sides: the library's host-only hook misift_test_adjust_bundle, compiled from the
functions the kernels run (bundle_core.hpp), must give the same bytes on every case; and in float64 the same restatement
is held to dense linear algebra, to central differences and to planted scenes.  test_gpu_bundle.py then holds the device
to the restatement byte for byte."""
import numpy as np
import pytest

import bundle_cases as BC
import refine_cases as RC
from test_fundamental_cpu import f32

f64 = np.float64


def test_library_exports_the_call_and_the_hook():
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_adjust_bundle_batch", "misift_test_adjust_bundle"):
        assert hasattr(L, name), name
    assert L.misift_adjust_bundle_batch(None, 1, 1, None, None, None, None, None, 1, None, None, None, 0, None, 2, 3, 0, 0,
                                        1.0, 1e-3, 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.misift_test_adjust_bundle(1, 1, None, None, None, None, None, 1, None, None, None, 0, None, 2, 3, 0, 0, 1.0,
                                       1e-3, 0, None, None, None, None, None, None, None, None, None) == -1


_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update(BC.cpu_cases())
    return _CASES


CASE_NAMES = ("2 images", "3 images", "4 images", "rejected then kept", "behind", "members", "views", "min_views 3",
              "hostile", "hostile gated", "bad offsets", "no track", "no loop", "cg 0", "cg 1", "cg 40", "huge lambda")


def test_case_names():
    assert set(_cases()) == set(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_the_hook(name):
    case = _cases()[name]
    e = BC.expected_bundle(case)
    BC.compare(BC.hook_bundle(case), e, name)
    if name in ("4 images", "hostile"):
        BC.compare(BC.hook_bundle(case, in_place=True), e, name + ", in place")


def test_the_shapes_of_the_device_tests_through_the_hook():
    """Every case test_gpu_bundle.py compares on the device, beyond the named ones above."""
    cases = [("%d images" % a[0], BC.image_count_case(*a)) for a in BC.IMAGE_SHAPES]
    cases += [("%d tracks" % n, BC.track_count_case(n)) for n in BC.TRACK_COUNTS]
    cases += [("T %d O %d" % a, BC.device_counts_case(*a)) for a in BC.DEVICE_COUNTS]
    cases += [("%s %s" % (name, a), c) for a in BC.SETTINGS for name, c in BC.settings_cases(*a)]
    cases += [("views", BC.views_case(num_loops=2, cg_iters=4, min_views=m)) for m in (2, 3)]
    cases += [("in place", BC.planted(40, 4, 1, orthonormalise=1)["case"])]
    for name, case in cases:
        BC.compare(BC.hook_bundle(case, in_place=name == "in place"), BC.expected_bundle(case), name)


def test_what_the_cases_are_built_to_hit():
    c = _cases()
    trace = BC.adjust(c["rejected then kept"])["trace"]
    assert any(a == "worse" and b == "kept" for a, b in zip(trace, trace[1:])), trace
    assert "behind" in BC.adjust(c["behind"])["trace"]
    assert BC.adjust(c["huge lambda"])["trace"] == ["singular"] * 3
    case, want = BC.member_counts_case(num_loops=2, cg_iters=3)
    e = BC.expected_bundle(case)
    assert e["cam_obs"].view(np.int32)[2:].tolist() == want
    assert e["cam_status"].view(np.int32).tolist() == [BC.HELD, BC.HELD, BC.FEW_OBS] + [BC.ADJUSTED] * 6
    # an inactive track: its two pre-members leave, its point comes back bit for bit
    e2, e3 = BC.expected_bundle(c["views"]), BC.expected_bundle(c["min_views 3"])
    P = e3["res"]["problem"]
    idle = np.nonzero(~P.active[:P.T])[0]
    assert len(idle) == 30 and (P.tcount[idle] == 2).all() and e2["res"]["problem"].active[:P.T].all()
    pts_in = np.ascontiguousarray(c["min_views 3"]["points"], f32).view(np.uint32).reshape(-1, 4)
    assert (e3["points_out"].reshape(-1, 4)[idle] == pts_in[idle]).all()
    assert max(h[3] for h in BC.adjust(c["cg 40"])["history"]) < 40          # CG ends early
    hist = BC.adjust(c["2 images"])["history"]
    assert all(h[3] == 0 for h in hist) and hist[0][2] == 1                  # no free camera: the points move alone
    e = BC.expected_bundle(c["no loop"])
    assert e["cam_out"].tobytes() == np.ascontiguousarray(c["no loop"]["cam"], f32).tobytes()
    pts_in = np.ascontiguousarray(c["no loop"]["points"], f32).view(np.uint32).reshape(-1, 4)
    assert (e["points_out"].reshape(-1, 4)[:, :3] == pts_in[:, :3]).all()    # [4t+3] takes the rms
    assert e["cost"][0] == e["cost"][1]


# ---- the definition, independently of the restatement, in float64

def _project(c, k, X):
    Xc = c[:9].reshape(3, 3) @ X + c[9:]
    return np.array([k[0] * Xc[0] / Xc[2] + k[2], k[1] * Xc[1] / Xc[2] + k[3]])


def _dense_step(P, s, lam):
    """The full damped normal equations of one step (free cameras, then active points), built from the per-member
    Jacobians: (x (nf, 6), delta (T, 3), the condition number)."""
    l = s["lin"]
    nf, act = len(P.free), np.nonzero(P.active)[0]
    cpos = {int(i): 6 * f for f, i in enumerate(P.free)}
    ppos = {int(t): 6 * nf + 3 * a for a, t in enumerate(act)}
    n = 6 * nf + 3 * len(act)
    J = np.zeros((2 * len(l), n))
    r = np.zeros(2 * len(l))
    for m in range(len(l)):
        i, t = int(P.img[m]), int(P.trk[m])
        for h in range(2):
            if i in cpos:
                J[2 * m + h, cpos[i]:cpos[i] + 6] = l[m, 6 * h:6 * h + 6]
            J[2 * m + h, ppos[t]:ppos[t] + 3] = l[m, 12 + 3 * h:15 + 3 * h]
            r[2 * m + h] = l[m, 18 + h]
    H = J.T @ J
    H[np.diag_indices(n)] *= 1 + lam
    sol = np.linalg.solve(H, J.T @ r)
    delta = np.zeros((len(P.pts0), 3))
    delta[act] = sol[6 * nf:].reshape(-1, 3)
    return sol[:6 * nf].reshape(nf, 6), delta, float(np.linalg.cond(H))


@pytest.mark.parametrize("nimages", [3, 4, 5])
def test_the_step_solves_the_full_damped_normal_equations(nimages):
    """With cg_iters = 6 x free cameras, CG has the reduced system solved, so the step is the solution of the full system
    of cameras and points.  Both are float64; the bound is the rounding of a solve, 1e3 x cond x 2.2e-16 of the step."""
    case = BC.planted(30 * nimages, nimages, 90 + nimages, lengths=(3, 4))["case"]
    P = BC.Problem(case, f64)
    nf = len(P.free)
    assert nf == nimages - 2
    lam = f64(1e-3)
    s = BC.lm_step(P, P.cams0, P.pts0, lam, 6 * nf, f64)
    x, delta, cond = _dense_step(P, s, float(lam))
    ex = np.abs(s["x"] - x).max() / np.abs(x).max()
    ed = np.abs(s["delta"] - delta).max() / np.abs(delta).max()
    print("%d free cameras: cond %.3g, |x - dense| %.3g, |delta - dense| %.3g (relative)" % (nf, cond, ex, ed))
    assert not s["fail"] and max(ex, ed) <= 1e3 * cond * 2.2e-16


def test_jacobians_and_the_cayley_update_against_central_differences():
    """Jc is the derivative of the projection along the Cayley update at 0, Jp along the point.  Central differences with
    h = 1e-6 in float64: the truncation is h^2 times a third derivative and the rounding 2.2e-16 x 2000 px / h = 4e-7 px
    per px of step, against entries of some hundreds: 1e-6 of the largest entry bounds both."""
    case = BC.planted(40, 4, 1)["case"]
    P = BC.Problem(case, f64)
    _, l = BC.linearise(P.cams0[P.img], P.K[P.img], P.pts0[P.trk], P.x, P.y, f64)
    h, worst = 1e-6, 0.0
    for m in range(0, len(l), 7):
        c, k, X = P.cams0[P.img[m]], P.K[P.img[m]], P.pts0[P.trk[m]]
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            g = (_project(RC.update(c, d, f64), k, X) - _project(RC.update(c, -d, f64), k, X)) / (2 * h)
            worst = max(worst, abs(g[0] - l[m, j]), abs(g[1] - l[m, 6 + j]))
        for j in range(3):
            d = np.zeros(3)
            d[j] = h
            g = (_project(c, k, X + d) - _project(c, k, X - d)) / (2 * h)
            worst = max(worst, abs(g[0] - l[m, 12 + j]), abs(g[1] - l[m, 15 + j]))
        assert np.allclose([P.x[m] - l[m, 18], P.y[m] - l[m, 19]], _project(c, k, X), rtol=0, atol=1e-9)
    print("central differences: worst %.3g against entries up to %.3g" % (worst, np.abs(l[:, :18]).max()))
    assert worst <= 1e-6 * np.abs(l[:, :18]).max()
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    C = RC.update(eye, np.array([0.3, -0.2, 0.5, 1, 2, 3], f64), f64)[:9].reshape(3, 3)
    assert np.abs(C @ C.T - np.eye(3)).max() < 1e-14                         # the Cayley map is orthogonal


def test_a_kept_step_lowers_the_cost_and_more_damping_shortens_the_step():
    """The damping multiplies the diagonal (Marquardt's scaling), so it is in the norm of that diagonal, sum of H_jj d_j^2,
    that the step shrinks as lambda grows; the plain length is printed beside it."""
    case = BC.planted(40, 4, 1, num_loops=1)["case"]
    r = BC.adjust(case, f64)
    assert r["trace"] == ["kept"] and r["cost"][1] < r["cost"][0]
    P = BC.Problem(case, f64)
    norm, plain = [], []
    for lam in (1e-3, 1.0):
        s = BC.lm_step(P, P.cams0, P.pts0, f64(lam), 12, f64)
        du = np.stack([s["U"][:, j, j] for j in range(6)], 1) / (1 + lam)
        dv = s["V"][:, (0, 3, 5)] / (1 + lam)
        norm.append(float(np.sqrt((du * s["x"] ** 2).sum() + (dv * s["delta"] ** 2).sum())))
        plain.append(float(np.sqrt((s["x"] ** 2).sum() + (s["delta"] ** 2).sum())))
    print("step length at lambda 1e-3 and at 1000 times that: %.4g, %.4g in the diagonal's norm (plain: %.4g, %.4g)" % (
        norm[0], norm[1], plain[0], plain[1]))
    assert norm[1] < norm[0]


# ---- planted scenes

SCENES = ((60, 4, 71), (90, 6, 72), (120, 8, 73))


def _cam_error(c, true):
    return float(np.abs(np.asarray(c, f64) - true).max())


@pytest.mark.parametrize("ntracks,nimages,seed", SCENES)
def test_planted_scenes_without_noise_reach_the_planted_state(ntracks, nimages, seed):
    sc = BC.planted(ntracks, nimages, seed, lengths=(3, 4, 5), noise=0.0, num_loops=8, orthonormalise=1)
    case = sc["case"]
    r = BC.adjust(case)
    P = r["problem"]
    start = np.asarray(case["cam"], f64).reshape(-1, 12)
    rms = BC.pooled_rms(r)
    err0 = [_cam_error(start[i], sc["true"][i]) for i in P.free]
    err1 = [_cam_error(r["cams"][i], sc["true"][i]) for i in P.free]
    print("planted %s: rms %.3g px, camera error %.3g -> %.3g, %s" % ((ntracks, nimages, seed), rms, max(err0), max(err1),
                                                                     r["trace"]))
    assert len(P.free) == nimages - 2 and rms < 0.01
    assert all(b < a for a, b in zip(err0, err1))


# max |fp32 - float64| over the cameras and over the points of the final state, and of the pooled rms in px, the same
# restatement in both formats (0.5 px noise, 6 steps of 10 CG iterations), the worst of SCENES.  The two formats take the
# same decisions on these scenes; the minimum is flat along the directions the noise leaves open.
MEASURED = {"cam": 7.48e-6, "point": 2.31e-5, "rms": 1.98e-6}


def test_planted_scenes_with_noise_against_float64():
    worst = dict.fromkeys(MEASURED, 0.0)
    for ntracks, nimages, seed in SCENES:
        case = BC.planted(ntracks, nimages, seed, lengths=(3, 4, 5), noise=0.5, num_loops=6, orthonormalise=1)["case"]
        r32, r64 = BC.adjust(case), BC.adjust(case, f64)
        P = r32["problem"]
        act = np.nonzero(P.active)[0]
        worst["cam"] = max(worst["cam"], float(np.abs(r32["cams"][P.free].astype(f64) - r64["cams"][P.free]).max()))
        worst["point"] = max(worst["point"], float(np.abs(r32["pts"][act].astype(f64) - r64["pts"][act]).max()))
        worst["rms"] = max(worst["rms"], abs(BC.pooled_rms(r32) - BC.pooled_rms(r64)))
        assert BC.pooled_rms(r32) < 2 * 0.5 * np.sqrt(2) and r32["kept"] >= 3
    print("planted with noise, |fp32 - fp64|: %s" % {k: "%.3g" % v for k, v in worst.items()})
    for k in MEASURED:
        assert worst[k] <= 2 * MEASURED[k], (k, worst[k])


# ---- against the parent's method

def test_joint_steps_against_alternation():
    """The scene of test_refine_cpu.test_alternation_with_triangulate: k joint steps beside k rounds of refine and
    triangulate (5 + 5 inner steps a round), both in the restatements, from the same cameras and triangulated points."""
    sc = RC.scene(RC.runs(150, 6, 67, lengths=(3, 4, 5)), 6, 67, noise=0.5, angle=0.02, shift=0.05, hold=(1,),
                  orthonormalise=1)
    case = sc["case"]

    def pooled(err):
        e = err[np.isfinite(err)].astype(f64)
        return float(np.sqrt((e ** 2).mean()))

    cam0 = np.asarray(case["cam"], f32)
    pts0, st0, err = RC.triangulate_under(case, cam0)
    alt, cam, pts, st = [pooled(err)], cam0, pts0, st0
    for _ in range(4):
        e = RC.expected_refine(RC.variant(case, points=pts, point_status=st))
        cam = e["cam_out"].view(f32).reshape(-1, 12)
        pts, st, err = RC.triangulate_under(case, cam)
        alt.append(pooled(err))
    joint = []
    for k in range(1, 5):
        bc = BC.bundle_case(RC.variant(case, points=pts0, point_status=st0), num_loops=k, cg_iters=10)
        e = BC.expected_bundle(bc)
        joint.append(BC.pooled_rms(e["res"]))
        assert e["cam_out"].reshape(-1, 12)[:2].tobytes() == cam0[:2].tobytes()          # the gauge stays
        assert len(e["res"]["problem"].slot) == int(np.isfinite(err).sum())             # the same observations
    print("pooled rms in px: start %.4g; alternation %s; joint %s" % (alt[0], ["%.4g" % v for v in alt[1:]],
                                                                     ["%.4g" % v for v in joint]))
    assert joint[3] < alt[4]
