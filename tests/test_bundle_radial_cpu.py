"""misift_adjust_bundle_radial_batch and misift_undistort_obs_batch without a GPU: bundle_radial_cases.adjust, the numpy
float32 restatement of the definition in include/misift.h, is pinned from both sides, as test_bundle_focal_cpu.py pins the
focal call: the library's host-only hooks misift_test_adjust_bundle_radial and misift_test_undistort_obs, compiled from
the functions the kernels run (bundle_core.hpp), must give the same bytes on every case; and in float64 the same
restatement is held to central differences of the cost (the k and s components of the gradient among them), to
numpy.linalg.solve on the full damped normal equations (6n + 3T + 2G unknowns), and to a dense-solve
Levenberg-Marquardt of the same problem, written here, on scenes planted with the model itself.
test_gpu_bundle_radial.py then holds the device to the restatement byte for byte."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_focal_cases as BF
import bundle_radial_cases as BD
import bundle_robust_cases as BR
import refine_cases as RC
from test_fundamental_cpu import f32

f64 = np.float64
EINVAL = -1


def test_library_exports_the_calls_the_hooks_and_the_bindings():
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_adjust_bundle_radial_batch", "misift_test_adjust_bundle_radial", "misift_undistort_obs_batch",
                 "misift_test_undistort_obs"):
        assert name in capi.SIGNATURES, name
        assert hasattr(L, name), name
    for a, b in (("misift_adjust_bundle_focal_batch", "misift_adjust_bundle_radial_batch"),
                 ("misift_test_adjust_bundle_focal", "misift_test_adjust_bundle_radial")):
        old, new = capi.SIGNATURES[a][1], capi.SIGNATURES[b][1]
        k = len(old) - 12                                        # the twelve outputs are the tail of the focal call
        assert len(new) == len(old) + 3 and new[:k] == old[:k] and new[k + 2:k + 14] == old[k:]
    assert callable(capi.Context.adjust_bundle_radial_batch) and callable(capi.Context.undistort_obs_batch)
    assert capi.MAX_RADIAL_GROUPS == BD.MAX_GROUPS == capi.MAX_FOCAL_GROUPS
    assert (capi.RADIAL_REFINED, capi.RADIAL_NO_MEMBER, capi.RADIAL_NOT_REFINED, capi.RADIAL_HELD) == (
        BD.REFINED, BD.NO_MEMBER, BD.NOT_REFINED, BD.HELD)
    assert L.misift_adjust_bundle_radial_batch(None, 1, 1, None, None, None, None, None, 1, None, None, None, 0, None, 2,
                                               3, 0, 0, 1.0, 1e-3, 0, 1, 2.0, 0, None, None, None, *([None] * 13)) == EINVAL
    assert L.misift_undistort_obs_batch(None, 1, None, None, 1, None, 0, None, None, None) == EINVAL


_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update(BD.cpu_cases())
    return _CASES


CASE_NAMES = ("2 images", "3 images", "8 images", "two groups", "some ungrouped", "empty groups", "8 groups, mixed",
              "held group", "all held", "members", "views", "hostile", "hostile observations", "no track", "no loop", "cg 0",
              "cg 1", "huge lambda", "far off", "behind, rejected then kept", "k not finite", "two groups, huber", "outlier scene, huber",
              "two groups, geman-mcclure", "outlier scene, geman-mcclure", "ngroups 0", "all -1", "nothing radial",
              "no lists")


def test_case_names():
    assert set(_cases()) == set(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_the_hook(name):
    case = _cases()[name]
    e = BD.expected_radial(case)
    BD.compare_all(BD.hook_bundle_radial(case), e, name)
    if name in ("two groups", "hostile"):
        BD.compare_all(BD.hook_bundle_radial(case, in_place=True), BR.in_place(e, case), name + ", in place")
        BD.compare_all(BD.hook_bundle_radial(case, weights=False), e, name + ", no obs_weight",
                       [k for k in BD.OUTPUTS if k != "obs_weight"])


FOCAL_NAMES = tuple(BF.cpu_cases())


@pytest.mark.parametrize("loss,cc", BD.LOSSES, ids=("none", "huber", "geman-mcclure"))
@pytest.mark.parametrize("name", FOCAL_NAMES)
def test_the_focal_cases_with_radial_on_equal_the_hook(name, loss, cc):
    case = BD.radial(dict(BF.cpu_cases()[name], loss=loss, loss_scale=cc), True)
    BD.compare_all(BD.hook_bundle_radial(case), BD.expected_radial(case), (name, loss))


def _radial(e):
    w = e["radial_out"][:3 * (len(e["radial_out"]) // 3)].reshape(-1, 3)
    return w[:, 0].copy().view(f32), w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)


def test_each_case_hits_what_it_is_built_for():
    c = _cases()
    E = {k: BD.expected_radial(c[k]) for k in ("2 images", "3 images", "two groups", "some ungrouped", "empty groups",
                                              "8 groups, mixed", "held group", "all held", "members", "views", "no loop",
                                              "cg 0", "hostile observations", "behind, rejected then kept", "all -1")}
    res = {k: e["res"] for k, e in E.items()}
    assert len(res["2 images"]["problem"].free) == 0 and res["2 images"]["kept"] >= 1   # k, s and the points alone
    assert res["2 images"]["coef"][0] != 0 and len(res["3 images"]["problem"].free) == 1
    P, Gr = res["two groups"]["problem"], res["two groups"]["groups"]
    per_track = [set(Gr.mg[P.trk == t].tolist()) for t in np.nonzero(P.active)[0]]
    assert all(s == {0, 1} for s in per_track) and len(per_track) >= 30                 # every track in two groups
    P, Gr = res["some ungrouped"]["problem"], res["some ungrouped"]["groups"]
    assert {-1} in [set(Gr.mg[P.trk == t].tolist()) for t in np.nonzero(P.active)[0]]   # a track with no grouped member
    k, members, status = _radial(E["empty groups"])
    assert status.tolist() == [BD.REFINED, BD.NO_MEMBER, BD.NO_MEMBER, BD.HELD] and members[1] == members[2] == 0
    assert k[0] != 0 and k[1] == f32(0.01) and k[2] == 0 and k[3] == f32(0.02) and members[3] > 0
    assert "worse" in res["empty groups"]["trace"][:-1] and res["empty groups"]["trace"][-1] == "kept"   # rejected, then kept
    k, members, status = _radial(E["8 groups, mixed"])
    assert status.tolist() == [0, 3, 0, 0, 3, 0, 0, 0] and (k[[1, 4]] == 0).all() and (k[[0, 2, 3, 5, 6, 7]] != 0).all()
    k, _, status = _radial(E["held group"])
    assert status.tolist() == [BD.HELD, BD.REFINED] and k[0] == c["held group"]["k0"][0] != 0 and k[1] != 0
    k, _, status = _radial(E["all held"])
    assert status.tolist() == [BD.HELD] and k[0] == c["all held"]["k0"][0] and res["all held"]["kept"] >= 1
    assert BD.radial_on(c["all held"]) and res["all held"]["scale"][0] != 1
    assert E["members"]["cam_obs"].view(np.int32)[2:].tolist() == [5, 6, 7, 255, 256, 257, 513]
    P = res["views"]["problem"]
    assert sorted(set(P.tcount[:P.T].tolist())) == [2, 3, 7, 301]
    assert (_radial(E["no loop"])[2] == BD.NOT_REFINED).all() and (_radial(E["cg 0"])[2] == BD.REFINED).all()
    assert _radial(E["no loop"])[0][0] == 0 and _radial(E["cg 0"])[0][0] == 0
    r = res["hostile observations"]
    P = r["problem"]
    assert 5 in P.slot and 40 not in P.slot and 77 not in P.slot and 120 not in P.slot and r["kept"] >= 1
    assert res["behind, rejected then kept"]["trace"] == ["kept"] + ["behind"] * 3 + ["kept"]
    assert len(res["behind, rejected then kept"]["groups"].klive) == 1
    assert _radial(E["all -1"])[1].tolist() == [0, 0] and (_radial(E["all -1"])[2] == BD.NO_MEMBER).all()


def test_a_trial_coefficient_that_is_not_finite_turns_the_step_away():
    """"k not finite": the steps that are turned away are turned away by the coefficient alone.  Their trial k_g is
    infinite while the trial s_g is finite and positive and every trial point is finite (no camera is free), and a step
    whose k_g + x_k stays below FLT_MAX is kept."""
    case = _cases()["k not finite"]
    steps = []
    with np.errstate(all="ignore"):
        res = BD.adjust(case, f32, steps=steps)
    assert res["trace"] == ["not finite", "not finite", "kept", "not finite", "kept", "not finite"]
    P, Gr = res["problem"], res["groups"]
    assert len(P.free) == 0 and Gr.live == [0] and Gr.klive == [0] and len(P.slot) == 12
    act = np.nonzero(P.active)[0]
    for why, st in zip(res["trace"], steps):
        assert not st["fail"] and np.isfinite(st["pts"][act]).all() and np.isfinite(st["xk"][0])
        assert np.isfinite(st["s"][0]) and 0.8 < st["s"][0] < 1
        assert np.isinf(st["k"][0]) == (why == "not finite") and st["k"][0] > 0
    assert np.isfinite(res["coef"][0]) and res["coef"][0] > f32(case["k0"][0]) and res["kept"] == 2


@pytest.mark.parametrize("name", ("ngroups 0", "all -1", "nothing radial", "no lists"))
def test_with_nothing_radial_the_hook_gives_the_focal_hooks_bytes(name):
    case = _cases()[name]
    assert not BD.radial_on(case)
    got, foc = BD.hook_bundle_radial(case), BF.hook_bundle_focal(case)
    for k in BF.OUTPUTS:
        assert got[k].tobytes() == foc[k].tobytes(), k
    _, _, status = _radial(got)
    want = BD.HELD if name in ("nothing radial", "no lists") else BD.NO_MEMBER
    assert (status == want).all() and len(status) == case["ngroups"]


def test_argument_errors_of_the_hook():
    from cudasift_amd import capi
    base = _cases()["two groups"]

    def rc(case, **ptr):
        a = BR.hook_args(case)
        out = {k: np.zeros(m, np.uint32) for k, m in BD.sizes(case).items()}
        p = {k: out[k].ctypes.data for k in BD.OUTPUTS}
        group, flags, k0 = BD.host_lists(case)
        lists = dict(radial=flags.ctypes.data, k0=k0.ctypes.data)
        for k, v in ptr.items():
            (lists if k in lists else p)[k] = v
        return capi.lib().misift_test_adjust_bundle_radial(
            case["max_tracks"], case["max_obs"], a["offs"].ctypes.data, a["obs"].ctypes.data, a["summ"].ctypes.data,
            a["pts"].ctypes.data, a["st"].ctypes.data, case["nimages"], a["cam"].ctypes.data, a["pair"].ctypes.data,
            a["K"].ctypes.data, 0, None, 2, 3, 1, 1, 10.0, 1e-3, 0, 0, 0.0, case["ngroups"], group.ctypes.data,
            lists["radial"], lists["k0"], *[p[k] for k in BD.OUTPUTS])
    assert rc(base) == 0
    assert rc(BD.radial(base, [1, 2])) == EINVAL and rc(BD.radial(base, [-1, 0])) == EINVAL
    assert rc(BD.radial(base, [1, 1], [0.0, np.nan])) == EINVAL and rc(BD.radial(base, [1, 1], [np.inf, 0.0])) == EINVAL
    assert rc(base, radial=None) == EINVAL and rc(base, k0=None) == EINVAL and rc(base, radial=None, k0=None) == 0
    assert rc(base, radial_out=None) == EINVAL and rc(base, focal=None) == EINVAL and rc(base, intrinsics_out=None) == EINVAL


# ---- float64

def _state64(case):
    P = BD.problem(case, f64)
    return P, BD.RGroups(case, P)


def _loss_args(case):
    return (case["loss"],) + (BR.scale_of(case, f64) if case["loss"] else (None, None))


GRADIENT_CASES = (("none", BD.NONE, 0.0), ("huber", BD.HUBER, 2.0), ("geman-mcclure", BD.GEMAN_MCCLURE, 4.0))


@pytest.mark.parametrize("tag,loss,cc", GRADIENT_CASES, ids=[g[0] for g in GRADIENT_CASES])
def test_gradient_agrees_with_central_differences_of_the_cost(tag, loss, cc):
    """J^T r over every kind of unknown (a camera's six, a point's three, s_g, k_g) against central differences of
    half the sum of rho: a wrong sign of the radial column fails here."""
    case = BD.alternating(BC.planted(40, 4, 1, lengths=(3, 4))["case"], loss=loss, loss_scale=cc)
    P, Gr = _state64(case)
    la = _loss_args(case)
    s, k = np.array([1.03, 0.96]), np.array([-0.05, 0.03])
    cams, pts = P.cams0, P.pts0
    l, f, rk, _, _, _, _ = BD.jacobian(P, Gr, cams, pts, s, k, *la)
    half = lambda cams_, pts_, s_, k_: 0.5 * BD.costs(P, Gr, cams_, pts_, s_, k_, *la)[2].sum()
    h = 1e-6
    for g in range(2):
        for vec, col, name in ((s, f, "s"), (k, rk, "k")):
            up, dn = vec.copy(), vec.copy()
            up[g] += h
            dn[g] -= h
            num = ((half(cams, pts, up, k) - half(cams, pts, dn, k)) if name == "s" else
                   (half(cams, pts, s, up) - half(cams, pts, s, dn))) / (2 * h)
            sel = Gr.mg == g
            mine = -(col[sel, 0] * l[sel, 18] + col[sel, 1] * l[sel, 19]).sum()     # d(half)/dtheta = -J^T r
            assert abs(num - mine) <= 1e-5 * max(abs(mine), 1.0), (name, g, num, mine)
            assert abs(mine) > 1e-3
    i = int(P.free[0])
    m = P.of_image[i]
    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        cp, cm = cams.copy(), cams.copy()
        cp[i], cm[i] = RC.update(cams[i], d, f64), RC.update(cams[i], -d, f64)
        num = (half(cp, pts, s, k) - half(cm, pts, s, k)) / (2 * h)
        mine = -(l[m, j] * l[m, 18] + l[m, 6 + j] * l[m, 19]).sum()
        assert abs(num - mine) <= 1e-5 * max(abs(mine), 1.0), ("camera", j, num, mine)
    t = int(np.nonzero(P.active)[0][0])
    m = np.nonzero(P.trk == t)[0]
    for j in range(3):
        pp, pm = pts.copy(), pts.copy()
        pp[t, j] += h
        pm[t, j] -= h
        num = (half(cams, pp, s, k) - half(cams, pm, s, k)) / (2 * h)
        mine = -(l[m, 12 + j] * l[m, 18] + l[m, 15 + j] * l[m, 19]).sum()
        assert abs(num - mine) <= 1e-5 * max(abs(mine), 1.0), ("point", j, num, mine)


def _dense_step(P, Gr, st, lam):
    """numpy.linalg.solve of the full damped normal equations of a step, 6n + 3T + 2G unknowns:
    (x (nf, 6), xg (G,), xk (G,), delta (T, 3))."""
    l, f, rk = st["lin"], st["f"], st["rk"]
    nf, act = len(P.free), np.nonzero(P.active)[0]
    fpos = np.full(P.n, -1)
    fpos[P.free] = np.arange(nf)
    tpos = np.full(len(P.pts0), -1)
    tpos[act] = np.arange(len(act))
    G = Gr.G
    ncol = 6 * nf + 2 * G + 3 * len(act)
    J, r = np.zeros((2 * len(l), ncol)), np.zeros(2 * len(l))
    for m in range(len(l)):
        for h, (cam, pt, rr) in enumerate(((0, 12, 18), (6, 15, 19))):
            row = 2 * m + h
            if fpos[P.img[m]] >= 0:
                J[row, 6 * fpos[P.img[m]]:6 * fpos[P.img[m]] + 6] = l[m, cam:cam + 6]
            if Gr.mg[m] >= 0:
                J[row, 6 * nf + Gr.mg[m]] = f[m, h]
                J[row, 6 * nf + G + Gr.mg[m]] = rk[m, h]
            t = 6 * nf + 2 * G + 3 * tpos[P.trk[m]]
            J[row, t:t + 3] = l[m, pt:pt + 3]
            r[row] = l[m, rr]
    A = J.T @ J
    A[np.diag_indices(ncol)] *= 1 + lam
    for g in range(G):
        if g not in Gr.live:
            A[6 * nf + g, 6 * nf + g] = 1.0
        if g not in Gr.klive:
            A[6 * nf + G + g, 6 * nf + G + g] = 1.0
    sol = np.linalg.solve(A, J.T @ r)
    delta = np.zeros((len(P.pts0), 3))
    delta[act] = sol[6 * nf + 2 * G:].reshape(-1, 3)
    return sol[:6 * nf].reshape(-1, 6), sol[6 * nf:6 * nf + G], sol[6 * nf + G:6 * nf + 2 * G], delta


@pytest.mark.parametrize("loss,cc", BD.LOSSES, ids=("none", "huber", "geman-mcclure"))
def test_one_step_with_cg_run_out_is_the_dense_solve(loss, cc):
    """A missing cross term (U_fk, U_ck, wk in the gather) fails here."""
    base = BF.focal(BC.planted(40, 4, 1)["case"], [0, 1, 0, -1], 2, loss=loss, loss_scale=cc, fscale=(1.05, 0.95))
    case = BD.radial(BD.distort_obs(base, [BD.corner_k(base, -0.1), BD.corner_k(base, 0.06)]), True)
    P, Gr = _state64(case)
    lam = f64(1e-3)
    st = BD.lm_step(P, Gr, P.cams0, P.pts0, np.ones(2), np.zeros(2), lam, 300, f64, *_loss_args(case))
    assert not st["fail"]
    x, xg, xk, delta = _dense_step(P, Gr, st, lam)
    assert np.abs(st["x"] - x).max() <= 1e-7 * np.abs(x).max()
    assert np.abs(st["xg"] - xg).max() <= 1e-7 * np.abs(xg).max() and np.abs(xg).min() > 1e-3
    assert np.abs(st["xk"] - xk).max() <= 1e-7 * np.abs(xk).max() and np.abs(xk).min() > 1e-3
    assert np.abs(st["delta"] - delta).max() <= 1e-7 * np.abs(delta).max()


@pytest.mark.parametrize("loss,cc", BD.LOSSES, ids=("none", "huber", "geman-mcclure"))
def test_kept_steps_have_a_falling_cost(loss, cc):
    for dt in (f32, f64):
        res = BD.adjust(BD.alternating(BC.planted(60, 4, 2, num_loops=6)["case"], loss=loss, loss_scale=cc), dt)
        cost = res["cost"][0]
        assert res["kept"] >= 2
        for c2, _, kept, _ in res["history"]:
            if kept:
                assert c2 < cost
                cost = c2
        assert cost == res["cost"][1]


# ---- recovery, against a dense-solve LM in float64

def _dense_lm(case):
    """Levenberg-Marquardt on the same problem with every step solved exactly: the yardstick.  The sets, the Jacobian and
    the cost are the restatement's in float64; the step is numpy.linalg.solve, the damping schedule the call's."""
    P, Gr = _state64(case)
    la = _loss_args(case)
    G1 = max(Gr.G, 1)
    cams, pts, s, k = P.cams0.copy(), P.pts0.copy(), np.ones(G1), BD.flags_of(case)[1].astype(f64)
    cost = BD.costs(P, Gr, cams, pts, s, k, *la)[4]
    lam = 1e-3
    for _ in range(case["num_loops"]):
        l, f, rk, _, _, _, _ = BD.jacobian(P, Gr, cams, pts, s, k, *la)
        x, xg, xk, delta = _dense_step(P, Gr, dict(lin=l, f=f, rk=rk), lam)
        cams2, pts2, s2, k2 = cams.copy(), pts + delta, s.copy(), k.copy()
        for fi, i in enumerate(P.free):
            cams2[i] = RC.update(cams[i], x[fi], f64)
        s2[Gr.live] = s[Gr.live] + xg[Gr.live]
        k2[Gr.klive] = k[Gr.klive] + xk[Gr.klive]
        front, _, _, _, cc = BD.costs(P, Gr, cams2, pts2, s2, k2, *la)
        if front.all() and (s2 > 0).all() and cc < cost:
            cams, pts, s, k, cost, lam = cams2, pts2, s2, k2, cc, max(lam / 10, 1e-7)
        else:
            lam *= 10
    sq = BD.costs(P, Gr, cams, pts, s, k, *la)[1]
    return dict(scale=s, coef=k, rms=float(np.sqrt(sq.sum() / len(sq))))


# MEASURED on the four scenes below (0.5 px noise, 8 steps, cg_iters 10), worst case.  k is compared in units of the
# planted coefficient of its group (relative), s_g relative, the pooled rms in px: the float64 restatement against the
# dense-solve LM, the float32 restatement against the float64 one, and the float64 restatement against the planted
# values.  Each test allows four times the figure.
MEASURED = {"k vs dense": 1.27e-2, "scale vs dense": 1.26e-2, "rms vs dense": 7.99e-3, "k f32 vs f64": 3.12e-2,
            "scale f32 vs f64": 1.02e-3, "rms f32 vs f64": 1.20e-3, "k vs planted": 7.46e-2, "scale vs planted": 1.42e-2}
# The same run with the 2 x 2 Schur block as the preconditioner of a group's two scalars ends at 2.84e-2 (k) and 1.79e-2
# (s_g) of the dense LM, no closer than the two diagonals: the call uses the diagonals.
SCENES = ((120, 8, 6, 1), (400, 24, 7, 1), (120, 8, 6, 2), (400, 24, 7, 2))
_FIGURES = {}


def _figures():
    if _FIGURES:
        return _FIGURES
    worst = dict.fromkeys(MEASURED, 0.0)
    for ntracks, nimages, seed, groups in SCENES:
        sc = BD.recovery_scene(ntracks, nimages, seed, groups)
        case, ps, pk = sc["case"], 1 / sc["fscale"], sc["k"]
        r64, r32, dense = BD.adjust(case, f64), BD.adjust(case, f32), _dense_lm(case)
        blk = BD.adjust(case, f64, block=True)
        foc64, foc32 = BF.adjust(sc["focal_case"], f64), BF.adjust(sc["focal_case"], f32)
        fig = {"k vs dense": np.abs((r64["coef"] - dense["coef"]) / pk).max(),
               "scale vs dense": np.abs(r64["scale"] / dense["scale"] - 1).max(),
               "rms vs dense": abs(BD.pooled_rms(r64) - dense["rms"]),
               "k f32 vs f64": np.abs((r32["coef"].astype(f64) - r64["coef"]) / pk).max(),
               "scale f32 vs f64": np.abs(r32["scale"].astype(f64) / r64["scale"] - 1).max(),
               "rms f32 vs f64": abs(BD.pooled_rms(r32) - BD.pooled_rms(r64)),
               "k vs planted": np.abs((r64["coef"] - pk) / pk).max(),
               "scale vs planted": np.abs(r64["scale"] / ps - 1).max()}
        print("scene %s: k %s (planted %s, dense %s, 2x2 block %s) scale %s (planted %s, dense %s, 2x2 block %s) rms %.4f "
              "(dense %.4f, 2x2 block %.4f, focal call %.3f) %s" % (
                  (ntracks, nimages, seed, groups), r64["coef"], pk, dense["coef"], blk["coef"], r64["scale"], ps,
                  dense["scale"], blk["scale"], BD.pooled_rms(r64), dense["rms"], BD.pooled_rms(blk), BF.pooled_rms(foc64),
                  {k: float("%.3g" % v) for k, v in fig.items()}))
        print("   2x2 block against dense: k %.3g, scale %.3g" % (np.abs((blk["coef"] - dense["coef"]) / pk).max(),
                                                                  np.abs(blk["scale"] / dense["scale"] - 1).max()))
        # the condition of the issue: the focal call must end above the radial call, or the scene shows nothing
        assert BF.pooled_rms(foc64) > BD.pooled_rms(r64) and BF.pooled_rms(foc32) > BD.pooled_rms(r32)
        for k in worst:
            worst[k] = max(worst[k], float(fig[k]))
    _FIGURES.update(worst)
    return _FIGURES


def test_recovery_stays_within_four_times_the_measured_figures():
    worst = _figures()
    print("worst", worst)
    for k in MEASURED:
        assert worst[k] <= 4 * MEASURED[k], (k, worst[k])


def test_a_scene_planted_with_the_forward_model_ends_below_the_focal_call():
    """x_d = x_u * (1 + k r_u^2): the one-parameter inverse model leaves a remainder, recorded in include/misift.h."""
    sc = BD.recovery_scene(120, 8, 6, 1, forward=True)
    r64, foc = BD.adjust(sc["case"], f64), BF.adjust(sc["focal_case"], f64)
    print("forward model: rms %.4f px, focal call %.4f px, k %s against the forward %s" % (
        BD.pooled_rms(r64), BF.pooled_rms(foc), r64["coef"], sc["k"]))
    assert BD.pooled_rms(r64) < BF.pooled_rms(foc)
    assert np.sign(r64["coef"][0]) == -np.sign(sc["k"][0])


# ---- misift_undistort_obs_batch

def _words(kg, status=0):
    w = np.zeros((len(kg), 3), np.uint32)
    w[:, 0] = np.asarray(kg, f32).view(np.uint32)
    w[:, 2] = status
    return w.reshape(-1)


UNDISTORT_COUNTS = (0, 1, 63, 64, 65, 257, 10 ** 9, -3)


@pytest.mark.parametrize("O", UNDISTORT_COUNTS)
def test_undistort_hook_equals_the_restatement(O):
    case = BD.undistort_case(O)
    words = _words([0.07, -0.11, 0.0], BD.HELD)
    for in_place in (False, True):
        got = BD.hook_undistort(case, case["obs"], words, in_place)
        assert got.tobytes() == BD.expected_undistort(case, case["obs"], words, in_place).tobytes(), (O, in_place)


def test_undistort_with_k_zero_is_the_identity_bit_for_bit():
    case = BD.undistort_case(257)
    got = BD.hook_undistort(case, case["obs"], _words([0.0, 0.0, 0.0]))
    _, O = RC.counts(case)
    src = np.ascontiguousarray(case["obs"][:O])
    finite = np.isfinite(src["xpos"]) & np.isfinite(src["ypos"])                # slot 1 has a NaN: its y' is NaN too
    assert finite.sum() == O - 1 and got[:O][finite].tobytes() == src[finite].tobytes()
    assert np.isnan(got["xpos"][1]) and np.isnan(got["ypos"][1])
    moved = BD.hook_undistort(case, case["obs"], _words([0.07, -0.11, 0.0]))
    fr = case["obs"]["frame"][:O]
    ok = (fr >= 0) & (fr < case["nimages"])
    g = np.where(ok, np.asarray(case["group"])[np.where(ok, fr, 0)], -1)
    same = (moved["xpos"][:O].view(np.uint32) == case["obs"]["xpos"][:O].view(np.uint32))
    assert same[g < 0].all() and same[g == 2].all() and not same[(g == 0) | (g == 1)].all()
    assert (moved["frame"][:O] == fr).all() and (moved["record"][:O] == case["obs"]["record"][:O]).all()


def test_after_undistort_the_plain_call_reports_the_cost_the_radial_call_ended_at():
    """adjust -> undistort -> misift_test_adjust_bundle with num_loops 0 under d_intrinsics_out: the plain cost of the
    undistorted list under the final state.  The two differ by the fp32 rounding of x' alone: the radial call forms
    ru = x' - u from x' in registers, the plain call from x' rounded into the list, which is the same float, and
    fx*s_g comes back rounded from d_intrinsics_out as the radial call rounds it; so the costs agree to the bit unless
    the member sets differ.  Measured: 0 difference in every word; asserted: 4 ulp of the cost."""
    sc = BD.recovery_scene(120, 8, 6, 2)
    case = sc["case"]
    got = BD.hook_bundle_radial(case)
    obs2 = BD.hook_undistort(case, case["obs"], got["radial_out"])
    plain = BC.bundle_case(dict(case, obs=obs2, cam=got["cam_out"].view(f32).reshape(-1, 12),
                                points=got["points_out"].view(f32).reshape(-1, 4),
                                intrinsics=got["intrinsics_out"].view(f32).reshape(-1, 4)), num_loops=0, hold=case["hold"])
    for k in ("group", "ngroups", "radial", "k0", "loss", "loss_scale"):
        plain.pop(k)
    out = BC.hook_bundle(plain)
    end, again = got["cost"].view(f32)[1], out["cost"].view(f32)[0]
    print("radial call ended at %r, plain call on the undistorted list starts at %r" % (end, again))
    assert (out["cam_obs"] == got["cam_obs"]).all()
    assert abs(f64(end) - f64(again)) <= 4 * np.spacing(end)
