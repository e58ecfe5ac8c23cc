"""misift_adjust_bundle_focal_batch without a GPU: bundle_focal_cases.adjust, the numpy float32 restatement of the
definition in include/misift.h, is pinned from both sides, as test_bundle_robust_cpu.py pins the robust call: the
library's host-only hook misift_test_adjust_bundle_focal, compiled from the functions the kernels run (bundle_core.hpp),
must give the same bytes on every case; and in float64 the same restatement is held to central differences of the
projection (the focal column), to numpy.linalg.solve on the full damped normal equations (focal columns included), and to
a dense-solve Levenberg-Marquardt of the same problem, written here, on planted scenes whose focal lengths are given 10 %
off.  test_gpu_bundle_focal.py then holds the device to the restatement byte for byte."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_focal_cases as BF
import bundle_robust_cases as BR
import refine_cases as RC
from test_fundamental_cpu import f32

f64 = np.float64
EINVAL = -1


def test_library_exports_the_call_the_hook_and_the_binding():
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_adjust_bundle_focal_batch", "misift_test_adjust_bundle_focal"):
        assert name in capi.SIGNATURES, name
        assert hasattr(L, name), name
    for a, b in (("misift_adjust_bundle_robust_batch", "misift_adjust_bundle_focal_batch"),
                 ("misift_test_adjust_bundle_robust", "misift_test_adjust_bundle_focal")):
        old, new = capi.SIGNATURES[a][1], capi.SIGNATURES[b][1]
        k = len(old) - 10                                        # the ten outputs are the tail of the robust call
        assert len(new) == len(old) + 4 and new[:k] == old[:k] and new[k + 2:k + 12] == old[k:]
    assert callable(capi.Context.adjust_bundle_focal_batch)
    assert capi.MAX_FOCAL_GROUPS == BF.MAX_GROUPS == 8
    assert (capi.FOCAL_REFINED, capi.FOCAL_NO_MEMBER, capi.FOCAL_NOT_REFINED) == (BF.REFINED, BF.NO_MEMBER, BF.NOT_REFINED)
    assert L.misift_adjust_bundle_focal_batch(None, 1, 1, None, None, None, None, None, 1, None, None, None, 0, None, 2,
                                              3, 0, 0, 1.0, 1e-3, 0, 1, 2.0, 0, None, None, None, None, None, None, None,
                                              None, None, None, None, None, None) == EINVAL


_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update(BF.cpu_cases())
    return _CASES


CASE_NAMES = ("2 images", "3 images", "8 images", "two groups", "some ungrouped", "empty groups", "8 groups", "members",
              "views", "hostile", "no track", "no loop", "cg 0", "cg 1", "huge lambda", "far off",
              "behind, rejected then kept", "scale not positive", "all -1", "ngroups 0", "two groups, huber",
              "outlier scene, huber", "two groups, geman-mcclure", "outlier scene, geman-mcclure")


def test_case_names():
    assert set(_cases()) == set(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_the_hook(name):
    case = _cases()[name]
    e = BF.expected_focal(case)
    BF.compare_all(BF.hook_bundle_focal(case), e, name)
    if name in ("two groups", "hostile"):
        BF.compare_all(BF.hook_bundle_focal(case, in_place=True), BR.in_place(e, case), name + ", in place")
        BF.compare_all(BF.hook_bundle_focal(case, weights=False), e, name + ", no obs_weight",
                       [k for k in BF.OUTPUTS if k != "obs_weight"])


def _focal(e):
    w = e["focal"][:3 * (len(e["focal"]) // 3)].reshape(-1, 3)
    return w[:, 0].copy().view(f32), w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)


def test_each_case_hits_what_it_is_built_for():
    c = _cases()
    E = {k: BF.expected_focal(c[k]) for k in ("2 images", "3 images", "two groups", "some ungrouped", "empty groups",
                                             "8 groups", "members", "views", "no loop", "cg 0", "huge lambda",
                                             "behind, rejected then kept", "scale not positive", "all -1", "ngroups 0")}
    res = {k: e["res"] for k, e in E.items()}
    assert len(res["2 images"]["problem"].free) == 0 and res["2 images"]["kept"] >= 1      # the focal and the points alone
    assert res["2 images"]["scale"][0] != 1 and len(res["3 images"]["problem"].free) == 1
    P, Gr = res["two groups"]["problem"], res["two groups"]["groups"]
    per_track = [set(Gr.mg[P.trk == t].tolist()) for t in np.nonzero(P.active)[0]]
    assert all(s == {0, 1} for s in per_track) and len(per_track) >= 30                    # every track in two groups
    P, Gr = res["some ungrouped"]["problem"], res["some ungrouped"]["groups"]
    per_track = [set(Gr.mg[P.trk == t].tolist()) for t in np.nonzero(P.active)[0]]
    assert {-1} in per_track and {-1, 0} in per_track                                      # a track with no grouped member
    scale, members, status = _focal(E["empty groups"])
    assert status.tolist() == [BF.REFINED, BF.NO_MEMBER, BF.NO_MEMBER, BF.REFINED] and members[1] == members[2] == 0
    assert scale[1] == scale[2] == 1.0 and members[0] > 0 and members[3] > 0
    assert "worse" in res["empty groups"]["trace"][:-1] and res["empty groups"]["trace"][-1] == "kept"
    K, Ko = np.asarray(c["empty groups"]["intrinsics"], f32), E["empty groups"]["intrinsics_out"].view(f32).reshape(-1, 4)
    assert Ko[3].tobytes() == K[3].tobytes() and (Ko[[0, 1, 2], 0] != K[[0, 1, 2], 0]).all()  # image 3: a group, no member
    assert len(res["8 groups"]["groups"].live) == BF.MAX_GROUPS == c["8 groups"]["ngroups"]
    assert E["members"]["cam_obs"].view(np.int32)[2:].tolist() == [5, 6, 7, 255, 256, 257, 513]
    P = res["views"]["problem"]
    assert sorted(set(P.tcount[:P.T].tolist())) == [2, 3, 7, 301]
    for k in ("no loop", "cg 0", "huge lambda"):
        assert (np.asarray(res[k]["scale"]) == 1).all(), k
    assert (_focal(E["no loop"])[2] == BF.NOT_REFINED).all() and (_focal(E["cg 0"])[2] == BF.REFINED).all()
    assert E["no loop"]["intrinsics_out"].tobytes() == np.ascontiguousarray(c["no loop"]["intrinsics"], f32).tobytes()
    assert res["huge lambda"]["trace"] == ["singular"] * 3
    assert res["behind, rejected then kept"]["trace"] == ["behind"] * 3 + ["worse", "kept"]
    r = res["scale not positive"]
    assert r["trace"] == ["kept"] + ["not finite"] * 4
    assert all(np.isfinite(s[0]) and s[0] <= 0 for s in r["strace"][1:]) and r["scale"][0] > 0   # only the scale is at fault
    for k in ("all -1", "ngroups 0"):
        assert not BF.grouped(c[k])
        assert E[k]["intrinsics_out"].tobytes() == np.ascontiguousarray(c[k]["intrinsics"], f32).tobytes()
    assert _focal(E["all -1"])[1].tolist() == [0, 0] and (_focal(E["all -1"])[2] == BF.NO_MEMBER).all()
    counts = E["members"]["res"]["groups"].count
    assert counts[0] == E["members"]["summary"].view(np.int32)[2] > 256


def test_without_a_grouped_image_the_restatement_is_the_robust_one():
    """The first identity through the hook: the ten shared outputs equal misift_test_adjust_bundle_robust byte for byte,
    and with loss 0 the restatement of the plain call."""
    for loss, cc in BF.LOSSES:
        base = BC.planted(40, 4, 1)["case"]
        for group, G in (([-1] * 4, 3), ([], 0)):
            case = BF.focal(base, group, G, loss=loss, loss_scale=cc)
            got, rob = BF.hook_bundle_focal(case), BR.hook_bundle_robust(case)
            for k in BR.OUTPUTS:
                assert got[k].tobytes() == rob[k].tobytes(), (loss, G, k)
            if loss == BF.NONE:
                BR.compare_all(got, BR.expected_plain_with_weights(base), "plain", BR.OUTPUTS)


# ---- float64

def _state64(case):
    P = BF.Problem(case, f64)
    return P, BF.Groups(case, P)


def test_focal_column_agrees_with_central_differences():
    for case in (BF.two_group_track_case(), BF.two_group_track_case(loss=BF.HUBER, loss_scale=2.0)):
        P, Gr = _state64(case)
        s = np.array([1.03, 0.96])
        _, f, _, f0, w = BF.jacobian(P, Gr, P.cams0, P.pts0, s, case["loss"], *(BR.scale_of(case, f64) if case["loss"] else (None, None)))
        for g in range(2):
            h = 1e-6
            sp, sm = s.copy(), s.copy()
            sp[g] += h
            sm[g] -= h
            up = RC.view(P.cams0[P.img].T, Gr.intrinsics(P, sp).T, P.pts0[P.trk], P.x, P.y, f64)
            um = RC.view(P.cams0[P.img].T, Gr.intrinsics(P, sm).T, P.pts0[P.trk], P.x, P.y, f64)
            num = np.stack([-(up[6] - um[6]), -(up[7] - um[7])], 1) / (2 * h)    # ru = x - u: du/ds = -dru/ds
            mine = np.where((Gr.mg == g)[:, None], f0, 0)
            assert np.abs(num - mine).max() <= 1e-6 * np.abs(f0).max(), g
        assert np.abs(f - np.sqrt(w)[:, None] * f0).max() <= 1e-12 * np.abs(f0).max()


def _dense_step(P, Gr, st, lam):
    """numpy.linalg.solve of the full damped normal equations of a step: (x (nf, 6), xg (G,), delta (T, 3))."""
    l, f = st["lin"], st["f"]
    nf, act = len(P.free), np.nonzero(P.active)[0]
    fpos = np.full(P.n, -1)
    fpos[P.free] = np.arange(nf)
    tpos = np.full(len(P.pts0), -1)
    tpos[act] = np.arange(len(act))
    G = Gr.G
    ncol = 6 * nf + G + 3 * len(act)
    J, r = np.zeros((2 * len(l), ncol)), np.zeros(2 * len(l))
    for m in range(len(l)):
        for h, (cam, pt, rr) in enumerate(((0, 12, 18), (6, 15, 19))):
            row = 2 * m + h
            if fpos[P.img[m]] >= 0:
                J[row, 6 * fpos[P.img[m]]:6 * fpos[P.img[m]] + 6] = l[m, cam:cam + 6]
            if Gr.mg[m] >= 0:
                J[row, 6 * nf + Gr.mg[m]] = f[m, h]
            t = 6 * nf + G + 3 * tpos[P.trk[m]]
            J[row, t:t + 3] = l[m, pt:pt + 3]
            r[row] = l[m, rr]
    A = J.T @ J
    dead = [6 * nf + g for g in range(G) if g not in Gr.live]
    A[np.diag_indices(ncol)] *= 1 + lam
    for d in dead:
        A[d, d] = 1.0
    sol = np.linalg.solve(A, J.T @ r)
    delta = np.zeros((len(P.pts0), 3))
    delta[act] = sol[6 * nf + G:].reshape(-1, 3)
    return sol[:6 * nf].reshape(-1, 6), sol[6 * nf:6 * nf + G], delta


@pytest.mark.parametrize("loss,cc", BF.LOSSES, ids=("none", "huber", "geman-mcclure"))
def test_one_step_with_cg_run_out_is_the_dense_solve(loss, cc):
    case = BF.focal(BC.planted(40, 4, 1)["case"], [0, 1, 0, -1], 2, loss=loss, loss_scale=cc, fscale=(1.05, 0.95))
    P, Gr = _state64(case)
    c, c2 = BR.scale_of(case, f64) if loss else (None, None)
    lam = f64(1e-3)
    st = BF.lm_step(P, Gr, P.cams0, P.pts0, np.ones(2), lam, 200, f64, loss, c, c2)
    assert not st["fail"]
    x, xg, delta = _dense_step(P, Gr, st, lam)
    assert np.abs(st["x"] - x).max() <= 1e-8 * np.abs(x).max()
    assert np.abs(st["xg"] - xg).max() <= 1e-8 * np.abs(xg).max() and np.abs(xg).min() > 1e-3
    assert np.abs(st["delta"] - delta).max() <= 1e-8 * np.abs(delta).max()


@pytest.mark.parametrize("loss,cc", BF.LOSSES, ids=("none", "huber", "geman-mcclure"))
def test_kept_steps_have_a_falling_cost(loss, cc):
    for dt in (f32, f64):
        res = BF.adjust(BF.alternating(BC.planted(60, 4, 2, num_loops=6)["case"], loss=loss, loss_scale=cc), dt)
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
    loss = case["loss"]
    c, c2 = BR.scale_of(case, f64) if loss else (None, None)
    cams, pts, s = P.cams0.copy(), P.pts0.copy(), np.ones(max(Gr.G, 1))
    cost = BF.costs(P, Gr, cams, pts, s, loss, c, c2)[4]
    lam = 1e-3
    for _ in range(case["num_loops"]):
        l, f, _, _, _ = BF.jacobian(P, Gr, cams, pts, s, loss, c, c2)
        x, xg, delta = _dense_step(P, Gr, dict(lin=l, f=f), lam)
        cams2, pts2, s2 = cams.copy(), pts + delta, s.copy()
        for fi, i in enumerate(P.free):
            cams2[i] = RC.update(cams[i], x[fi], f64)
        s2[Gr.live] = s[Gr.live] + xg[Gr.live]
        front, _, _, _, cc = BF.costs(P, Gr, cams2, pts2, s2, loss, c, c2)
        if front.all() and (s2 > 0).all() and cc < cost:
            cams, pts, s, cost, lam = cams2, pts2, s2, cc, max(lam / 10, 1e-7)
        else:
            lam *= 10
    sq = BF.costs(P, Gr, cams, pts, s, loss, c, c2)[1]
    return dict(scale=s, rms=float(np.sqrt(sq.sum() / len(sq))))


# MEASURED on the four scenes below (0.5 px noise, 8 steps, cg_iters 10), worst case: the float64 restatement against the
# dense-solve LM (the final scale, relative; the pooled rms, px), the float32 restatement against the float64 one (the
# same), and the final scale against the planted one.  Each test allows twice the figure.
MEASURED = {"scale vs dense": 1.27e-2, "rms vs dense": 7.51e-3, "scale f32 vs f64": 9.77e-4, "rms f32 vs f64": 1.73e-3,
            "scale vs planted": 1.34e-2}
SCENES = ((120, 8, 6, 1), (400, 24, 7, 1), (120, 8, 6, 2), (400, 24, 7, 2))


def _figures():
    worst = dict.fromkeys(MEASURED, 0.0)
    for ntracks, nimages, seed, groups in SCENES:
        sc = BF.recovery_scene(ntracks, nimages, seed, groups)
        case, planted = sc["case"], 1 / sc["fscale"]
        r64, r32, dense = BF.adjust(case, f64), BF.adjust(case, f32), _dense_lm(case)
        rob = BR.adjust(case, f64)
        fig = {"scale vs dense": np.abs(r64["scale"] / dense["scale"] - 1).max(),
               "rms vs dense": abs(BF.pooled_rms(r64) - dense["rms"]),
               "scale f32 vs f64": np.abs(r32["scale"].astype(f64) / r64["scale"] - 1).max(),
               "rms f32 vs f64": abs(BF.pooled_rms(r32) - BF.pooled_rms(r64)),
               "scale vs planted": np.abs(r64["scale"] / planted - 1).max()}
        print("scene %s: scale %s (planted %s, dense %s) rms %.4f (dense %.4f, robust call %.3f) %s" % (
            (ntracks, nimages, seed, groups), r64["scale"], planted, dense["scale"], BF.pooled_rms(r64), dense["rms"],
            BR.pooled_rms(rob), {k: float("%.3g" % v) for k, v in fig.items()}))
        assert BR.pooled_rms(rob) > BF.pooled_rms(r64) and BR.pooled_rms(rob) > BF.pooled_rms(r32)
        for k in worst:
            worst[k] = max(worst[k], float(fig[k]))
    return worst


def test_recovery_stays_within_twice_the_measured_figures_of_the_dense_yardstick():
    worst = _figures()
    print("worst", worst)
    for k in MEASURED:
        assert worst[k] <= 2 * MEASURED[k], (k, worst[k])


def test_without_noise_the_focal_ends_closer_to_the_planted_one_than_it_started():
    for ntracks, nimages, seed, groups in SCENES:
        sc = BF.recovery_scene(ntracks, nimages, seed, groups, noise=0.0)
        planted = 1 / sc["fscale"]
        for dt in (f32, f64):
            s = np.asarray(BF.adjust(sc["case"], dt)["scale"], f64)[:groups]
            assert (np.abs(s / planted - 1) < np.abs(1 / planted - 1)).all(), ((ntracks, nimages, seed, groups), dt, s)
