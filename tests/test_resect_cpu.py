"""misift_resect_cameras_batch without a GPU: resect_cases.expected_resect, the numpy float32 restatement of the
definition in include/misift.h, which tests/test_gpu_resect.py holds the device to byte for byte.  Here the restatement
is pinned from both sides: the library's host-only hooks misift_test_resect_samples and misift_test_resect_solve,
compiled from the functions the kernels run, must equal it byte for byte, and on planted scenes its answers are held to
the same algorithm in float64 and to the planted cameras.  The premises of the GPU cases are asserted here too."""
import numpy as np
import pytest

import pose_cases as PC
import refine_cases as RC
import resect_cases as C
from test_fundamental_cpu import f32

K = PC.K_A


def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, the argument checks that need
    no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_resect_cameras_batch", "misift_test_resect_samples", "misift_test_resect_solve"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "resect_cameras_batch") and capi.CAM_RESECTED == C.RESECTED == -3
    assert L.misift_resect_cameras_batch(None, 1, 1, None, None, None, None, None, 1, None, 0, None, None, 6, 1, 1.0, 6, 0,
                                         0, None, None, None, None, None, None, None) == -1  # MISIFT_EINVAL
    out = np.zeros(6, np.int32)
    assert L.misift_test_resect_samples(1, 5, 1, out.ctypes.data) == -1
    assert L.misift_test_resect_samples(1, 6, -1, out.ctypes.data) == -1
    assert L.misift_test_resect_samples(1, 6, 1, None) == -1
    assert L.misift_test_resect_samples(1, 6, 0, None) == 0
    assert L.misift_test_resect_solve(None, None, None, None) == -1


@pytest.mark.parametrize("seed,n,num_loops", [(1, 6, 200), (0, 7, 100), (12345, 40, 1024), (2 ** 32 - 1, 2000, 300),
                                              (77, 2 ** 31 - 1, 50)])
def test_samples_equal_the_hook(seed, n, num_loops):
    want = C.draw6(seed, n, num_loops)
    assert (C.hook_samples(seed, n, num_loops) == want).all()
    assert (np.sort(want, 1)[:, 1:] != np.sort(want, 1)[:, :-1]).all() and want.min() >= 0 and want.max() < n
    if n == 6:
        assert (np.sort(want, 1) == np.arange(6)).all()          # every redraw loop has run


def _same_solve(xy, X, k4=K):
    """The hook equals the restatement byte for byte on every sample; returns (cams, valid)."""
    xy, X = np.asarray(xy, f32).reshape(-1, 6, 2), np.asarray(X, f32).reshape(-1, 6, 3)
    cams, valid = C.solve6(xy, X, k4)
    for i in range(len(xy)):
        h, v = C.hook_solve(xy[i], X[i], k4)
        assert v == int(valid[i]) and h.tobytes() == cams[i].tobytes(), (i, v, valid[i], h, cams[i])
    assert (cams[~valid] == 0).all() and np.isfinite(cams).all()
    return cams, valid


def _samples(sc, image, seed, num):
    slots, X, xy = RC.image_candidates(sc["case"], image)
    pos = C.draw6(seed, len(slots), num)
    return xy[pos], X[pos]


def test_solve_on_exact_and_noisy_samples():
    for noise, k4 in ((0.0, PC.K_A), (0.5, PC.K_B), (30.0, PC.K_A)):
        sc = C.planted((60, 60), 80, wrong=0.0, noise=noise)
        xy, X = _samples(sc, 0 if k4 == PC.K_A else 1, 3, 150)
        cams, valid = _same_solve(xy, X, k4)
        assert valid.all()
        R = cams[:, :9].reshape(-1, 3, 3).astype(np.float64)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5 and (np.linalg.det(R) > 0.99).all()


def test_solve_on_degenerate_samples():
    """Coplanar points (exactly: a zero pivot), duplicate points, one point six times, a NaN or an inf anywhere, huge and
    tiny coordinates: the hook and the restatement agree, and what must be invalid is."""
    xy, X = _samples(C.planted((60,), 81, wrong=0.0, noise=0.0), 0, 4, 40)
    plane = X.copy()
    plane[:, :, 2] = 4.0
    _, valid = _same_solve(xy, plane)
    assert not valid.any()
    tilted = X.copy()
    tilted[:, :, 2] = 0.25 * X[:, :, 0] - 0.5 * X[:, :, 1] + 6          # coplanar but for the rounding
    _same_solve(xy, tilted)
    dup = X.copy()
    dup[:, 3] = dup[:, 1]
    dupxy = xy.copy()
    dupxy[:, 3] = dupxy[:, 1]
    _same_solve(dupxy, dup)
    one = np.repeat(X[:, :1], 6, 1)
    _, valid = _same_solve(xy, one)
    assert not valid.any()
    for bad in (np.nan, np.inf, -np.inf):
        for at in range(6):
            a, b = xy[:5].copy(), X[:5].copy()
            a[0, at, 0], a[1, at, 1], b[2, at, 0], b[3, at, 1], b[4, at, 2] = (bad,) * 5
            _, valid = _same_solve(a, b)
            assert valid.tolist() == [False, at == 5, False, False, False], (bad, at)    # y of point 5 has no row
    with np.errstate(over="ignore"):
        for s in (1e-30, 1e-22, 1e-12, 1e-3, 1e3, 1e12, 1e18, 1e19, 1e30, 3e38):
            _same_solve(xy[:12], X[:12] * f32(s))
            _same_solve(xy[:12] * f32(s), X[:12])
    _, valid = _same_solve(xy[:12], X[:12] * f32(1e3))           # a scene in other units is the same problem
    assert valid.all()
    for k4 in ((1e-20, 1e20, 0.0, 0.0), (3e38, 3e38, -3e38, 3e38), (1e-38, 1e-38, 1e30, -1e30)):
        _same_solve(xy[:12], X[:12], k4)


def test_solve_against_float64_on_exact_samples():
    """The float32 solve against the same algorithm in float64 on exact samples (no noise; the points and positions as
    float32 holds them).  Measured over the 300 samples below: the largest deviation of an entry is 6.6e-4 in R and
    5.6e-3 in t, on the worst-conditioned sample; the median over the samples 9.3e-7 and 7.9e-6.  Asserted: four times
    each.  The float64 solve itself lies within 1.9e-2 of the planted camera on the worst sample (the inputs are rounded
    to float32), 1.4e-5 in the median."""
    worst, med = np.zeros(2), np.zeros(2)
    for seed in (81, 82, 83):
        sc = C.planted((60,), seed, wrong=0.0, noise=0.0)
        xy, X = _samples(sc, 0, seed, 100)
        c32, v32 = C.solve6(xy, X, K)
        c64, v64 = C.solve6(xy, X, K, np.float64)
        assert v32.all() and v64.all()
        d = np.abs(c32 - c64)
        dev = np.array([d[:, :9].max(1), d[:, 9:].max(1)])
        worst, med = np.maximum(worst, dev.max(1)), np.maximum(med, np.median(dev, 1))
        truth = np.abs(c64 - sc["true"][0][None]).max(1)
        print("seed %d: R %.3g (median %.3g), t %.3g (median %.3g); float64 to the planted camera %.3g (median %.3g)" % (
            seed, dev[0].max(), np.median(dev[0]), dev[1].max(), np.median(dev[1]), truth.max(), np.median(truth)))
        assert truth.max() < 4 * 1.9e-2 and np.median(truth) < 4 * 1.4e-5
    assert worst[0] < 4 * 6.6e-4 and worst[1] < 4 * 5.6e-3, worst
    assert med[0] < 4 * 9.3e-7 and med[1] < 4 * 7.9e-6, med


QUALITY_SEEDS = (91, 92, 93, 94)
QUALITY_COUNTS = (40, 400, 2000)


def _picked(sc, i, seed, dt=f32):
    slots, X, xy = RC.image_candidates(sc["case"], i)
    k = sc["case"]["intrinsics"][i]
    s = C.search(seed, k, X, xy, 1024, 4.0, dt)
    good = np.isin(slots, sc["good"][i])
    cam = s["cams"][s["index"]]
    return s, cam, C.count_inliers(cam[None], k, X[good], xy[good], 4.0, dt)[0] / good.sum(), (slots, X, xy, k)


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_search_quality_on_planted_scenes(seed):
    """40, 400 and 2000 candidates, a quarter wrong, 0.5 px noise, 1024 hypotheses, 4 px: the picked camera collects at
    least 90 % of the planted inliers, in float32 and in the float64 form of the algorithm."""
    sc = C.planted(QUALITY_COUNTS, seed)
    for i, n in enumerate(QUALITY_COUNTS):
        for dt in (f32, np.float64):
            s, cam, share, _ = _picked(sc, i, 1000 + seed, dt)
            eR, eC = C.pose_error(cam, sc["true"][i])
            print("seed %d, n %d, %s: %d inliers, %.1f %% of the planted ones, rotation %.2e rad, centre %.2e" % (
                seed, n, dt.__name__, s["inliers"], 100 * share, eR, eC))
            assert share >= 0.9, (seed, n, dt, share)
            assert s["inliers"] >= 0.9 * len(sc["good"][i]) and s["valid"][s["index"]]


def _matrix_error(cam, true12):
    cam, true12 = np.asarray(cam, np.float64), np.asarray(true12, np.float64)
    R, t, Rt, tt = cam[:9].reshape(3, 3), cam[9:], true12[:9].reshape(3, 3), true12[9:]
    return np.linalg.norm(R - Rt), np.linalg.norm(-R.T @ t + Rt.T @ tt)


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_resect_then_refine(seed):
    """The restatement of misift_refine_cameras_batch (max_error = thresh) behind the resection.  At num_loops 0 its
    member count is d_res_inliers: the same test.  After five loops the camera is as close to the planted one as refine
    gets from the planted camera itself when that is turned and moved by the resection's own error in a random direction
    (the worst of four directions; measured: 0.01 to 0.61 of it)."""
    sc = C.planted(QUALITY_COUNTS, seed)
    for i, n in enumerate(QUALITY_COUNTS):
        s, cam, _, (slots, X, xy, k) = _picked(sc, i, 1000 + seed)
        cam = cam.astype(f32)
        r0 = RC.expected_camera(cam, C.RESECTED, False, k, slots, X, xy, 6, 0, 4.0, 0)
        assert r0["status"] == RC.OK and r0["nobs"] == s["inliers"] and r0["as_given"]
        r5 = RC.expected_camera(cam, C.RESECTED, False, k, slots, X, xy, 6, 5, 4.0, 0)
        true = sc["true"][i]
        eR, eC = _matrix_error(cam, true)
        got = _matrix_error(r5["cam"], true)
        R, t = true[:9].reshape(3, 3), true[9:]
        rng = np.random.default_rng(10 * seed + i)
        ref = []
        for _ in range(4):
            D = PC.rodrigues(rng.normal(0, 1, 3), eR / np.sqrt(2))          # |D - I|_F = sqrt(2) angle
            d = rng.normal(0, 1, 3)
            R2, C2 = D @ R, -R.T @ t + eC * d / np.linalg.norm(d)
            start = np.concatenate([R2.reshape(9), -R2 @ C2]).astype(f32)
            ref.append(_matrix_error(RC.expected_camera(start, C.RESECTED, False, k, slots, X, xy, 6, 5, 4.0, 0)["cam"], true))
        bound = np.max(ref, 0)
        print("seed %d, n %d: resected %.2e %.2e, refined %.2e %.2e in %d steps, reference %.2e %.2e" % (
            seed, n, eR, eC, got[0], got[1], r5["steps"], bound[0], bound[1]))
        assert r5["steps"] > 0 and got[0] <= bound[0] and got[1] <= bound[1]
        assert got[0] < eR and got[1] < eC


# ---- the premises of the GPU cases

def _expected(name):
    case = C.gpu_cases()[name]
    e = C.expected_resect(case)
    return case, e, [x["status"] for x in e["entries"]], [x["cand"] for x in e["entries"]]


def test_premises_candidate_counts_and_chunks():
    _, e, st, cand = _expected("candidates 0 5 6")
    assert cand == [0, 5, 6] and st[:2] == [C.FEW_CAND, C.FEW_CAND] and st[2] in (C.OK, C.NO_MODEL)
    _, e, st, cand = _expected("candidates 7 511 512")
    assert cand == [7, 511, 512] and st[1:] == [C.OK, C.OK]
    case, e, st, cand = _expected("candidates 513 1025")
    assert cand == [1025, 513] and st == [C.OK, C.OK] and case["max_cand"] % 16 != 0
    assert e["summary"].view(np.int32)[2] == sum(x["inliers"] for x in e["entries"]) > 900
    case, e, st, cand = _expected("max_cand one below n")
    assert cand == [512, 513, 1025] and st == [C.OK, C.OVER, C.OVER] and case["max_cand"] == 512
    assert (e["res_cam"].view(f32)[12:] == 0).all() and e["res_inliers"].view(np.int32).tolist()[1:] == [0, 0]
    _, e, st, cand = _expected("max_cand 1025")
    assert cand == [1025] and st == [C.OK]
    _, e, st, cand = _expected("no candidates")
    assert cand == [0] and st == [C.FEW_CAND]


def test_premises_loops_selection_and_counts():
    for L in (1, 63, 64, 65, 100):
        case, e, st, cand = _expected("num_loops %d" % L)
        assert case["num_loops"] == L and cand == [63] and len(e["entries"][0]["search"]["counts"]) == L
    case, e, st, cand = _expected("nsel 0")
    assert len(e["res_cam"]) == 0 and e["summary"].view(np.int32).tolist() == [RC.counts(case)[0]] + [0] * 7
    _, e, st, cand = _expected("nsel 3 of different status")
    assert cand == [27, 93, 43] and st == [C.FEW_CAND, C.OVER, C.OK]
    small = C.small_scene()["case"]
    T0, O0 = RC.counts(small)
    full = C.expected_resect(C.resect_case(small, [0, 3], num_loops=32))
    seen = set()
    for name, (case, e, st, cand) in ((n, _expected(n)) for n in C.gpu_cases() if n.startswith("T ")):
        T, O = RC.counts(case)
        assert e["summary"].view(np.int32)[0] == T
        seen.add((T < T0, T == small["max_tracks"], O < O0, O == small["max_obs"], T == 0, O == 0))
        same = e["res_cand"].tobytes() == full["res_cand"].tobytes()
        assert same == (T >= T0 and O >= O0), name
    assert len(seen) >= 6


def test_premises_hostile_inputs():
    case, e, st, cand = _expected("hostile")
    clean = C.expected_resect(C.resect_case(C.small_scene()["case"], [0, 1, 3], num_loops=48))
    assert st == [C.OK] * 3 and sum(cand) < sum(x["cand"] for x in clean["entries"])
    key, _ = RC.candidate_keys(case)
    for o in (20, 33, 47, 48, 60, 61, 62):
        assert key[o] == -1
    assert (key[10:17] == -1).all()
    case, e, st, cand = _expected("bad offsets")
    key, owner = RC.candidate_keys(case)
    assert owner[7] == 9 and owner[4] == -1 and owner[5] == -1 and owner[19] == -1 and owner[20] == -1
    _, e, st, cand = _expected("one point")
    assert st == [C.NO_MODEL] * 2 and cand == [20, 9]
    assert all(not x["search"]["valid"].any() and x["inliers"] == 0 for x in e["entries"])
    _, e, st, cand = _expected("coplanar")
    assert st == [C.NO_MODEL] * 2 and cand == [30, 50] and all(not x["search"]["valid"].any() for x in e["entries"])
    sc = C.small_scene()
    slots, X, _ = RC.image_candidates(sc["case"], 0)
    true = sc["true"][0]
    depth = X.astype(np.float64) @ true[6:9] + true[11]
    assert (depth < 0).sum() == 3                                # candidates behind the camera, never inliers


def test_premises_min_inliers_pairs_seeds_and_ties():
    got = [_expected("min_inliers count %+d" % d) for d in (-1, 0, 1)]
    c = got[1][1]["entries"][0]["inliers"]
    assert [g[0]["min_inliers"] for g in got] == [c - 1, c, c + 1] and c > 7
    assert [g[2] for g in got] == [[C.OK], [C.OK], [C.NO_MODEL]]
    assert got[2][1]["res_inliers"].view(np.int32)[0] == c and (got[2][1]["res_cam"] == 0).all()
    for install in (0, 1):
        case, e, st, cand = _expected("only_unset, install %d" % install)
        assert case["images"].tolist() == [3, 0, 2, 1] and case["cam_pair"].tolist() == [C.UNSET, C.ROOT, 1, C.RESECTED]
        assert st == [C.SKIPPED, C.OK, C.SKIPPED, C.SKIPPED] and cand == [0, 43, 0, 0]
        changed = e["cam"].tobytes() != np.ascontiguousarray(case["cam"], f32).tobytes()
        assert changed == bool(install)
        assert e["cam_pair"].view(np.int32).tolist() == ([C.RESECTED, C.ROOT, 1, C.RESECTED] if install else
                                                         case["cam_pair"].tolist())
        assert e["cam"][12:].tobytes() == np.ascontiguousarray(case["cam"], f32)[1:].tobytes()
    case, e, st, cand = _expected("install over set cameras")
    assert st == [C.OK] * 4 and (e["cam_pair"].view(np.int32) == C.RESECTED).all()
    (_, a, sa, _), (_, b, sb, _) = _expected("seed a"), _expected("seed b")
    assert sa == sb == [C.OK, C.OK]
    for x, y in zip(a["entries"], b["entries"]):
        assert (x["search"]["samples"] != y["search"]["samples"]).any()
    assert (C.draw6(0, 60, 8) == C.draw6(1, 60, 8)).all()        # srand(0) is srand(1)
    _, e, st, cand = _expected("tie")
    for x in e["entries"]:
        counts = x["search"]["counts"]
        assert (counts == counts.max()).sum() >= 2 and x["search"]["index"] == np.nonzero(counts == counts.max())[0][0]
        assert x["inliers"] == x["cand"]
    _, e, st, cand = _expected("thresh inf")
    assert st == [C.OK] and e["entries"][0]["inliers"] >= 40     # no gate: whatever lies in front counts


def test_premise_of_the_chain_case():
    """With pair 4 = (4, 5) of the 8-camera scene made unusable (no record in front), link_poses leaves images 5, 6 and 7
    without a camera."""
    import posegraph_cases as G
    pc = dict(G.planted_scene()["case"])
    front = pc["num_front"].copy()
    front[4] = 0
    pc["num_front"] = front
    with np.errstate(all="ignore"):
        linked = G.expected_link_poses(pc)
    assert linked["cam_pair"].view(np.int32).tolist()[5:] == [C.UNSET] * 3
    assert (linked["cam_pair"].view(np.int32)[:5] != C.UNSET).all()
