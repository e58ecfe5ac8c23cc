"""misift_align_points_batch, misift_correspond_tracks_batch and misift_transform_scene_batch without a device: the numpy
restatement of include/misift.h (align_cases.py) pinned byte for byte to the library's host hooks, which compile the
functions the kernels run (align_core.hpp); the float32 restatement against the same algorithm in float64 and against a
float64 numpy.linalg.svd Umeyama; the properties of the rotation; planted scenes; the reprojection invariant of the scene
transform; and the premises of the cases test_gpu_align.py runs."""
import numpy as np
import pytest

import align_cases as C
import refine_cases as RC
from align_cases import f32

f64 = np.float64
EPS = float(np.finfo(f32).eps)


def _bytes_equal(a, b):
    return np.ascontiguousarray(a, f32).tobytes() == np.ascontiguousarray(b, f32).tobytes()


# ---- the restatement pinned to the hooks

@pytest.mark.parametrize("n", (3, 4, 1000))
@pytest.mark.parametrize("seed", (1, 12345))
def test_draws_match_hook(n, seed):
    got, want = C.hook_samples(seed, n, 300), C.draw3(seed, n, 300)
    assert (got == want).all()
    assert (got >= 0).all() and (got < n).all()
    assert (got[:, 0] != got[:, 1]).all() and (got[:, 0] != got[:, 2]).all() and (got[:, 1] != got[:, 2]).all()


def _triples():
    """name -> (a (L, 3, 3), b (L, 3, 3)) float32."""
    rng = np.random.default_rng(11)
    out = {}
    a = rng.uniform(-4, 4, (200, 3, 3))
    R, t = C.rotation(rng), rng.uniform(-5, 5, 3)
    out["random"] = (a, 1.7 * a @ R.T + t + rng.normal(0, 0.01, a.shape))
    out["unrelated"] = (a, rng.uniform(-4, 4, a.shape))
    out["mirrored"] = (a, (1.7 * a @ R.T + t) * np.array([1, 1, -1.0]))
    line = rng.uniform(-3, 3, (20, 3, 1)) * np.array([1.0, 0.0, 0.0])
    out["collinear"] = (line, 2 * line + np.array([1.0, 0, 0]))                  # on an axis: exactly collinear in float32
    skew = rng.uniform(-3, 3, (20, 3, 1)) * np.array([1.0, 2.0, -0.5])
    out["nearly collinear"] = (skew, 2 * skew)                                   # collinear up to rounding
    out["coincident"] = (np.tile(rng.uniform(-3, 3, (20, 1, 3)), (1, 3, 1)), a[:20])
    out["two coincident"] = (np.concatenate([a[:20, :2], a[:20, 1:2]], 1), a[:20] + 1)
    out["b coincident"] = (a[:20], np.tile(rng.uniform(-3, 3, (20, 1, 3)), (1, 3, 1)))
    out["huge"] = (a[:40] * 1e20, a[:40] * 3e20 @ R.T)
    out["huge b"] = (a[:40], a[:40] * 1e30 @ R.T)
    out["subnormal"] = (a[:40] * 1e-41, a[:40] * 2e-41 @ R.T)
    out["tiny"] = (a[:40] * 1e-18, a[:40] * 1e-18 @ R.T)
    bad = np.tile(a[:27], (1, 1, 1)).copy()
    for j, v in enumerate((np.nan, np.inf, -np.inf) * 9):
        bad[j].reshape(-1)[j % 9] = v
    out["non-finite a"] = (bad, a[:27])
    out["non-finite b"] = (a[:27], bad)
    return {k: (np.asarray(x, f64).astype(f32), np.asarray(y, f64).astype(f32)) for k, (x, y) in out.items()}


def test_solve_matches_hook():
    """Every family of triples, byte for byte, the validity included; the degenerate families are INVALID and an INVALID
    solve is thirteen copies of the one quiet NaN."""
    nan13 = np.full(13, np.uint32(0x7fc00000)).view(f32)
    with np.errstate(all="ignore"):
        for name, (a, b) in _triples().items():
            h, ok = C.solve3(a, b)
            for j in range(len(a)):
                got, valid = C.hook_solve(a[j], b[j])
                assert valid == int(ok[j]), (name, j)
                assert _bytes_equal(got, h[j]), (name, j, got, h[j])
                if not valid:
                    assert _bytes_equal(got, nan13), (name, j)
            print(name, "valid %d of %d" % (ok.sum(), len(ok)))
            if name in ("collinear", "nearly collinear", "two coincident", "coincident", "b coincident", "non-finite a", "non-finite b", "huge", "huge b",
                        "subnormal"):
                assert not ok.any(), name
            if name in ("random", "mirrored", "unrelated", "tiny"):
                assert ok.all(), name


@pytest.mark.parametrize("n,seed", ((40, 1), (400, 2), (700, 3), (1025, 4)))
def test_refit_matches_hook(n, seed):
    """Step 6 from the transform of the first three correspondences that are planted inliers, at 0, 1 and 5 refits and at
    two thresholds: the transform, the members, the refits kept and the rms, byte for byte."""
    p = C.planted_pairs(n, seed)
    k = np.nonzero(p["good"])[0][:3]
    h0, ok = C.solve3(p["a"][k][None], p["b"][k][None])
    assert ok[0]
    for thresh in (0.05, 0.5, np.inf):
        for loops in (0, 1, 5):
            want = C.refit(p["a"], p["b"], h0[0], thresh, loops)
            h, members, kept, rms = C.hook_refit(p["a"], p["b"], h0[0], thresh, loops)
            assert (members, kept) == (want["members"], want["kept"]), (thresh, loops)
            assert _bytes_equal(h, want["h"]) and _bytes_equal(rms, want["rms"]), (thresh, loops)
            assert want["kept"] <= loops
    # an INVALID transform has no members: nothing is refitted and the rms is 0
    nan13 = np.full(13, np.nan, f32)
    h, members, kept, rms = C.hook_refit(p["a"], p["b"], nan13, 0.05, 3)
    assert (members, kept, float(rms)) == (0, 0, 0.0) and _bytes_equal(h, nan13)
    assert C.refit(p["a"], p["b"], nan13, 0.05, 3)["members"] == 0


def test_transform_matches_hook():
    case = C.transform_case()
    cams = C.one_nan(C.transform_cameras(case["sim"], case["cam"]))
    for i in range(case["nimages"]):
        assert _bytes_equal(C.hook_transform_camera(case["sim"], case["cam"][i]), cams[i]), i
    pts = C.one_nan(C.transform_points(case["sim"], case["points"][:, :3]))
    for t in range(case["max_tracks"]):
        assert _bytes_equal(C.hook_transform_point(case["sim"], case["points"][t, :3]), pts[t]), t
    e = C.expected_transform(case)
    same = e["cam_out"].reshape(-1, 12) == np.ascontiguousarray(case["cam"]).reshape(-1).view(np.uint32).reshape(-1, 12)
    assert same[[2, 6]].all() and not same[[0, 1, 5]].all(1).any()           # unset copied; root, linked, resected moved
    assert (e["cam_out"].reshape(-1, 12)[7] == 0x7fc00000).any()
    off = C.expected_transform(dict(case, sim_status=2))
    assert off["cam_out"].tobytes() == case["cam"].tobytes() and off["points_out"].tobytes() == case["points"].tobytes()


# ---- float32 against float64

def umeyama64(a, b):
    """Umeyama's least-squares similarity transform in float64 with numpy.linalg.svd, the scale as the call defines it
    (Horn's symmetric sqrt(sb / sa))."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    ca, cb = a.mean(0), b.mean(0)
    da, db = a - ca, b - cb
    U, S, Vt = np.linalg.svd(db.T @ da)
    D = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = np.sqrt((db * db).sum() / (da * da).sum())
    return R, cb - s * R @ ca, s, S


def _errors(h, R, t, s, scale):
    """(max |dR|, max |dt| relative to `scale`, |ds| / s)."""
    h = np.asarray(h, f64)
    return (np.abs(h[:9].reshape(3, 3) - R).max(), np.abs(h[9:12] - t).max() / scale, abs(h[12] - s) / s)


def _triple_errors():
    rng = np.random.default_rng(21)
    a = rng.uniform(-4, 4, (1000, 3, 3)).astype(f32)
    b = np.zeros_like(a)
    for j in range(len(a)):
        b[j] = (rng.uniform(0.5, 3) * a[j].astype(f64) @ C.rotation(rng).T + rng.uniform(-5, 5, 3)).astype(f32)
    h32, ok32 = C.solve3(a, b, f32)
    h64, ok64 = C.solve3(a, b, f64)
    assert ok32.all() and ok64.all()
    well, tail = np.zeros((2, 3)), np.zeros((2, 3))
    nwell = 0
    for j in range(len(a)):
        R, t, s, S = umeyama64(a[j], b[j])
        scale = np.abs(t).max() + s * np.abs(a[j]).max()
        e = np.array([_errors(h32[j], h64[j][:9].reshape(3, 3), h64[j][9:12], h64[j][12], scale),
                      _errors(h32[j], R, t, s, scale)])
        if S[1] / S[0] >= 0.05:
            well, nwell = np.maximum(well, e), nwell + 1
        else:
            tail = np.maximum(tail, e)
    return well, tail, nwell


# measured over the fixed seeds (worst error of the float32 restatement: R absolute, t relative to |t| + s |a|, s relative)
TRIPLE_VS_F64 = (2.56e-6, 1.30e-6, 6.2e-7)         # against the same algorithm in float64, sigma2 / sigma1 >= 0.05
TRIPLE_VS_SVD = (2.56e-6, 1.30e-6, 6.2e-7)         # against the float64 numpy.linalg.svd Umeyama
MANY_VS_F64 = (1.04e-6, 2.63e-7, 4.3e-7)          # 4 .. 400 noisy points through the 256-slot sums
MANY_VS_SVD = (1.04e-6, 2.63e-7, 4.3e-7)


def test_float32_triples_against_float64():
    """1000 exact triples (scale 0.5 .. 3, any rotation, |t| <= 5) restricted to sigma2 / sigma1 >= 0.05 of the moment
    matrix.  The asserted bounds are 4 x the measured worst errors in TRIPLE_VS_F64 / TRIPLE_VS_SVD (the margin covers
    libm / numpy version differences in float64 only).  Measured over the 844 such triples: R 6.4e-7 absolute, t 3.2e-7
    relative, s 1.5e-7 relative, against either yardstick alike; the ill-conditioned tail (sigma2 / sigma1 < 0.05, reported,
    not asserted) reaches R 1.4e-4 and t 1.0e-4."""
    well, tail, nwell = _triple_errors()
    print("well-conditioned %d of 1000: vs f64 R %.3g t %.3g s %.3g; vs svd R %.3g t %.3g s %.3g" % (
        nwell, *well[0], *well[1]))
    print("ill-conditioned tail: vs f64 R %.3g t %.3g s %.3g; vs svd R %.3g t %.3g s %.3g" % (*tail[0], *tail[1]))
    assert nwell > 800
    assert (well[0] <= TRIPLE_VS_F64).all() and (well[1] <= TRIPLE_VS_SVD).all()


def _many_errors():
    rng = np.random.default_rng(22)
    worst = np.zeros((2, 3))
    for n in (4, 5, 17, 64, 255, 256, 257, 400):
        for rep in range(6):
            p = C.planted_pairs(n, 1000 + 10 * n + rep, wrong=0.0, noise=0.01)
            k = rng.choice(n, 3, replace=False)
            h0, ok = C.solve3(p["a"][k][None], p["b"][k][None])
            r32 = C.refit(p["a"], p["b"], h0[0], np.inf, 1, f32)
            r64 = C.refit(p["a"], p["b"], h0[0], np.inf, 1, f64)
            assert r32["kept"] == 1 and r64["kept"] == 1 and r32["members"] == n
            R, t, s, _ = umeyama64(p["a"], p["b"])
            scale = np.abs(t).max() + s * np.abs(p["a"]).max()
            h = r64["h"]
            worst = np.maximum(worst, [_errors(r32["h"], h[:9].reshape(3, 3), h[9:12], h[12], scale),
                                       _errors(r32["h"], R, t, s, scale)])
    return worst


def test_float32_many_points_against_float64():
    """4 .. 400 noisy correspondences fitted by one refit over all of them (thresh +inf), so through the 256-slot sums.
    The asserted bounds are 4 x the measured worst errors.  Measured: R 2.6e-7, t 6.6e-8 relative, s 1.1e-7 relative,
    against either yardstick alike."""
    worst = _many_errors()
    print("many points: vs f64 R %.3g t %.3g s %.3g; vs svd R %.3g t %.3g s %.3g" % (*worst[0], *worst[1]))
    assert (worst[0] <= MANY_VS_F64).all() and (worst[1] <= MANY_VS_SVD).all()


def test_rotation_is_proper():
    """R^T R = I and det R = +1 on every valid solve, mirrored correspondences included (where U V^T alone would be a
    reflection).  The bound: R is assembled from two columns normalised to 1 within 2 eps each, which one-sided Jacobi
    leaves orthogonal to rounding whatever the conditioning, and their cross product; an entry of R^T R is a sum of
    three products of nine such terms, so 64 eps is generous to the roundings and to nothing else."""
    worst = 0.0
    with np.errstate(all="ignore"):
        for name, (a, b) in _triples().items():
            h, ok = C.solve3(a, b)
            for x in h[ok].astype(f64):
                R = x[:9].reshape(3, 3)
                worst = max(worst, np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1))
    print("rotation: worst deviation %.3g (%.1f eps)" % (worst, worst / EPS))
    assert worst <= 64 * EPS


# ---- planted scenes

@pytest.mark.parametrize("n", (40, 400, 2000))
@pytest.mark.parametrize("dt", (f32, f64), ids=("float32", "float64"))
def test_planted_scenes(n, dt):
    """A quarter of the correspondences displaced by 2 units, 0.01 noise, thresh 0.05, 256 hypotheses, three seeds: the
    picked count reaches 90 % of the planted inliers; the refit never lowers the count and lowers the rms."""
    for seed in (1, 2, 3):
        p = C.planted_pairs(n, 200 + seed)
        s = C.search(seed, p["a"], p["b"], 256, 0.05, dt)
        planted = int(p["good"].sum())
        r0 = C.refit(p["a"], p["b"], s["hyps"][s["index"]], 0.05, 0, dt)
        r5 = C.refit(p["a"], p["b"], s["hyps"][s["index"]], 0.05, 5, dt)
        print(n, dt.__name__, seed, "planted", planted, "picked", s["inliers"], "refitted", r5["members"], "kept",
              r5["kept"], "rms %.4g -> %.4g" % (r0["rms"], r5["rms"]))
        assert s["inliers"] >= 0.9 * planted
        assert r0["members"] == s["inliers"] and r5["members"] >= r0["members"]
        assert r5["kept"] >= 1 and r5["rms"] < r0["rms"]
        R, t, sc = r5["h"][:9].reshape(3, 3).astype(f64), r5["h"][9:12].astype(f64), float(r5["h"][12])
        assert np.abs(R - p["R"]).max() < 0.01 and abs(sc - p["s"]) < 0.01 * p["s"] and np.abs(t - p["t"]).max() < 0.05


# ---- the reprojection invariant

REPROJECTION_MOVES = 1.22e-3                      # px: 4 x the measured 3.05e-4


def test_reprojection_is_unchanged_by_the_transform():
    """Every observation of a planted scene reprojected through the restatement of triangulate's view (refine_cases.view)
    under the cameras and points as given and as expected_transform leaves them, in float32: the residuals move by no
    more than REPROJECTION_MOVES px (4 x the measured worst, 3.05e-4 px at coordinates up to 1920 px, whose float32
    spacing is 1.2e-4 px)."""
    case = RC.spread_case(300)
    T, O = RC.counts(case)
    sim = C.transform_case()["sim"]
    tc = dict(sim=sim, sim_status=0, max_tracks=case["max_tracks"], export_summary=case["export_summary"],
              points=case["points"], point_status=case["point_status"], nimages=case["nimages"], cam=case["cam"],
              cam_pair=case["cam_pair"])
    e = C.expected_transform(tc)
    pts2, cam2 = e["points_out"].view(f32).reshape(-1, 4), e["cam_out"].view(f32).reshape(-1, 12)
    pts1, cam1 = np.asarray(case["points"], f32).reshape(-1, 4), np.asarray(case["cam"], f32).reshape(-1, 12)
    offs, obs = case["track_offsets"], case["obs"]
    worst, seen = 0.0, 0
    for t in range(T):
        if case["point_status"][t] != 0:
            continue
        for o in range(offs[t], offs[t + 1]):
            i = int(obs["frame"][o])
            if case["cam_pair"][i] == C.UNSET:
                continue
            k = np.asarray(case["intrinsics"][i], f32)
            x, y = obs["xpos"][o:o + 1], obs["ypos"][o:o + 1]
            r1 = RC.view(cam1[i], k, pts1[t:t + 1, :3], x, y, f32)
            r2 = RC.view(cam2[i], k, pts2[t:t + 1, :3], x, y, f32)
            assert r1[2][0] > 0 and r2[2][0] > 0
            assert abs(float(r2[2][0]) / float(r1[2][0]) - float(sim[12])) < 1e-5          # the depth scales with s
            worst = max(worst, abs(float(r1[6][0]) - float(r2[6][0])), abs(float(r1[7][0]) - float(r2[7][0])))
            seen += 1
    print("reprojection: %d observations, residuals move by at most %.3g px" % (seen, worst))
    assert seen > 200 and worst <= REPROJECTION_MOVES


# ---- the premises of the cases

def _entries(name):
    return C.expected_align(C.gpu_cases()[name])["entries"]


def test_align_case_premises():
    cases = C.gpu_cases()
    st = lambda name: [x["status"] for x in _entries(name)]     # noqa: E731
    cand = lambda name: [x["cand"] for x in _entries(name)]     # noqa: E731
    assert cand("candidates 0 2 3 4") == [0, 2, 3, 4] and st("candidates 0 2 3 4") == [1, 1, 0, 0]
    assert cand("candidates 511 512") == [511, 512] and st("candidates 511 512") == [0, 0]
    assert cand("candidates 513 1025") == [1025, 513] and st("candidates 513 1025") == [0, 0]
    assert int(cases["src_cap 37"]["ranges"][0][1]) == 37 and cand("src_cap 37") == [30]
    assert cand("count negative, stride 8") == [50, 0] and st("count negative, stride 8") == [0, 1]
    assert cand("count below at beyond") == [40, 80, 80, 80]
    assert st("four entries") == [0, 1, 2, 0]
    assert len({int(r[2]) for r in cases["four entries"]["ranges"]}) == 4
    assert st("min_inliers count -1") == [0] and st("min_inliers count +0") == [0] and st("min_inliers count +1") == [2]
    e = _entries("thresh inf")
    assert all(x["search"]["index"] == 0 and x["search"]["valid"][0] and x["inliers"] == x["cand"] for x in e)
    assert (e[0]["search"]["counts"][e[0]["search"]["valid"]] == e[0]["cand"]).all()
    a, b = _entries("seed a"), _entries("seed b")
    assert any((x["search"]["samples"] != y["search"]["samples"]).any() for x, y in zip(a, b))
    h = _entries("hostile")[0]
    assert h["cand"] == 120 - 5 - 3 - 3 - 2 - 2 and h["status"] == 0
    assert not set(h["index"].tolist()) & {0, 1, 2, 3, 4, 10, 11, 12, 20, 21, 22, 30, 31, 40, 41}
    assert {13, 23} <= set(h["index"].tolist()) and not h["member"][np.isin(h["index"], (13, 23))].any()
    assert st("collinear, identical") == [2, 2, 2] and cand("collinear, identical") == [40, 20, 40]
    assert all(not x["search"]["valid"].any() for x in _entries("collinear, identical"))
    r0, r1, r5 = (_entries("refit_loops %d" % r)[0] for r in (0, 1, 5))
    assert (r0["kept"], r1["kept"]) == (0, 1) and r5["kept"] >= 2
    assert r0["inliers"] <= r1["inliers"] <= r5["inliers"] and r5["sim"][13] < r0["sim"][13]
    t = _entries("turned away")[0]
    assert t["status"] == 0 and t["kept"] < 3 and t["refit"]["history"][-1] < t["inliers"], t["refit"]["history"]
    w = _entries("slots wrap")[0]
    assert w["inliers"] > 2 * 256 and w["kept"] >= 1
    assert cases["no inlier, no status"]["src_status"] is None and not cases["no inlier, no status"]["want_inlier"]
    assert len(cases["nsel 0"]["ranges"]) == 0
    for L in (1, 63, 64, 65, 100):
        assert cases["num_loops %d" % L]["num_loops"] == L
    for name, case in cases.items():                             # the inlier words are -1, 0 or 1 inside the ranges
        e = C.expected_align(case)
        inl = e["inlier"].view(np.int32)
        for r, x in zip(case["ranges"], e["entries"]):
            got = inl[r[0]:r[0] + r[1]]
            assert set(got.tolist()) <= {-1, 0, 1}, name
            assert (got >= 0).sum() == x["cand"] and (got == 1).sum() == (x["inliers"] if x["status"] == 0 else 0), name


def test_correspond_case_premises():
    cases = C.correspond_cases()
    for T in (0, 1, 255, 256, 257):
        e = C.expected_correspond(cases["T_A %d" % T])
        s = e["summary"].view(np.int32)
        assert s[0] == T and s[4] == 0 and (T < 5 or 0 < s[3] < T)
        assert s[2] == 2 * s[3]                                  # two of a track's three records are in B
    for name in ("shift +5", "shift -9"):
        c = cases[name]
        e, base = C.expected_correspond(c), C.expected_correspond(dict(c, shift=0))
        s = e["summary"].view(np.int32)
        assert s[3] > 20 and s[4] == 0 and base["summary"].view(np.int32)[3] < s[3]
    s = C.expected_correspond(cases["shift out of range"])["summary"].view(np.int32)
    z = C.expected_correspond(dict(cases["shift out of range"], shift=0))["summary"].view(np.int32)
    assert s[2] < z[2] and z[3] > 20
    e = C.expected_correspond(cases["conflict"])
    assert e["map"].view(np.int32)[:3].tolist() == [-2, 2, -1] and e["summary"].view(np.int32)[:5].tolist() == [3, 3, 7, 1, 1]
    assert (e["map"][3:] == C.POISON_WORD).all()
    c = cases["stale and hostile"]
    e, clean = C.expected_correspond(c), C.expected_correspond(C.correspond_case(60, 95))
    assert 0 < e["summary"].view(np.int32)[2] < clean["summary"].view(np.int32)[2]
    assert e["summary"].view(np.int32)[1] == c["b"]["max_tracks"]
