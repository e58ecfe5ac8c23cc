"""misift_recover_pose_planar_batch without a GPU: pose_planar_cases.expected_planar, the numpy float32 restatement of the
definition in include/misift.h, which tests/test_gpu_pose_planar.py holds the device to byte for byte.  Here the
restatement is pinned from both sides: the library's host-only hooks misift_test_pose_planar_decompose and
misift_test_pose_planar_vote, compiled from the functions the kernel runs, must equal it byte for byte, and on planted
planar scenes its answer must agree with its float64 twin and with the planted pose."""
import numpy as np
import pytest

import pose_cases as PC
import pose_planar_cases as PP
from test_fundamental_cpu import GATES, expected_find, f32, gate
from test_pose_cpu import EPS, direction_error, hook_vote

f64 = np.float64


# ---- the hooks

def hook_decompose(H, K8, min_baseline):
    """(model, s1, s3, hyps (4, 16), F (2, 9)) from misift_test_pose_planar_decompose, and its 84 floats."""
    from cudasift_amd import capi
    H, K8 = np.ascontiguousarray(H, f32).reshape(9), np.ascontiguousarray(K8, f32).reshape(8)
    out, model = np.full(84, 3.5, f32), np.full(1, -77, np.int32)
    assert capi.lib().misift_test_pose_planar_decompose(H.ctypes.data, K8.ctypes.data, f32(min_baseline),
                                                        out.ctypes.data, model.ctypes.data) == 0
    return int(model[0]), out


def flat(dec):
    """A decompose() result in the hook's layout."""
    return np.concatenate([[dec["s1"], dec["s3"]], dec["hyps"].reshape(-1), dec["F"].reshape(-1)]).astype(f32)


def hook_votes(H, F, hyp84, K8, xy, g, thresh_h, thresh_f, planar_ratio=PP.RATIO, min_inliers=PP.MIN_INLIERS):
    """(h_in, f_in, votes (n, 4)) as bool arrays and decision9 (nH, nF, candidate, the four votes, pick, alternative)
    from misift_test_pose_planar_vote."""
    from cudasift_amd import capi
    H, K8 = np.ascontiguousarray(H, f32).reshape(9), np.ascontiguousarray(K8, f32).reshape(8)
    F = None if F is None else np.ascontiguousarray(F, f32).reshape(9)
    xy, g = np.ascontiguousarray(xy, f32).reshape(-1, 4), np.ascontiguousarray(g, np.uint8)
    n = len(xy)
    h_in, f_in, votes = np.full(n, 7, np.uint8), np.full(n, 7, np.uint8), np.full((n, 4), 7, np.uint8)
    dec = np.full(9, -77, np.int32)
    assert capi.lib().misift_test_pose_planar_vote(H.ctypes.data, None if F is None else F.ctypes.data,
                                                   hyp84.ctypes.data, K8.ctypes.data, xy.ctypes.data, g.ctypes.data, n,
                                                   f32(thresh_h), f32(thresh_f), f32(planar_ratio), int(min_inliers),
                                                   h_in.ctypes.data, f_in.ctypes.data, votes.ctypes.data,
                                                   dec.ctypes.data) == 0
    assert set(np.unique(np.concatenate([h_in, f_in, votes.reshape(-1)]))) <= {0, 1}
    assert dec[:2].tolist() == [h_in.sum(), f_in.sum()] and dec[3:7].tolist() == votes.sum(0).tolist() and dec[2] in (0, 1)
    return h_in.astype(bool), f_in.astype(bool), votes.astype(bool), dec


def hook_planar(recs, n, H, F, K8, **kw):
    """Steps 1-8 put together from the hooks alone, the decision of step 2 and the pick of step 7 included: what
    expected_planar returns."""
    p = dict(PP.PARAMS, **kw)
    xy = PC.coordinates(recs, n)
    g = gate(recs[:len(xy)], *GATES)
    model, out = hook_decompose(H, K8, p["min_baseline"])
    dec = hook_votes(H, F, out, K8, xy, g, p["thresh_h"], p["thresh_f"], p["planar_ratio"], p["min_inliers"])[3]
    res = dict(model=PP.GENERAL, hf=dec[:2].copy())
    if not dec[2]:
        return res
    res["model"] = model
    if model == PP.INVALID:
        return res
    hyps = out[2:66].reshape(4, 16)
    votes = dec[3:7].copy() if model == PP.PLANE else np.zeros(4, np.int32)
    best, alt = (int(dec[7]), int(dec[8])) if model == PP.PLANE else (0, 0)
    xyz = hook_vote(hyps[best, :12], K8, xy)[1]
    if model == PP.ROTATION:
        xyz[:] = PC.ONE_NAN
    res.update(pose=hyps[best, :12].copy(), pose_alt=hyps[alt, :12].copy(), num_front=int(votes[best]), votes=votes,
               plane=hyps[best, 12:].copy(), xyz=xyz, best=best, alt=alt)
    return res


def same_as_hooks(recs, n, H, F, K8, what, **kw):
    """The hooks equal the restatement byte for byte; returns expected_planar's dict."""
    with np.errstate(all="ignore"):
        e = PP.expected_planar(recs, n, H, F, K8, **kw)
    h = hook_planar(recs, n, H, F, K8, **kw)
    assert h["model"] == e["model"] and h["hf"].tolist() == e["hf"].tolist(), (what, h["model"], e["model"], h["hf"], e["hf"])
    if e["model"] > 0:
        assert h["votes"].tolist() == e["votes"].tolist() and (h["best"], h["alt"]) == (e["best"], e["alt"]), \
            (what, h["votes"], e["votes"])
        for k in ("pose", "pose_alt", "plane"):
            assert h[k].tobytes() == e[k].astype(f32).tobytes(), (what, k, h[k], e[k])
        assert h["num_front"] == e["num_front"], what
        bad = np.nonzero((h["xyz"].view(np.uint32) != e["xyz"].view(np.uint32)).any(1))[0]
        assert len(bad) == 0, (what, "xyz rows", bad[:8], h["xyz"][bad[:2]], e["xyz"][bad[:2]])
    return e


# ---- tests

def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, the argument checks that need
    no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_recover_pose_planar_batch", "misift_test_pose_planar_decompose",
                 "misift_test_pose_planar_vote"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "recover_pose_planar_batch")
    fr, K = np.zeros(1, np.int32), np.array(PC.K_A + PC.K_B, f32)
    tail = (None,) * 10
    assert L.misift_recover_pose_planar_batch(None, 1, fr.ctypes.data, K.ctypes.data, None, 1, None, None, 8, 0.85, 0.95,
                                              1.0, 1.0, 0.8, 8, 0.02, *tail) == -1    # MISIFT_EINVAL
    assert L.misift_recover_pose_planar_batch(None, -1, None, None, None, 1, None, None, 8, 0.85, 0.95, 1.0, 1.0, 0.8, 8,
                                              0.02, *tail) == -1
    assert L.misift_test_pose_planar_decompose(None, None, 0.0, None, None) == -1
    assert L.misift_test_pose_planar_vote(None, None, None, None, None, None, 0, 1.0, 1.0, 0.8, 8, None, None, None,
                                          None) == -1
    assert L.misift_test_pose_planar_vote(K.ctypes.data, None, K.ctypes.data, K.ctypes.data, None, None, 1, 1.0, 1.0,
                                          0.8, 8, None, None, None, K.ctypes.data) == -1


def test_hostile_matrices_equal_the_hook():
    """Each H is what it was chosen for, and the hook agrees byte for byte: non-finite entries, H = 0, det < 0, det = 0,
    rank 1, an exact rotation, ties of w, b at min_baseline, H scaled by 1e-20 and 1e20, random H, and tiny and huge
    focal lengths and principal points."""
    seen = {}
    for name, H, K8, mb, model in PP.hostile_matrices() + PP.baseline_edges():
        trace = {}
        with np.errstate(all="ignore"):
            dec = PP.decompose(H, K8, mb, trace=trace)
        hm, out = hook_decompose(H, K8, mb)
        assert hm == dec["model"] and out.tobytes() == flat(dec).tobytes(), (name, hm, dec["model"], out, flat(dec))
        assert model is None or dec["model"] == model, (name, dec["model"])
        if dec["model"] == PP.INVALID:
            assert not out.any()
        if dec["model"] == PP.ROTATION:
            assert not out[2:66].reshape(4, 16)[:, 9:].any() and not out[66:].any() and out[2:11].any()
        seen[name] = (dec, trace)
    with np.errstate(all="ignore"):
        assert PP.normalise(np.zeros(9, f32), PC.K_UNIT8) is None
    ref = seen["planted"][0]["hyps"].astype(f64)
    for name in ("scaled by 1e-20", "scaled by 1e20", "negated"):    # neither the scale of H nor its sign matters
        assert np.abs(seen[name][0]["hyps"].astype(f64) - ref).max() < 1e-5, name
    assert seen["det < 0"][0]["hyps"][0, :9].tolist() == [1, 0, 0, 0, -1, 0, 0, 0, -1]      # -H: half a turn about x
    assert seen["identity"][0]["hyps"][0, :9].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert seen["identity"][0]["s1"] == 1 and seen["identity"][0]["s3"] == 1
    rot = PC.rodrigues([0.2, -0.5, 0.7], 0.3)
    assert np.abs(seen["a rotation"][0]["hyps"][0, :9].astype(f64).reshape(3, 3) - rot).max() < 16 * EPS
    w = seen["a tie of w for mid"][1]
    assert w["w"][0] == w["w"][1] and (w["hi"], w["mid"], w["lo"]) == (2, 0, 1)              # the first of a tie wins
    w = seen["a tie of w for hi"][1]
    assert w["w"][0] == w["w"][1] and (w["hi"], w["mid"], w["lo"]) == (0, 1, 2)
    shear = seen["a shear"][0]["hyps"]
    d = [PP.pose_distance(shear[k, :12], np.eye(3), [1, 0, 0]) for k in range(4)]
    k = int(np.argmin(d))                                        # R = I, t = x, N = z, d = 2 is one of the four
    assert d[k] < 64 * EPS and np.abs(shear[k, 12:].astype(f64) - [0, 0, 1, 2]).max() < 64 * EPS, (d, shear[k])
    edges = [seen[n][1]["b"] for n, *_ in PP.baseline_edges()]
    assert edges[0] == edges[1] == edges[2]


def test_all_planted_scenes_equal_the_hooks():
    """The 48 planted scenes: counts, decision, hypotheses, votes, pick, alternative, plane and depths from the hooks
    equal the restatement byte for byte."""
    for (bl, off) in PP.SETTINGS:
        for i in range(PP.SCENES_EACH):
            s = PP.scene(bl, off, i)
            e = same_as_hooks(s["recs"], len(s["recs"]), s["H"], None, s["K8"], "scene %g %g %d" % (bl, off, i))
            hm, out = hook_decompose(s["H"], s["K8"], PP.MIN_BASELINE)
            assert e["model"] == hm == PP.PLANE and out.tobytes() == flat(e["dec"]).tobytes(), (bl, off, i)


def _frames():
    """(name, recs, H, F, K8, keyword arguments): the record sets of the byte comparisons."""
    out = []
    for (bl, off) in PP.SETTINGS:
        s = PP.scene(bl, off, 0)
        out.append(("scene %g %g" % (bl, off), s["recs"], s["H"], None, s["K8"], {}))
    s = PP.scene(0.5, 0.1, 1)
    F = PC.planted(seed=4)["F"]                                  # some F: its inliers are counted, nothing else
    out.append(("with an F", s["recs"], s["H"], F, s["K8"], dict(planar_ratio=0.0)))
    recs, H, K8 = PP.hostile_frame()
    out.append(("hostile records", recs, H, F, K8, dict(planar_ratio=0.0)))
    recs, H, K8 = PP.tie_frame()
    out.append(("a tie of the rotations", recs, H, None, K8, dict(thresh_h=1e-3, thresh_f=1e-3)))
    recs, H, K8 = PP.deno0_frame()
    out.append(("deno = 0", recs, H, None, K8, dict(thresh_h=1e-3, thresh_f=1e-3, min_inliers=4)))
    r = PP.planar_scene(seed=7, baseline=0.0)
    out.append(("rotation only", r["recs"], r["H"], None, r["K8"], {}))
    return out


def test_frames_equal_the_hooks():
    """Counts, votes, pick, alternative, plane and depths from the hooks equal the restatement byte for byte, and each
    record set is what it was chosen for."""
    seen = {}
    for name, recs, H, F, K8, kw in _frames():
        seen[name] = same_as_hooks(recs, len(recs), H, F, K8, name, **kw)
        print("%s: model %d, nH nF %s, votes %s" % (name, seen[name]["model"], seen[name]["hf"].tolist(),
                                                    seen[name].get("votes")))
    s = PP.scene(0.5, 0.0, 0)
    for n in (-1, 0):
        e = same_as_hooks(s["recs"], n, s["H"], None, s["K8"], "count %d" % n)
        assert e["model"] == PP.GENERAL and e["hf"].tolist() == [0, 0]
    e = seen["hostile records"]
    bad = ~np.isfinite(PC.coordinates(PP.hostile_frame()[0], 200)).all(1)
    assert e["model"] == PP.PLANE and bad.sum() >= 15 and e["hf"][0] >= 100 and e["hf"][1] < e["hf"][0]
    assert (e["xyz"][bad].view(np.uint32) == PC.NAN_BITS).all(1).sum() >= 15
    e = seen["a tie of the rotations"]
    assert e["model"] == PP.PLANE and e["votes"].max() == 40 and sorted(e["votes"].tolist())[-2] == 40, e["votes"]
    assert e["best"] < 2 and e["alt"] >= 2                       # the smallest k of the tie is the pick
    e = seen["deno = 0"]                                         # the four records with deno = 0 are no inliers
    assert e["hf"].tolist() == [8, 0] and e["model"] != PP.GENERAL
    assert seen["rotation only"]["model"] == PP.ROTATION and seen["rotation only"]["num_front"] == 0


def test_deno_zero_is_no_inlier():
    """A record with deno = 0: errx = erry = 0 - nom, and 0 < thresh^2 * 0 is false even where nom is 0, too."""
    H = PP.DENO0_H
    xy = np.array([[4, 1, 7, 7], [4, 0, 0, 0], [5, 2, 5, 2]], f32)
    recs = PC.records(xy, 3)
    got = PP.h_inliers(H, xy, 1.0)
    assert got.tolist() == [False, False, True]
    dec = PP.decompose(H, PC.K_UNIT8, 0.0)
    h_in = hook_votes(H, None, flat(dec), PC.K_UNIT8, xy, gate(recs, *GATES), 1.0, 1.0)[0]
    assert h_in.tolist() == got.tolist()


# R^T R - I of a planar hypothesis.  R = [p q s] [v2 u N]^T: were both bases orthonormal, R would be a rotation.  v2 and
# u are orthonormal to the roundings of the Jacobi sweeps and of u's division by dd = sqrtf(s1 - s3), a few EPS each; p
# = Hn v2 has unit length because s2 = 1 by the scaling, and q = Hn u has unit length because u is chosen so -- but a
# and c are square roots of the differences x = 1 - s3 and x = s1 - 1, which carry the rounding of s1 and s3, an EPS of
# s1 <= 2.2; the root's absolute error is that over 2 sqrt(x), and the scenes' smallest x is 0.0087 (s1 = 1.0087 at
# baseline 0.1): 12 EPS per root, two roots, over dd >= 0.42, doubled in |q|^2: 58 EPS.  With 24 EPS for the rest (the
# bound of test_pose_cpu.py) that is under 96 EPS, 5.7e-6.  Measured over the 48 scenes: 1.30e-6.
PLANAR_ORTHO_BOUND = 96 * EPS
ORTHO_MEASURED = 1.30e-6


def test_float64_properties():
    """In float64, on the float32 outputs of the 48 scenes: each of the four hypotheses reproduces Hn as R + T N^T with
    T = t / d, to the roundings of one 3x3 product; R stays a rotation; |t| = |N| = 1."""
    worst = dict(h=0.0, ortho=0.0, unit=0.0)
    for (bl, off) in PP.SETTINGS:
        for i in range(PP.SCENES_EACH):
            s = PP.scene(bl, off, i)
            dec = PP.decompose(s["H"], s["K8"], PP.MIN_BASELINE)
            assert dec["model"] == PP.PLANE
            Hn = dec["Hn"].astype(f64)
            for k in range(4):
                h = dec["hyps"][k].astype(f64)
                R, t, N, d = h[:9].reshape(3, 3), h[9:12], h[12:15], h[15]
                worst["h"] = max(worst["h"], float(np.abs(R + np.outer(t / d, N) - Hn).max()))
                worst["ortho"] = max(worst["ortho"], float(np.abs(R.T @ R - np.eye(3)).max()))
                worst["unit"] = max(worst["unit"], abs(np.linalg.norm(t) - 1), abs(np.linalg.norm(N) - 1))
                assert np.linalg.det(R) > 0.99 and d > 0
    print("largest |R + T N^T - Hn| %.3g, |R^T R - I| %.3g, ||t| - 1| or ||N| - 1| %.3g" % (
        worst["h"], worst["ortho"], worst["unit"]))
    # T = (Hn - R) N exactly reproduces Hn on N; on v2 and u, Hn and R agree by construction (R v2 = p = Hn v2) up to the
    # orthonormality above, times |Hn| <= sqrt(s1) < 1.5
    assert worst["h"] <= 1.5 * PLANAR_ORTHO_BOUND and worst["ortho"] <= PLANAR_ORTHO_BOUND, worst
    assert worst["unit"] <= 48 * EPS, worst


def exact_homography(s):
    """H = K2 (R + t N^T / d) K1^-1 of a scene's planted pose and plane, h8 = 1, rounded to float32."""
    K1, K2 = PC.kmat(s["K8"][:4].astype(f64)), PC.kmat(s["K8"][4:].astype(f64))
    H = K2 @ (s["R"] + np.outer(s["t"], s["N"]) / s["d"]) @ np.linalg.inv(K1)
    return (H / H[2, 2]).astype(f32).reshape(9)


# Rounding the exact H to float32 perturbs A = K2^-1 H K1 by up to 2^-24 (1 + (cx / fx)^2) relative to its largest entry,
# about 1e-7; the eigenvectors of A^T A move by that over the gap min(s1 - 1, 1 - s3), at least 0.03 in the 24 scenes
# used here: 3.3e-6 per entry, and the combined distance sums a dozen entries: 4e-5.  Measured: 3.45e-7 for the twin and
# 7.77e-6 for the float32 restatement, which adds its own arithmetic (FP32_MEASURED below).
EXACT_BOUND = 4e-5
EXACT_MEASURED = 3.45e-7


def test_planted_pose_is_among_the_four():
    """With the exact H of the planted pose and plane (rounded to float32), the planted (R, t, N, d) is one of the four
    hypotheses of the float64 twin, and of the float32 restatement within the twin's distance plus FP32_BOUND."""
    worst = [0.0, 0.0]
    for (bl, off) in PP.SETTINGS[::2]:
        for i in range(PP.SCENES_EACH):
            s = PP.scene(bl, off, i)
            H = exact_homography(s)
            d64, d32 = PP.decompose(H, s["K8"], PP.MIN_BASELINE, ft=f64), PP.decompose(H, s["K8"], PP.MIN_BASELINE)
            assert d64["model"] == d32["model"] == PP.PLANE
            truth = np.concatenate([s["N"], [s["d"]]])
            dist = [PP.pose_distance(d64["hyps"][k, :12], s["R"], s["t"]) for k in range(4)]
            k = int(np.argmin(dist))
            plane = float(np.abs(d64["hyps"][k, 12:] - truth).max())
            worst[0] = max(worst[0], dist[k], plane / max(1.0, s["d"]))
            d = PP.pose_distance(d32["hyps"][k, :12], s["R"], s["t"])
            worst[1] = max(worst[1], d)
            assert d <= dist[k] + FP32_BOUND, (bl, i, d, dist[k])
    print("planted pose among the four: float64 twin %.3g, float32 %.3g" % tuple(worst))
    assert worst[0] <= EXACT_BOUND, worst


# ---- planted planar scenes

_RESULTS = {}


def scene_results(bl, off):
    """Per scene of a setting: (scene, the float32 answer, the twin's answer), computed once."""
    if (bl, off) not in _RESULTS:
        rows = []
        for i in range(PP.SCENES_EACH):
            s = PP.scene(bl, off, i)
            n = len(s["recs"])
            with np.errstate(all="ignore"):
                rows.append((s, PP.expected_planar(s["recs"], n, s["H"], None, s["K8"]),
                             PP.expected_planar(s["recs"], n, s["H"], None, s["K8"], ft=f64)))
        _RESULTS[(bl, off)] = rows
    return _RESULTS[(bl, off)]


def better(e, s):
    """(distance to the planted pose of the better of pick and alternative, which hypothesis that is)."""
    dp, da = PP.pose_distance(e["pose"], s["R"], s["t"]), PP.pose_distance(e["pose_alt"], s["R"], s["t"])
    return (dp, e["best"]) if dp <= da else (da, e["alt"])


# The float32 result against its float64 twin on the same float32 H and records: the distance between hypothesis k of
# the two, k the one nearest the planted pose.  Measured over the 48 scenes: 2.34e-6 at baseline 0.5 and 6.84e-6
# at baseline 0.1 (the roundings of 1 - s3 and s1 - 1 under their roots, see PLANAR_ORTHO_BOUND).  The bound asserted on
# the float32 result's distance to the planted pose is the twin's own distance on that scene plus four times this.
FP32_MEASURED = 6.84e-6
FP32_BOUND = 4 * FP32_MEASURED


@pytest.mark.parametrize("bl,off", PP.SETTINGS, ids=["baseline %g off %g" % s for s in PP.SETTINGS])
def test_planted_planar_scenes(bl, off):
    """12 scenes per setting, 400 matches, 0.5 px noise, H a least-squares fit of the on-plane matches.  In EVERY scene
    the planted pose is d_pose or d_pose_alt: the hypothesis nearest the planted pose is the pick or the alternative, the
    twin agrees on which, and the float32 distance is within the twin's own plus FP32_BOUND.  With a tenth of the points
    off the plane at baseline 0.5 it is the pick in every scene."""
    diff = 0.0
    for i, (s, e, e64) in enumerate(scene_results(bl, off)):
        assert e["model"] == e64["model"] == PP.PLANE and e["hf"][0] >= 0.85 * s["on"].sum()
        hyps = e["dec"]["hyps"]
        dist = [PP.pose_distance(hyps[k, :12], s["R"], s["t"]) for k in range(4)]
        near = int(np.argmin(dist))
        d32, k32 = better(e, s)
        d64, k64 = better(e64, s)
        gap = PP.pose_distance(hyps[near, :12], e64["dec"]["hyps"][near, :9], e64["dec"]["hyps"][near, 9:12])
        diff = max(diff, gap)
        print("baseline %g off %g scene %d: votes %s pick %d alt %d nearest %d, distance %.3g (float64 %.3g), "
              "float32 - float64 %.3g" % (bl, off, i, e["votes"].tolist(), e["best"], e["alt"], near, d32, d64, gap))
        assert near in (e["best"], e["alt"]) and k32 == near and k64 == near, (i, near, e["best"], e["alt"], e["votes"])
        assert d32 <= d64 + FP32_BOUND, (i, d32, d64)
        assert d64 < 0.05, (i, d64)                              # the planted pose, not merely the nearest of four
        if (bl, off) == (0.5, 0.1):
            assert e["best"] == near and e64["best"] == near, (i, e["votes"])
        plane = np.abs(hyps[near, 12:15].astype(f64) - s["N"]).max()
        assert plane < 0.05, (i, plane)
    print("baseline %g off %g: largest float32 - float64 distance %.3g" % (bl, off, diff))
    assert diff <= FP32_BOUND


_FPATH = {}


def f_path(bl, i):
    """misift_find_fundamental_batch restated on an exactly planar scene: (F, its inlier count)."""
    if (bl, i) not in _FPATH:
        s = PP.scene(bl, 0.0, i)
        n = len(s["recs"])
        with np.errstate(all="ignore"):
            _FPATH[(bl, i)] = expected_find(s["recs"], n, 9 + i, 256, *GATES, PP.THRESH_F, max_pts=n)
    return _FPATH[(bl, i)]


@pytest.mark.parametrize("bl", [0.5, 0.1])
def test_the_fundamental_path_fails_on_planar_scenes(bl):
    """The reason for the call.  On the exactly planar scenes the existing restatements of find_fundamental ->
    recover_pose give a direction of t further than 0.5 from the planted one in the majority of scenes, with every
    match an inlier and in front; the better of the new call's pick and alternative stays within its bound (above).
    Measured: the F path fails so in 12 of 12 scenes at either baseline (direction errors 0.63 to 1.48)."""
    failed = 0
    for i, (s, e, e64) in enumerate(scene_results(bl, 0.0)):
        n = len(s["recs"])
        F, found = f_path(bl, i)
        with np.errstate(all="ignore"):
            p = PC.expected_pose(s["recs"], n, F, s["K8"], *GATES, PP.THRESH_F)
        err = direction_error(p["pose"][9:], s["t"])
        mine = direction_error(e["pose"][9:] if better(e, s)[1] == e["best"] else e["pose_alt"][9:], s["t"])
        print("baseline %g scene %d: F path %d inliers, %d in front, direction error %.3g; planar call %.3g" % (
            bl, i, found, p["num_front"], err, mine))
        failed += err > 0.5
        assert found >= 0.95 * n                                 # an excellent inlier count
        assert better(e, s)[0] <= better(e64, s)[0] + FP32_BOUND
    assert failed > PP.SCENES_EACH // 2, failed


# ---- the decision

def test_decision_on_scenes():
    """With F from the F path: a planar scene gives model 1, a two-plane and a general scene model 0, a rotation-only
    scene model 2 with the planted rotation."""
    s = PP.scene(0.5, 0.0, 0)
    e = same_as_hooks(s["recs"], len(s["recs"]), s["H"], f_path(0.5, 0)[0], s["K8"], "planar with F")
    assert e["model"] == PP.PLANE and e["hf"][0] >= PP.RATIO * e["hf"][1] > 0
    for name, kw in (("two planes", dict(second_plane=0.45)), ("general", dict(general=True)),
                     ("rotation only", dict(baseline=0.0))):
        s = PP.planar_scene(seed=7, **kw)
        n = len(s["recs"])
        with np.errstate(all="ignore"):
            F = expected_find(s["recs"], n, 5, 256, *GATES, PP.THRESH_F, max_pts=n)[0]
        e = same_as_hooks(s["recs"], n, s["H"], F, s["K8"], name)
        print("%s: model %d, nH nF %s" % (name, e["model"], e["hf"].tolist()))
        if name == "rotation only":
            assert e["model"] == PP.ROTATION and e["num_front"] == 0 and not e["pose"][9:].any()
            # 0.5 px on 400 matches: the fit's rotation is good to 1e-3
            assert np.linalg.norm(e["pose"][:9].astype(f64).reshape(3, 3) @ s["R"].T - np.eye(3)) < 2e-3
        else:
            assert e["model"] == PP.GENERAL and e["hf"][1] >= 0.95 * n and e["hf"][0] < PP.RATIO * e["hf"][1]
            assert set(e) == {"model", "hf"}


def library_candidate(nH, nF, ratio, min_inliers):
    """planar_candidate of the library through misift_test_pose_planar_vote: nF records on the line y2 = y1, which F =
    [x]x takes, the first nH of them also fixed points, which H = I takes.  nF = 0: F = 0, which takes no record."""
    assert nH <= nF or nF == 0
    n = max(nH, nF)
    x = (np.arange(n, dtype=f32) + 1) / f32(8)
    xy = np.stack([x, x * 2, x, x * 2], 1)
    xy[nH:, 2] += f32(0.5)
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], f32) if nF else np.zeros(9, f32)
    dec = hook_votes(np.eye(3, dtype=f32), F, np.zeros(84, f32), PC.K_UNIT8, xy, np.ones(n, np.uint8), 1e-3, 1e-3, ratio,
                     min_inliers)[3]
    assert dec[:2].tolist() == [nH, nF], dec
    return bool(dec[2])


def test_decision_at_the_thresholds():
    """nH one below, at and above min_inliers, and (float)nH exactly planar_ratio * nF."""
    recs, H, K8 = PP.tie_frame()
    kw = dict(thresh_h=1e-3, thresh_f=1e-3)
    assert PP.expected_planar(recs, 40, H, None, K8, **kw)["hf"][0] == 40
    for n, mi, model in ((7, 8, PP.GENERAL), (8, 8, PP.PLANE), (9, 8, PP.PLANE), (3, 4, PP.GENERAL), (4, 4, PP.PLANE)):
        e = same_as_hooks(recs, n, H, None, K8, "nH %d min_inliers %d" % (n, mi), min_inliers=mi, **kw)
        assert e["model"] == model and e["hf"].tolist() == [n, 0], (n, mi, e["model"], e["hf"])
    assert f32(0.8) * f32(10) == f32(8) and f32(0.5) * f32(16) == f32(8)
    for nH, nF, ratio, want in ((8, 10, 0.8, True), (8, 16, 0.5, True), (8, 17, 0.5, False), (7, 16, 0.5, False),
                                (8, 0, 0.8, True), (8, 10, np.nextafter(f32(0.8), f32(1)), False)):
        assert PP.candidate(nH, nF, True, ratio, 4) == want, (nH, nF, ratio)
        assert PP.candidate(nH, nF, False, ratio, 4)
        assert library_candidate(nH, nF, ratio, 4) == want, (nH, nF, ratio)
    # the same through the records: RATIO_F takes every record of the frame, H the first 8
    r16, H, F, K8 = PP.ratio_frame()
    e = same_as_hooks(r16, 16, H, F, K8, "nH == ratio nF", planar_ratio=0.5, **kw)
    assert e["hf"].tolist() == [8, 16] and e["model"] == PP.PLANE
    e = same_as_hooks(r16, 16, H, F, K8, "nH < ratio nF", planar_ratio=np.nextafter(f32(0.5), f32(1)), **kw)
    assert e["hf"].tolist() == [8, 16] and e["model"] == PP.GENERAL
