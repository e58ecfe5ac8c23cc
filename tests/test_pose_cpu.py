"""misift_recover_pose_batch without a GPU: pose_cases.expected_pose, the numpy float32 restatement of the definition in
include/misift.h, which tests/test_gpu_pose.py holds the device to byte for byte.  Here the restatement is pinned from
both sides: the library's host-only hooks misift_test_pose_decompose and misift_test_pose_vote, compiled from the
functions the kernel runs, must equal it byte for byte, and on planted scenes its answer must agree with a float64
decomposition and with the planted pose."""
import numpy as np
import pytest

import pose_cases as PC
from test_fundamental_cpu import GATES, f32, gate

EPS = 2.0 ** -24                                                 # half an ulp of 1: the rounding error of one operation


# ---- the hooks

def hook_decompose(F, K8):
    from cudasift_amd import capi
    F, K8 = np.ascontiguousarray(F, f32).reshape(9), np.ascontiguousarray(K8, f32).reshape(8)
    out, valid = np.full((4, 12), 3.5, f32), np.full(1, -77, np.int32)
    assert capi.lib().misift_test_pose_decompose(F.ctypes.data, K8.ctypes.data, out.ctypes.data, valid.ctypes.data) == 0
    return out, bool(valid[0])


def hook_vote(pose12, K8, xy):
    from cudasift_amd import capi
    pose12, K8 = np.ascontiguousarray(pose12, f32).reshape(12), np.ascontiguousarray(K8, f32).reshape(8)
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 4)
    front, xyz = np.full(len(xy), 7, np.uint8), np.full((len(xy), 4), 3.5, f32)
    assert capi.lib().misift_test_pose_vote(pose12.ctypes.data, K8.ctypes.data, xy.ctypes.data, len(xy),
                                            front.ctypes.data, xyz.ctypes.data) == 0
    assert set(np.unique(front)) <= {0, 1}
    return front.astype(bool), xyz


def hook_inliers(recs, n, F, thresh):
    """inl(F) from the Sampson terms of the library's hook."""
    from cudasift_amd import capi
    xy = PC.coordinates(recs, n)
    F = np.ascontiguousarray(F, f32).reshape(9)
    e2, den = np.zeros(len(xy), f32), np.zeros(len(xy), f32)
    assert capi.lib().misift_test_fundamental_sampson(F.ctypes.data, xy.ctypes.data, len(xy), e2.ctypes.data,
                                                      den.ctypes.data) == 0
    with np.errstate(all="ignore"):
        return gate(recs[:len(xy)], *GATES) & (e2 < (f32(thresh) * f32(thresh)) * den)


def hook_pose(recs, n, F, K8, thresh):
    """Steps 1-7 put together from the hooks: what expected_pose returns."""
    hyps, valid = hook_decompose(F, K8)
    xy = PC.coordinates(recs, n)
    votes = np.zeros(4, np.int32)
    if valid:
        member = hook_inliers(recs, n, F, thresh)
        for k in range(4):
            votes[k] = int((hook_vote(hyps[k], K8, xy)[0] & member).sum())
    best = int(np.argmax(votes))
    xyz = hook_vote(hyps[best], K8, xy)[1]
    if not valid:
        xyz[:] = PC.ONE_NAN
    return dict(pose=hyps[best].copy(), num_front=int(votes[best]), votes=votes, xyz=xyz, valid=valid, best=best,
                hyps=hyps)


def same_as_hooks(recs, n, F, K8, thresh, what):
    """The hooks equal the restatement byte for byte; returns expected_pose's dict."""
    with np.errstate(all="ignore"):
        e = PC.expected_pose(recs, n, F, K8, *GATES, thresh)
    h = hook_pose(recs, n, F, K8, thresh)
    assert h["valid"] == e["valid"] and h["hyps"].tobytes() == e["hyps"].tobytes(), (what, h["hyps"], e["hyps"])
    assert h["votes"].tolist() == e["votes"].tolist() and h["best"] == e["best"], (what, h["votes"], e["votes"])
    assert h["pose"].tobytes() == e["pose"].tobytes() and h["num_front"] == e["num_front"], what
    bad = np.nonzero((h["xyz"].view(np.uint32) != e["xyz"].view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (what, "xyz rows", bad[:8], h["xyz"][bad[:2]], e["xyz"][bad[:2]])
    return e


# ---- float64

def decompose64(E):
    """The four (R, t) of E in float64 by SVD: (4, 12), in the order of the definition up to which is which."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    out = []
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            out.append(np.concatenate([R.reshape(9), t]))
    return np.array(out)


def essential64(F, K8):
    K1, K2 = PC.kmat(K8[:4].astype(np.float64)), PC.kmat(K8[4:].astype(np.float64))
    return K2.T @ np.asarray(F, np.float64).reshape(3, 3) @ K1


def nearest(h64, pose):
    """The largest entry difference between pose (12,) and the closest of the four float64 hypotheses."""
    return float(np.abs(h64 - pose.astype(np.float64)).max(1).min())


def rotation_error(R, Rgt):
    """|| R Rgt^T - I ||_F: 2 sqrt(2) sin(angle / 2), well conditioned at small angles (an arccos of the trace is not)."""
    return float(np.linalg.norm(np.asarray(R, np.float64).reshape(3, 3) @ Rgt.T - np.eye(3)))


def direction_error(t, tgt):
    """|| t - tgt ||: 2 sin(angle / 2) between two unit vectors."""
    return float(np.linalg.norm(np.asarray(t, np.float64) - tgt))


# ---- tests

def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, the argument checks that need
    no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_recover_pose_batch", "misift_test_pose_decompose", "misift_test_pose_vote"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "recover_pose_batch")
    fr, K = np.zeros(1, np.int32), np.array(PC.K_A + PC.K_B, f32)
    assert L.misift_recover_pose_batch(None, 1, fr.ctypes.data, K.ctypes.data, None, 1, None, None, 8, 0.85, 0.95, 1.0,
                                       None, None, None, None, None) == -1          # MISIFT_EINVAL
    assert L.misift_recover_pose_batch(None, -1, None, None, None, 1, None, None, 8, 0.85, 0.95, 1.0, None, None, None,
                                       None, None) == -1
    assert L.misift_test_pose_decompose(None, None, None, None) == -1
    assert L.misift_test_pose_vote(None, None, None, 0, None, None) == -1
    assert L.misift_test_pose_vote(K.ctypes.data, K.ctypes.data, None, 1, None, None) == -1


@pytest.mark.parametrize("name,kw", PC.scenes(), ids=[s[0] for s in PC.scenes()])
def test_scenes_equal_the_hooks(name, kw):
    """Byte equality on every planted scene, and the scenes' premises: the planted hypothesis wins with at least 0.9 of
    the rows, and the runner-up gets at most 0.1."""
    s = PC.scene(kw)
    n = len(s["recs"])
    e = same_as_hooks(s["recs"], n, s["F"], s["K8"], PC.THRESH, name)
    assert e["valid"]
    order = np.sort(e["votes"])[::-1]
    print("%s: votes %s" % (name, e["votes"].tolist()))
    assert order[0] >= 0.9 * n and order[1] <= 0.1 * n, (name, e["votes"])
    assert rotation_error(e["pose"][:9], s["R"]) < 0.1 and direction_error(e["pose"][9:], s["t"]) < 0.35, name


ORTHO_BOUND = 24 * EPS


def test_rotations_are_rotations():
    """R^T R - I and det R - 1 of all four hypotheses of every valid entry, evaluated in float64 on the float32 R.

    The bound: an entry of R is a sum of three products of entries of u and v, which are unit and mutually orthogonal
    to a few roundings each (a division by a rounded square root, a rounded cross product, and columns that the
    Jacobi sweeps leave orthogonal to the last bit they can resolve); an entry of R^T R collects three such entries
    of each factor.  24 roundings of 2^-24, 1.43e-6, bounds that with room for nothing else; the largest values
    measured over the scenes and the valid hostile matrices were 8.27e-7 (R^T R - I) and 9.72e-7 (det R - 1)."""
    worst = [0.0, 0.0]
    cases = [(n, PC.scene(kw)["F"], PC.scene(kw)["K8"]) for n, kw in PC.scenes()]
    cases += [(n, F, K8) for n, F, K8, what in PC.hostile_matrices() if what == "valid"]
    for name, F, K8 in cases:
        hyps, valid = PC.decompose(F, K8)
        assert valid, name
        for k in range(4):
            R = hyps[k, :9].astype(np.float64).reshape(3, 3)
            worst[0] = max(worst[0], float(np.abs(R.T @ R - np.eye(3)).max()))
            worst[1] = max(worst[1], abs(float(np.linalg.det(R)) - 1))
            assert abs(float(np.linalg.norm(hyps[k, 9:].astype(np.float64))) - 1) <= 4 * EPS, (name, k)
    print("largest |R^T R - I| %.3g, largest |det R - 1| %.3g" % tuple(worst))
    assert worst[0] <= ORTHO_BOUND and worst[1] <= ORTHO_BOUND, worst


CHAIN_MEASURED = 4.13e-7                                           # see test_chain_against_float64
CHAIN_BOUND = 4 * CHAIN_MEASURED
SVD_MEASURED = 4.13e-7
SVD_BOUND = 4 * SVD_MEASURED


def test_chain_against_float64():
    """Steps 1-4 from the float32 F against a float64 SVD decomposition of K2^T F K1 of that same F (the whole chain), and
    steps 2-4 alone against a float64 decomposition of the float32 E of step 1: the largest entry difference of R and t
    between each of the four hypotheses and the closest float64 one.

    Measured over the 48 scenes: the whole chain differs by at most 4.13e-7 (CHAIN_MEASURED) and steps 2-4 alone by at
    most 4.13e-7 (SVD_MEASURED), the same scene setting both: the cancelling sums of step 1 (cx2 F00 cx1 is of the size
    of F22) cost no more than the decomposition does.  The bounds asserted are four times these, 1.65e-6."""
    chain = svd = 0.0
    for name, kw in PC.scenes():
        s = PC.scene(kw)
        hyps, valid = PC.decompose(s["F"], s["K8"])
        assert valid
        h64 = decompose64(essential64(s["F"], s["K8"]))
        e64 = decompose64(PC.essential(s["F"], s["K8"])[0])
        a, b = max(nearest(h64, hyps[k]) for k in range(4)), max(nearest(e64, hyps[k]) for k in range(4))
        print("%s: whole chain %.3g, steps 2-4 %.3g" % (name, a, b))
        chain, svd = max(chain, a), max(svd, b)
    print("largest: whole chain %.3g, steps 2-4 %.3g" % (chain, svd))
    assert chain <= CHAIN_BOUND and svd <= SVD_BOUND, (chain, svd)


TRUTH_R_MEASURED = 6.12e-7                                         # see test_exact_F_recovers_the_planted_pose
TRUTH_T_MEASURED = 1.49e-7
TRUTH_R_BOUND, TRUTH_T_BOUND = 4 * TRUTH_R_MEASURED, 4 * TRUTH_T_MEASURED


def test_exact_F_recovers_the_planted_pose():
    """With the exact F of the planted pose (rounded to float32) the picked pose against the planted one: the rotation as
    || R Rgt^T - I ||_F, the translation as || t - tgt ||.

    Measured over the 24 scenes with an exact F: at most 6.12e-7 for the rotation (TRUTH_R_MEASURED) and 1.49e-7 for
    the direction of t (TRUTH_T_MEASURED).  The bounds asserted are four times these, 2.45e-6 and 5.96e-7."""
    worst = [0.0, 0.0]
    for name, kw in PC.scenes():
        if kw["fit"]:
            continue
        s = PC.scene(kw)
        with np.errstate(all="ignore"):
            e = PC.expected_pose(s["recs"], len(s["recs"]), s["F"], s["K8"], *GATES, PC.THRESH)
        r, t = rotation_error(e["pose"][:9], s["R"]), direction_error(e["pose"][9:], s["t"])
        print("%s: rotation %.3g, direction %.3g" % (name, r, t))
        worst = [max(worst[0], r), max(worst[1], t)]
    print("largest: rotation %.3g, direction %.3g" % tuple(worst))
    assert worst[0] <= TRUTH_R_BOUND and worst[1] <= TRUTH_T_BOUND, worst


def test_hostile_matrices_equal_the_hook():
    """Each F is what it was chosen for, and the hook agrees byte for byte."""
    seen = {}
    for name, F, K8, what in PC.hostile_matrices():
        trace = []
        with np.errstate(all="ignore"):
            hyps, valid = PC.decompose(F, K8, trace=trace)
            E, A = PC.essential(F, K8)
        hh, hv = hook_decompose(F, K8)
        assert hv == valid and hh.tobytes() == hyps.tobytes(), (name, hh, hyps)
        assert valid == (what == "valid"), name
        if not valid:
            assert not hyps.any()
        seen[name] = (E, A, trace, hyps)
    assert seen["zeros"][1] is None and not seen["zeros"][0].any()
    assert np.isnan(seen["a NaN"][0]).any() and np.isinf(seen["an inf"][0]).any() and np.isinf(seen["E overflows"][0]).all()
    with np.errstate(all="ignore"):
        small, big = seen["near 1e-30"][0], seen["near 1e30"][0]
        assert (small * small).max() == 0 and np.isinf(big * big).any()      # without the prescale the norms are 0 or inf
    ref = PC.decompose(PC.scene(dict(seed=3))["F"], PC.scene(dict(seed=3))["K8"])[0]
    for name in ("near 1e-30", "near 1e30"):                     # the scale of F does not matter (nor its sign: which
        assert max(nearest(ref.astype(np.float64), h) for h in seen[name][3]) < 1e-5, name       # hypothesis is which)
    E, A, trace, _ = seen["one entry"]
    assert np.count_nonzero(E) == 1 and A is not None            # valid up to step 3: w[i2] = 0
    assert seen["gamma 0 in the first pair"][2][0] == 0 and any(g != 0 for g in seen["gamma 0 in the first pair"][2])
    assert not any(seen["forward motion"][2])                    # no rotation at all
    fwd = seen["forward motion"][3]
    assert fwd[2].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1] and fwd[3, 9:].tolist() == [0, 0, -1]


def test_hostile_frames_equal_the_hooks():
    """Each record set is what it was chosen for, and the hooks agree byte for byte."""
    seen = {}
    for name, recs, F, K8, thresh in PC.hostile_frames():
        e = same_as_hooks(recs, len(recs), F, K8, thresh, name)
        assert e["valid"], name
        seen[name] = (recs, e)
        print("%s: votes %s" % (name, e["votes"].tolist()))
    recs, e = seen["non-finite coordinates"]
    bad = ~np.isfinite(PC.coordinates(recs, len(recs))).all(1)
    assert bad.sum() >= 15 and e["num_front"] >= 150
    assert (e["xyz"][bad].view(np.uint32) == PC.NAN_BITS).all(1).sum() >= 15          # NaN and inf: four quiet NaNs
    assert np.isin(e["xyz"].view(np.uint32) & 0x7FFFFFFF, [PC.NAN_BITS]).sum() == np.isnan(e["xyz"]).sum()
    recs, e = seen["at the epipole"]
    xy = PC.coordinates(recs, len(recs))
    den = PC.depth_terms(e["pose"], K8, xy)[0]
    flat = np.nonzero(den == 0)[0]
    assert e["best"] == 2 and len(flat) >= 25 and (e["xyz"][flat].view(np.uint32) == PC.NAN_BITS).all()
    assert e["num_front"] == len(recs) - len(flat), (e["votes"], len(flat))
    recs, e = seen["behind both cameras"]
    planted = PC.planted(seed=13, n=100, behind=1.0)
    assert e["num_front"] >= 90 and direction_error(e["pose"][9:], -planted["t"]) < 0.1      # t comes out reversed
    front = [hook_vote(h, K8, PC.coordinates(recs, len(recs)))[0].sum() for h in e["hyps"]]
    assert min(front) == 0, front                                # the planted pose itself sees every record behind
    recs, e = seen["some behind both cameras"]
    planted = PC.planted(seed=14, n=100, behind=0.3)
    assert direction_error(e["pose"][9:], planted["t"]) < 0.1 and 55 <= e["num_front"] <= 85
    neg = (e["xyz"][:, 2] < 0) & (e["xyz"][:, 3] < 0)
    assert 15 <= neg.sum() <= 45, neg.sum()                      # negative depths are stored as computed


def test_entries_without_records():
    """A frame of count -1 or 0 with a valid F: hypothesis 0 and no vote; an invalid F: zeros and NaN rows."""
    s = PC.scene(dict(seed=3))
    for n in (-1, 0):
        e = same_as_hooks(s["recs"], n, s["F"], s["K8"], PC.THRESH, "count %d" % n)
        assert e["valid"] and e["best"] == 0 and e["num_front"] == 0 and not e["votes"].any() and len(e["xyz"]) == 0
        assert e["pose"].tobytes() == e["hyps"][0].tobytes() and e["pose"].any()
    e = same_as_hooks(s["recs"], 20, np.zeros(9, f32), s["K8"], PC.THRESH, "invalid")
    assert not e["valid"] and not e["pose"].any() and not e["votes"].any()
    assert (e["xyz"].view(np.uint32) == PC.NAN_BITS).all() and e["xyz"].shape == (20, 4)


CHAIN_SCENE_R_MEASURED, CHAIN_SCENE_T_MEASURED = 2.95e-4, 4.21e-3      # see test_chain_scene_recovers_the_planted_pose
CHAIN_SCENE_R_BOUND, CHAIN_SCENE_T_BOUND = 4 * CHAIN_SCENE_R_MEASURED, 4 * CHAIN_SCENE_T_MEASURED


def test_chain_scene_recovers_the_planted_pose():
    """find -> improve -> recover_pose restated on pose_cases.chain_scene(): 400 matches, a quarter of them wrong, 0.5 px
    noise.  The device runs the same chain in test_gpu_pose.py and is held to these bounds, too.

    Measured: 2.95e-4 for the rotation (|| R Rgt^T - I ||_F) and 4.21e-3 for the direction of t (|| t - tgt ||): the noise
    of the matches, not the arithmetic.  The bounds asserted are four times these, 1.18e-3 and 1.68e-2."""
    c = PC.expected_chain()
    s, e = c["scene"], c["pose"]
    r, t = rotation_error(e["pose"][:9], s["R"]), direction_error(e["pose"][9:], s["t"])
    print("chain scene: %d -> %d inliers, votes %s, rotation %.3g, direction %.3g" % (c["found"], c["fit"],
                                                                                     e["votes"].tolist(), r, t))
    assert c["found"] >= 150 and c["fit"] >= c["found"] and e["num_front"] >= 0.95 * c["fit"]
    assert r <= CHAIN_SCENE_R_BOUND and t <= CHAIN_SCENE_T_BOUND, (r, t)
