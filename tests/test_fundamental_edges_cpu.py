"""The inputs of fundamental_cases.py without a GPU: at every one of them the numpy restatement of test_fundamental_cpu
equals the library's host hooks byte for byte, and the facts the GPU file (test_gpu_fundamental_edges.py) relies on hold:
the scale sweep holds a denormal sqrtf argument, a valid F with subnormal entries and invalid samples at both ends; the
lattice samples hold pivot ties; the extreme thresholds count nothing or everything; the mixed scenes still have an
all-inlier sample, and the picked F counts every finite planted inlier and no hostile record.

NaN: the payload and sign of a computed NaN are the processor's choice, so e*e and den are compared with every NaN mapped
to one; match_error is an output and is compared bit for bit (the header stores the one quiet NaN 0x7fc00000)."""
import numpy as np
import pytest

import fundamental_cases as FC
from test_fundamental_cpu import (GATES, _same_solve, expected_find, expected_score, f32, fundamental_error, gate,
                                  hypotheses, planted_scene, sampson, sampson64, solve8)


def _one_nan(a):
    a = np.array(a, f32)
    a[np.isnan(a)] = np.uint32(FC.NAN_BITS).view(f32)
    return a


# ---- forced samples

def test_forced_samples_equal_the_hook():
    named = FC.forced_samples()
    names = [n for n, _ in named]
    F, ok = _same_solve(np.stack([s for _, s in named]))         # byte equality with misift_test_fundamental_solve
    by = dict(zip(names, zip(F, ok)))
    for n in names[:2] + [n for n in names if "column" in n] + ["two points"]:
        assert not by[n][1] and (by[n][0].view(np.uint32) == 0).all(), n
    assert by["plain"][1] and by["slanted line"][1]              # rounding hides the slanted line's deficiency
    # the three kinds of the sweep
    args = {n: FC.sqrt_arguments(s) for n, s in named if n.startswith("scale")}
    denormal_sqrt = [n for n, a in args.items() if FC.is_subnormal(a).any() and by[n][1]]
    subnormal_F = [n for n in args if by[n][1] and FC.is_subnormal(by[n][0]).any()]
    assert len(denormal_sqrt) == 3, denormal_sqrt                # valid although a sqrtf argument is a denormal
    assert len(subnormal_F) == 4 and all("1e+19" in n for n in subnormal_F), subnormal_F
    scale = {n: float(n.split()[1]) for n in args}
    assert all(not by[n][1] for n in args if scale[n] <= 1e-19 or scale[n] >= 1e20)
    assert all(by[n][1] for n in args if 1e-18 <= scale[n] <= 1e19)
    assert not any(FC.is_subnormal(by[n][0]).any() for n in args if scale[n] == 1e18)
    assert len(set(scale.values())) >= 48 + 4
    # the lattices: valid, with a tie in the pivot search
    for i, s in enumerate(FC.LATTICES):
        assert by["lattice %d" % i][1] and FC.pivot_ties(s) >= 1, i
    assert FC.pivot_ties(dict(named)["plain"]) == 0


def test_forced_frames_hold_exactly_the_sample():
    for i, (name, s) in enumerate(FC.forced_samples()[:6]):
        fr = FC.forced_frame(s, 8 + i * 8, i)
        v = gate(fr, *GATES)
        assert v.sum() == 8 and len(fr) == 16 + i * 8
        got = np.stack([fr[k][v] for k in FC.POS], 1)
        assert got.tobytes() == np.asarray(s, f32).tobytes(), name
        assert (~np.isfinite(np.stack([fr[k][~v] for k in FC.POS]))).sum() >= 2 + 2 * i      # the rejected rows are hostile


# ---- Sampson and error terms

@pytest.mark.parametrize("name,F", FC.score_matrices(), ids=[n for n, _ in FC.score_matrices()])
def test_sampson_and_error_terms(name, F):
    from cudasift_amd import capi
    L = capi.lib()
    n = 2000
    recs = FC.score_frame(n, 31)
    xy = np.ascontiguousarray(np.stack([recs[k] for k in FC.POS], 1))
    e2, den, err = (np.full(n, 3.5, f32) for _ in range(3))
    assert L.misift_test_fundamental_sampson(F.ctypes.data, xy.ctypes.data, n, e2.ctypes.data, den.ctypes.data) == 0
    ee, dd = sampson(F, *xy.T)
    assert _one_nan(e2).tobytes() == _one_nan(ee[0]).tobytes()
    assert _one_nan(den).tobytes() == _one_nan(dd[0]).tobytes()
    assert L.misift_test_fundamental_error(e2.ctypes.data, den.ctypes.data, n, err.ctypes.data) == 0
    want = fundamental_error(ee[0], dd[0])
    assert err.tobytes() == want.tobytes()
    out, fit = expected_score(recs, n, F, *GATES, 1.0)
    assert out["match_error"].tobytes() == want.tobytes()
    nan = np.isnan(want)
    assert (want[nan].view(np.uint32) == FC.NAN_BITS).all()
    with np.errstate(invalid="ignore"):
        assert np.isposinf(want[~(dd[0] > 0)]).all()
    with np.errstate(all="ignore"):
        assert fit == int((gate(recs, *GATES) & (ee[0] < dd[0])).sum())
    if name in ("nan", "-0"):
        assert np.isposinf(want).all() and fit == 0
    if name == "1e-30":                                          # den underflows to 0 wherever the positions are small
        small = np.abs(xy).max(1) < 1e6
        assert small.sum() > 100 and (dd[0][small] == 0).all() and np.isposinf(want[small]).all()
    if name == "1e30":                                           # den overflows: inf / inf
        plain = (np.abs(xy).max(1) < 1920) & (np.abs(xy).min(1) > 1)
        assert plain.sum() > 100 and np.isposinf(dd[0][plain]).all() and np.isnan(want[plain]).all()
    if name == "subnormal":
        assert FC.is_subnormal(F).all()
    if name == "rank 3":
        assert abs(np.linalg.det(F.reshape(3, 3).astype(np.float64))) > 1e-3
        assert np.isfinite(want).sum() > 100


def test_error_hook_on_signed_nans():
    """Every NaN the square root can see (either sign, any payload) comes out as 0x7fc00000, den <= 0 or NaN as +inf."""
    from cudasift_amd import capi
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0x3F800000, 0, 0x80000000, 1],
                    np.uint32).view(f32)
    e2, den = (np.ascontiguousarray(v.ravel()) for v in np.meshgrid(bits, bits))
    out = np.full(len(e2), 3.5, f32)
    assert capi.lib().misift_test_fundamental_error(e2.ctypes.data, den.ctypes.data, len(e2), out.ctypes.data) == 0
    want = fundamental_error(e2, den)
    assert out.tobytes() == want.tobytes()
    with np.errstate(all="ignore"):
        assert np.isposinf(out[~(den > 0)]).all()
    assert (out[np.isnan(out)].view(np.uint32) == FC.NAN_BITS).all() and np.isnan(out).sum() >= 8
    assert capi.lib().misift_test_fundamental_error(None, None, 1, out.ctypes.data) == -1


# ---- thresholds

def test_extreme_thresholds():
    c = FC.THRESH_SCENE
    recs, _, _ = planted_scene(c["seed"], n=c["n"])
    _, Fh, _ = hypotheses(recs, c["n"], c["find_seed"], c["loops"], *GATES, 1.0)
    assert np.abs(Fh[0]).max() > 0
    with np.errstate(over="ignore"):
        for t, want in zip(FC.THRESHOLDS, (0, 0, c["n"], c["n"], c["n"])):
            F, n = expected_find(recs, c["n"], c["find_seed"], c["loops"], *GATES, t, 256)
            _, fit = expected_score(recs, c["n"], F, *GATES, t)
            assert n == want and fit == want, (t, n, fit)
            assert F.tobytes() == Fh[0].tobytes(), t             # every count equal: hypothesis 0's F


# ---- gate values

def test_gate_values():
    recs, passes = FC.gate_frame(1)
    assert (gate(recs, *GATES) == passes).all()
    assert 8 <= passes.sum() < len(passes)
    vals = FC.gate_values()
    assert vals[6][0] > f32(GATES[0]) and vals[7][1] < f32(GATES[1])
    assert np.nextafter(vals[6][0], f32(0)) == f32(GATES[0]) and np.nextafter(vals[7][1], f32(1)) == f32(GATES[1])


# ---- mixed scenes

@pytest.mark.parametrize("loops", FC.MIXED_LOOPS)
@pytest.mark.parametrize("seed", FC.MIXED_SEEDS)
def test_mixed_scene(seed, loops):
    """A tenth of the records hostile: some sample is still all-finite and all-inlier, the picked F counts every finite
    planted inlier and no hostile record, and its float64 residual on the finite planted inliers stays below the 0.05 px
    that test_planted_scene_against_float64_geometry derives (the same inputs, the same reasoning)."""
    recs, inl, hostile = FC.mixed_scene(seed)
    n = len(recs)
    fin = inl & ~hostile
    assert hostile.sum() == n // 10 and gate(recs, *GATES).all()
    idx, F, counts = hypotheses(recs, n, FC.MIXED_FIND_SEED, loops, *GATES, 1.0)
    _, ok = solve8(*[recs[k][idx] for k in FC.POS])
    good = int(fin[idx].all(1).sum())
    print("scene %d, %d loops: %d all-finite all-inlier samples, %d invalid hypotheses" % (seed, loops, good,
                                                                                          (~ok).sum()))
    assert good >= 1 and (~ok).sum() >= loops // 4
    Fp, c = expected_find(recs, n, FC.MIXED_FIND_SEED, loops, *GATES, 1.0, max_pts=608)
    e2, den = sampson(Fp, *[recs[k] for k in FC.POS])
    with np.errstate(invalid="ignore"):
        counted = e2[0] < den[0]
    assert counted[fin].all() and not counted[hostile].any() and c == counted.sum()
    assert fin.sum() <= c <= fin.sum() + 3                       # a 1 px band catches about 2 / 1080 of the 150 outliers
    out, fit = expected_score(recs, n, Fp, *GATES, 1.0)
    assert fit == c and (out["match_error"][fin] < 1.0).all()
    bad = hostile & ~np.isfinite(np.stack([recs[k] for k in FC.POS])).all(0)
    assert bad.sum() >= 20 and not (out["match_error"][bad] < 1.0).any()
    d = sampson64(Fp, recs[fin])
    print("count %d of %d finite planted inliers, float64 residual max %.2e px" % (c, fin.sum(), d.max()))
    assert d.max() < 0.05, d.max()
