"""misift_find_fundamental_batch / misift_score_fundamental_batch without a GPU: expected_find and expected_score, the
numpy restatement of the definition in include/misift.h (op by op in float32, vectorised over the hypotheses), which
tests/test_gpu_fundamental.py holds the device to byte for byte.  Here the restatement is pinned from both sides: the
library's host-only hooks, compiled from the headers the kernels include, must equal it byte for byte, and on planted
two-view scenes its answers must agree with float64 epipolar geometry."""
import numpy as np
import pytest

f32 = np.float32
GATES = (0.85, 0.95)                                             # min_score, max_ambiguity
SCALE = f32(11.3137085)                                          # 8 sqrt(2) as the header writes it


# ---- the expected answer, restated in numpy

def libc_stream(seed, n):
    """The first n values of rand() after srand(seed), from the library's restatement (pinned to libc itself in
    test_homography_batch_cpu)."""
    from cudasift_amd import capi
    out = np.zeros(n, np.int32)
    assert capi.lib().misift_test_libc_rand(seed, n, out.ctypes.data) == 0
    return out


def draw8(seed, num_valid, num_loops):
    """(num_loops, 8) positions: per hypothesis eight draws first, then p[1..7] in turn redrawn while they repeat an
    earlier one; all hypotheses from one stream."""
    need = 64 * num_loops + 64
    while True:
        r = iter(libc_stream(seed, need).tolist())
        out = np.zeros((num_loops, 8), np.int64)
        try:
            for i in range(num_loops):
                p = [next(r) % num_valid for _ in range(8)]
                for k in range(1, 8):
                    while p[k] in p[:k]:
                        p[k] = next(r) % num_valid
                out[i] = p
            return out
        except StopIteration:
            need *= 4


def _normalise(x, y):
    L = x.shape[0]
    sx, sy = np.zeros(L, f32), np.zeros(L, f32)
    for k in range(8):
        sx = sx + x[:, k]
        sy = sy + y[:, k]
    cx, cy = sx * f32(0.125), sy * f32(0.125)
    d = np.zeros(L, f32)
    for k in range(8):
        dx, dy = x[:, k] - cx, y[:, k] - cy
        d = d + np.sqrt(dx * dx + dy * dy)
    return cx, cy, SCALE / d


def _finite(v):
    return np.abs(v) <= f32(3.402823466e+38)


def solve8(x1, y1, x2, y2):
    """x*, y*: (L, 8) float32, one sample per row.  Returns F (L, 9) float32 and valid (L,); invalid rows are zeros."""
    x1, y1, x2, y2 = (np.ascontiguousarray(v, f32) for v in (x1, y1, x2, y2))
    L = x1.shape[0]
    ar = np.arange(L)
    with np.errstate(all="ignore"):
        c1x, c1y, s1 = _normalise(x1, y1)
        c2x, c2y, s2 = _normalise(x2, y2)
        u1, v1 = (x1 - c1x[:, None]) * s1[:, None], (y1 - c1y[:, None]) * s1[:, None]
        u2, v2 = (x2 - c2x[:, None]) * s2[:, None], (y2 - c2y[:, None]) * s2[:, None]
        A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], 2).astype(f32)   # L, 8, 9
        col = np.tile(np.arange(9), (L, 1))
        ok = np.ones(L, bool)
        for k in range(8):
            mag = np.abs(A[:, k:, k:]).reshape(L, -1)
            mag = np.where(np.isnan(mag), f32(-1), mag)          # a NaN never wins
            j = np.argmax(mag, 1)                                # row-major, the first maximum
            pr, pc = k + j // (9 - k), k + j % (9 - k)
            t = A[ar, k, :].copy(); A[ar, k, :] = A[ar, pr, :]; A[ar, pr, :] = t            # noqa: E702
            t = A[ar, :, k].copy(); A[ar, :, k] = A[ar, :, pc]; A[ar, :, pc] = t            # noqa: E702
            t = col[ar, k].copy(); col[ar, k] = col[ar, pc]; col[ar, pc] = t                # noqa: E702
            piv = A[:, k, k].copy()
            ok &= (piv != 0) & _finite(piv)
            for r in range(k + 1, 8):
                f = A[:, r, k] / piv
                A[:, r, k + 1:] = A[:, r, k + 1:] - f[:, None] * A[:, k, k + 1:]
        z = np.zeros((L, 9), f32)
        z[:, 8] = 1
        for k in range(7, -1, -1):
            s = np.zeros(L, f32)
            for c in range(k + 1, 9):
                s = s + A[:, k, c] * z[:, c]
            z[:, k] = (-s) / A[:, k, k]
        n = np.zeros((L, 9), f32)
        n[ar[:, None], col] = z
        t1x, t1y, t2x, t2y = -(s1 * c1x), -(s1 * c1y), -(s2 * c2x), -(s2 * c2y)
        g = np.zeros((L, 9), f32)
        for i in range(3):
            g[:, 3 * i + 0] = n[:, 3 * i + 0] * s1
            g[:, 3 * i + 1] = n[:, 3 * i + 1] * s1
            g[:, 3 * i + 2] = (n[:, 3 * i + 0] * t1x + n[:, 3 * i + 1] * t1y) + n[:, 3 * i + 2]
        F = np.zeros((L, 9), f32)
        for j in range(3):
            F[:, 0 + j] = s2 * g[:, 0 + j]
            F[:, 3 + j] = s2 * g[:, 3 + j]
            F[:, 6 + j] = (t2x * g[:, 0 + j] + t2y * g[:, 3 + j]) + g[:, 6 + j]
        ok &= _finite(F).all(1)
    F[~ok] = 0
    return F, ok


def sampson(F, x1, y1, x2, y2):
    """e*e and den of every match (N,) under every F (L, 9): two (L, N) float32 arrays."""
    F = np.ascontiguousarray(F, f32).reshape(-1, 9)
    Fk = [F[:, k][:, None] for k in range(9)]
    x1, y1, x2, y2 = (np.ascontiguousarray(v, f32)[None, :] for v in (x1, y1, x2, y2))
    with np.errstate(all="ignore"):
        a0 = Fk[0] * x1 + Fk[1] * y1 + Fk[2]
        a1 = Fk[3] * x1 + Fk[4] * y1 + Fk[5]
        a2 = Fk[6] * x1 + Fk[7] * y1 + Fk[8]
        b0 = Fk[0] * x2 + Fk[3] * y2 + Fk[6]
        b1 = Fk[1] * x2 + Fk[4] * y2 + Fk[7]
        e = x2 * a0 + y2 * a1 + a2
        den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1
        return e * e, den


def gate(recs, min_score, max_ambiguity):
    with np.errstate(invalid="ignore"):
        return (recs["score"] > f32(min_score)) & (recs["ambiguity"] < f32(max_ambiguity))


def hypotheses(recs, n, seed, num_loops, min_score, max_ambiguity, thresh):
    """Every hypothesis of a frame that takes part (8 <= n, at least 8 valid): (samples as record indices (L, 8),
    F (L, 9), counts (L,)), or None."""
    if n < 8:
        return None
    p = recs[:n]
    v = np.nonzero(gate(p, min_score, max_ambiguity))[0]
    if len(v) < 8:
        return None
    idx = v[draw8(seed, len(v), num_loops)]
    x1, y1, x2, y2 = p["xpos"], p["ypos"], p["match_xpos"], p["match_ypos"]
    F, _ = solve8(x1[idx], y1[idx], x2[idx], y2[idx])
    e2, den = sampson(F, x1[v], y1[v], x2[v], y2[v])
    t2 = f32(thresh) * f32(thresh)
    with np.errstate(all="ignore"):
        counts = (e2 < t2 * den).sum(1)
    return idx, F, counts


def expected_find(recs, n, seed, num_loops, min_score, max_ambiguity, thresh, max_pts):
    """(F as 9 float32, the inlier count) of one entry: recs = the frame's records, n = its device count."""
    if n > max_pts:
        return np.zeros(9, f32), -1
    h = hypotheses(recs, n, seed, num_loops, min_score, max_ambiguity, thresh)
    if h is None:
        return np.zeros(9, f32), 0
    _, F, counts = h
    best = int(np.argmax(counts))                                # the largest count at the smallest index
    return F[best].copy(), int(counts[best])


def fundamental_error(e2, den):
    """match_error from the Sampson terms: +inf where den > 0 is false, and the one quiet NaN 0x7fc00000 for a NaN."""
    with np.errstate(all="ignore"):
        d = np.sqrt(np.asarray(e2, f32) / np.asarray(den, f32))
        d = np.where(np.isnan(d), np.uint32(0x7FC00000).view(f32), d)
        return np.where(den > 0, d, f32(np.inf)).astype(f32)


def expected_score(recs, n, F, min_score, max_ambiguity, thresh):
    """(the frame's records with match_error of rows < max(n, 0) rewritten, num_fit)."""
    out = recs.copy()
    n = max(int(n), 0)
    p = out[:n]
    e2, den = sampson(F, p["xpos"], p["ypos"], p["match_xpos"], p["match_ypos"])
    e2, den = e2[0], den[0]
    t2 = f32(thresh) * f32(thresh)
    with np.errstate(all="ignore"):
        err = fundamental_error(e2, den)
        fit = gate(p, min_score, max_ambiguity) & (e2 < t2 * den)
    out["match_error"][:n] = err
    return out, int(fit.sum())


# ---- planted two-view scenes

def planted_scene(seed, n=2000, outliers=0.25, noise=0.0):
    """n matches between two 1920 x 1080 pinhole views of random 3-D points, `outliers` of them (at random rows) replaced
    by uniform random positions in the second view.  Returns (records that pass GATES, planted-inlier mask, the float64
    ground-truth F with (x2, y2, 1) F (x1, y1, 1)^T = 0)."""
    from cudasift_amd import capi
    rng = np.random.default_rng(seed)
    X = rng.uniform([-4, -3, 6], [4, 3, 14], (n, 3))
    K = np.array([[1400.0, 0, 960], [0, 1400, 540], [0, 0, 1]])
    a = 0.05 + 0.05 * (seed % 5)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([1.0, 0.1, 0.2])
    p1 = (K @ X.T).T
    p1 = p1[:, :2] / p1[:, 2:]
    p2 = (K @ (R @ X.T + t[:, None])).T
    p2 = p2[:, :2] / p2[:, 2:]
    if noise:
        p2 = p2 + rng.normal(0, noise, (n, 2))
    inl = np.ones(n, bool)
    inl[rng.choice(n, int(n * outliers), replace=False)] = False
    p2[~inl] = rng.uniform([0, 0], [1920, 1080], (int((~inl).sum()), 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    Fgt = Ki.T @ tx @ R @ Ki
    recs = np.zeros(n, capi.POINT_DTYPE)
    recs["xpos"], recs["ypos"], recs["match_xpos"], recs["match_ypos"] = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    recs["score"], recs["ambiguity"], recs["match"] = 0.97, 0.3, np.arange(n)
    recs["match_error"] = -7.0
    return recs, inl, Fgt


def sampson64(F, recs):
    """The Sampson distance of every record under F, in float64."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    h1 = np.stack([recs["xpos"], recs["ypos"], np.ones(len(recs))], 1).astype(np.float64)
    h2 = np.stack([recs["match_xpos"], recs["match_ypos"], np.ones(len(recs))], 1).astype(np.float64)
    a, b = h1 @ F.T, h2 @ F
    e = (h2 * a).sum(1)
    return np.abs(e) / np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


SCENE_SEEDS = (1, 2, 3)
SCENE_LOOPS = 256
SCENE_FIND_SEED = 77


# ---- tests

def test_library_exports_the_calls():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the bindings, the NULL-context checks."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_find_fundamental_batch", "misift_score_fundamental_batch", "misift_test_fundamental_samples",
                 "misift_test_fundamental_solve", "misift_test_fundamental_sampson", "misift_test_fundamental_error"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "find_fundamental_batch") and hasattr(capi.Context, "score_fundamental_batch")
    fr, sd = np.zeros(1, np.int32), np.ones(1, np.uint32)
    assert L.misift_find_fundamental_batch(None, 1, fr.ctypes.data, sd.ctypes.data, None, 1, None, None, 8, 8, 16, 0.85,
                                           0.95, 1.0, None, None) == -1                     # MISIFT_EINVAL
    assert L.misift_score_fundamental_batch(None, 1, fr.ctypes.data, None, 1, None, None, 8, 0.85, 0.95, 1.0, None,
                                            None) == -1
    assert SCALE == f32(8 * np.sqrt(2.0))


@pytest.mark.parametrize("seed", [0, 7, 2**32 - 1])
@pytest.mark.parametrize("num_valid", [8, 9, 1000])
@pytest.mark.parametrize("num_loops", [1, 17, 300])
def test_fundamental_samples(seed, num_valid, num_loops):
    from cudasift_amd import capi
    got = np.zeros((num_loops, 8), np.int32)
    assert capi.lib().misift_test_fundamental_samples(seed, num_valid, num_loops, got.ctypes.data) == 0
    assert np.array_equal(got, draw8(seed, num_valid, num_loops))
    assert all(len(set(row)) == 8 for row in got.tolist()) and got.min() >= 0 and got.max() < num_valid


def test_sample_hook_arguments():
    from cudasift_amd import capi
    out = np.zeros(64, np.int32)
    assert capi.lib().misift_test_fundamental_samples(1, 7, 4, out.ctypes.data) == -1       # fewer than 8 valid records
    assert capi.lib().misift_test_fundamental_samples(1, 8, -1, out.ctypes.data) == -1
    assert capi.lib().misift_test_fundamental_samples(1, 8, 2, None) == -1


def _hook_solve(xy):
    from cudasift_amd import capi
    xy = np.ascontiguousarray(xy, f32).reshape(8, 4)
    F, ok = np.full(9, 3.5, f32), np.full(1, 77, np.int32)
    assert capi.lib().misift_test_fundamental_solve(xy.ctypes.data, F.ctypes.data, ok.ctypes.data) == 0
    return F, int(ok[0])


def _same_solve(samples):
    """samples (L, 8, 4): the hook on each equals the restatement on all, byte for byte.  Returns (F, valid)."""
    samples = np.ascontiguousarray(samples, f32)
    F, ok = solve8(samples[:, :, 0], samples[:, :, 1], samples[:, :, 2], samples[:, :, 3])
    for i, xy in enumerate(samples):
        Fh, okh = _hook_solve(xy)
        assert okh == int(ok[i]) and Fh.tobytes() == F[i].tobytes(), (i, okh, ok[i], Fh, F[i])
    return F, ok


def test_solve_on_random_samples():
    rng = np.random.default_rng(3)
    F, ok = _same_solve(rng.uniform(0, 1920, (300, 8, 4)))
    assert ok.all() and (np.abs(F).max(1) > 0).all()
    recs, inl, _ = planted_scene(1)
    idx = np.nonzero(inl)[0][rng.integers(0, inl.sum(), (200, 8))]
    xy = np.stack([recs[k][idx] for k in ("xpos", "ypos", "match_xpos", "match_ypos")], 2)
    _same_solve(xy)
    _same_solve(rng.uniform(-1e-3, 1e-3, (50, 8, 4)))            # tiny and huge magnitudes
    _same_solve(rng.uniform(-1e18, 1e18, (50, 8, 4)))


def test_solve_on_degenerate_samples():
    rng = np.random.default_rng(4)
    base = rng.uniform(0, 1920, (8, 4)).astype(f32)
    same = np.tile(base[:1], (8, 1))                             # 8 identical points: d = 0, s = inf
    # collinear in both views, on horizontal lines at integer y: the centred y is exactly 0, five columns vanish
    line = base.copy()
    line[:, 1], line[:, 3] = 300.0, 512.0
    bad = []
    for v in (np.inf, -np.inf, np.nan):
        for c in range(4):
            s = base.copy()
            s[int(rng.integers(0, 8)), c] = v
            bad.append(s)
    F, ok = _same_solve(np.stack([same, line] + bad))
    assert not ok.any() and (F.view(np.uint32) == 0).all()
    slanted = base.copy()                                        # a slanted line: rounding decides; only equality is claimed
    slanted[:, 1], slanted[:, 3] = f32(0.37) * slanted[:, 0] + f32(11), f32(-1.3) * slanted[:, 2] + f32(900)
    two = base.copy()                                            # only two distinct points
    two[2:] = two[1]
    _same_solve(np.stack([slanted, two]))


def test_sampson_terms():
    from cudasift_amd import capi
    rng = np.random.default_rng(5)
    xy = rng.uniform(0, 1920, (500, 4)).astype(f32)
    xy[7, 0], xy[9, 3], xy[11, 2] = np.nan, np.inf, -np.inf
    for F in (rng.normal(0, 1, 9), rng.normal(0, 1e-6, 9), np.zeros(9), np.full(9, np.nan), np.full(9, 1e30)):
        F = np.ascontiguousarray(F, f32)
        e2, den = np.full(500, 3.5, f32), np.full(500, 3.5, f32)
        assert capi.lib().misift_test_fundamental_sampson(F.ctypes.data, xy.ctypes.data, 500, e2.ctypes.data,
                                                          den.ctypes.data) == 0
        ee, dd = sampson(F, xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3])
        assert e2.tobytes() == ee[0].tobytes() and den.tobytes() == dd[0].tobytes()


def test_entries_that_take_no_part():
    recs, _, _ = planted_scene(1, n=64)
    z = np.zeros(9, f32)
    for n, want in ((0, 0), (7, 0), (-1, 0), (65, -1)):
        F, c = expected_find(recs, n, 1, 16, *GATES, 1.0, max_pts=64)
        assert c == want and F.tobytes() == z.tobytes()
    recs["score"][7:] = 0.1                                      # 7 valid records
    F, c = expected_find(recs, 64, 1, 16, *GATES, 1.0, max_pts=64)
    assert c == 0 and F.tobytes() == z.tobytes()
    out, fit = expected_score(recs, 64, z, *GATES, 1.0)
    assert fit == 0 and np.isposinf(out["match_error"]).all()


@pytest.mark.parametrize("seed", SCENE_SEEDS)
def test_planted_scene_against_float64_geometry(seed):
    """Noise-free scene, thresh 1: some sample is all-inlier, the picked F counts every planted inlier, expected_score
    puts them below thresh, and in float64 the planted matches lie on the picked F's epipolar lines.

    The bound on that float64 residual, 0.05 px: the positions are rounded to float32 (half an ulp at 1024..2048 is
    6e-5 px) and a minimal 8-point solve amplifies input error by the conditioning of its sample, two to three orders
    of magnitude for 8 random points of a wide-baseline scene; an F from a contaminated sample, the failure this test
    looks for, leaves residuals of the order of the threshold, 1 px."""
    recs, inl, Fgt = planted_scene(seed)
    assert inl.sum() == 1500
    assert sampson64(Fgt, recs[inl]).max() < 1e-3                # the ground truth itself, on float32 positions
    idx, F, counts = hypotheses(recs, len(recs), SCENE_FIND_SEED, SCENE_LOOPS, *GATES, 1.0)
    assert inl[idx].all(1).any(), "no all-inlier sample: choose another seed"
    Fp, c = expected_find(recs, len(recs), SCENE_FIND_SEED, SCENE_LOOPS, *GATES, 1.0, max_pts=2048)
    assert c == counts.max() and Fp.tobytes() == F[int(np.argmax(counts))].tobytes()
    e2, den = sampson(Fp, recs["xpos"], recs["ypos"], recs["match_xpos"], recs["match_ypos"])
    counted = e2[0] < den[0]
    assert counted[inl].all(), int((~counted[inl]).sum())
    assert counted[~inl].sum() <= 10, int(counted[~inl].sum())   # a 1 px band around a line catches about 2 / 1080 of the 500
    assert c == counted.sum()
    out, fit = expected_score(recs, len(recs), Fp, *GATES, 1.0)
    assert fit == c and (out["match_error"][inl] < 1.0).all()
    for k in out.dtype.names:
        if k != "match_error":
            assert out[k].tobytes() == recs[k].tobytes(), k
    d = sampson64(Fp, recs[inl])
    print("scene %d: count %d, outliers counted %d, float64 residual of the planted matches max %.2e px"
          % (seed, c, counted[~inl].sum(), d.max()))
    assert d.max() < 0.05, d.max()
