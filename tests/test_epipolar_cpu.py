"""misift_match_epipolar_batch without a GPU: the gate and the gather, through the library's host-only hooks, which are
compiled from the header and the functions the kernel runs (epipolar_core.hpp, the grid function and the span functions
of kernels_guided.hip).

- The gate hook must equal the numpy float32 restatement of the contract byte for byte.
- The gather must be conservative: every record that passes the gate lies in a cell the row visits.  The cases aim at
  the absolute rounding error of e, which does not shrink with the radius: points at radius (1 +- k 2^-20) from the line,
  coordinates up to 1e5, radii down to 1e-3, axis-parallel and diagonal lines, corners, degenerate grids.
- The gather must be selective, so that "visit everything" cannot pass: a generic line crosses at most gx + gy - 1 = 127
  of the 4096 cells and the band adds at most one cell on each side, 381 cells = 9.3 %; the bound of 0.15 leaves the
  rest for slab margins.  A rectified-stereo line touches at most 2 grid rows plus margin: 3/64 + 0.02."""
import numpy as np
import pytest

from epipolar_util import STEREO, STEREO_V, f32, gate_np, lines_np, planted_F, points_on_lines

RADII = (1e-30, 1e-3, 0.5, 2.0, 64.0, float("inf"))


def _hooks(F, xy1, xy2, radius):
    """(pass, visited, (gx, gy)) from the two hooks."""
    from cudasift_amd import capi
    L = capi.lib()
    F = np.ascontiguousarray(F, f32).reshape(9)
    xy1 = np.ascontiguousarray(xy1, f32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, f32).reshape(-1, 2)
    n1, n2 = len(xy1), len(xy2)
    ps = np.full((n1, n2), 7, np.uint8)
    vis = np.full((n1, n2), 7, np.uint8)
    g = np.zeros(2, np.int32)
    assert L.misift_test_epipolar_gate(F.ctypes.data, xy1.ctypes.data, n1, xy2.ctypes.data, n2, radius,
                                       ps.ctypes.data) == 0
    assert L.misift_test_epipolar_gather(F.ctypes.data, xy1.ctypes.data, n1, xy2.ctypes.data, n2, radius,
                                         vis.ctypes.data, g.ctypes.data) == 0
    assert ((ps | vis) <= 1).all()
    return ps.astype(bool), vis.astype(bool), (int(g[0]), int(g[1]))


def _check(F, xy1, xy2, radius, what):
    """Gate == numpy, pass within visited.  Returns (pass, visited, grid)."""
    xy1 = np.ascontiguousarray(xy1, f32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, f32).reshape(-1, 2)
    ps, vis, g = _hooks(F, xy1, xy2, radius)
    exp = gate_np(F, xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1], radius)
    assert np.array_equal(ps, exp), (what, "gate differs from numpy in", int((ps != exp).sum()))
    missed = ps & ~vis
    assert not missed.any(), (what, "candidates in unvisited cells", np.argwhere(missed)[:4].tolist(), g)
    return ps, vis, g


def _scene(seed, n1=120, n2=400):
    """Rows and records on 1920 x 1080; the first n1 records sit near the rows' lines under planted_F(seed)."""
    rng = np.random.default_rng(seed)
    F = planted_F(seed)
    xy1 = np.stack([rng.uniform(0, 1920, n1), rng.uniform(0, 1080, n1)], 1).astype(f32)
    across = rng.choice([0.0, 5e-4, 0.3, 0.49, 0.51, 1.9, 2.1, 60.0], n1) * rng.choice([-1.0, 1.0], n1)
    x, y, _ = points_on_lines(F, xy1[:, 0], xy1[:, 1], rng, across)
    xy2 = np.stack([rng.uniform(0, 1920, n2), rng.uniform(0, 1080, n2)], 1)
    xy2[:n1, 0], xy2[:n1, 1] = x, y
    return F, xy1, xy2.astype(f32)


# ---- the gate

@pytest.mark.parametrize("radius", RADII)
def test_gate_hook_equals_numpy(radius):
    total = 0
    for seed in range(4):
        F, xy1, xy2 = _scene(seed)
        ps, _, _ = _check(F, xy1, xy2, radius, "planted %d" % seed)
        total += int(ps.sum())
        if radius == float("inf"):
            assert ps.all()
    if 1e-3 <= radius:
        assert total > 50, total                                  # the planted points are found
    F, xy1, xy2 = _scene(9)
    xy2[5] = (np.nan, 3.0)
    xy2[6] = (np.inf, 3.0)
    xy2[7] = (4.0, -np.inf)
    ps, vis, _ = _check(F, xy1, xy2, radius, "non-finite records")
    assert not ps[:, 5:8].any() and not vis[:, 5:8].any()
    small = (xy1 * f32(0.05)).astype(f32)                         # x + y + 1 < 160: (1e-25 * 160)^2 underflows to 0
    assert (lines_np(np.full(9, 1e-25, f32), small[:, 0], small[:, 1])[3] == 0).all()
    for name, G, rows in (("nan", np.full(9, np.nan, f32), xy1), ("zero", np.zeros(9, f32), xy1),
                          ("1e20", np.full(9, 1e20, f32), xy1), ("1e-25", np.full(9, 1e-25, f32), small),
                          ("one nan", np.where(np.arange(9) == 4, np.nan, F.reshape(9)), xy1)):
        ps, vis, _ = _check(G, rows, xy2, radius, name)
        assert not ps.any(), name                                 # n2 overflows / underflows to 0 / is a NaN
        assert not vis.any(), name                                # and such a row walks nothing
    _check(np.full(9, 1e-25, f32), xy1, xy2, radius, "1e-25, subnormal n2")


def test_gate_infinite_right_hand_side_from_finite_radius():
    """radius^2 * n2 overflows with both finite: every record with a finite e*e is a candidate, and all are visited."""
    F, xy1, xy2 = _scene(3)
    G = (F * f32(1e12)).astype(f32)
    ps, vis, _ = _check(G, xy1, xy2, 1e18, "overflowing product")
    assert ps.any() and vis[ps].all()
    e_fin = gate_np(G, xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1], float("inf"))
    assert np.array_equal(ps, e_fin)


# ---- the gather is conservative

def _line_F(a0, a1, a2):
    """F under which the row (0, 0) has exactly the line a0 x2 + a1 y2 + a2 = 0 (float32 coefficients)."""
    F = np.zeros((3, 3), f32)
    F[0, 2], F[1, 2], F[2, 2] = a0, a1, a2
    return F


def _near_line(a, size, off, radius, rng, npts):
    """Records at float64 distance radius (1 +- k 2^-20), k = 0..8, and at 0 from the line a (float32 coefficients) at
    positions along it inside the square [off, off + size]^2, the square's corners (so that it is the bounding box), and
    random records."""
    a0, a1, a2 = (float(v) for v in a)
    n = np.hypot(a0, a1)
    nx, ny = a0 / n, a1 / n
    c = off + size / 2
    d0 = (a0 * c + a1 * c + a2) / n
    px, py = c - d0 * nx, c - d0 * ny                              # the point of the line nearest the centre
    s = rng.uniform(-0.7, 0.7, npts) * size
    k = rng.integers(0, 9, npts)
    d = radius * (1.0 + rng.choice([-1.0, 1.0], npts) * k * 2.0 ** -20) * rng.choice([-1.0, 1.0, 0.0], npts, p=[.45, .45, .1])
    x, y = px - s * ny + d * nx, py + s * nx + d * ny
    keep = (x >= off) & (x <= off + size) & (y >= off) & (y <= off + size)
    corners = np.array([[off, off], [off + size, off], [off, off + size], [off + size, off + size]], np.float64)
    rnd = off + rng.uniform(0, size, (npts // 4, 2))
    return np.concatenate([np.stack([x[keep], y[keep]], 1), corners, rnd]).astype(f32)


def _angles():
    """(a0, a1) of exactly horizontal, vertical and 45-degree lines, near-degenerate and generic ones."""
    out = [(0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (0.0, -1.0), (-1.0, 0.0),
           (1e-30, 1.0), (1.0, 1e-30), (1e-6, 1.0), (1.0, -1e-6), (1e-3, -1.0)]
    for t in (0.1, 0.7, 1.3, 2.0, 2.9):
        out.append((np.sin(t), np.cos(t)))
    return out


@pytest.mark.parametrize("size,off", [(64.0, 0.0), (1000.0, 0.0), (1920.0, -700.0), (16384.0, 0.0), (300.0, 1e5),
                                      (16384.0, -1e5)])
@pytest.mark.parametrize("radius", [1e-3, 0.5])
def test_gather_is_conservative_near_the_band_edge(size, off, radius):
    rng = np.random.default_rng(int(size) + int(abs(off)) + int(radius * 10))
    passed = pairs = 0
    for a0, a1 in _angles():
        for scale in (1.0, 1e-6, 3e5):
            for where in ("inside", "corner", "outside"):
                if where == "inside":
                    qx, qy = off + rng.uniform(0.2, 0.8, 2) * size
                elif where == "corner":                            # through a corner of the bounding box
                    qx, qy = rng.choice([off, off + size], 2)
                else:                                              # beyond the box along the normal: misses it wholly
                    qx, qy = off + size / 2, off + size / 2
                a = np.array([a0, a1, 0.0]) * scale
                a[2] = -(a[0] * qx + a[1] * qy)
                if where == "outside":
                    a[2] += 1.5 * size * np.hypot(a[0], a[1])
                a = a.astype(f32)
                xy2 = _near_line(a, size, off, radius, rng, 160)
                ps, vis, _ = _check(_line_F(*a), [(0.0, 0.0)], xy2, radius, (size, off, radius, a0, a1, scale, where))
                passed += int(ps.sum())
                pairs += ps.size
                if where == "outside":
                    assert not vis.any(), ("a line that misses the box visits nothing", a)
    assert passed > 500 and pairs > 10000, (passed, pairs)


@pytest.mark.parametrize("radius", [1e-3, 0.5, 2.0])
def test_gather_is_conservative_on_planted_scenes_and_degenerate_grids(radius):
    for seed in range(3):
        F, xy1, xy2 = _scene(seed, 200, 800)
        _check(F, xy1, xy2, radius, "scene")
        # all records collinear: a 1 x N and an N x 1 grid
        flat = xy2.copy()
        flat[:, 1] = f32(333.25)
        _, _, g = _check(F, xy1, flat, radius, "collinear, horizontal")
        assert g[1] == 1
        _check(STEREO, [(5.0, 333.25), (5.0, 333.25 + 0.9 * radius), (5.0, 400.0)], flat, radius, "collinear on the line")
        flat = xy2.copy()
        flat[:, 0] = f32(1000.5)
        _, _, g = _check(F, xy1, flat, radius, "collinear, vertical")
        assert g[0] == 1
        _check(F, xy1, xy2[:1], radius, "a single record")
        _check(F, xy1, xy2[:0], radius, "no record")
    # the grid saturates at 64 x 64
    rng = np.random.default_rng(5)
    F = planted_F(5)
    xy1 = np.stack([rng.uniform(0, 1920, 64), rng.uniform(0, 1080, 64)], 1).astype(f32)
    x, y, _ = points_on_lines(F, xy1[:, 0], xy1[:, 1], rng, rng.uniform(-1.2, 1.2, 64) * radius)
    xy2 = np.stack([rng.uniform(0, 1920, 4100), rng.uniform(0, 1080, 4100)], 1)
    xy2[:64, 0], xy2[:64, 1] = x, y
    ps, _, g = _check(F, xy1, xy2, radius, "n2 = 4100")
    assert g == (64, 64) and ps.any()
    for G in (STEREO, STEREO_V):
        _check(G, xy1, xy2, radius, "stereo")
        _check(G, xy2[:200], xy2, radius, "stereo, rows on the records")


def test_infinite_radius_visits_everything():
    F, xy1, xy2 = _scene(2)
    ps, vis, g = _check(F, xy1, xy2, float("inf"), "inf")
    assert g == (1, 1) and ps.all() and vis.all()


# ---- the gather is selective

def test_gather_is_selective():
    rng = np.random.default_rng(77)
    xy2 = np.stack([rng.uniform(0, 1920, 2000), rng.uniform(0, 1080, 2000)], 1).astype(f32)
    frac = []
    for _ in range(500):                                           # generic lines through two points of the image
        (xa, xb), (ya, yb) = rng.uniform(0, 1920, 2), rng.uniform(0, 1080, 2)
        a0, a1 = ya - yb, xb - xa
        ps, vis, g = _check(_line_F(a0, a1, -(a0 * xa + a1 * ya)), [(0.0, 0.0)], xy2, 2.0, "generic line")
        assert g == (64, 64)
        frac.append(vis.mean())
    assert np.mean(frac) <= 0.15, np.mean(frac)
    xy1 = np.stack([rng.uniform(0, 1920, 500), rng.uniform(0, 1080, 500)], 1).astype(f32)
    ps, vis, _ = _check(STEREO, xy1, xy2, 2.0, "stereo")
    assert vis.mean() <= 3 / 64 + 0.02, vis.mean()
    assert vis.any(1).all()
    ps, vis, _ = _check(STEREO_V, xy1, xy2, 2.0, "vertical stereo")
    assert vis.mean() <= 3 / 64 + 0.02, vis.mean()


def test_hooks_reject_bad_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    F = np.zeros(9, f32)
    xy = np.zeros(2, f32)
    out = np.zeros(1, np.uint8)
    g = np.zeros(2, np.int32)
    assert L.misift_test_epipolar_gate(None, xy.ctypes.data, 1, xy.ctypes.data, 1, 1.0, out.ctypes.data) == -1
    assert L.misift_test_epipolar_gate(F.ctypes.data, xy.ctypes.data, -1, xy.ctypes.data, 1, 1.0, out.ctypes.data) == -1
    assert L.misift_test_epipolar_gather(F.ctypes.data, xy.ctypes.data, 1, xy.ctypes.data, 1, 0.0, out.ctypes.data,
                                         g.ctypes.data) == -1
    assert L.misift_test_epipolar_gather(F.ctypes.data, xy.ctypes.data, 1, xy.ctypes.data, 1, 1.0, out.ctypes.data,
                                         None) == -1
