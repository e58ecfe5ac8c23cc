"""Hostile keypoint geometry for misift_match_guided_batch and misift_match_epipolar_batch (test_guided_cases_cpu.py pins
the host hooks and the premises on every scene, test_gpu_guided_hostile.py runs the device against the restatements of
test_gpu_guided_match.py and test_gpu_epipolar_match.py).  No GPU in here, and cudasift_amd.capi is imported inside
functions only.

A scene is (name, kind, pairs, matrices, radius, set-1 frames, set-2 frames, counts of both); kind is "guided" (the
matrices are homographies) or "epipolar" (fundamental matrices).  Every scene exists for both kinds: the set-2 geometry
is shared, the set-1 rows are placed so that their projection (or their epipolar line) hits what the scene plants.
Set-1 frames hold 129, 65, 64, 63 and 1 rows (the 64-row items of the match kernels), one set-2 frame holds 2100 records
(three 1024-thread strides of the bin kernel), the others at most 300.  Descriptors are L2-normalised, so a copy of a
row's descriptor is the row's best score wherever it is a candidate; every tenth planted partner has a duplicate (same
position, same descriptor), so ties for the best score occur.  All other fields are poisoned as batch_util.frames
poisons them.

Scenes:
  offset        boxes at -700, +1e5, -1e5 and 3e6 (fp32 spacing 0.25: many records share a coordinate) and a box 16384
                wide; partners inside the gate
  nonfinite     NaN, +inf and -inf in xpos or ypos of 5 % of the records, record 0 and the last among them; a frame
                with no finite record and one with exactly one; set-1 rows with a non-finite position
  degenerate    all records at one point (129 and 300 of them), on one horizontal line, on one vertical line
  outlier       a record at 3e38 and one at -1e30 among ordinary ones: astronomically wide cells
  outlier_inf   the same with radius = +inf
  greedy        1500 records within 0.75 r of the projection (line) of one row of a 65-row frame, 200 of them with the
                row's descriptor; the other rows have 0 to 3 candidates
  leaving       guided: projections just outside the box next to records on its edge, H translating by +-1e4 and 1e30,
                a denominator that is negative for half the rows and 0 on the line x = 256; epipolar: one line per pair
                (every row of the pair has it) with slopes 1e-6 and 1e-30 on a box at 1e5, through a corner, missing the
                box
  radius_small  1e-3 on a box at 1e5 (spacing 2^-7: only exact coincidences pass)
  radius_huge   1e19 (r*r finite); epipolar: 1e18 with F scaled by 1e12, so r*r * n2 overflows with both factors finite
  witness_unit  records on which the contract's gate and a gate with one product fused disagree (a product of the gate's
                own sum, or of the sums over the matrix), unit box, r = 0.25
  witness_500   the same in [0, 500)^2, r = 10
"""
import collections
import functools

import numpy as np

from epipolar_util import STEREO, STEREO_V, f32, gate_np, planted_F

Scene = collections.namedtuple("Scene", "name kind pairs mats radius fr1 fr2 counts1 counts2")

KINDS = ("guided", "epipolar")
NAMES = ("offset", "nonfinite", "degenerate", "outlier", "outlier_inf", "greedy", "leaving", "radius_small",
         "radius_huge", "witness_unit", "witness_500")
ROWS = (129, 65, 64, 63, 1)
RECS = (2100, 300, 129, 200, 77)
GREEDY_ROW, GREEDY_N, GREEDY_BEST = 32, 1500, 200
WITNESS = {"witness_unit": (1.0, 0.25), "witness_500": (500.0, 10.0)}        # extent, radius
WITNESS_DRAWS = 200000
NONFINITE = (np.nan, np.inf, -np.inf)


# ---- the gates, restated in numpy float32

def _sum3(c0, c1, c2, x, y, fused):
    """c0*x + c1*y + c2 in float32, left to right.  fused "x" / "y": what a contracting compiler could make of it, the
    product c0*x (c1*y) fused into the first sum: that product exact in float64, the sum rounded to float32 once."""
    if fused is None:
        return c0 * x + c1 * y + c2
    u, v = ((c0, x), (c1, y)) if fused == "x" else ((c1, y), (c0, x))
    return (np.float64(u[0]) * u[1].astype(np.float64) + (v[0] * v[1]).astype(np.float64)).astype(f32) + c2


def _gate_core(kind, M, x1, y1, x2, y2, radius, fused, fused_m):
    """The gate of either call on arrays that broadcast against each other.  With fused and fused_m None it is the
    contract's (guided: the gate of test_gpu_guided_match._expected operation by operation; epipolar:
    epipolar_util.gate_np).  fused: one product of the gate's own sum fused (guided: ddx*ddx or ddy*ddy; epipolar: x2*a0
    or y2*a1 of e).  fused_m: one product fused in each sum over the matrix (the projection's three sums, or the line's
    a0, a1, a2)."""
    h = np.asarray(M, f32).reshape(9)
    r2 = f32(radius) * f32(radius)
    with np.errstate(all="ignore"):
        if kind == "guided":
            den = _sum3(h[6], h[7], h[8], x1, y1, fused_m)
            px = _sum3(h[0], h[1], h[2], x1, y1, fused_m) / den
            py = _sum3(h[3], h[4], h[5], x1, y1, fused_m) / den
            dx, dy = px - x2, py - y2
            if fused is None:
                return dx * dx + dy * dy < r2
            u, v = (dx, dy) if fused == "x" else (dy, dx)
            u = u.astype(np.float64)
            return (u * u + (v * v).astype(np.float64)).astype(f32) < r2
        from epipolar_util import finite
        a0 = _sum3(h[0], h[1], h[2], x1, y1, fused_m)
        a1 = _sum3(h[3], h[4], h[5], x1, y1, fused_m)
        a2 = _sum3(h[6], h[7], h[8], x1, y1, fused_m)
        n2 = a0 * a0 + a1 * a1
        ok = finite(a0) & finite(a1) & finite(a2) & finite(n2)
        if fused is None:
            e = x2 * a0 + y2 * a1 + a2
        else:
            u, ua, v, va = (x2, a0, y2, a1) if fused == "x" else (y2, a1, x2, a0)
            e = (u.astype(np.float64) * ua.astype(np.float64) + (v * va).astype(np.float64)).astype(f32) + a2
        return ok & (e * e < r2 * n2)


def gate(kind, M, xy1, xy2, radius, fused=None, fused_m=None):
    """(n1, n2) bool: record j is a candidate of row i."""
    xy1, xy2 = np.asarray(xy1, f32).reshape(-1, 2), np.asarray(xy2, f32).reshape(-1, 2)
    if kind == "epipolar" and fused is None and fused_m is None:
        return gate_np(M, xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1], radius)
    return _gate_core(kind, M, xy1[:, 0, None], xy1[:, 1, None], xy2[None, :, 0], xy2[None, :, 1], radius, fused, fused_m)


def gate_diag(kind, M, xy1, xy2, radius, fused=None, fused_m=None):
    """(n,) bool: record i is a candidate of row i."""
    xy1, xy2 = np.asarray(xy1, f32).reshape(-1, 2), np.asarray(xy2, f32).reshape(-1, 2)
    return _gate_core(kind, M, xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1], radius, fused, fused_m)


def xy(p):
    return np.stack([p["xpos"], p["ypos"]], 1)


# ---- building blocks

def _homography(i, persp=True):
    from test_gpu_guided_match import _homography as h
    return h(i, persp)


def _translation(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], f32)


def _shift_F(F, ox, oy):
    """F of the same two views with both images' coordinates moved by (ox, oy)."""
    T = np.array([[1, 0, -ox], [0, 1, -oy], [0, 0, 1]], np.float64)
    G = T.T @ np.asarray(F, np.float64).reshape(3, 3) @ T
    return (G / np.abs(G).max()).astype(f32)


def _records(n, seed):
    """n records with L2-normalised random descriptors and every other field poisoned (batch_util.frames)."""
    from cudasift_amd import capi
    from synth import descriptors_to_points, synth_descriptors
    rng = np.random.default_rng(seed)
    p = descriptors_to_points(synth_descriptors(n, 7000 + seed, True), capi.POINT_DTYPE)
    for k in ("xpos", "ypos", "scale", "orientation", "score", "ambiguity", "match_xpos", "match_ypos", "match_error"):
        p[k] = rng.random(n, dtype=np.float32) * 500
    p["match"] = rng.integers(-5, 5000, n)
    return p


def _aim(kind, M, t, rng, span):
    """float32 set-1 positions whose projection (guided) or epipolar line (epipolar) under M hits the points t of image
    2, in float64 geometry; the free coordinate of an epipolar row is drawn from span."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 2)
    th = np.concatenate([t, np.ones((len(t), 1))], 1)
    with np.errstate(all="ignore"):
        if kind == "guided":
            q = th @ np.linalg.inv(M).T
            return (q[:, :2] / q[:, 2:]).astype(f32)
        c = th @ M                                                 # t^T F (x, y, 1)^T = 0
        free = rng.uniform(span[0], span[1], len(t))
        by_y = np.abs(c[:, 1]) >= np.abs(c[:, 0])
        y = -(c[:, 0] * free + c[:, 2]) / c[:, 1]
        x = -(c[:, 1] * free + c[:, 2]) / c[:, 0]
        return np.where(by_y[:, None], np.stack([free, y], 1), np.stack([x, free], 1)).astype(f32)


def _finite(p):
    return np.isfinite(p).all(1)


def _far(kind, xy2, n, rng, radius):
    """n points of image 2 with no record near them.  guided: inside and around the box, at least 2 r from every finite
    record (a disc that may leave the box).  epipolar: three extents beyond the box along its diagonal."""
    p = xy2[_finite(xy2) & (np.abs(xy2) < 1e9).all(1)].astype(np.float64)
    if len(p) == 0:
        p = np.array([[250.0, 250.0]])
    lo, hi = p.min(0), p.max(0)
    r = min(float(radius), 1e3)
    ext = np.maximum(hi - lo, 50 * r)
    if kind == "epipolar":
        return (lo + hi) / 2 + 3 * ext * rng.choice([-1.0, 1.0], (n, 1)) + rng.uniform(-0.2, 0.2, (n, 2)) * ext
    out = np.zeros((0, 2))
    while len(out) < n:
        q = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (4 * n + 16, 2))
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(2).min(1)
        out = np.concatenate([out, q[d2 > (2 * r) ** 2]])
    return out[:n]


def _plant(a, b, rows, partner, dup=True):
    """Record partner[k] of b carries the descriptor of row rows[k] of a; every tenth partner is copied (position and
    descriptor) into the record behind it where that record is finite and nobody's partner."""
    b["data"][partner] = a["data"][rows]
    if not dup:
        return
    taken = set(int(j) for j in partner)
    for j in partner[::10]:
        j = int(j)
        if j + 1 < len(b) and j + 1 not in taken and np.isfinite(b["xpos"][j + 1]) and np.isfinite(b["ypos"][j + 1]):
            for k in ("xpos", "ypos", "data"):
                b[k][j + 1] = b[k][j]
            taken.add(j + 1)


def _poison_rows(a, every, start=3):
    """Every `every`-th row of a from `start` gets a non-finite position."""
    for k, r in enumerate(range(start, len(a), every)):
        a[("xpos", "ypos")[k % 2]][r] = NONFINITE[k % 3]


def _pair(kind, M, n1, xy2, seed, radius, span, *, jitter=0.3, partners=None):
    """One pair: a set-2 frame at the positions xy2 and a set-1 frame of n1 rows.  The first half of the rows (at least
    one) aim at a finite even-indexed record each, within jitter * radius per axis; the others aim at _far points."""
    rng = np.random.default_rng(seed)
    xy2 = np.asarray(xy2, f32)
    a, b = _records(n1, 2 * seed), _records(len(xy2), 2 * seed + 1)
    b["xpos"], b["ypos"] = xy2[:, 0], xy2[:, 1]
    ok = np.nonzero(_finite(xy2) & (np.abs(xy2) < 1e9).all(1))[0]
    ok = ok[ok % 2 == 0] if (ok % 2 == 0).any() else ok
    k = (n1 + 1) // 2 if len(ok) else 0
    t = _far(kind, xy2, n1, rng, radius)
    partner = np.zeros(0, np.int64)
    if k:
        partner = rng.permutation(ok)[:k] if len(ok) >= k else rng.choice(ok, k)
        if partners is not None:
            partner = np.asarray(partners)[:k]
        t[:k] = xy2[partner].astype(np.float64) + rng.uniform(-jitter, jitter, (k, 2)) * min(radius, 1e3)
    p1 = _aim(kind, M, t, rng, span)
    a["xpos"], a["ypos"] = p1[:, 0], p1[:, 1]
    if k:
        _plant(a, b, np.arange(k), partner, dup=len(np.unique(partner)) == k)
    return a, b


def _scene(name, kind, radius, items):
    """items: (M, set-1 frame, set-2 frame) per pair; the set-2 frames are stored in reverse order, pair i = (i, n-1-i)."""
    n = len(items)
    fr1 = [it[1] for it in items]
    fr2 = [it[2] for it in items][::-1]
    return Scene(name, kind, [(i, n - 1 - i) for i in range(n)], [np.asarray(it[0], f32).reshape(3, 3) for it in items],
                 float(radius), fr1, fr2, [len(p) for p in fr1], [len(p) for p in fr2])


def _box(rng, n, ox, oy, w, h=None):
    h = w if h is None else h
    p = np.stack([ox + rng.uniform(0, w, n), oy + rng.uniform(0, h, n)], 1)
    return p.astype(f32)


def _mat(kind, i, ext=500.0):
    return _homography(i) if kind == "guided" else planted_F(i, ext, ext)


# ---- the scenes

def _offset(kind):
    rng = np.random.default_rng(101)
    g = kind == "guided"
    spec = [(-700.0, 500.0, _homography(1) if g else _shift_F(planted_F(1, 500.0, 500.0), -700.0, -700.0), None),
            (1e5, 300.0, _translation(1e5, 1e5) if g else STEREO, (0.0, 300.0) if g else None),
            (-1e5, 300.0, _homography(2) if g else STEREO_V, None),
            (3e6, 64.0, _translation(3e6, 3e6) if g else STEREO, (0.0, 64.0) if g else None),
            (0.0, 16384.0, _homography(0) if g else planted_F(0, 16384.0, 16384.0), None)]
    items = []
    for i, (off, w, M, span) in enumerate(spec):
        items.append((M,) + _pair(kind, M, ROWS[i], _box(rng, RECS[i], off, off, w), 110 + i, 2.0,
                                  span or (off, off + w)))
    return _scene("offset", kind, 2.0, items)


def _sprinkle(p, rng, frac=0.05):
    """NaN, +inf, -inf into x or y of frac of the records, record 0 and the last among them."""
    n = len(p)
    idx = np.unique(np.concatenate([[0, n - 1], rng.choice(n, max(int(frac * n), 1), replace=False)]))
    for k, j in enumerate(idx):
        p[j, k % 2] = NONFINITE[k % 3]
    return p


def _nonfinite(kind):
    rng = np.random.default_rng(201)
    boxes = [_sprinkle(_box(rng, 2100, 0, 0, 500), rng), _sprinkle(_box(rng, 300, 0, 0, 500), rng, 1.0),
             _box(rng, 300, 0, 0, 500), _sprinkle(_box(rng, 129, 0, 0, 500), rng), _sprinkle(_box(rng, 200, 0, 0, 500), rng)]
    one = boxes[2][150].copy()
    _sprinkle(boxes[2], rng, 1.0)
    boxes[2][150] = one                                            # exactly one finite record
    items = []
    for i, p in enumerate(boxes):
        M = _mat(kind, i)
        a, b = _pair(kind, M, ROWS[i], p, 210 + i, 8.0, (0.0, 500.0))
        _poison_rows(a, 8)
        items.append((M, a, b))
    return _scene("nonfinite", kind, 8.0, items)


def _degenerate(kind):
    rng = np.random.default_rng(301)
    line_h = _box(rng, 2100, 0, 0, 500)
    line_h[:, 1] = f32(333.25)
    line_v = _box(rng, 200, 0, 0, 500)
    line_v[:, 0] = f32(200.5)
    line_h2 = _box(rng, 77, 0, 0, 500)
    line_h2[:, 1] = f32(12.0)
    boxes = [line_h, np.tile(np.array([[123.5, 77.25]], f32), (300, 1)), np.tile(np.array([[401.0, 250.125]], f32), (129, 1)),
             line_v, line_h2]
    items = []
    for i, p in enumerate(boxes):
        M = _mat(kind, i)
        items.append((M,) + _pair(kind, M, ROWS[i], p, 310 + i, 2.0, (0.0, 500.0)))
    return _scene("degenerate", kind, 2.0, items)


def _outlier(kind, radius, name):
    rng = np.random.default_rng(401)
    items = []
    for i, n in enumerate((2100, 300, 300, 300, 300)):
        p = _box(rng, n, 0, 0, 500)
        p[17, 0] = f32(3e38)
        p[n - 90, 1] = f32(-1e30)
        M = _mat(kind, i)
        a, b = _pair(kind, M, ROWS[i], p, 410 + i, min(radius, 2.0), (0.0, 500.0))
        _poison_rows(a, 5)
        items.append((M, a, b))
    return _scene(name, kind, radius, items)


def _greedy(kind):
    """Pair 0: 65 rows against 2100 records; row GREEDY_ROW has GREEDY_N candidates, GREEDY_BEST of them with its own
    descriptor, row k otherwise k % 4 planted records, and the remaining records lie far from every row.  Pair 1: an
    ordinary pair."""
    rng = np.random.default_rng(501)
    r, n1, n2 = 1.0, 65, 2100
    M = _homography(3) if kind == "guided" else STEREO
    k = np.arange(n1)
    if kind == "guided":
        t = np.stack([30.0 + 50.0 * (k % 9), 30.0 + 55.0 * (k // 9)], 1)            # a lattice, 50 apart
        gap = np.array([25.0, 27.0])
    else:
        t = np.stack([rng.uniform(0, 500, n1), 20.0 + 7.0 * k], 1)                  # lines y2 = 20 + 7 k
        gap = np.array([0.0, 3.5])
    p = np.zeros((n2, 2))
    owner = np.full(n2, -1)
    slots = rng.permutation(n2)
    ang, rad = rng.uniform(0, 2 * np.pi, GREEDY_N), 0.75 * r * np.sqrt(rng.uniform(0, 1, GREEDY_N))
    g = slots[:GREEDY_N]
    p[g] = t[GREEDY_ROW] + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    owner[g[:GREEDY_BEST]] = GREEDY_ROW
    used = GREEDY_N
    for row in k:
        if row == GREEDY_ROW:
            continue
        for _ in range(row % 4):
            j = slots[used]
            used += 1
            p[j] = t[row] + rng.uniform(-0.3, 0.3, 2) * r
            owner[j] = row
    rest = slots[used:]
    p[rest] = t[rng.integers(0, n1, len(rest))] + gap + rng.uniform(-0.5, 0.5, (len(rest), 2))
    if kind == "epipolar":                                          # along the line anywhere
        p[:, 0] = rng.uniform(0, 500, n2)
    a, b = _records(n1, 520), _records(n2, 521)
    p = p.astype(f32)
    b["xpos"], b["ypos"] = p[:, 0], p[:, 1]
    p1 = _aim(kind, M, t, rng, (0.0, 500.0))
    a["xpos"], a["ypos"] = p1[:, 0], p1[:, 1]
    has = owner >= 0
    b["data"][has] = a["data"][owner[has]]
    M1 = _mat(kind, 1)
    return _scene("greedy", kind, r, [(M, a, b), (M1,) + _pair(kind, M1, 64, _box(rng, 129, 0, 0, 500), 530, r,
                                                               (0.0, 500.0))])


def _line_pair(a_line, n1, n2, size, off, seed, radius):
    """A pair in which every row has the line a_line (test_epipolar_cpu._line_F) and the records are
    test_epipolar_cpu._near_line's: at radius (1 +- k 2^-20) from it, on it, the box corners and random ones, n2 in all.
    The passing records carry the rows' descriptors in turn, every tenth row on two of them."""
    from test_epipolar_cpu import _line_F, _near_line
    rng = np.random.default_rng(seed)
    p = _near_line(a_line, size, off, radius, rng, n2)
    keep = np.ones(len(p), bool)
    if len(p) > n2:                                                # drop random ones from the end, never the corners
        keep[len(p) - (len(p) - n2):] = False
    p = p[keep]
    if len(p) < n2:
        p = np.concatenate([p, _box(rng, n2 - len(p), off, off, size)])
    F = _line_F(*a_line)
    a, b = _records(n1, 2 * seed), _records(n2, 2 * seed + 1)
    b["xpos"], b["ypos"] = p[:, 0], p[:, 1]
    a["xpos"], a["ypos"] = rng.uniform(0, 500, n1).astype(f32), rng.uniform(0, 500, n1).astype(f32)
    ok = np.nonzero(gate_np(F, [0.0], [0.0], p[:, 0], p[:, 1], radius)[0])[0]
    if len(ok):
        ok = rng.permutation(ok)
        rows = np.arange(min(n1, len(ok)))
        b["data"][ok[rows]] = a["data"][rows]
        spare = ok[len(rows):]
        for s, row in zip(spare, rows[::10]):
            b["data"][s] = a["data"][row]
    return F, a, b


def _line_through(a0, a1, qx, qy, shift=0.0):
    a = np.array([a0, a1, 0.0])
    a[2] = -(a[0] * qx + a[1] * qy) + shift * np.hypot(a[0], a[1])
    return a.astype(f32)


def _leaving(kind):
    rng = np.random.default_rng(601)
    r = 2.0
    if kind == "epipolar":
        s = np.sin(0.7), np.cos(0.7)
        items = [_line_pair(_line_through(1e-6, 1.0, 1e5 + 120.0, 1e5 + 171.0), ROWS[0], RECS[0], 300.0, 1e5, 610, r),
                 _line_pair(_line_through(s[0], s[1], -700.0 + 1920.0, -700.0), ROWS[1], RECS[1], 1920.0, -700.0, 611, r),
                 _line_pair(_line_through(1e-30, 1.0, 1e5 + 40.0, 1e5 + 66.5), ROWS[2], RECS[2], 300.0, 1e5, 612, r),
                 _line_pair(_line_through(s[0], s[1], 250.0, 250.0, 1.5 * 500.0), ROWS[3], RECS[3], 500.0, 0.0, 613, r),
                 _line_pair(_line_through(0.0, 1.0, 250.0, 250.0, -1.5 * 500.0), ROWS[4], RECS[4], 500.0, 0.0, 614, r)]
        return _scene("leaving", kind, r, items)
    corners = np.array([[0, 0], [500, 0], [0, 500], [500, 500]], f32)
    # pair 0: 64 records on the box's edges, each the partner of a row whose projection lies 0.5 r outside the box
    n_edge = 64
    s = rng.uniform(5, 495, n_edge)
    side = np.arange(n_edge) % 4
    edge = np.stack([np.where(side == 0, 0.0, np.where(side == 1, 500.0, s)),
                     np.where(side == 2, 0.0, np.where(side == 3, 500.0, s))], 1)
    out = np.stack([np.where(side == 0, -1.0, np.where(side == 1, 1.0, 0.0)),
                    np.where(side == 2, -1.0, np.where(side == 3, 1.0, 0.0))], 1)
    p = _box(rng, RECS[0], 0, 0, 500)
    p[0:2 * n_edge:2] = edge.astype(f32)
    p[-4:] = corners
    M = _homography(4)
    a, b = _pair(kind, M, ROWS[0], p, 620, r, None, partners=np.arange(0, 2 * n_edge + 2, 2))
    t = _far(kind, p, ROWS[0], rng, r)
    t[:n_edge] = edge + 0.5 * r * out
    t[n_edge:n_edge + 30] = (edge + 3.0 * r * out)[:30]               # 3 r outside: the disc leaves the box, no candidate
    p1 = _aim(kind, M, t, rng, None)
    a["xpos"], a["ypos"] = p1[:, 0], p1[:, 1]
    items = [(M, a, b)]
    for i, (tx, ty) in ((1, (1e4, 1e4)), (2, (1e30, 1e30))):
        M = _translation(tx, ty)
        a, b = _pair(kind, _translation(0, 0), ROWS[i], np.concatenate([_box(rng, RECS[i] - 4, 0, 0, 500), corners]),
                     620 + i, r, None)
        items.append((M, a, b))
    # pair 3: den = x / 256 - 1: negative for the rows left of x = 256, 0 on it
    M = np.array([[1, 0, 0], [0, 1, 0], [2.0 ** -8, 0, -1]], f32)
    a, b = _pair(kind, M, ROWS[3], _box(rng, RECS[3], 0, 0, 500), 623, r, None)
    a["xpos"][40:52] = f32(256.0)
    items.append((M, a, b))
    M = _translation(-1e4, -1e4)
    a, b = _pair(kind, _translation(0, 0), ROWS[4], _box(rng, RECS[4], 0, 0, 500), 624, r, None)
    items.append((M, a, b))
    return _scene("leaving", kind, r, items)


def _radius_small(kind):
    """Records on the lattice 1e5 + k / 128: exactly representable, so a row aimed at one hits it exactly (err 0) and
    every other record is at least 2^-7 away."""
    rng = np.random.default_rng(701)
    items = []
    for i in range(5):
        p = (1e5 + rng.integers(0, 300 * 128, (RECS[i], 2)) / 128.0).astype(f32)
        if kind == "guided":
            M, span = _translation(1e5, 1e5), None
        else:
            M, span = (STEREO, STEREO_V)[i % 2], (1e5, 1e5 + 300.0)
        items.append((M,) + _pair(kind, M, ROWS[i], p, 710 + i, 1e-3, span, jitter=0.0))
    return _scene("radius_small", kind, 1e-3, items)


def _radius_huge(kind):
    rng = np.random.default_rng(801)
    items = []
    for i in range(5):
        p = _box(rng, RECS[i], 0, 0, 500)
        if i == 0:
            p[17, 0] = f32(3e38)
            p[2010, 1] = f32(-1e30)
        M = _homography(i) if kind == "guided" else (planted_F(i, 500.0, 500.0) * f32(1e12)).astype(f32)
        a, b = _pair(kind, M, ROWS[i], p, 810 + i, 2.0, (0.0, 500.0))
        _poison_rows(a, 5)
        items.append((M, a, b))
    return _scene("radius_huge", kind, 1e19 if kind == "guided" else 1e18, items)


WITNESS_F = {1.0: 0.6, 500.0: 300.0}                               # c of the rows' lines a0 x2 + a1 y2 = c


@functools.lru_cache(maxsize=None)
def witnesses(kind, ext, radius, family):
    """The seeded search: WITNESS_DRAWS (row, record) pairs with the record at float64 distance radius (1 + k 2^-22),
    |k| <= 8 (family "matrix": |k| <= 1), from the row's projection (line).  Returns (M, xy1, xy2, form, found).
    family "gate": the pairs on which the contract's gate and the gate with product form "x" or "y" of its own sum fused
    disagree, 65 of "x" and 64 of "y"; found = how many the search gave of each.  guided: H is the identity, so a row
    projects onto itself exactly.  epipolar: F = diag(1, 1, -c), so the row (x, y) has the line x x2 + y y2 = c with
    exactly the row's coordinates as coefficients.  No fusing of the sums over the matrix changes either.
    family "matrix": a matrix with nine working entries (an affine H, so that den = 1; planted_F), and the pairs on which
    the contract's gate disagrees with BOTH ways of fusing one product into each sum over the matrix (form "xy"), 129 of
    them."""
    rng = np.random.default_rng(int(ext) + 9 + (family == "matrix"))
    n = WITNESS_DRAWS
    t = rng.uniform(0, 2 * np.pi, n)
    kmax = 8 if family == "gate" else 1                          # the matrix sums move the gate by less: stay closer
    d = radius * (1.0 + rng.integers(-kmax, kmax + 1, n) * 2.0 ** -22)
    if kind == "guided":
        M = np.eye(3, dtype=f32) if family == "gate" else _homography(2, persp=False)
        p1 = rng.uniform(0.3 * ext, 0.7 * ext, (n, 2)).astype(f32)
        h = M.astype(np.float64)
        proj = np.stack([_sum3(*M[0], p1[:, 0], p1[:, 1], None), _sum3(*M[1], p1[:, 0], p1[:, 1], None)], 1)
        assert (h[2] == (0, 0, 1)).all()
        p2 = (proj.astype(np.float64) + d[:, None] * np.stack([np.cos(t), np.sin(t)], 1)).astype(f32)
    else:
        if family == "gate":
            M = np.diag([1.0, 1.0, -WITNESS_F[ext]]).astype(f32)
            p1 = rng.uniform(0.3, 1.0, (n, 2)).astype(f32)
        else:
            M = planted_F(2, ext, ext)
            p1 = rng.uniform(0.1 * ext, 0.9 * ext, (n, 2)).astype(f32)
        a = np.stack([_sum3(*M[k], p1[:, 0], p1[:, 1], None) for k in range(3)], 1).astype(np.float64)
        nrm = np.hypot(a[:, 0], a[:, 1])
        q = rng.uniform(0.2 * ext, 0.8 * ext, n)                   # one coordinate of a point of the line
        by_y = np.abs(a[:, 1]) >= np.abs(a[:, 0])
        with np.errstate(all="ignore"):
            foot = np.where(by_y[:, None], np.stack([q, -(a[:, 0] * q + a[:, 2]) / a[:, 1]], 1),
                            np.stack([-(a[:, 1] * q + a[:, 2]) / a[:, 0], q], 1))
        p2 = (foot + (d * rng.choice([-1.0, 1.0], n) / nrm)[:, None] * a[:, :2]).astype(f32)
        inside = (p2 >= 0).all(1) & (p2 <= ext).all(1)
        p1, p2 = p1[inside], p2[inside]
    plain = gate_diag(kind, M, p1, p2, radius)
    if family == "gate":
        wx = np.nonzero(plain != gate_diag(kind, M, p1, p2, radius, fused="x"))[0]
        wy = np.nonzero(plain != gate_diag(kind, M, p1, p2, radius, fused="y"))[0]
        wy = np.setdiff1d(wy, wx[:65])
        sel = np.concatenate([wx[:65], wy[:64]])
        form = ["x"] * len(wx[:65]) + ["y"] * len(wy[:64])
        return M, p1[sel], p2[sel], form, (len(wx), len(wy))
    both = np.nonzero((plain != gate_diag(kind, M, p1, p2, radius, fused_m="x"))
                      & (plain != gate_diag(kind, M, p1, p2, radius, fused_m="y")))[0]
    sel = both[:129]
    return M, p1[sel], p2[sel], ["xy"] * len(sel), (len(both),)


def _witness(kind, name):
    """Pair 0: the witnesses of the gate's own sum.  Pair 1: 64 rows with no candidate in the same set-2 frame.  Pair 2:
    the witnesses of the sums over the matrix.  Record i of a witness frame is the only carrier of row i's descriptor."""
    ext, radius = WITNESS[name]
    fr1, fr2, mats = [], [], []
    for k, family in enumerate(("gate", "matrix")):
        M, p1, p2, _, _ = witnesses(kind, ext, radius, family)
        n = len(p1)
        a, b = _records(n, 900 + int(ext) + 10 * k), _records(n, 901 + int(ext) + 10 * k)
        a["xpos"], a["ypos"] = p1[:, 0], p1[:, 1]
        b["xpos"], b["ypos"] = p2[:, 0], p2[:, 1]
        b["data"] = a["data"]
        fr1.append(a)
        fr2.append(b)
        mats.append(M)
    far = _records(64, 902 + int(ext))
    rng = np.random.default_rng(903)
    if kind == "guided":
        far["xpos"], far["ypos"] = (rng.uniform(10, 11, 64) * ext).astype(f32), (rng.uniform(10, 11, 64) * ext).astype(f32)
    else:
        far["xpos"], far["ypos"] = rng.uniform(0.005, 0.01, 64).astype(f32), rng.uniform(0.005, 0.01, 64).astype(f32)
    return Scene(name, kind, [(0, 0), (1, 0), (2, 1)], [mats[0], mats[0], mats[1]], radius, [fr1[0], far, fr1[1]], fr2,
                 [len(fr1[0]), 64, len(fr1[1])], [len(p) for p in fr2])


@functools.lru_cache(maxsize=None)
def scene(kind, name):
    assert kind in KINDS
    if name in WITNESS:
        return _witness(kind, name)
    if name == "outlier":
        return _outlier(kind, 2.0, name)
    if name == "outlier_inf":
        return _outlier(kind, float("inf"), name)
    return {"offset": _offset, "nonfinite": _nonfinite, "degenerate": _degenerate, "greedy": _greedy,
            "leaving": _leaving, "radius_small": _radius_small, "radius_huge": _radius_huge}[name](kind)


# ---- the calls restated from their contracts (what test_gpu_guided_match.py and test_gpu_epipolar_match.py hold the
# device to): the gate in numpy float32, then the oracle's exact, full matcher on the candidates in index order

def expected_guided(pairs, Hs, radius, max_pts, recs1, counts1, offs1, stride1, recs2, counts2, offs2, stride2):
    """Set 1 and num_found after misift_match_guided_batch, restated from the contract with the oracle's matcher."""
    from batch_util import orc, span
    o = orc()
    exp = recs1.copy()
    nf = np.zeros(len(pairs), np.int32)
    r2 = np.float32(radius) * np.float32(radius)
    for i, (f1, f2) in enumerate(pairs):
        n1, n2 = max(int(counts1[f1]), 0), max(int(counts2[f2]), 0)
        if n1 > max_pts or n2 > max_pts:
            nf[i] = -1
            continue
        if n1 == 0 or n2 == 0:
            continue
        s1 = span(offs1, stride1, f1, n1)
        p1 = exp[s1].copy()
        p2 = recs2[span(offs2, stride2, f2, n2)]
        h = np.asarray(Hs[i], np.float32).reshape(9)
        x, y = p1["xpos"], p1["ypos"]
        with np.errstate(all="ignore"):
            den = h[6] * x + h[7] * y + h[8]
            px = (h[0] * x + h[1] * y + h[2]) / den
            py = (h[3] * x + h[4] * y + h[5]) / den
            for r in range(n1):
                dx = px[r] - p2["xpos"]
                dy = py[r] - p2["ypos"]
                cand = np.nonzero(dx * dx + dy * dy < r2)[0]
                row = p1[r:r + 1]
                if len(cand) == 0:
                    row["score"], row["ambiguity"], row["match"] = 0.0, 0.0, -1
                    row["match_xpos"], row["match_ypos"] = 0.0, 0.0
                    continue
                o.match(row, 1, p2[cand].copy(), len(cand), full=True, exact=True)
                if row["match"][0] >= 0:
                    row["match"] = cand[row["match"][0]]
                    nf[i] += 1
        exp[s1] = p1
    return exp, nf


def expected_epipolar(pairs, Fs, radius, max_pts, recs1, counts1, offs1, stride1, recs2, counts2, offs2, stride2):
    """Set 1 and num_found after misift_match_epipolar_batch, restated from the contract with the oracle's matcher."""
    from batch_util import orc, span
    o = orc()
    exp = recs1.copy()
    nf = np.zeros(len(pairs), np.int32)
    for i, (f1, f2) in enumerate(pairs):
        n1, n2 = max(int(counts1[f1]), 0), max(int(counts2[f2]), 0)
        if n1 > max_pts or n2 > max_pts:
            nf[i] = -1
            continue
        if n1 == 0 or n2 == 0:
            continue
        s1 = span(offs1, stride1, f1, n1)
        p1 = exp[s1].copy()
        p2 = recs2[span(offs2, stride2, f2, n2)]
        gate = gate_np(Fs[i], p1["xpos"], p1["ypos"], p2["xpos"], p2["ypos"], radius)
        for r in range(n1):
            cand = np.nonzero(gate[r])[0]
            row = p1[r:r + 1]
            if len(cand) == 0:
                row["score"], row["ambiguity"], row["match"] = 0.0, 0.0, -1
                row["match_xpos"], row["match_ypos"] = 0.0, 0.0
                continue
            o.match(row, 1, p2[cand], len(cand), full=True, exact=True)      # p2[cand] is a fresh array
            if row["match"][0] >= 0:
                row["match"] = cand[row["match"][0]]
                nf[i] += 1
        exp[s1] = p1
    return exp, nf


# ---- the expected answers, computed once per scene

@functools.lru_cache(maxsize=None)
def expected(kind, name):
    """(scene, packed set 1, its offsets, packed set 2, its offsets, expected set-1 frames, expected num_found) from
    expected_guided or expected_epipolar; the arrays are shared: leave them unchanged."""
    from batch_util import layout, span
    _expected = expected_guided if kind == "guided" else expected_epipolar
    s = scene(kind, name)
    r1, o1, _ = layout(s.fr1, s.counts1, False, min_stride=0, pad_error=0.0)
    r2, o2, _ = layout(s.fr2, s.counts2, False, min_stride=0, pad_error=0.0)
    exp, enf = _expected(s.pairs, s.mats, s.radius, 8192, r1, s.counts1, o1, 0, r2, s.counts2, o2, 0)
    ef = [exp[span(o1, 0, f, n)] for f, n in enumerate(s.counts1)]
    for a in (r1, r2, exp, enf):
        a.flags.writeable = False
    return s, r1, o1, r2, o2, ef, enf
