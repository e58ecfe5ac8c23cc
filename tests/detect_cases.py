"""Planted pyramid levels for the production detector (dog_scan_all_kernel, refine_all_kernel in kernels_dog.hip) and what
the oracle makes of them.

Context.detect_levels (misift_test_detect_levels) lays levels of OUR choosing into the arena and runs the scan and the
refinement of an extraction call on them.  This module builds the levels — Gaussian blobs of either sign on a flat or
gently sloped background, aimed at the places where those kernels can go wrong — and states two expectations per frame
and level, both from the oracle's DoG planes orc.laplace(level, noct, o):

  detections   orc.findpoints(planes, thresh, subsampling, lowest_scale / subsampling, edge_limit=10) — the definition;
  candidates   model_candidates(): the scan's necessary in-row test restated in numpy float32 on planes 1..5, rows
               1..h-2, columns 1..w-2: a value passes if it is strictly above max(thresh, its in-row neighbours) or strictly
               below min(-thresh, ...), the neighbours being columns x-1..x+1 of planes s-1, s, s+1 where those are among the
               five.  This is scan_row with its wave-uniform shortcuts removed; minima and maxima ignore NaN as fminf / fmaxf do.

refine_np() restates refine_math on the planes (26-neighbour test, edge test, sub-pixel solve with its fallback, scale
floor) so that the CPU tests can COUNT which branch a planted blob takes; it is never an expectation for the device.

A case is a dict: name, geom (w, h, noct), frames (each a list of levels, coarsest first), thresh, lowest_scale, and
`aim`, the path it is for.  test_detect_cases_cpu.py proves every aim on the oracle and the model."""
import functools

import numpy as np

from oracle import pyoracle as orc

F = np.float32
CQ_CAP = 64                       # candidates a wavefront queues in LDS (kernels_dog.hip)
STRIP = 240                       # columns per strip: 60 tester lanes x 4
GEOM_R = (483, 150, 3)            # ragged width (483 % 4 == 3): 483x150, 241x75, 120x37; three strips on the finest level
GEOM_Q = (484, 150, 3)            # width % 4 == 0 on the finest level: 484x150, 242x75, 121x37
GEOM_T = (67, 65, 4)              # coarsest level 8x8: just above the limit of misift_tiny_call
SMALL_FRAMES = 4                  # the context's default: batches above it size their segments by another rule
BG = 100.0


def level_sizes(w, h, noct):
    out = []
    for _ in range(noct):
        out.append((w, h))
        w, h = w // 2, h // 2
    return out[::-1]


def cand_cap(w, h):
    return max(w * h // 4, 16384)


# ------------------------------------------------------------------ content
def flat(w, h, value=BG):
    return np.full((h, w), value, F)


def plant(w, h, blobs, slope=(0.0, 0.0), reach=5.0):
    """A level of w x h: background BG + slope . (x, y), plus blobs (cx, cy, sx, sy, amp): amp * exp(-(dx^2 / 2 sx^2 +
    dy^2 / 2 sy^2)), each cut off outside |dx| <= reach * sx, |dy| <= reach * sy — a window symmetric about the centre,
    so a blob centred on a half-integer leaves bit-equal values in the pixels that mirror each other.  float64, rounded once."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = BG + slope[0] * x + slope[1] * y
    for cx, cy, sx, sy, amp in blobs:
        x0, x1 = max(0, int(np.ceil(cx - reach * sx))), min(w - 1, int(np.floor(cx + reach * sx)))
        y0, y1 = max(0, int(np.ceil(cy - reach * sy))), min(h - 1, int(np.floor(cy + reach * sy)))
        if x1 < x0 or y1 < y0:
            continue
        dx, dy = x[y0:y1 + 1, x0:x1 + 1] - cx, y[y0:y1 + 1, x0:x1 + 1] - cy
        a[y0:y1 + 1, x0:x1 + 1] += amp * np.exp(-(dx * dx / (2 * sx * sx) + dy * dy / (2 * sy * sy)))
    return a.astype(F)


def lattice(w, h, phase=0, pitch=13, sigma=2.0, amp=60.0, frac=0.0, borders=True):
    """A sheared lattice: blob (i, j) at x = 2 + (pitch - 2) * i + j, y = 2 + pitch * j + (i + phase) % pitch, signs
    alternating.  As i runs over `pitch` lattice columns the blobs of one lattice row visit every image row of its band;
    every band is one column further right than the one above, so the blobs of pitch - 2 bands visit every image column
    (h >= pitch * (pitch - 2) + 4).  No two blobs come closer than pitch - 3.  The outermost two rows and columns on every
    side get blobs of their own (`borders`): there the expectation is whatever the oracle says."""
    px = pitch - 2
    blobs = []
    for j in range(0, h // pitch + 1):
        for i in range(-2, w // px + 1):
            cx = 2 + px * i + j
            cy = 2 + pitch * j + (i + phase) % pitch
            if 2 <= cx <= w - 3 and 2 <= cy <= h - 3:
                sgn = 1.0 if (i + j) % 2 == 0 else -1.0
                blobs.append((cx + frac * (((3 * i + j) % 5) - 2) / 4.0, cy + frac * (((i + 3 * j) % 5) - 2) / 4.0,
                              sigma, sigma, sgn * amp))
    if borders:                                          # where the lattice leaves room: at least 9 px to its nearest blob
        pos = [(b[0], b[1]) for b in blobs]
        spots = [(x, (1, h - 2, 0, h - 1)[(n // 10) % 4]) for n, x in enumerate(range(8, w - 8))] + \
                [((1, w - 2, 0, w - 1)[(n // 10) % 4], y) for n, y in enumerate(range(8, h - 8))]
        extra = []
        for cx, cy in spots:
            other = np.array(pos + extra, np.float64).reshape(-1, 2)
            if len(other) == 0 or np.hypot(other[:, 0] - cx, other[:, 1] - cy).min() >= 9.0:
                extra.append((cx, cy))
        blobs += [(cx, cy, sigma, sigma, amp if k % 3 else -amp) for k, (cx, cy) in enumerate(extra)]
    return plant(w, h, blobs)


def lattice_frame(geom, phase=0, **kw):
    """One lattice per level; levels under 60 rows get a denser one (pitch 9: their few lattice columns still visit every row)."""
    return [lattice(w, h, phase + k, **(kw if h >= 60 else dict(kw, pitch=9, sigma=1.6)))
            for k, (w, h) in enumerate(level_sizes(*geom))]


def flat_frame(geom):
    return [flat(w, h) for w, h in level_sizes(*geom)]


TIE_SPOTS = [(60.5, 40.0), (121.0, 40.5), (180.5, 40.5), (239.5, 80.0), (300.0, 110.5), (360.5, 75.5), (420.0, 30.5),
             (30.5, 120.5)]                             # half-integer x, y, both; one astride the strip seam 239 | 240


def tie_spots(w, h):
    """The spots that fit a level of w x h (they are laid out for the finest one)."""
    return [(cx, cy) for cx, cy in TIE_SPOTS if cx < w - 12 and cy < h - 12]


def tie_pixels(cx, cy):
    """The two or four pixels (x, y) that mirror each other about a spot."""
    xs = [int(cx)] if cx == int(cx) else [int(np.floor(cx)), int(np.floor(cx)) + 1]
    ys = [int(cy)] if cy == int(cy) else [int(np.floor(cy)), int(np.floor(cy)) + 1]
    return [(x, y) for y in ys for x in xs]


def tie_level(w, h, raise_ulps=None, sigma=2.2):
    """Isolated blobs on a flat background, centred between two (or four) pixels; raise_ulps[k] ulps of its own value are
    added to (blob of positive sign) or taken from the first of spot k's tying pixels."""
    spots = tie_spots(w, h)
    a = plant(w, h, [(cx, cy, sigma, sigma, (60.0 if k % 2 == 0 else -60.0)) for k, (cx, cy) in enumerate(spots)])
    for k, (cx, cy) in enumerate(spots):
        x, y = tie_pixels(cx, cy)[0]
        for _ in range(raise_ulps[k] if raise_ulps is not None else 0):
            a[y, x] = np.nextafter(a[y, x], F(np.inf) if k % 2 == 0 else F(-np.inf))
    return a


def spot_detections(pts, cx, cy):
    return int(((np.abs(pts["xpos"] - cx) < 3) & (np.abs(pts["ypos"] - cy) < 3)).sum())


def broken_tie_level(w, h, noct, o, thresh, sigma):
    """tie_level with every tie broken by the SMALLEST raise (1, 2, 4 ... ulps of the pixel) at which the oracle sees exactly
    one keypoint at the spot.  (One ulp of a pixel near 160 is 1.5e-5; a DoG tap spreads a fraction of it into blurs that
    are themselves rounded to that grid, so a single ulp usually vanishes in the planes: docs/LOG.md.)
    Returns (level, ulps per spot)."""
    spots = tie_spots(w, h)
    ulps = [0] * len(spots)
    for step in range(0, 16):
        trial = [u if u else 2 ** step for u in ulps]
        pts, n = oracle_detections(tie_level(w, h, trial, sigma), noct, o, thresh, 0.0)
        for k, (cx, cy) in enumerate(spots):
            if not ulps[k] and spot_detections(pts[:n], cx, cy) == 1:
                ulps[k] = 2 ** step
        if all(ulps):
            break
    assert all(ulps), ulps
    return tie_level(w, h, ulps, sigma), ulps


def edge_level(w, h):
    """Elongated blobs, sy fixed and sx / sy swept from 1 to 3.2 (both signs, three rows): tra^2 / det crosses 10 inside."""
    blobs = []
    for r, cy in enumerate((30, 75, 120)):
        for k in range(15):
            ratio = 1.0 + 0.15 * k + 0.05 * r
            blobs.append((18 + 31 * k, cy, 1.8 * ratio, 1.8, 60.0 if (k + r) % 2 else -60.0))
    return plant(w, h, blobs)


def subpixel_level(w, h, seed):
    """Blobs at sub-pixel offsets up to +-0.5 px and overlapping pairs (centres 3-5 px apart, which pulls the quadratic
    fit's offset past half a pixel)."""
    rng = np.random.default_rng(seed)
    blobs = []
    k = 0
    for cy in range(14, h - 14, 22):
        for cx in range(14, w - 30, 26):
            ox, oy = rng.uniform(-0.5, 0.5, 2)
            sgn = 1.0 if k % 2 else -1.0
            s = 1.6 + 0.9 * rng.random()
            blobs.append((cx + ox, cy + oy, s, s, sgn * 60.0))
            if k % 3 == 0:                                # an overlapping partner of the same sign
                d = 3.0 + 2.0 * rng.random()
                t = rng.uniform(0, 2 * np.pi)
                blobs.append((cx + ox + d * np.cos(t), cy + oy + d * np.sin(t), s, s, sgn * (30.0 + 30.0 * rng.random())))
            k += 1
    return plant(w, h, blobs, slope=(0.01, -0.02))


def noise_band_level(w, h, seed, rows, cols_per_strip=None, amp=20.0):
    """Flat but for white noise in `rows` (a range); cols_per_strip limits it to the first so many columns of every strip."""
    rng = np.random.default_rng(seed)
    a = flat(w, h).astype(np.float64)
    n = rng.uniform(-amp, amp, (len(rows), w))
    if cols_per_strip is not None:
        n[:, (np.arange(w) % STRIP) >= cols_per_strip] = 0.0
    a[rows.start:rows.stop] += n
    return a.astype(F)


def queue_level(w, h, seed):
    """Two bands: full-width noise (more than CQ_CAP pre-candidates per strip and row: direct append) and noise in the
    first columns of each strip only (rows that hold fewer but pass CQ_CAP together: the flush)."""
    a = noise_band_level(w, h, seed, range(30, 42))
    b = noise_band_level(w, h, seed + 1, range(90, 110), cols_per_strip=36)
    return (a.astype(np.float64) + b - BG).astype(F)


NONFINITE_AT = dict(nan=(200, 70), inf=(330, 32))       # (x, y): centre of the 3 x 3 NaN patch, the inf pixel


def nonfinite_level(w, h):
    blobs = []
    k = 0
    for cy in range(12, h - 10, 21):
        for cx in range(12, w - 10, 24):
            if all(abs(cx - px) >= 22 or abs(cy - py) >= 22 for px, py in NONFINITE_AT.values()):
                blobs.append((cx, cy, 2.0, 2.0, 60.0 if k % 2 else -60.0))
            k += 1
    a = plant(w, h, blobs)
    x, y = NONFINITE_AT["nan"]
    a[y - 1:y + 2, x - 1:x + 2] = np.nan
    x, y = NONFINITE_AT["inf"]
    a[y, x] = np.inf
    return a, blobs


# ------------------------------------------------------------------ the oracle's planes, detections, the model
_planes_cache = {}


def planes_of(level, noct, o):
    """orc.laplace(level, noct, o): [7, h, w] float32; cached by content (a reference is computed once and left unchanged)."""
    key = (level.shape, noct, o, hash(level.tobytes()))
    if key not in _planes_cache:
        p = orc.laplace(level, noct, o)
        p.setflags(write=False)
        _planes_cache[key] = p
    return _planes_cache[key]


def oracle_detections(level, noct, o, thresh, lowest_scale, max_pts=32768):
    """(records, n) of orc.findpoints on the level's own planes, lowest_scale and subsampling passed as orc.extract passes
    them per octave."""
    sub = float(2 ** (noct - o))
    pts, n = orc.findpoints(planes_of(level, noct, o), thresh, sub, F(lowest_scale) / F(sub), max_pts, edge_limit=10.0)
    return pts, n


def _shift_x(p, d):
    """p[..., x + d] with NaN outside (ignored by fmin / fmax)."""
    out = np.full_like(p, np.nan)
    if d < 0:
        out[..., -d:] = p[..., :d]
    elif d > 0:
        out[..., :-d] = p[..., d:]
    else:
        out[...] = p
    return out


def model_mask(planes, thresh):
    """[5, h, w] bool: the scan's necessary in-row test on planes 1..5."""
    P = np.asarray(planes[1:6], F)
    _, h, w = P.shape
    t = F(thresh)
    with np.errstate(invalid="ignore"):
        hi = np.full(P.shape, t, F)
        lo = np.full(P.shape, -t, F)
        for s in range(5):
            for ds in (-1, 0, 1):
                if not 0 <= s + ds < 5:
                    continue
                for d in (-1, 0, 1):
                    if ds == 0 and d == 0:
                        continue
                    nb = _shift_x(P[s + ds], d)
                    hi[s] = np.fmax(hi[s], nb)
                    lo[s] = np.fmin(lo[s], nb)
        m = (P > hi) | (P < lo)
    m[:, 0, :] = m[:, h - 1, :] = False
    m[:, :, 0] = m[:, :, w - 1] = False
    return m


def codes_of(mask):
    s, y, x = np.nonzero(mask)
    return (x.astype(np.uint32) | (y.astype(np.uint32) << 14) | (s.astype(np.uint32) << 28))


def model_candidates(level, noct, o, thresh):
    """Sorted uint32 codes x | y << 14 | s << 28 (s = 0..4 for DoG planes 1..5) the scan must write for this level."""
    return np.sort(codes_of(model_mask(planes_of(level, noct, o), thresh)))


def decode(codes):
    c = np.asarray(codes, np.uint32)
    return (c & 0x3fff).astype(int), ((c >> 14) & 0x3fff).astype(int), (c >> 28).astype(int)


def strip_row_counts(mask):
    """[nstrips, h]: pre-candidates (all five planes) per strip of 240 columns and row."""
    _, h, w = mask.shape
    per = mask.sum(axis=0)
    ns = (w + STRIP - 1) // STRIP
    return np.stack([per[:, k * STRIP:(k + 1) * STRIP].sum(axis=1) for k in range(ns)])


def refine_np(planes, thresh, lowest_scale, edge_limit=10.0):
    """refine_math restated on the oracle's planes in numpy float32, for every interior pixel of planes 1..5 that passes
    the 26-neighbour test.  Returns a dict of arrays over those extrema: x, y, s, edge_ok, fallback (the |pd| > 0.5
    branch), scale_ok, kept, xpos, ypos, scale.  For counting paths, not an expectation."""
    D = np.asarray(planes, F)
    _, h, w = D.shape
    t = F(thresh)
    ext = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(5):
            v = D[s + 1, 1:h - 1, 1:w - 1]
            hi = np.full(v.shape, t, F)
            lo = np.full(v.shape, -t, F)
            for p in (s, s + 1, s + 2):
                for dy in (0, 1, 2):
                    for dx in (0, 1, 2):
                        if p == s + 1 and dy == 1 and dx == 1:
                            continue
                        nb = D[p, dy:h - 2 + dy, dx:w - 2 + dx]
                        hi = np.fmax(hi, nb)
                        lo = np.fmin(lo, nb)
            yy, xx = np.nonzero((v > hi) | (v < lo))
            ext += [(s, y + 1, x + 1) for y, x in zip(yy, xx)]
        ext = np.array(ext, int).reshape(-1, 3)
        s, y, x = ext[:, 0], ext[:, 1], ext[:, 2]
        g = lambda dp, dy, dx: D[s + 1 + dp, y + dy, x + dx]
        val = g(0, 0, 0)
        two = F(2.0)
        dxx = two * val - g(0, 0, -1) - g(0, 0, 1)
        dyy = two * val - g(0, -1, 0) - g(0, 1, 0)
        dxy = F(0.25) * (g(0, 1, 1) + g(0, -1, -1) - g(0, -1, 1) - g(0, 1, -1))
        tra = dxx + dyy
        det = dxx * dyy - dxy * dxy
        edge_ok = tra * tra < F(edge_limit) * det
        dx = F(0.5) * (g(0, 0, 1) - g(0, 0, -1))
        dy = F(0.5) * (g(0, 1, 0) - g(0, -1, 0))
        ds = F(0.5) * (g(-1, 0, 0) - g(1, 0, 0))
        dss = two * val - g(1, 0, 0) - g(-1, 0, 0)
        dxs = F(0.25) * (g(1, 0, 1) + g(-1, 0, -1) - g(-1, 0, 1) - g(1, 0, -1))
        dys = F(0.25) * (g(1, 1, 0) + g(-1, -1, 0) - g(1, -1, 0) - g(-1, 1, 0))
        idxx = dyy * dss - dys * dys
        idxy = dys * dxs - dxy * dss
        idxs = dxy * dys - dyy * dxs
        idet = F(1.0) / (idxx * dxx + idxy * dxy + idxs * dxs)
        idyy = dxx * dss - dxs * dxs
        idys = dxy * dxs - dxx * dys
        idss = dxx * dyy - dxy * dxy
        pdx = idet * (idxx * dx + idxy * dy + idxs * ds)
        pdy = idet * (idxy * dx + idyy * dy + idys * ds)
        pds = idet * (idxs * dx + idys * dy + idss * ds)
        h5 = F(0.5)
        fb = (pdx < -h5) | (pdx > h5) | (pdy < -h5) | (pdy > h5) | (pds < -h5) | (pds > h5)
        pdx = np.where(fb, dx / dxx, pdx)
        pdy = np.where(fb, dy / dyy, pdy)
        pds = np.where(fb, ds / dss, pds)
        scm = np.array([np.float32(2.0) ** (F(k) / F(5)) for k in range(5)], F)       # powf(2, s / NUM_SCALES)
        sc = (scm[s] * orc.det_eval(0, (pds * F(0.2)).astype(F))).astype(F) if len(s) else np.zeros(0, F)
        scale_ok = sc >= F(lowest_scale)
    return dict(x=x, y=y, s=s, edge_ok=edge_ok, fallback=fb, scale_ok=scale_ok, kept=edge_ok & scale_ok,
                xpos=(x + pdx).astype(F), ypos=(y + pdy).astype(F), scale=sc, val=val)


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def case(name):
    """The named case (built once)."""
    c = _BUILDERS[name]()
    c["name"] = name
    for f in c["frames"]:
        for a in f:
            a.setflags(write=False)
    return c


def _mk(geom, frames, thresh, aim, lowest_scale=0.0, detections=True, max_pts=4096):
    return dict(geom=geom, frames=frames, thresh=float(F(thresh)), lowest_scale=float(F(lowest_scale)), aim=aim,
                detections=detections, max_pts=max_pts)


def _lattice(geom, nframes):
    def build():
        frames = []
        for f in range(nframes):
            if nframes > 1 and f == 1:
                frames.append(flat_frame(geom))                     # one flat frame between two busy ones
            else:
                frames.append(lattice_frame(geom, phase=3 * f))
        return _mk(geom, frames, 2.0, "rows, columns, strip and segment seams, quad positions, borders")
    return build


TIE_SIGMA = (1.6, 2.2, 2.2)
TIE_THRESH = 1.0


def _ties(ulp):
    def build():
        sizes = level_sizes(*GEOM_Q)
        if ulp:
            made = [broken_tie_level(w, h, GEOM_Q[2], k + 1, TIE_THRESH, TIE_SIGMA[k]) for k, (w, h) in enumerate(sizes)]
            c = _mk(GEOM_Q, [[m[0] for m in made]], TIE_THRESH, "ties broken by the smallest raise of one pixel that the planes show")
            c["ulps"] = [m[1] for m in made]
            return c
        frame = [tie_level(w, h, None, TIE_SIGMA[k]) for k, (w, h) in enumerate(sizes)]
        return _mk(GEOM_Q, [frame], TIE_THRESH, "exact ties between neighbouring pixels")
    return build


def _case_edge():
    frame = [edge_level(w, h) for w, h in level_sizes(*GEOM_R)]
    return _mk(GEOM_R, [frame], 1.0, "the edge test tra^2 < 10 det on either side")


def _case_subpixel():
    n = SMALL_FRAMES + 1
    frames = [[subpixel_level(w, h, 10 * f + k) for k, (w, h) in enumerate(level_sizes(*GEOM_R))] for f in range(n)]
    frames[1] = flat_frame(GEOM_R)
    return _mk(GEOM_R, frames, 1.0, "sub-pixel solve and its |pd| > 0.5 fallback; batch above small_frames")


def _case_queue():
    frame = [queue_level(w, h, 50 + k) if k == 2 else flat(w, h) for k, (w, h) in enumerate(level_sizes(*GEOM_R))]
    frame[1] = noise_band_level(*level_sizes(*GEOM_R)[1], 60, range(20, 30))
    return _mk(GEOM_R, [frame], 1e-3, "wave queue: direct append and flush, below the list capacity", max_pts=16384)


def _case_overflow():
    sizes = level_sizes(*GEOM_R)
    frame = [flat(*sizes[0]), noise_band_level(*sizes[1], 70, range(20, 30)), noise_band_level(*sizes[2], 71, range(0, 150))]
    return _mk(GEOM_R, [frame], 1e-3, "more candidates than the finest octave's list holds", detections=False)


def _case_nonfinite():
    sizes = level_sizes(*GEOM_Q)
    frame = [lattice(*sizes[0], 1), lattice(*sizes[1], 2), nonfinite_level(*sizes[2])[0]]
    return _mk(GEOM_Q, [frame], 2.0, "NaN and inf pixels")


def _case_tiny4():
    frames = [lattice_frame(GEOM_T, phase=f, pitch=9, sigma=1.6) for f in range(2)]
    return _mk(GEOM_T, frames, 1.0, "four octaves, coarsest level 8 x 8")


_BUILDERS = {
    "lattice_r1": _lattice(GEOM_R, 1), "lattice_r5": _lattice(GEOM_R, SMALL_FRAMES + 1),
    "lattice_q1": _lattice(GEOM_Q, 1), "lattice_q5": _lattice(GEOM_Q, SMALL_FRAMES + 1),
    "ties": _ties(False), "ties_ulp": _ties(True), "edge": _case_edge, "subpixel": _case_subpixel,
    "queue": _case_queue, "overflow": _case_overflow, "nonfinite": _case_nonfinite, "tiny4": _case_tiny4,
}
CASE_NAMES = list(_BUILDERS)


def with_params(c, thresh=None, lowest_scale=None, name=None):
    """The same levels under another threshold / scale floor."""
    d = dict(c)
    if thresh is not None:
        d["thresh"] = float(F(thresh))
    if lowest_scale is not None:
        d["lowest_scale"] = float(F(lowest_scale))
    d["name"] = name or c["name"]
    return d


@functools.lru_cache(maxsize=None)
def ulp_cases():
    """Threshold and scale floor at the ulp, on the single-frame ragged lattice: (name, case, frame, octave, key of the
    detection concerned, whether it must be present)."""
    base = case("lattice_r1")
    w, h, noct = base["geom"]
    o = noct
    level = base["frames"][0][o - 1]
    planes = planes_of(level, noct, o)
    r = refine_np(planes, base["thresh"], 0.0)
    k = np.flatnonzero(r["kept"] & (r["x"] > 100) & (r["y"] > 40))
    # the weakest extremum there: a threshold equal to its |DoG| removes it and nothing else
    i = k[np.argmin(np.abs(r["val"][k]))]
    v = F(abs(r["val"][i]))
    at = (int(r["x"][i]), int(r["y"][i]), int(r["s"][i]))
    pts, n = oracle_detections(level, noct, o, base["thresh"], 0.0)
    j = int(np.argmin(np.abs(pts["xpos"][:n] - r["xpos"][i]) + np.abs(pts["ypos"][:n] - r["ypos"][i])))
    sc = F(pts["scale"][j])
    return [
        ("thresh_eq", with_params(base, thresh=v, name="thresh_eq"), at, False),
        ("thresh_below", with_params(base, thresh=np.nextafter(v, F(0)), name="thresh_below"), at, True),
        ("floor_eq", with_params(base, lowest_scale=sc, name="floor_eq"), at, True),
        ("floor_above", with_params(base, lowest_scale=np.nextafter(sc, F(np.inf)), name="floor_above"), at, False),
    ]


def all_runs():
    """Every (name, case) the GPU module runs: the cases and the ulp variants of the lattice."""
    return [(n, case(n)) for n in CASE_NAMES] + [(n, c) for n, c, _, _ in ulp_cases()]


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per frame and octave index k = o - 1 of the named run: dict(codes=sorted model codes, pts, n = oracle detections)."""
    c = dict(all_runs())[name]
    w, h, noct = c["geom"]
    out = []
    for frame in c["frames"]:
        row = []
        for k, level in enumerate(frame):
            pts, n = oracle_detections(level, noct, k + 1, c["thresh"], c["lowest_scale"]) if c["detections"] else (np.zeros(0, orc.POINT_DTYPE), 0)
            row.append(dict(codes=model_candidates(level, noct, k + 1, c["thresh"]), pts=pts[:n].copy(), n=n))
        out.append(row)
    return out
