"""Planted detections for the production per-keypoint kernels (bin_detections, orient_all*, renumber_dups, descr_all*,
descr_big) and the oracle's answer to them.

The kernels read Detection records out of the staging area; Context.describe_detections (misift_test_describe_detections)
puts records of OUR choosing there, next to pyramid levels of our choosing, and runs the launch sequence of an extraction
call from the binning on.  This module builds the levels and the records — aimed at the places where those kernels change
their path — and computes what the oracle (oracle/sift_oracle.c, the restated reference) makes of them.

A case is one frame: `levels` (coarsest first, like the reference's octave numbers 1 ... noct; the last is the finest level
of w x h) and per level an [n, 5] float32 array of (xpos, ypos, scale, sharpness, edgeness) in level coordinates, plus a
class label per record.  Every record of a case has its own sharpness, so util.associate pairs records exactly.

What the position classes aim at (cudasift_amd/csrc/kernels_points.hip):
  inside    orient_core: unclamped fetches iff xpos - 7 >= 1 and xpos + 8 <= w - 2 (same in y)
  window    patch_fetch: unclamped window loads iff floor(xpos) - 19 >= 0 and floor(xpos) - 19 + 40 <= w
  sane      patch_geom / orient_all_kernel: the int conversion guard, -64 < xpos < w + 64
  binade    orient_core: the shared 13 x 13 grid is used iff (xp + k) + 1 == xp + (k + 1) for every sample column / row
  reach     patch_geom: the LDS window is used iff 10.6067 * (0.75 * scale) + 1 <= patch_reach (17.9)
  cinterior descr_core (descr_big, descr_all_gather): unclamped fetches iff px -+ (10.6067 * 0.75 * scale + 2.5) in [1, w - 2]
The predicates below restate them in numpy float32; test_points_cases_cpu.py proves that every class has members on the
sides it claims."""
import numpy as np

F = np.float32
REACH_LIMIT = F(17.9)                 # PATCH_REACH
GEOM_A = (187, 131, 3)                # an ordinary frame with odd sizes: 187x131, 93x65, 46x32
GEOM_B = (97, 61, 4)                  # coarse levels under 40 and under 13: 97x61, 48x30, 24x15, 12x7


def level_sizes(w, h, noct):
    """[(w, h)] of the pyramid levels, coarsest first (pyramid_levels: halved with integer division per level)."""
    out = []
    for _ in range(noct):
        out.append((w, h))
        w, h = w // 2, h // 2
    return out[::-1]


# ------------------------------------------------------------------ level content (values in [0, 255])
def _blur(a, sigma):
    """Separable Gaussian with clamp-to-edge borders (plain numpy; float64)."""
    r = max(1, int(3 * sigma + 0.5))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        pad = [(r, r) if ax == axis else (0, 0) for ax in (0, 1)]
        p = np.pad(a, pad, mode="edge")
        a = sum(k[i] * np.take(p, np.arange(i, i + a.shape[axis]), axis=axis) for i in range(2 * r + 1))
    return a


def content(kind, w, h, seed=0):
    """One level of the named content, float32 [h, w]."""
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "flat":
        a = np.full((h, w), 97.0)
    elif kind == "ramp+x":
        a = 255.0 * x / max(w - 1, 1)
    elif kind == "ramp-x":
        a = 255.0 * (1.0 - x / max(w - 1, 1))
    elif kind == "ramp+y":
        a = 255.0 * y / max(h - 1, 1)
    elif kind == "ramp-y":
        a = 255.0 * (1.0 - y / max(h - 1, 1))
    elif kind == "ramp_diag":
        a = 255.0 * (x + y) / max(w + h - 2, 1)
    elif kind == "ramp_diag_noisy":                    # 45-degree gradient everywhere, texture on top
        a = 40.0 + 1.1 * (x + y) * 160.0 / max(w + h - 2, 1) + 12.0 * _blur(rng.standard_normal((h, w)), 1.2)
    elif kind == "step":
        a = np.where(x + 0.3 * y < 0.55 * w, 40.0, 210.0)
    elif kind == "corner":                             # L-shaped corners on a 24-pixel lattice: two orientation peaks
        a = np.where(((x % 24) >= 12) & ((y % 24) >= 12), 215.0, 45.0)
        a = _blur(a, 0.8)
    elif kind == "grating":                            # point-symmetric about every crest: two opposite, nearly equal peaks
        u = (x * np.cos(0.6) + y * np.sin(0.6))
        a = 128.0 + 100.0 * np.cos(2.0 * np.pi * u / 14.0)
    elif kind == "checker":
        a = np.where(((x // 6) + (y // 6)) % 2 == 0, 30.0, 220.0)
    elif kind == "impulse":
        a = np.full((h, w), 20.0)
        a[h // 2, w // 2] = 255.0
    elif kind == "noise":
        a = rng.uniform(0.0, 255.0, (h, w))
    elif kind == "blurred_noise":
        b = _blur(rng.standard_normal((h, w)), 2.0)
        a = 128.0 + 60.0 * b / b.std()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.clip(a, 0.0, 255.0), F)


CONTENT_KINDS = ("flat", "ramp+x", "ramp-x", "ramp+y", "ramp-y", "ramp_diag", "step", "corner", "grating", "checker", "impulse",
                 "noise", "blurred_noise")


# ------------------------------------------------------------------ predicates of the kernels, in float32
def reach_of(scale):
    """patch_geom: 10.6067f * (0.75f * scale) + 1.0f with each operation rounded to float32 (no contraction: hipcc
    builds the library with -ffp-contract=off, the kernels write their fused operations out)."""
    s = np.asarray(scale, F)
    return (F(10.6067) * (F(0.75) * s)).astype(F) + F(1.0)


def sane(x, y, w, h):
    x, y = np.asarray(x, F), np.asarray(y, F)
    return (x > F(-64.0)) & (y > F(-64.0)) & (x < F(w + 64)) & (y < F(h + 64))


def orient_inside_1d(p, n):
    p = np.asarray(p, F)
    return ((p - F(7.0)) >= F(1.0)) & ((p + F(8.0)) <= F(n - 2))


def window_interior_1d(p, n):
    """patch_fetch along one axis, for a sane coordinate: x0 = floor(p) - 19 >= 0 and x0 + 40 <= n."""
    x0 = np.floor(np.asarray(p, F)).astype(np.int64) - 19
    return (x0 >= 0) & (x0 + 40 <= n)


def binade_safe_1d(p):
    """orient_core's `same` over one coordinate: every (xp + k) + 1 == xp + (k + 1) and (xp + k) - 1 == xp + (k - 1)."""
    xp = (np.asarray(p, F) - F(4.5)).astype(F)
    ok = np.ones(xp.shape, bool)
    for k in range(10):
        ok &= ((xp + F(k)).astype(F) + F(1.0)).astype(F) == (xp + F(k + 1)).astype(F)
        ok &= ((xp + F(k + 1)).astype(F) - F(1.0)).astype(F) == (xp + F(k)).astype(F)
    return ok


def descr_interior_1d(p, scale, n):
    """descr_core along one axis: p - reach >= 1 and p + reach <= n - 2 with reach = 10.6067f * (0.75f * scale) + 2.5f."""
    p = np.asarray(p, F)
    r = (F(10.6067) * (F(0.75) * np.asarray(scale, F))).astype(F) + F(2.5)
    return ((p - r) >= F(1.0)) & ((p + r) <= F(n - 2))


def around(v):
    """[one ulp below v, v, one ulp above v] as float32."""
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def around_wide(v, n=3):
    """The 2 n + 1 float32 values from n ulps below v to n ulps above.  (xpos + 8 <= w - 2 is decided after the sum is
    rounded: where xpos + 8 lies in the next binade, 121 + 8 for instance, one ulp of xpos is half an ulp of the sum and
    the first value that fails is two ulps above the threshold.)"""
    out = [F(v)]
    for _ in range(n):
        out = [np.nextafter(out[0], F(-np.inf))] + out + [np.nextafter(out[-1], F(np.inf))]
    return out


def reach_scales():
    """Scales whose reach is one ulp below 17.9f, 17.9f itself and one ulp above: [(scale, reach)] — every float32 scale
    around the crossing that lands on one of the three values (the scale's ulp maps to about one ulp of the reach)."""
    want = around(REACH_LIMIT)
    s = F((17.9 - 1.0) / (10.6067 * 0.75))
    for _ in range(64):
        s = np.nextafter(s, F(-np.inf))
    out = []
    for _ in range(128):
        r = reach_of(s)
        if any(r == t for t in want):
            out.append((F(s), F(r)))
        s = np.nextafter(s, F(np.inf))
    return out


# ------------------------------------------------------------------ detection classes
class _Builder:
    """Collects the records of one frame; hands out the unique sharpness values."""

    def __init__(self, name, geom, kinds, seed):
        w, h, noct = geom
        self.name, self.geom = name, geom
        self.sizes = level_sizes(w, h, noct)
        self.kinds = list(kinds)
        assert len(self.kinds) == noct
        self.levels = [content(k, lw, lh, seed + i) for i, (k, (lw, lh)) in enumerate(zip(self.kinds, self.sizes))]
        self.rows = [[] for _ in range(noct)]
        self.labels = [[] for _ in range(noct)]
        self.rng = np.random.default_rng(seed)
        self.serial = 0

    def add(self, k, label, x, y, scale):
        """Records at level index k (0 = coarsest): broadcast x, y, scale."""
        x, y, scale = np.broadcast_arrays(np.asarray(x, F), np.asarray(y, F), np.asarray(scale, F))
        for xi, yi, si in zip(x.ravel(), y.ravel(), scale.ravel()):
            self.serial += 1
            sharp = F(3.0) + F(self.serial) * F(1.0 / 256.0)                 # exact in float32: unique per record
            edge = F(1.5) + F(self.serial % 7) * F(0.25)
            self.rows[k].append((xi, yi, si, sharp, edge))
            self.labels[k].append(label)

    def scales(self, n, lo=0.5, hi=2.1):
        return self.rng.uniform(lo, hi, n).astype(F)

    def interior(self, k, n, label="interior"):
        w, h = self.sizes[k]
        self.add(k, label, self.rng.uniform(0.0, w - 1.0, n), self.rng.uniform(0.0, h - 1.0, n), self.scales(n))

    def fill_to(self, k, n):
        """Interior records until level k holds exactly n."""
        assert len(self.rows[k]) <= n, (self.name, k, len(self.rows[k]), n)
        self.interior(k, n - len(self.rows[k]))

    def case(self):
        dets = [np.array(r, F).reshape(-1, 5) for r in self.rows]
        return {"name": self.name, "geom": self.geom, "kinds": self.kinds, "levels": self.levels, "dets": dets,
                "labels": [np.array(l, dtype=object) for l in self.labels]}


def border_coords(n):
    """Coordinates of the border class along an axis of n pixels: on the first / last pixel, half a pixel in, slightly
    outside, and on either side of the +-64 guard."""
    return [0.0, 0.5, n - 1.0, n - 0.5, -0.4, n + 3.0, -63.5, -64.0, -64.5, n + 63.5, n + 64.0, n + 64.5]


def _case_interior():
    b = _Builder("interior", GEOM_A, ("checker", "noise", "blurred_noise"), 11)
    b.fill_to(0, 64)
    b.fill_to(1, 257)
    b.fill_to(2, 300)
    return b.case()


def _case_border():
    b = _Builder("border", GEOM_A, ("step", "ramp_diag", "blurred_noise"), 12)
    for k in (1, 2):
        w, h = b.sizes[k]
        bx, by = border_coords(w), border_coords(h)
        gx, gy = np.meshgrid(bx, by)                                           # the corners and their surroundings
        b.add(k, "border", gx.ravel(), gy.ravel(), b.scales(gx.size))
        mid_x, mid_y = b.rng.uniform(25, w - 25, len(by)), b.rng.uniform(25, h - 25, len(bx))
        b.add(k, "border", mid_x, by, b.scales(len(by)))                       # the four edges
        b.add(k, "border", bx, mid_y, b.scales(len(bx)))
    w, h = b.sizes[0]
    b.add(0, "border", border_coords(w), b.rng.uniform(0, h - 1, 12), b.scales(12))
    return b.case()


def _case_thresholds():
    b = _Builder("thresholds", GEOM_A, ("ramp+x", "ramp-y", "blurred_noise"), 13)
    k = 2
    w, h = b.sizes[k]
    for n, axis in ((w, 0), (h, 1)):
        vals = []
        for v in (8.0, n - 10.0):                       # orient_core's inside test
            vals += [("inside", t) for t in around_wide(v)]
        for v in (19.0, n - 21.0, n - 20.0):            # patch_fetch: floor(p) = 19 and n - 21 (n - 20: the first clamped one)
            vals += [("window", t) for t in around(v)]
        for label, t in vals:
            for rep in range(3):
                other = b.rng.uniform(30.0, (h if axis == 0 else w) - 30.0)
                x, y = (t, other) if axis == 0 else (other, t)
                b.add(k, label, x, y, b.scales(1))
    for label, vx, vy in (("inside", 8.0, 8.0), ("inside", w - 10.0, h - 10.0), ("window", 19.0, 19.0),
                          ("window", w - 20.0, h - 20.0), ("window", 19.0, h - 20.0)):
        for tx in around(vx):                           # both axes on the threshold at once
            for ty in around(vy):
                b.add(k, label, tx, ty, b.scales(1))
    # descr_core's interior test (descr_big and the gather kernel): p - reach == 1 and p + reach == n - 2
    for s in (F(0.6), F(1.3), F(2.0)):
        r = (F(10.6067) * (F(0.75) * s)).astype(F) + F(2.5)
        for n, axis in ((w, 0), (h, 1)):
            for v in (F(1.0) + r, F(n - 2) - r):
                for t in around_wide(v):
                    other = b.rng.uniform(40.0, (h if axis == 0 else w) - 40.0)
                    x, y = (t, other) if axis == 0 else (other, t)
                    b.add(k, "cinterior", x, y, s)
    b.interior(0, 20)
    b.interior(1, 30)
    return b.case()


def _case_binade():
    b = _Builder("binade", GEOM_A, ("ramp+y", "grating", "blurred_noise"), 14)
    k = 2
    w, h = b.sizes[k]
    safe_x, safe_y = F(50.25), F(41.25)                 # xp + k stays inside one binade: safe
    for p2 in (4, 8, 16, 32, 64, 128):
        for j in range(11):
            at = F(p2 - j + 4.5)                                               # (xpos - 4.5) + j == p2 exactly
            below = at                                                         # ... just below p2: the largest xpos whose
            while ((below - F(4.5)).astype(F) + F(j)).astype(F) >= F(p2):      # sum stays under the power of two
                below = np.nextafter(below, F(-np.inf))
            for t in (at, below):
                b.add(k, "binade_x", t, safe_y, b.scales(1))
                b.add(k, "binade_y", safe_x, t, b.scales(1))                   # only y can be unsafe
            b.add(k, "binade_xy", below, below, b.scales(1))
    b.interior(0, 20)
    b.interior(1, 40)
    return b.case()


def _case_reach():
    b = _Builder("reach", GEOM_A, ("ramp-x", "corner", "ramp_diag_noisy"), 15)
    k = 2
    w, h = b.sizes[k]
    spots = [(w / 2.0 + 0.3, h / 2.0 - 0.2), (12.5, 60.25), (w - 9.75, 55.5), (70.5, 6.25), (88.25, h - 14.5),
             (17.75, 15.5), (w - 12.5, h - 11.25), (3.5, h - 2.5), (w - 1.0, 2.0)]
    for s, _ in reach_scales():                          # one ulp below / at / one ulp above 17.9: interior and within 20 px of
        for x, y in spots:                               # every border and corner, on 45-degree content
            b.add(k, "reach_edge", x, y, s)
    for x, y in ((23.5, 16.25), (9.5, 20.5), (30.25, 3.5)):
        for s, _ in reach_scales():
            b.add(1, "reach_edge", x, y, s)              # ... and on the corner lattice
    for s in (2.2, 2.35, 2.6):                           # a little over the limit: a window a column or two short would do for
        for x, y in spots:                               # most samples of these, so a wrong limit shows only on them
            b.add(k, "reach_over", x, y, F(s))
    far = [(w / 2.0, h / 2.0), (5.5, 7.25), (w - 4.0, h - 6.5), (-20.0, 40.0), (60.0, h + 30.5), (-63.5, -63.5),
           (w + 63.5, h + 63.5), (w + 64.5, 20.0)]
    for s in (3.0, 8.0, 40.0):                           # well above: the sample grid lies mostly or wholly outside the level
        for x, y in far:
            b.add(k, "reach_big", x, y, F(s))
            b.add(0, "reach_big", x / 4.0, y / 4.0, F(s))
    for x, y in far[:5] + spots[:5]:                     # tiny scales
        b.add(k, "reach_tiny", x, y, F(0.05))
        b.add(k, "reach_tiny", x + 0.37, y + 0.61, F(0.011))
    b.interior(1, 20)
    return b.case()


def _case_flat():
    b = _Builder("flat", GEOM_A, ("impulse", "flat", "impulse"), 16)
    b.interior(1, 40, "flat")
    w, h = b.sizes[1]
    b.add(1, "flat", border_coords(w)[:6], b.rng.uniform(0, h - 1, 6), b.scales(6))
    b.add(1, "flat", [30.0, 40.5], [20.0, 33.25], [F(3.0), F(8.0)])           # flat through descr_big as well
    for k in (0, 2):                                     # far from the impulse: every fetch reads the background
        w, h = b.sizes[k]
        n = 12 if k == 0 else 40
        x = np.where(b.rng.random(n) < 0.5, b.rng.uniform(0, w / 2 - 13, n), b.rng.uniform(w / 2 + 14, w - 1, n))
        b.add(k, "flat", x, b.rng.uniform(0, h - 1, n), b.scales(n, 0.5, 0.8))
        b.add(k, "impulse_near", w / 2 + b.rng.uniform(-4, 4, 8), h / 2 + b.rng.uniform(-4, 4, 8), b.scales(8))
    return b.case()


def _case_dups():
    """Content with two orientation peaks: corners, a grating (opposite peaks), a checkerboard."""
    b = _Builder("dups", GEOM_A, ("checker", "grating", "corner"), 17)
    w, h = b.sizes[2]
    cx, cy = np.meshgrid(np.arange(12, w - 6, 24), np.arange(12, h - 6, 24))   # the L corners of the lattice
    for dx, dy in ((0.0, 0.0), (0.5, 0.5), (-0.75, 0.4), (1.25, -1.0)):
        b.add(2, "dups", cx.ravel() + dx, cy.ravel() + dy, b.scales(cx.size, 0.8, 1.6))
    w, h = b.sizes[1]
    u = np.arange(14.0, 70.0, 14.0)                                            # crests of the grating: u = 14 m
    for t in (-8.0, 0.0, 6.5):
        x = u * np.cos(0.6) - t * np.sin(0.6)
        y = u * np.sin(0.6) + t * np.cos(0.6) + 12.0
        b.add(1, "dups", x, y, b.scales(len(u), 0.8, 1.8))
        b.add(1, "dups", x + 0.02, y - 0.01, b.scales(len(u), 0.8, 1.8))
    w, h = b.sizes[0]
    gx, gy = np.meshgrid(np.arange(6.0, w - 3, 6.0), np.arange(6.0, h - 3, 6.0))  # checkerboard crossings
    b.add(0, "dups", gx.ravel(), gy.ravel(), b.scales(gx.size, 0.6, 1.2))
    return b.case()


def _case_counts():
    """An empty octave between two others; 63 and 65 records (one short of / one over a wavefront's worth)."""
    b = _Builder("counts", GEOM_A, ("noise", "checker", "step"), 18)
    b.fill_to(0, 63)
    b.fill_to(2, 65)
    return b.case()


def _case_small():
    """Levels smaller than the 40 x 40 descriptor window and the 13 x 13 orientation grid: clamped on both sides at once."""
    b = _Builder("small", GEOM_B, ("noise", "blurred_noise", "checker", "corner"), 19)
    w, h = b.sizes[0]                                     # 12 x 7
    b.add(0, "small", w / 2.0 + 0.25, h / 2.0 - 0.5, F(1.1))                   # an octave with ONE record
    for k in (1, 2, 3):
        w, h = b.sizes[k]
        n = (0, 40, 64, 120)[k]
        b.interior(k, n, "small" if k < 3 else "interior")
        bx, by = border_coords(w)[:6], border_coords(h)[:6]
        gx, gy = np.meshgrid(bx, by)
        b.add(k, "small" if k < 3 else "border", gx.ravel(), gy.ravel(), b.scales(gx.size))
        b.add(k, "small" if k < 3 else "border", [-63.5, -64.5, w + 63.5, w + 64.0], [h / 2.0] * 4, b.scales(4))
        b.add(k, "small" if k < 3 else "reach_big", [w / 2.0, 1.5], [h / 2.0, h - 1.0], [F(3.0), F(8.0)])
    return b.case()


_BUILDERS = {"interior": _case_interior, "border": _case_border, "thresholds": _case_thresholds, "binade": _case_binade,
             "reach": _case_reach, "flat": _case_flat, "dups": _case_dups, "counts": _case_counts, "small": _case_small}
CASE_NAMES = tuple(_BUILDERS)
_cache = {}


def case(name):
    """The named case (built once; treat as read-only)."""
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def empty_case(geom=GEOM_A):
    """A frame without a single detection (flat levels)."""
    key = ("empty",) + tuple(geom)
    if key not in _cache:
        b = _Builder("empty", geom, ("flat",) * geom[2], 20)
        _cache[key] = b.case()
    return _cache[key]


MULTI = ("border", None, "reach", "counts", "dups")      # five frames of one call; None: the empty frame


def multi_frames():
    return [case(n) if n else empty_case() for n in MULTI]


def tile_order(c):
    """The case with every octave's records in the order deterministic mode gives the staging area (bin_detections_kernel:
    32 x 32-pixel tiles row-major, keys clamped into the level, then det_less: y, x, scale, sharpness).  With the records
    supplied in this order the oracle's rule at capacity — first come, first kept, second orientations appended in keypoint
    order — names the same survivors as the device's."""
    out = dict(c, dets=[], labels=[])
    for (w, h), d, l in zip(level_sizes(*c["geom"]), c["dets"], c["labels"]):
        tx, ty = (w >> 5) + 1, (h >> 5) + 1
        kx = np.clip(d[:, 0].astype(np.int32) >> 5, 0, tx - 1)                 # (int)xpos: truncation, as the kernel's cast
        ky = np.clip(d[:, 1].astype(np.int32) >> 5, 0, ty - 1)
        order = np.lexsort((d[:, 3], d[:, 2], d[:, 0], d[:, 1], ky * tx + kx))
        out["dets"].append(np.ascontiguousarray(d[order]))
        out["labels"].append(l[order])
    return out


def total(c):
    return int(sum(len(d) for d in c["dets"]))


def count_big(c, max_pts, patch_reach=REACH_LIMIT):
    """Records descr_all defers to descr_big: not sane, or reach > patch_reach — counted once per keypoint, and only where
    the keypoint's own record lies below capacity (without duplicates in the way: the callers use roomy capacities)."""
    n = 0
    for (w, h), d in zip(level_sizes(*c["geom"]), c["dets"]):
        n += int((~sane(d[:, 0], d[:, 1], w, h) | (reach_of(d[:, 2]) > F(patch_reach))).sum())
    assert total(c) <= max_pts
    return n


# ------------------------------------------------------------------ the oracle's answer
_expect_cache = {}


def expected(c, max_pts, fracbits=8, scale_up=False, fix_numpts=False):
    """What ExtractSift makes of the case's detections, by the oracle alone and exactly as its extract_octave does:
    octave after octave, coarsest first, the records are appended behind the previous octave's second orientations,
    orc.orientations then orc.descriptors run on them, and the 17 counters follow the reference's protocol.
    Returns (points[max_pts], numPts, counters[17], stats) — cached per argument set; do not modify."""
    key = (c["name"], id(c), max_pts, fracbits, bool(scale_up), bool(fix_numpts))
    if key in _expect_cache:
        return _expect_cache[key]
    from oracle import pyoracle as orc
    w, h, noct = c["geom"]
    pts = np.zeros(max_pts, orc.POINT_DTYPE)
    cnt = np.zeros(17, np.int64)
    orc.stats_reset()
    for o in range(1, noct + 1):
        level, d = c["levels"][o - 1], c["dets"][o - 1]
        sub = float(2 ** (noct - o))
        start = int(cnt[2 * o - 1])
        cnt[2 * o] = start + len(d)
        for i in range(min(len(d), max(0, max_pts - start))):
            r = pts[start + i]
            r["xpos"], r["ypos"], r["scale"], r["sharpness"], r["edgeness"] = d[i]
            r["subsampling"] = sub
        fst, tot = min(start, max_pts), min(int(cnt[2 * o]), max_pts)
        end = orc.orientations(level, pts, fst, tot, max_pts, fracbits)        # counts the appended duplicates from `tot` on
        cnt[2 * o + 1] = cnt[2 * o] + (end - tot)
        tot2 = min(int(cnt[2 * o + 1]), max_pts)
        orc.descriptors(level, pts, fst, tot2, sub, fracbits)
    st = orc.stats()
    num = int(min(cnt[2 * noct + (1 if fix_numpts else 0)], max_pts))
    if scale_up:                                           # RescalePositions: the first numPts records (Appendix B #1)
        for f in ("xpos", "ypos", "scale"):
            pts[f][:num] *= F(0.5)
    out = (pts, num, cnt.astype(np.uint32), st)
    _expect_cache[key] = out
    return out


def written(cnt, noct, max_pts):
    """Records of a call that exist in the array: all segments, capped."""
    return int(min(int(cnt[2 * noct + 1]), max_pts))
