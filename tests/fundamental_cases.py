"""Inputs of the fundamental-matrix edge tests (test_fundamental_edges_cpu.py pins the numpy restatement and the host
hooks at every one of them, test_gpu_fundamental_edges.py runs the device against the restatement).  No GPU in here, and
cudasift_amd.capi is imported inside functions only.

What the cases are for: the degenerate and non-finite samples of the 8-point solve, coordinate scales from where every
distance underflows to where every product overflows, F matrices a caller may hand to score, thresholds whose square
leaves the float range, and scenes in which a tenth of the records carry a hostile position."""
import numpy as np

from batch_util import span
from test_fundamental_cpu import GATES, expected_find, expected_score, f32, planted_scene, solve8

POS = ("xpos", "ypos", "match_xpos", "match_ypos")
TINY = np.finfo(np.float32).tiny                                 # the smallest normal float32
NAN_BITS = 0x7FC00000                                            # the one NaN match_error may hold


def bit_positions(n, rng):
    """(n, 4) float32 of random bit patterns: NaN payloads of both signs, infinities, subnormals, any exponent."""
    return rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)


def is_subnormal(v):
    v = np.abs(np.asarray(v, f32))
    return (v > 0) & (v < TINY)


# ---- forced samples: (name, (8, 4) float32 = x1 y1 x2 y2 per match)

# decades from 1e-22 to 1e25; between them the scales at which dx*dx + dy*dy of a sample is subnormal but not zero (the
# argument of sqrtf is then a denormal), and 1e19 again with more draws: there F itself has subnormal entries
SCALES = [10.0 ** e for e in range(-22, 26)] + [3e-19, 4e-19, 5e-19, 7e-19, 1e-18, 1e19, 1e19, 1e19]


# Eight matches on small integer lattices, found by search: the normalised system holds equal largest entries, so the
# pivot search meets a tie, and a search that lets the LAST maximum win gives other bits of F for every order of the eight
# (the header's rule is the first maximum)
LATTICES = (
    [[-1, -2, 2, -1], [-1, -2, -1, 0], [2, 1, 1, 0], [1, -1, 1, 0], [-1, -2, 0, 0], [0, 0, -2, 1], [1, 0, 1, -2],
     [-1, 1, 2, -2]],
    [[1, 2, 2, 0], [1, 1, -2, -2], [1, -2, 0, -2], [2, 2, -1, -1], [-2, -2, -1, -2], [2, 2, 1, 1], [0, 1, 2, 2],
     [-2, 1, 0, 0]],
    [[1, 0, -2, 1], [0, -1, 2, 1], [2, 0, 0, 2], [-1, 0, 1, -1], [-1, 0, -1, 2], [1, 2, -1, 0], [0, -1, -1, 2],
     [-1, 0, 0, 1]],
    [[0, 0, 2, 2], [1, 1, -1, -1], [0, 2, 2, 1], [-2, -2, 2, -1], [2, 0, 1, 0], [-1, 1, -1, -1], [0, 0, 0, 2],
     [2, 0, 0, 2]],
)


def pivot_ties(sample):
    """How many steps of the elimination of `sample` (in its own order) meet more than one largest entry."""
    from test_fundamental_cpu import _normalise
    s = np.asarray(sample, f32)[None]
    x1, y1, x2, y2 = (s[:, :, c] for c in range(4))
    c1x, c1y, s1 = _normalise(x1, y1)
    c2x, c2y, s2 = _normalise(x2, y2)
    u1, v1, u2, v2 = (x1 - c1x) * s1, (y1 - c1y) * s1, (x2 - c2x) * s2, (y2 - c2y) * s2
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], 2)[0].astype(f32)
    ties = 0
    for k in range(8):
        mag = np.abs(A[k:, k:])
        ties += int((mag == mag.max()).sum() > 1)
        r, c = np.unravel_index(np.argmax(mag), mag.shape)
        A[[k, k + r]] = A[[k + r, k]]
        A[:, [k, k + c]] = A[:, [k + c, k]]
        for i in range(k + 1, 8):
            A[i, k + 1:] = A[i, k + 1:] - (A[i, k] / A[k, k]) * A[k, k + 1:]
    return ties


def forced_samples():
    rng = np.random.default_rng(4)
    base = rng.uniform(0, 1920, (8, 4)).astype(f32)
    out = [("identical", np.tile(base[:1], (8, 1)))]
    line = base.copy()
    line[:, 1], line[:, 3] = 300.0, 512.0
    out.append(("axis-parallel line", line))
    slanted = base.copy()
    slanted[:, 1], slanted[:, 3] = f32(0.37) * slanted[:, 0] + f32(11), f32(-1.3) * slanted[:, 2] + f32(900)
    out.append(("slanted line", slanted))
    two = base.copy()
    two[2:] = two[1]
    out.append(("two points", two))
    for v in (np.nan, np.inf, -np.inf):
        for c in range(4):
            s = base.copy()
            s[int(rng.integers(0, 8)), c] = v
            out.append(("%s in column %d" % (v, c), s))
    for i, scale in enumerate(SCALES):
        out.append(("scale %g #%d" % (scale, i), rng.uniform(-scale, scale, (8, 4)).astype(f32)))
    for i, s in enumerate(LATTICES):
        out.append(("lattice %d" % i, np.array(s, f32)))
    out.append(("plain", base))
    return out


def sqrt_arguments(s):
    """dx*dx + dy*dy of both point sets of a sample, as fundamental_normalise forms them: (16,) float32."""
    s = np.asarray(s, f32)
    args = []
    with np.errstate(all="ignore"):
        for x, y in ((s[:, 0], s[:, 1]), (s[:, 2], s[:, 3])):
            sx, sy = f32(0), f32(0)
            for k in range(8):
                sx, sy = sx + x[k], sy + y[k]
            dx, dy = x - sx * f32(0.125), y - sy * f32(0.125)
            args.append(dx * dx + dy * dy)
    return np.concatenate(args)


def solve_all(samples):
    """solve8 on a list of (8, 4) samples: (F (L, 9), valid (L,))."""
    a = np.stack(samples).astype(f32)
    return solve8(a[:, :, 0], a[:, :, 1], a[:, :, 2], a[:, :, 3])


def forced_frame(sample, extra, seed):
    """A frame whose only valid records are the 8 matches of `sample`, at random rows among `extra` records that fail the
    gate and hold random bit patterns (and NaN, +inf, -inf) as positions; every other byte random.  Every hypothesis of the frame is a
    permutation of the sample."""
    from cudasift_amd import capi
    rng = np.random.default_rng(seed)
    n = 8 + extra
    recs = np.frombuffer(rng.bytes(576 * n), capi.POINT_DTYPE).copy()
    pos = bit_positions(n, rng)
    rows = np.sort(rng.choice(n, 8, replace=False))
    for j, r in enumerate(np.setdiff1d(np.arange(n), rows)[::4]):            # every fourth of them surely non-finite
        pos[r, j % 4] = (np.nan, np.inf, -np.inf)[j % 3]
    pos[rows] = sample
    for c, k in enumerate(POS):
        recs[k] = pos[:, c]
    recs["score"], recs["ambiguity"] = 0.85, 0.3                 # score == min_score: rejected
    half = rng.random(n) < 0.5
    recs["score"][half], recs["ambiguity"][half] = 0.97, 0.95    # ambiguity == max_ambiguity: rejected
    recs["score"][rows], recs["ambiguity"][rows] = 0.97, 0.3
    return recs


# ---- F matrices a caller may hand to score: (name, 9 float32)

def score_matrices():
    rng = np.random.default_rng(6)
    sub = rng.uniform(-1, 1, 9).astype(f32) * f32(1e-39)
    mixed = rng.normal(0, 1, 9).astype(f32)
    mixed[4] = np.nan
    return [("nan", np.full(9, np.nan, f32)), ("+inf", np.full(9, np.inf, f32)), ("-inf", np.full(9, -np.inf, f32)),
            ("1e30", np.full(9, 1e30, f32)), ("1e-30", np.full(9, 1e-30, f32)), ("-0", np.full(9, -0.0, f32)),
            ("subnormal", sub), ("rank 3", rng.normal(0, 1, 9).astype(f32)), ("one nan", mixed)]


def score_frame(n, seed):
    """n records that all pass the gate: three quarters with random bit patterns as positions, a quarter with positions
    of a 1920 x 1080 frame (so finite errors are compared, too); every other byte random."""
    from cudasift_amd import capi
    rng = np.random.default_rng(seed)
    recs = np.frombuffer(rng.bytes(576 * n), capi.POINT_DTYPE).copy()
    pos = bit_positions(n, rng)
    plain = rng.random(n) < 0.25
    pos[plain] = rng.uniform(0, 1920, (int(plain.sum()), 4)).astype(f32)
    for c, k in enumerate(POS):
        recs[k] = pos[:, c]
    recs["score"], recs["ambiguity"] = 0.97, 0.3
    recs["score"][rng.random(n) < 0.1] = 0.85                    # a tenth fails the gate: scored, not counted
    return recs


# ---- thresholds: thresh * thresh is 0 for the first two, 1e38 for the third and +inf for the last two

THRESHOLDS = (1e-30, 1e-23, 1e19, 1e20, float("inf"))
THRESH_SCENE = dict(seed=1, n=200, find_seed=5, loops=32)


# ---- gate values: (score, ambiguity, passes)

def gate_values(min_score=0.85, max_ambiguity=0.95):
    up, down = np.nextafter(f32(min_score), f32(np.inf)), np.nextafter(f32(max_ambiguity), f32(-np.inf))
    nan, inf = f32(np.nan), f32(np.inf)
    return [(nan, f32(0.3), False), (inf, f32(0.3), True), (-inf, f32(0.3), False), (f32(0.97), nan, False),
            (f32(0.97), -inf, True), (f32(0.97), inf, False), (up, f32(0.3), True), (f32(0.97), down, True),
            (up, down, True), (f32(min_score), f32(0.3), False), (f32(0.97), f32(max_ambiguity), False)]


def gate_frame(seed, n=120):
    """A planted scene whose records carry gate_values() in turn (a third of them keep the scene's own passing values).
    Returns (records, passes)."""
    recs, _, _ = planted_scene(seed, n=n)
    vals = gate_values()
    passes = np.ones(n, bool)
    for k, r in enumerate(r for r in range(n) if r % 3):
        recs["score"][r], recs["ambiguity"][r], passes[r] = vals[k % len(vals)]
    return recs, passes


# ---- mixed scenes

HOSTILE = (np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40, 3e38)
MIXED_SEEDS = (1, 2, 3)
MIXED_FIND_SEED = 77
MIXED_LOOPS = (64, 256)


def mixed_scene(seed, n=600):
    """planted_scene(seed, n) with a tenth of its (all valid) records carrying one of HOSTILE in one of the four position
    fields.  Returns (records, planted-inlier mask, hostile mask)."""
    recs, inl, _ = planted_scene(seed, n=n)
    rng = np.random.default_rng(9000 + seed)
    rows = rng.choice(n, n // 10, replace=False)
    hostile = np.zeros(n, bool)
    hostile[rows] = True
    for i, r in enumerate(rows):
        recs[POS[int(rng.integers(0, 4))]][r] = HOSTILE[i % len(HOSTILE)]
    return recs, inl, hostile


# ---- the batches of test_gpu_fundamental.py and test_gpu_fundamental_refine.py

NOISE = 0.5                                                      # px, on the positions of the refinement's scenes

MAX_PTS = 2000
# frame -> records held; frame 10 has count -1, frame 11 one record more than max_pts, frames 12..14 are gated down to
# 7, 8 and 9 valid records; frame 15 is in no entry
SIZES = [0, 7, 8, 9, 63, 64, 65, 512, 513, 2000, 40, MAX_PTS + 1, 100, 100, 100, 30]
COUNTS = SIZES[:10] + [-1] + SIZES[11:]
SEL = [9, 3, 12, 0, 14, 7, 11, 1, 13, 5, 10, 2, 8, 4, 6]         # not in frame order
SEEDS = [1, 2, 3, 0, 2**32 - 1, 12345, 7, 8, 9, 10, 11, 2**31, 13, 14, 15]


def batch_records(n, seed, keep=None):
    """n records of a planted scene with every byte outside the fields in play random; from 10 records on a fifth of them
    fails the gate (keep: exactly that many pass)."""
    rng = np.random.default_rng(1000 + seed)
    from cudasift_amd import capi
    recs = np.frombuffer(rng.bytes(576 * n), capi.POINT_DTYPE).copy()
    if n == 0:
        return recs
    scene, _, _ = planted_scene(seed, n=n)
    for k in ("xpos", "ypos", "match_xpos", "match_ypos", "score", "ambiguity", "match", "match_error"):
        recs[k] = scene[k]
    if keep is None:
        fail = (rng.random(n) < 0.2) & (n >= 10)                 # the frames of 8 and 9 records keep them all
    else:
        fail = np.ones(n, bool)
        fail[rng.choice(n, keep, replace=False)] = False
    recs["score"][fail & (rng.random(n) < 0.5)] = 0.85           # score == min_score: rejected
    recs["ambiguity"][fail & (recs["score"] > 0.85)] = 0.95      # ambiguity == max_ambiguity: rejected
    return recs


def make_batch():
    keep = {12: 7, 13: 8, 14: 9}
    return [batch_records(n, f, keep.get(f)) for f, n in enumerate(SIZES)]


def expected_find_score(sel, seeds, recs, counts, offs, stride, loops, thresh, max_pts):
    F, num, fit = np.zeros((len(sel), 9), np.float32), np.zeros(len(sel), np.int32), np.zeros(len(sel), np.int32)
    after = recs.copy()
    for i, (f, s) in enumerate(zip(sel, seeds)):
        n = int(counts[f])
        sl = span(offs, stride, f, max(n, 0))
        F[i], num[i] = expected_find(recs[sl], n, s, loops, *GATES, thresh, max_pts)
        after[sl], fit[i] = expected_score(recs[sl], n, F[i], *GATES, thresh)
    return F, num, after, fit


def noisy_records(n, seed):
    """n records of a noisy planted scene with every byte outside the fields in play random; from 10 records on a fifth
    of them fails the gate."""
    from cudasift_amd import capi
    rng = np.random.default_rng(2000 + seed)
    recs = np.frombuffer(rng.bytes(576 * n), capi.POINT_DTYPE).copy()
    if n == 0:
        return recs
    scene, _, _ = planted_scene(seed, n=n, noise=NOISE)
    for k in ("xpos", "ypos", "match_xpos", "match_ypos", "score", "ambiguity", "match", "match_error"):
        recs[k] = scene[k]
    fail = (rng.random(n) < 0.2) & (n >= 10)
    recs["score"][fail & (rng.random(n) < 0.5)] = 0.85           # score == min_score: rejected
    recs["ambiguity"][fail & (recs["score"] > 0.85)] = 0.95      # ambiguity == max_ambiguity: rejected
    return recs


def start_F(recs, seed):
    """A start F: the best of 32 hypotheses; below 8 records (find gives zeros) the scene's ground truth."""
    if len(recs) >= 8:
        return expected_find(recs, len(recs), seed, 32, *GATES, 1.0, max_pts=len(recs))[0]
    Fgt = planted_scene(seed, n=8)[2]
    return (Fgt / np.abs(Fgt).max()).astype(np.float32).reshape(9)
