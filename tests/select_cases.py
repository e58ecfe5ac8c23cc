"""misift_select_pairs_batch (preemptive matching): the numpy restatement of its three stages and the cases its tests
share (test_select_cpu.py holds the host hook to the restatement, test_gpu_select.py the device).  A plain module: no
tests, no fixtures; cudasift_amd.capi is imported inside functions only.

A case is a dict: recs (POINT_DTYPE records as uploaded), q (their int8 descriptors), counts, offs (or None), stride,
and the arguments top, min_score, max_ambiguity, min_votes, k, max_pairs.  expected(case) gives the six outputs at their
stated sizes (at least one word each), every entry the call does not write holding POISON_WORD."""
import functools

import numpy as np

from batch_util import POISON_WORD, layout, match_np, quantize_np, span

f32 = np.float32
OUTPUTS = ("sel", "sel_counts", "votes", "pairs", "pair_votes", "summary")
MAX_TOP, MAX_FRAMES = 256, 4096
ARGS = ("top", "min_score", "max_ambiguity", "min_votes", "k", "max_pairs")


# ---- the restatement

def keys_np(scale):
    """Stage 1: the bit pattern of scale where scale > 0 (a NaN compares false), else 0."""
    scale = np.ascontiguousarray(scale, f32)
    with np.errstate(invalid="ignore"):
        return np.where(scale > 0, scale.view(np.uint32), 0).astype(np.int64)


def chosen_np(scale, top):
    """The frame-local indices of the min(n, top) largest keys: key descending, then index ascending."""
    k = keys_np(scale)
    return np.lexsort((np.arange(len(k)), -k))[:top].astype(np.int32)


def votes_np(pa, qa, pb, qb, min_score, max_ambiguity):
    """Stage 2 for one pair: the rows of misift_match_pairs_batch_i8(mutual = 1) on the two gathered subsets that pass
    the gate of misift_link_tracks_batch with max_error = +inf."""
    if len(pa) == 0 or len(pb) == 0:
        return 0
    fw = match_np(pa, qa, pb, qb)
    rv = match_np(pb, qb, pa, qa)["match"]
    m = fw["match"]
    mutual = (m >= 0) & (rv[np.clip(m, 0, len(pb) - 1)] == np.arange(len(pa)))
    with np.errstate(invalid="ignore"):
        gate = (fw["score"] > f32(min_score)) & (fw["ambiguity"] < f32(max_ambiguity))
    return int((mutual & gate).sum())


def neighbours_np(V, f, min_votes, k):
    g = np.arange(len(V))
    ok = (g != f) & (V[f] >= min_votes)
    order = np.lexsort((g, -V[f].astype(np.int64)))
    return order[ok[order]][:k]


def frame_records(case, f):
    n = max(int(case["counts"][f]), 0)
    sl = span(case["offs"], case["stride"], f, n)
    return case["recs"][sl], case["q"][sl]


def stage12(case):
    """(sel, sel_counts, V) of the case, computed once per (records, top, gate) and shared by its variants."""
    memo = case["memo"]
    key = (case["top"], float(f32(case["min_score"])), float(f32(case["max_ambiguity"])))
    if key not in memo:
        n, top = len(case["counts"]), case["top"]
        sel = np.full((n, top), -1, np.int32)
        cnt = np.zeros(n, np.int32)
        sub = []
        for f in range(n):
            p, q = frame_records(case, f)
            c = chosen_np(p["scale"], top)
            sel[f, :len(c)], cnt[f] = c, len(c)
            sub.append((p[c], q[c]))
        V = np.zeros((n, n), np.int32)
        for a in range(n):
            for b in range(a + 1, n):
                V[a, b] = V[b, a] = votes_np(*sub[a], *sub[b], case["min_score"], case["max_ambiguity"])
        memo[key] = (sel, cnt, V)
    return memo[key]


def selected_np(V, min_votes, k):
    n = len(V)
    keep = np.zeros((n, n), bool)
    lonely = np.zeros(n, bool)
    for f in range(n):
        nb = neighbours_np(V, f, min_votes, k)
        keep[f, nb] = True
        lonely[f] = len(nb) == 0
    keep |= keep.T
    a, b = np.nonzero(np.triu(keep, 1))                         # row-major: ascending (a, b)
    return np.stack([a, b], 1).astype(np.int32), lonely


def expected(case, poison=POISON_WORD):
    """The six outputs, name -> int32 array of the stated size."""
    n, top, mp = len(case["counts"]), case["top"], case["max_pairs"]
    sel, cnt, V = stage12(case)
    pairs, lonely = selected_np(V, case["min_votes"], case["k"])
    P = len(pairs)
    w = min(P, mp)
    blank = lambda words: np.full(max(words, 1), poison, np.uint32).view(np.int32)      # noqa: E731
    out = {k: blank(s) for k, s in zip(OUTPUTS, (n * top, n, n * n, 2 * mp, mp, 8))}
    out["sel"][:n * top] = sel.reshape(-1)
    out["sel_counts"][:n] = cnt
    out["votes"][:n * n] = V.reshape(-1)
    out["pairs"][:2 * w] = pairs[:w].reshape(-1)
    out["pair_votes"][:w] = V[pairs[:w, 0], pairs[:w, 1]]
    counts = np.asarray(case["counts"])
    out["summary"][:] = [P, w, int((lonely & (counts > 0)).sum()), int((counts > top).sum()),
                         int(V.max()) if n else 0, 0, 0, 0]
    return out


def brute(case):
    """Stages 1 to 3 by plain Python loops over lists, for tiny cases: (sel rows, V, pairs)."""
    n, top = len(case["counts"]), case["top"]
    chosen = []
    for f in range(n):
        p, q = frame_records(case, f)
        key = []
        for s in p["scale"].tolist():
            key.append(int(f32(s).view(np.uint32)) if s > 0 else 0)
        idx = sorted(range(len(key)), key=lambda r: (-key[r], r))[:top]
        chosen.append((idx, [[int(x) for x in q[r]] for r in idx]))
    V = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            qa, qb = chosen[a][1], chosen[b][1]
            S = [[sum(x * y for x, y in zip(ra, rb)) for rb in qb] for ra in qa]
            v = 0
            for i, row in enumerate(S):
                best, m = 0, -1
                for j, s in enumerate(row):
                    if s > best:
                        best, m = s, j
                if m < 0:
                    continue
                second = max([0] + [s for j, s in enumerate(row) if j != m])
                cbest, crow = 0, -1
                for r in range(len(S)):
                    if S[r][m] > cbest:
                        cbest, crow = S[r][m], r
                score = f32(best) * f32(2.0 ** -16)
                amb = (f32(second) * f32(2.0 ** -16)) / (score + f32(1e-6))
                if crow == i and score > f32(case["min_score"]) and amb < f32(case["max_ambiguity"]):
                    v += 1
            V[a][b] = V[b][a] = v
    nb = []
    for f in range(n):
        cand = [g for g in range(n) if g != f and V[f][g] >= case["min_votes"]]
        nb.append(set(sorted(cand, key=lambda g: (-V[f][g], g))[:case["k"]]))
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if b in nb[a] or a in nb[b]]
    return [c[0] for c in chosen], V, pairs


# ---- scenes

def unit_descriptors(rng, n):
    """SIFT-like: non-negative, unit length, no entry above 0.2 before the last normalisation."""
    d = rng.gamma(0.5, 1.0, (n, 128)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True) + f32(1e-12)
    d = np.minimum(d, f32(0.2))
    return d / (np.linalg.norm(d, axis=1, keepdims=True) + f32(1e-12))


def view(rng, desc, scale, factor, noise):
    """A frame's view of scene points: descriptors with noise, renormalised; scales times the frame's factor."""
    d = np.maximum(desc + rng.normal(0, noise, desc.shape).astype(f32), 0)
    d /= np.linalg.norm(d, axis=1, keepdims=True) + f32(1e-12)
    return d.astype(f32), (scale * f32(factor)).astype(f32)


def records(desc, scale, rng):
    """POINT_DTYPE records: the descriptors and scales given, random positions, the other fields random so that a
    field read by mistake shows."""
    from cudasift_amd import capi
    n = len(desc)
    p = np.zeros(n, capi.POINT_DTYPE)
    for k in ("xpos", "ypos", "sharpness", "edgeness", "orientation", "score", "ambiguity", "match_error"):
        p[k] = rng.random(n, dtype=f32) * 500
    p["match"] = rng.integers(-5, 5000, n)
    p["data"], p["scale"] = desc, scale
    return p


def make_case(frames, counts, padded, **args):
    """frames: the records of every frame (a frame of count -1 keeps records the call must not look at in a padded
    layout, and none in a packed one)."""
    from cudasift_amd import capi
    if len(frames):
        recs, offs, stride = layout(frames, counts, padded, min_stride=1, pad_error=-7.0)
    else:
        recs, offs, stride = np.zeros(0, capi.POINT_DTYPE), None if padded else np.zeros(1, np.int32), int(padded)
    if len(recs) == 0:
        recs = np.zeros(1, capi.POINT_DTYPE)                     # a batch without records still has a buffer
    case = dict(recs=recs, q=quantize_np(recs["data"]).reshape(len(recs), 128), counts=np.asarray(counts, np.int32),
                offs=None if offs is None else offs[:len(counts)].astype(np.int32), stride=stride, memo={})
    case.update(dict(min_score=0.85, max_ambiguity=0.95, min_votes=2, k=2, max_pairs=len(counts) * len(counts)))
    case.update(args)
    assert set(ARGS) <= set(case)
    return case


def variant(case, **args):
    """The case under other arguments: the records, and with them the memo of stages 1 and 2, are shared."""
    return dict(case, **args)


def pool_scene(sizes, seed, pool, noise=0.01):
    """Every frame views `size` points of one pool of scene points (so any two frames share some), scales planted per
    point times a per-frame factor."""
    rng = np.random.default_rng(seed)
    desc = unit_descriptors(rng, pool)
    scale = np.exp(rng.normal(1.0, 0.8, pool)).astype(f32)
    out = []
    for n in sizes:
        idx = rng.permutation(pool)[:n] if n <= pool else rng.integers(0, pool, n)
        d, s = view(rng, desc[idx], scale[idx], rng.uniform(0.8, 1.25), noise)
        out.append(records(d, s, rng))
    return out


def size_counts(top):
    """The frame counts the issue names: -1, 0, 1, top - 1, top, top + 1, 3 top."""
    return [-1, 0, 1, max(top - 1, 0), top, top + 1, 3 * top]


@functools.lru_cache(maxsize=None)
def size_case(top, padded):
    counts = size_counts(top)
    sizes = [5 if c < 0 else c for c in counts]                  # the frame of count -1 has records behind it when padded
    fr = pool_scene(sizes, 1000 + top, 3 * top + 7)
    return make_case(fr, counts, padded, top=top, min_votes=1, k=2)


@functools.lru_cache(maxsize=None)
def frames_case(nframes, top=8, padded=False, seed=7):
    """nframes frames of 5 to 30 records over a pool of 40 points."""
    rng = np.random.default_rng(seed + nframes)
    sizes = rng.integers(5, 31, nframes).tolist()
    fr = pool_scene(sizes, seed * 31 + nframes, 40)
    return make_case(fr, sizes, padded, top=top, min_votes=2, k=3)


SPECIAL_SCALES = [0.0, -0.0, -3.5, float("nan"), float("inf"), float("-inf"), 1e-42, 1.4e-45, 2.5, 2.5, 2.5]


@functools.lru_cache(maxsize=None)
def scale_case(kind):
    """`equal`: every scale of a frame the same, so the lowest indices are chosen.  `special`: zero, negative, NaN,
    +inf, -inf and subnormal scales among a few ordinary ones, fewer positive keys than top in one frame."""
    rng = np.random.default_rng(50 if kind == "equal" else 51)
    fr = pool_scene([40, 33, 12, 40], 52, 60)
    for i, p in enumerate(fr):
        if kind == "equal":
            p["scale"] = f32(1.5 + i)
        else:
            s = np.array(SPECIAL_SCALES * 4, f32)[:len(p)]
            p["scale"] = s[rng.permutation(len(s))]
    return make_case(fr, [40, 33, 12, 40], kind == "equal", top=24, min_votes=1, k=3)


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """Descriptors repeated inside a frame tie S along a row (in the other frame's view) and down a column; all-zero
    descriptors never match.  max_ambiguity 2 lets the tied rows through the gate, so the tie rules decide the votes."""
    rng = np.random.default_rng(60)
    fr = pool_scene([24, 24, 24], 61, 24, noise=0.0)             # every frame sees every point, exactly
    for p in fr:
        p["scale"] = np.linspace(9, 1, len(p)).astype(f32)       # chosen in index order
        src = rng.permutation(12)[:5]
        p["data"][src + 12] = p["data"][src]                     # five records twice
        p["data"][rng.integers(0, 24, 3)] = 0                    # and some without a descriptor
    return make_case(fr, [24, 24, 24], False, top=24, min_votes=1, k=2, max_ambiguity=2.0)


def _gate_frames():
    """Frame 0: one record; frame 1: two records, the first the better match of frame 0's."""
    rng = np.random.default_rng(70)
    d = unit_descriptors(rng, 3)
    d[1] = view(rng, d[0:1], np.ones(1, f32), 1.0, 0.02)[0][0]
    scale = np.ones(1, f32)
    return [records(d[0:1], scale, rng), records(d[1:3], np.array([2, 1], f32), rng)]


@functools.lru_cache(maxsize=None)
def gate_cases():
    """{name: case} on two frames whose one candidate row has score sc and ambiguity am: min_score exactly sc (no vote)
    and one ulp below (a vote); max_ambiguity exactly am (no vote) and one ulp above (a vote)."""
    base = make_case(_gate_frames(), [1, 2], False, top=2, min_votes=1, k=1, min_score=0.0, max_ambiguity=10.0)
    p0, q0 = frame_records(base, 0)
    p1, q1 = frame_records(base, 1)
    row = match_np(p0, q0, p1, q1)
    sc, am = f32(row["score"][0]), f32(row["ambiguity"][0])
    assert row["match"][0] == 0 and 0 < am < 1 and sc > 0.5
    return dict(score_at=variant(base, min_score=float(sc), memo={}),
                score_below=variant(base, min_score=float(np.nextafter(sc, f32(0))), memo={}),
                ambiguity_at=variant(base, max_ambiguity=float(am), memo={}),
                ambiguity_above=variant(base, max_ambiguity=float(np.nextafter(am, f32(2))), memo={}))


@functools.lru_cache(maxsize=None)
def vote_case():
    """Nine frames, two of them (3 and 6) byte-identical copies of frame 1: V[f][3] == V[f][6] == V[f][1] for every
    other f, so neighbours tie in V and the smaller frame wins."""
    fr = pool_scene([60, 50, 70, 50, 45, 64, 50, 30, 55], 80, 90)
    fr[3], fr[6] = fr[1].copy(), fr[1].copy()
    return make_case(fr, [len(p) for p in fr], True, top=32, min_votes=1, k=2)


def vote_variants():
    """{name: case}: min_votes = a V that occurs while V - 1 occurs too (pairs exactly at min_votes and one below), and
    one more (the pairs that were at it now fall one below); k = 1, 2 and nframes; max_pairs = 0, P - 1, P, P + 1."""
    base = vote_case()
    V = stage12(base)[2]
    vals = np.unique(V[np.triu_indices(len(V), 1)])
    both = [int(v) for v in vals if v >= 2 and v - 1 in vals]   # some pair has exactly this count, another one less
    at = both[len(both) // 2]
    out = dict(min_votes_at=variant(base, min_votes=at, k=9), min_votes_above=variant(base, min_votes=at + 1, k=9),
               k1=variant(base, k=1), k2=variant(base, k=2), k_all=variant(base, k=9))
    P = len(selected_np(V, base["min_votes"], 2)[0])
    assert P >= 2
    for name, mp in (("none", 0), ("short", P - 1), ("exact", P), ("room", P + 1)):
        out["max_pairs_" + name] = variant(base, k=2, max_pairs=mp)
    return out


@functools.lru_cache(maxsize=None)
def strip_case():
    """100 frames: 4950 pairs, more than the 4096 strips of one frame the vote kernel plans on 256 CUs, so a workgroup
    walks two frames b and reuses its staging buffer."""
    return frames_case(100, top=16, seed=9)


@functools.lru_cache(maxsize=None)
def long_frame_case():
    """A frame of 9000 records, more than the 8192 keys the selection keeps on chip: coarse scales, so that the keys tie
    in their thousands, the largest of them planted behind index 8192, and the tie at the threshold decided by index."""
    fr = pool_scene([9000, 300, 20], 85, 200)
    for p in fr:
        p["scale"] = np.round(p["scale"]) + f32(1)
    fr[0]["scale"][8500:8530] = 100
    fr[0]["scale"][8200:8210] = 50
    return make_case(fr, [9000, 300, 20], False, top=64, min_votes=1, k=2)


# ---- the planted ring (the quality condition, and the chain)

def ring_scene(nframes, window, step, clutter, seed, noise=0.01):
    """nframes frames on a ring over nframes * step scene points: frame f sees the `window` points from f * step on
    (wrapping), plus `clutter` records nobody else sees.  Scales are planted per point times a per-frame factor.
    Returns (frames, seen): seen[f] = the set of scene points of frame f."""
    rng = np.random.default_rng(seed)
    npts = nframes * step
    desc = unit_descriptors(rng, npts)
    scale = np.exp(rng.normal(1.0, 0.8, npts)).astype(f32)
    fr, seen = [], []
    for f in range(nframes):
        idx = (f * step + np.arange(window)) % npts
        d, s = view(rng, desc[idx], scale[idx], rng.uniform(0.8, 1.25), noise)
        cd = unit_descriptors(rng, clutter)
        cs = np.exp(rng.normal(1.0, 0.8, clutter)).astype(f32)
        order = rng.permutation(window + clutter)
        fr.append(records(np.concatenate([d, cd])[order], np.concatenate([s, cs])[order], rng))
        seen.append(set(idx.tolist()))
    return fr, seen


@functools.lru_cache(maxsize=None)
def ring_case():
    """24 frames; a window of 100 points every 40, so neighbours share 60 points, second neighbours 20 and nobody else
    any; 100 records of clutter per frame; top 64, k 4."""
    fr, seen = ring_scene(24, 100, 40, 100, 90)
    case = make_case(fr, [len(p) for p in fr], False, top=64, min_votes=4, k=4)
    return case, seen


@functools.lru_cache(maxsize=None)
def small_ring_case():
    """The chain's scene: 8 frames, a window of 30 points every 12, 10 records of clutter."""
    fr, seen = ring_scene(8, 30, 12, 10, 91)
    case = make_case(fr, [len(p) for p in fr], False, top=24, min_votes=3, k=2)
    return case, seen


def all_cases():
    """{name: case}: everything the byte-for-byte tests run."""
    out = {}
    for i, top in enumerate((1, 31, 32, 33, 64, 65, 255, 256)):
        out["sizes_top%d" % top] = size_case(top, bool(i % 2))
    out["sizes_top32_padded"] = size_case(32, True)
    out["sizes_top33_packed"] = size_case(33, False)
    for n in (0, 1, 2, 3, 65):
        out["frames_%d" % n] = frames_case(n, padded=n == 3)
    out["frames_65_top33"] = frames_case(65, top=33, padded=True)
    out["strips_100"] = strip_case()
    out["long_frame"] = long_frame_case()
    out["scale_equal"], out["scale_special"] = scale_case("equal"), scale_case("special")
    out["duplicates"] = duplicate_case()
    out.update({"gate_" + k: v for k, v in gate_cases().items()})
    out["votes"] = vote_case()
    out.update({"votes_" + k: v for k, v in vote_variants().items()})
    out["ring_small"] = small_ring_case()[0]
    return out
