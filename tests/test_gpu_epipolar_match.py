"""misift_match_epipolar_batch: epipolar-guided matching of many frame pairs of device-resident batches.

Every row of set 1 is matched only against the set-2 records within `radius` of its epipolar line under the pair's F.
The expected records are restated from the contract (guided_cases.expected_epipolar): the gate in numpy float32
(epipolar_util.gate_np: every operation rounded, sums left to right), then the oracle's exact, full matcher on the row's candidates in ascending index
order.  All bytes of both sets are compared: only the five match fields of set-1 rows of some pair may change."""
import functools

import numpy as np
import pytest

from batch_util import MATCH_FIELDS, frames, guarded_context, layout, same_bytes, span
from epipolar_util import STEREO, STEREO_V, f32, planted_F, points_on_lines
from guided_cases import expected_epipolar as _expected
from synth import descriptors_to_points, synth_descriptors

pytestmark = pytest.mark.gpu

SIZES1 = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, 50, 77]   # frame 12: count -1; frame 13: in no pair
COUNTS1 = SIZES1[:12] + [-1, 77]
SIZES2 = [4100, 2000, 129, 128, 127, 64, 33, 32, 31, 20, 1, 0, 300]
PAIRS = [(i, (5 * i + 2) % 13) for i in range(13)]
# one set-2 frame in several pairs; frame 1 is also set 1 of a pair; frame 6 has count -1
KEYFRAME_PAIRS = [(0, 1), (2, 1), (5, 1), (7, 3), (10, 3), (11, 4), (13, 1), (1, 12), (6, 3)]
EXTENT = 500.0                                        # batch_util.frames puts positions into [0, 500)^2


def _fund(i):
    return planted_F(i, EXTENT, EXTENT)


def _plant(fr1, fr2, pairs, Fs, seed):
    """Put copies of half of each pair's set-1 records into set 2 at a random position along their epipolar line, within
    0.2 px across it (so radius 0.5 has candidates), and a duplicate (same position and descriptor) of every 7th copy, so
    ties for the best score occur."""
    rng = np.random.default_rng(seed)
    for (f1, f2), F in zip(pairs, Fs):
        a, b = fr1[f1], fr2[f2]
        k = min(len(a), len(b)) // 2
        if k == 0:
            continue
        x, y, _ = points_on_lines(F, a["xpos"][:k], a["ypos"][:k], rng, rng.uniform(-0.2, 0.2, k), EXTENT, EXTENT)
        dst = rng.permutation(len(b))[:k]
        b["xpos"][dst] = x.astype(f32)
        b["ypos"][dst] = y.astype(f32)
        b["data"][dst] = a["data"][:k]
        dup = dst[::7]
        dup = dup[dup + 1 < len(b)]
        for k2 in ("xpos", "ypos", "data"):
            b[k2][dup + 1] = b[k2][dup]


def _run(c, pairs, Fs, radius, recs1, counts1, offs1, stride1, recs2=None, counts2=None, offs2=None, stride2=0,
         max_pts=8192):
    """One misift_match_epipolar_batch; returns (set 1 after, set 2 after or None, num_found)."""
    from cudasift_amd import capi
    d1, c1 = c.upload(recs1), c.upload(np.asarray(counts1, np.int32))
    o1 = c.upload(offs1) if offs1 is not None else None
    dF = c.upload(np.ascontiguousarray(Fs, np.float32).reshape(-1))
    nf = c.upload(np.full(len(pairs), 0x5EED, np.int32))
    if recs2 is None:
        c.match_epipolar_batch(pairs, d1, len(counts1), c1, dF, radius, o1, stride1, max_pts=max_pts, num_found=nf)
        c.sync()
        return c.download(d1, (len(recs1),), capi.POINT_DTYPE), None, c.download(nf, (len(pairs),), np.int32)
    d2, c2 = c.upload(recs2), c.upload(np.asarray(counts2, np.int32))
    o2 = c.upload(offs2) if offs2 is not None else None
    c.match_epipolar_batch(pairs, d1, len(counts1), c1, dF, radius, o1, stride1, d2, len(counts2), c2, o2, stride2,
                           max_pts=max_pts, num_found=nf)
    c.sync()
    return (c.download(d1, (len(recs1),), capi.POINT_DTYPE), c.download(d2, (len(recs2),), capi.POINT_DTYPE),
            c.download(nf, (len(pairs),), np.int32))


def _parity_case(seed):
    f1 = frames(SIZES1, seed, False)
    f2 = frames(SIZES2, seed + 1, False)
    Fs = [_fund(i) for i in range(len(PAIRS))]
    _plant(f1, f2, PAIRS, Fs, seed + 2)
    return f1, f2, Fs


@functools.lru_cache(maxsize=None)
def _parity_expected(radius):
    """The parity case and its expected set-1 frames and num_found, computed once per radius on the packed layout; the
    layouts of the tests only place the same frames differently (frame 12, count -1, stays as it was)."""
    f1, f2, Fs = _parity_case(3)
    r1, o1, _ = layout(f1, COUNTS1, False, min_stride=0, pad_error=0.0)
    r2, o2, _ = layout(f2, SIZES2, False, min_stride=0, pad_error=0.0)
    exp, enf = _expected(PAIRS, Fs, radius, 8192, r1, COUNTS1, o1, 0, r2, SIZES2, o2, 0)
    ef = [exp[span(o1, 0, f, n)] if c >= 0 else f1[f] for f, (n, c) in enumerate(zip(SIZES1, COUNTS1))]
    return f1, f2, Fs, ef, enf


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("radius", [0.5, 3.0, 64.0])
def test_parity_with_oracle(ctx, radius, padded):
    f1, f2, Fs, ef, enf = _parity_expected(radius)
    r1, o1, s1 = layout(f1, COUNTS1, padded, min_stride=0, pad_error=0.0)
    r2, o2, s2 = layout(f2, SIZES2, padded, min_stride=0, pad_error=0.0)
    exp, _, _ = layout(ef, COUNTS1, padded, min_stride=0, pad_error=0.0)
    got1, got2, nf = _run(ctx, PAIRS, Fs, radius, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    same_bytes(got1, exp, "set 1")
    same_bytes(got2, r2, "set 2 (read only)")
    assert np.array_equal(nf, enf), (nf, enf)
    assert enf.sum() > 100, enf
    # ties for the best score were planted: the smallest index wins, and the runner-up is the same score
    sl = span(o1, s1, 10, 2000)
    tie = got1["ambiguity"][sl] == got1["score"][sl] / (got1["score"][sl] + np.float32(1e-6))
    assert (tie & (got1["match"][sl] >= 0)).sum() > 10


def test_keyframe_pairs_and_shared_buffer(ctx):
    """A set-2 frame in several pairs, and d_recs1 == d_recs2 (frames of one packed batch against each other)."""
    sizes = [300, 2000, 129, 1, 33, 64, 0, 128, 127, 31, 500, 77, 4100, 20]
    counts = sizes[:6] + [-1] + sizes[7:]
    fr = frames(sizes, 11, False)
    Fs = [_fund(i) for i in range(len(KEYFRAME_PAIRS))]
    _plant(fr, fr, KEYFRAME_PAIRS, Fs, 12)
    recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    exp, enf = _expected(KEYFRAME_PAIRS, Fs, 4.0, 8192, recs, counts, offs, 0, recs, counts, offs, 0)
    got, _, nf = _run(ctx, KEYFRAME_PAIRS, Fs, 4.0, recs, counts, offs, 0)
    # set 2 is the input batch itself: the oracle read the positions and descriptors of `recs`, which the call never
    # writes, so every byte of the shared buffer must equal the restated set 1
    same_bytes(got, exp, "shared batch")
    assert np.array_equal(nf, enf), (nf, enf)
    assert enf.max() > 50, enf


@pytest.mark.parametrize("name,F", [("horizontal", STEREO), ("vertical", STEREO_V)])
def test_rectified_stereo(ctx, name, F):
    """Exactly axis-parallel lines (a0 == 0 or a1 == 0): y2 = y1, and x2 = x1."""
    sizes1, sizes2 = [700, 129, 64], [2000, 4100, 33]
    f1 = frames(sizes1, 81, False)
    f2 = frames(sizes2, 82, False)
    rng = np.random.default_rng(83)
    for a, b in zip(f1, f2):                           # partners on the line, at a disparity along it
        k = min(len(a), len(b)) // 2
        dst = rng.permutation(len(b))[:k]
        along, across = rng.uniform(0, EXTENT, k).astype(f32), a["ypos" if name == "horizontal" else "xpos"][:k]
        b["xpos"][dst], b["ypos"][dst] = (along, across) if name == "horizontal" else (across, along)
        b["data"][dst] = a["data"][:k]
    r1, o1, _ = layout(f1, sizes1, False, min_stride=0, pad_error=0.0)
    r2, o2, _ = layout(f2, sizes2, False, min_stride=0, pad_error=0.0)
    pairs = [(0, 0), (1, 1), (2, 2)]
    for radius in (0.5, 3.0):
        exp, enf = _expected(pairs, [F] * 3, radius, 8192, r1, sizes1, o1, 0, r2, sizes2, o2, 0)
        got1, got2, nf = _run(ctx, pairs, [F] * 3, radius, r1, sizes1, o1, 0, r2, sizes2, o2, 0)
        same_bytes(got1, exp, "set 1, %s, radius %g" % (name, radius))
        same_bytes(got2, r2, "set 2")
        assert np.array_equal(nf, enf) and enf[0] >= 350, (nf, enf)


@pytest.mark.parametrize("n1,n2", [(2000, 4100), (33, 129)])
def test_unbounded_radius_equals_exact_full_match(ctx, n1, n2):
    """radius = +inf and a finite non-zero F: every record is a candidate, so the call equals misift_match in exact, full
    mode."""
    f1 = frames([n1], 21, False)
    f2 = frames([n2], 22, False)
    got, _, nf = _run(ctx, [(0, 0)], [_fund(4)], float("inf"), f1[0], [n1], None, n1, f2[0], [n2], None, n2)
    ctx.set_options(match_full=1, match_exact_top2=1)
    try:
        exp = ctx.match(f1[0].copy(), n1, f2[0].copy(), n2)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    same_bytes(got, exp, "set 1")
    assert nf[0] == (exp["match"] >= 0).sum() == n1


def test_epipolar_match_rejects_decoys(ctx):
    """Each row's true partner sits on its epipolar line with a perturbed descriptor; an exact copy of the row's
    descriptor (a higher score) sits 3 radii off the line.  misift_match_batch takes the decoy; the epipolar call takes
    the partner for every row."""
    from cudasift_amd import capi
    n, radius = 1024, 2.0
    rng = np.random.default_rng(31)
    F = planted_F(2)
    d1 = synth_descriptors(n, 41, l2=True)
    noisy = d1 + rng.normal(0.0, 0.02, d1.shape).astype(np.float32)
    partner = (noisy / np.linalg.norm(noisy, axis=1, keepdims=True)).astype(np.float32)
    s1 = descriptors_to_points(d1, capi.POINT_DTYPE)
    s1["xpos"] = rng.uniform(100, 1800, n).astype(np.float32)
    s1["ypos"] = rng.uniform(100, 1000, n).astype(np.float32)
    px, py, _ = points_on_lines(F, s1["xpos"], s1["ypos"], rng, rng.uniform(-0.5, 0.5, n))
    qx, qy, _ = points_on_lines(F, s1["xpos"], s1["ypos"], rng, 3 * radius * rng.choice([-1.0, 1.0], n))
    s2 = descriptors_to_points(np.concatenate([partner, d1]), capi.POINT_DTYPE)   # partners 0..n-1, decoys n..2n-1
    s2["xpos"] = np.concatenate([px, qx]).astype(np.float32)
    s2["ypos"] = np.concatenate([py, qy]).astype(np.float32)
    c1 = ctx.upload(np.array([n], np.int32))
    c2 = ctx.upload(np.array([2 * n], np.int32))
    d2 = ctx.upload(s2)
    dg = ctx.upload(s1)
    db = ctx.upload(s1)
    dF = ctx.upload(F.reshape(-1))
    nf = ctx.match_epipolar_batch([(0, 0)], dg, 1, c1, dF, radius, None, n, d2, 1, c2, None, 2 * n)
    ctx.match_batch([(0, 0)], db, 1, c1, None, n, d2, 1, c2, None, 2 * n)
    ctx.sync()
    guided = ctx.download(dg, (n,), capi.POINT_DTYPE)
    glob = ctx.download(db, (n,), capi.POINT_DTYPE)
    assert np.array_equal(glob["match"], np.arange(n) + n)
    assert np.array_equal(guided["match"], np.arange(n))
    assert ctx.download(nf, (1,), np.int32)[0] == n
    exp, enf = _expected([(0, 0)], [F], radius, 8192, s1, [n], None, n, s2, [2 * n], None, 2 * n)
    same_bytes(guided, exp, "epipolar rows")
    assert enf[0] == n


def test_chain_behind_real_extraction(ctx, stereo):
    """extract packed -> match_batch -> find_fundamental_batch -> match_epipolar_batch with find's F ->
    score_fundamental_batch, with no host read in between, on a crop of the stereo pair, both ways round."""
    from cudasift_amd import capi
    B, h, w, mp, radius = 2, 480, 640, 4096, 2.0
    fr = np.stack([im[200:200 + h, 300:300 + w] for im in stereo]).astype(np.float32)
    d = ctx.upload(np.ascontiguousarray(fr))
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    pairs = [(0, 1), (1, 0)]
    sel = [0, 1]
    gates = dict(min_score=0.85, max_ambiguity=0.95)
    ctx.match_batch(pairs, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0)
    dF, dn = ctx.find_fundamental_batch(sel, [7, 8], packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp, num_loops=512,
                                        thresh=1.0, **gates)
    dnf = ctx.match_epipolar_batch(pairs, packed, B, cnt.ptr, dF, radius, cnt.ptr + 4 * B, 0, max_pts=mp)
    dfit = ctx.score_fundamental_batch(sel, packed, B, cnt.ptr, dF, cnt.ptr + 4 * B, 0, thresh=1.0, **gates)
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    counts, offs = ci[:B], ci[B:]
    got = ctx.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    F = ctx.download(dF, (B, 9), np.float32)
    ninl = ctx.download(dn, (B,), np.int32)
    nf = ctx.download(dnf, (B,), np.int32)
    fit = ctx.download(dfit, (B,), np.int32)
    assert (counts > 100).all() and (counts <= mp).all(), counts
    assert (ninl > 20).all(), ninl
    exp, enf = _expected(pairs, list(F), radius, mp, got, counts, offs, 0, got, counts, offs, 0)
    for i, (f1, _) in enumerate(pairs):
        s1 = span(offs, 0, f1, int(counts[f1]))
        for k in MATCH_FIELDS:
            assert np.array_equal(exp[s1][k].view(np.uint32), got[s1][k].view(np.uint32)), (f1, k)
        assert F[i].any()
        # the Sampson distance never exceeds the distance to the line in image 2, which the gate bounds by the radius
        m = got[s1]["match"] >= 0
        assert (got[s1]["match_error"][m] < radius * (1 + 1e-3)).all(), f1
    assert np.array_equal(nf, enf), (nf, enf)
    assert (nf > 50).all() and (fit > 10).all(), (nf, fit)


def test_edge_cases(ctx):
    """NaN F, zero F, F with 1e20 entries, a line that misses the frame: no candidate, no fault.  A radius whose square
    underflows with records exactly on the line: 0 < 0 is false.  max_pts overflow on either side: -1, set 1 untouched.
    Two runs: the same bytes."""
    sizes1, sizes2 = [150, 60, 90, 80, 70, 40, 45], [50, 150, 90, 80, 70, 40, 45]
    f1 = frames(sizes1, 51, False)
    f2 = frames(sizes2, 52, False)
    r1, o1, _ = layout(f1, sizes1, False, min_stride=0, pad_error=0.0)
    miss = np.array([[0, 0, 1], [0, 0, 0], [0, 0, -5000]], f32)    # every row's line is x2 = 5000
    pairs = [(i, i) for i in range(7)]
    Fs = [_fund(0), _fund(1), np.full((3, 3), np.nan, f32), np.zeros((3, 3), f32), STEREO, np.full((3, 3), 1e20, f32),
          miss]
    f2[4]["ypos"] = f1[4]["ypos"][:70]                 # exactly on the line y2 = y1: e = 0, still not < fl(1e-30^2) * n2 = 0
    r2, o2, _ = layout(f2, sizes2, False, min_stride=0, pad_error=0.0)
    for radius in (1e-30, 50.0):
        got1, got2, nf = _run(ctx, pairs, Fs, radius, r1, sizes1, o1, 0, r2, sizes2, o2, 0, max_pts=100)
        again1, _, nf2 = _run(ctx, pairs, Fs, radius, r1, sizes1, o1, 0, r2, sizes2, o2, 0, max_pts=100)
        same_bytes(got1, again1, "two runs")
        assert np.array_equal(nf, nf2)
        exp, enf = _expected(pairs, Fs, radius, 100, r1, sizes1, o1, 0, r2, sizes2, o2, 0)
        same_bytes(got1, exp, "set 1, radius %g" % radius)
        same_bytes(got2, r2, "set 2")
        assert np.array_equal(nf, enf), (nf, enf)
        assert nf[0] == -1 and nf[1] == -1 and (nf[[2, 3, 5, 6]] == 0).all(), nf
        for f in (0, 1):                               # over max_pts: untouched
            sl = span(o1, 0, f, sizes1[f])
            same_bytes(got1[sl], r1[sl], "frame %d over max_pts" % f)
        for f in (2, 3, 5, 6):                         # NaN, zero, overflowing F, a line off the frame: nothing matched
            sl = span(o1, 0, f, sizes1[f])
            assert (got1["match"][sl] == -1).all() and (got1["score"][sl] == 0).all()
            assert (got1["ambiguity"][sl] == 0).all() and (got1["match_xpos"][sl] == 0).all()
            assert (got1["match_ypos"][sl] == 0).all()
        sl = span(o1, 0, 4, 70)
        if radius < 1:
            assert nf[4] == 0 and (got1["match"][sl] == -1).all()
        else:
            assert nf[4] == 70


def test_argument_errors(ctx):
    """Every MISIFT_EINVAL case returns before anything is enqueued: the poisoned outputs stay as they were."""
    from cudasift_amd import capi
    L = capi.lib()
    fr = frames([32, 32], 61, False)
    recs_h = np.concatenate(fr)
    recs = ctx.upload(recs_h)
    counts = ctx.upload(np.array([32, 32], np.int32))
    dF = ctx.upload(np.tile(STEREO.reshape(-1), 2))
    poison = np.full(4, 0x5EED, np.int32)
    nf = ctx.upload(poison)

    def call(pairs, npairs=None, r=None, c=None, m=None, radius=10.0, max_pts=64, stride=32, nframes=2, c_ctx=None):
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        r = recs.ptr if r is None else r
        c = counts.ptr if c is None else c
        m = dF.ptr if m is None else m
        return L.misift_match_epipolar_batch(ctx.h if c_ctx is None else c_ctx, len(p) if npairs is None else npairs,
                                             p.ctypes.data, r, nframes, c, None, stride, r, nframes, c, None, stride, m,
                                             radius, max_pts, nf.ptr)
    assert call([(0, 1), (0, 0)]) == -1                 # set-1 frame 0 twice
    assert call([(0, 2)]) == -1                         # set-2 index out of range
    assert call([(-1, 0)]) == -1                        # set-1 index out of range
    assert call([(0, 1)], npairs=-1) == -1
    assert call([(0, 1)], r=0) == -1                    # NULL records
    assert call([(0, 1)], c=0) == -1                    # NULL counts
    assert call([(0, 1)], m=0) == -1                    # NULL fundamental matrices
    assert call([(0, 1)], radius=float("nan")) == -1
    assert call([(0, 1)], radius=0.0) == -1
    assert call([(0, 1)], radius=-1.0) == -1
    assert call([(0, 1)], max_pts=0) == -1
    assert call([(0, 1)], stride=-1) == -1              # no offsets and a negative stride
    assert call([(0, 1)], nframes=0) == -1
    assert call(np.zeros((0, 2)), npairs=0) == 0        # no-op
    ctx.sync()
    assert ctx.download(recs, (64,), capi.POINT_DTYPE).tobytes() == recs_h.tobytes()
    assert np.array_equal(ctx.download(nf, (4,), np.int32), poison)
    assert call([(1, 1), (0, 1)]) == 0                  # a set-2 frame in two pairs is fine
    ctx.sync()
    assert (ctx.download(nf, (2,), np.int32) >= 0).all()


def test_guard_mode(ctx):
    """A fresh guarded context (temp and plan buffers start NaN-poisoned, 64 KiB guard bands): no band damaged, the same
    bytes as the unguarded context."""
    from cudasift_amd import capi
    f1, f2, Fs = _parity_case(71)
    r1, o1, s1 = layout(f1, COUNTS1, False, min_stride=0, pad_error=0.0)
    r2, o2, s2 = layout(f2, SIZES2, False, min_stride=0, pad_error=0.0)
    with guarded_context(3) as g:
        got = _run(g, PAIRS, Fs, 3.0, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
        inf = _run(g, [(10, 1)], [_fund(1)], float("inf"), r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    assert capi.check_guards() >= 0
    again = _run(ctx, PAIRS, Fs, 3.0, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    same_bytes(got[0], again[0], "guarded vs unguarded")
    assert np.array_equal(got[2], again[2])
    again = _run(ctx, [(10, 1)], [_fund(1)], float("inf"), r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    same_bytes(inf[0], again[0], "guarded vs unguarded, radius inf")
