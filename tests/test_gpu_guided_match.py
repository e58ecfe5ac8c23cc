"""misift_match_guided_batch: homography-guided matching of many frame pairs of device-resident batches.

Every row of set 1 is matched only against the set-2 records within `radius` of its projection through the pair's H.
The expected records are restated from the contract (guided_cases.expected_guided): the gate in numpy float32 (every
operation rounded, C's left-to-right order), then the oracle's exact, full matcher on the row's candidates in ascending index order.  All bytes
of both sets are compared: only the five match fields of set-1 rows of some pair may change."""
import numpy as np
import pytest

from batch_util import MATCH_FIELDS, frames, guarded_context, layout, same_bytes, span
from guided_cases import expected_guided as _expected
from synth import descriptors_to_points, synth_descriptors, synth_frame

pytestmark = pytest.mark.gpu

SIZES1 = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, 50, 77]   # frame 12: count -1; frame 13: in no pair
COUNTS1 = SIZES1[:12] + [-1, 77]
SIZES2 = [4100, 2000, 129, 128, 127, 64, 33, 32, 31, 20, 1, 0, 300]
PAIRS = [(i, (5 * i + 2) % 13) for i in range(13)]
# one set-2 frame in several pairs; frame 1 is also set 1 of a pair; frame 6 has count -1
KEYFRAME_PAIRS = [(0, 1), (2, 1), (5, 1), (7, 3), (10, 3), (11, 4), (13, 1), (1, 12), (6, 3)]
IMPROVE = dict(min_score=0.0, max_ambiguity=0.80, thresh=3.0)


def _homography(i, persp=True):
    """A non-trivial H (rotation, scale, shear, translation and, with persp, perspective terms and H[8] != 1)."""
    a = 0.15 + 0.05 * i
    s = 1.0 + 0.02 * (i % 5)
    H = np.array([[s * np.cos(a), -s * np.sin(a) + 0.01, 12.0 + i],
                  [s * np.sin(a), s * np.cos(a), -7.0 + 0.5 * i],
                  [2e-5 * (i % 3) if persp else 0.0, -1e-5 if persp else 0.0, 1.0 + (0.03 if persp else 0.0)]])
    return H.astype(np.float32)


def _plant(fr1, fr2, pairs, Hs, seed):
    """Put copies of half of each pair's set-1 records into set 2, near H * (their positions) (within 0.3 px, so radius 0.5
    has candidates), and a duplicate (same position and descriptor) of some of them, so ties for the best score occur."""
    rng = np.random.default_rng(seed)
    for (f1, f2), H in zip(pairs, Hs):
        a, b = fr1[f1], fr2[f2]
        k = min(len(a), len(b)) // 2
        if k == 0:
            continue
        x = np.stack([a["xpos"][:k], a["ypos"][:k], np.ones(k, np.float32)]).astype(np.float64)
        q = H.astype(np.float64) @ x
        dst = rng.permutation(len(b))[:k]
        b["xpos"][dst] = (q[0] / q[2] + rng.uniform(-0.2, 0.2, k)).astype(np.float32)
        b["ypos"][dst] = (q[1] / q[2] + rng.uniform(-0.2, 0.2, k)).astype(np.float32)
        b["data"][dst] = a["data"][:k]
        dup = dst[::7]
        dup = dup[dup + 1 < len(b)]
        for k2 in ("xpos", "ypos", "data"):
            b[k2][dup + 1] = b[k2][dup]


def _run(c, pairs, Hs, radius, recs1, counts1, offs1, stride1, recs2=None, counts2=None, offs2=None, stride2=0,
         max_pts=8192):
    """One misift_match_guided_batch; returns (set 1 after, set 2 after or None, num_found)."""
    from cudasift_amd import capi
    d1, c1 = c.upload(recs1), c.upload(np.asarray(counts1, np.int32))
    o1 = c.upload(offs1) if offs1 is not None else None
    dH = c.upload(np.ascontiguousarray(Hs, np.float32).reshape(-1))
    nf = c.upload(np.full(len(pairs), 0x5EED, np.int32))
    if recs2 is None:
        c.match_guided_batch(pairs, d1, len(counts1), c1, dH, radius, o1, stride1, max_pts=max_pts, num_found=nf)
        c.sync()
        return c.download(d1, (len(recs1),), capi.POINT_DTYPE), None, c.download(nf, (len(pairs),), np.int32)
    d2, c2 = c.upload(recs2), c.upload(np.asarray(counts2, np.int32))
    o2 = c.upload(offs2) if offs2 is not None else None
    c.match_guided_batch(pairs, d1, len(counts1), c1, dH, radius, o1, stride1, d2, len(counts2), c2, o2, stride2,
                         max_pts=max_pts, num_found=nf)
    c.sync()
    return (c.download(d1, (len(recs1),), capi.POINT_DTYPE), c.download(d2, (len(recs2),), capi.POINT_DTYPE),
            c.download(nf, (len(pairs),), np.int32))


def _parity_case(seed):
    f1 = frames(SIZES1, seed, False)
    f2 = frames(SIZES2, seed + 1, False)
    Hs = [_homography(i) for i in range(len(PAIRS))]
    _plant(f1, f2, PAIRS, Hs, seed + 2)
    return f1, f2, Hs


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("radius", [0.5, 10.0, 64.0])
def test_parity_with_oracle(ctx, radius, padded):
    f1, f2, Hs = _parity_case(3)
    r1, o1, s1 = layout(f1, COUNTS1, padded, min_stride=0, pad_error=0.0)
    r2, o2, s2 = layout(f2, SIZES2, padded, min_stride=0, pad_error=0.0)
    exp, enf = _expected(PAIRS, Hs, radius, 8192, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    got1, got2, nf = _run(ctx, PAIRS, Hs, radius, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
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
    Hs = [_homography(i) for i in range(len(KEYFRAME_PAIRS))]
    _plant(fr, fr, KEYFRAME_PAIRS, Hs, 12)
    recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    exp, enf = _expected(KEYFRAME_PAIRS, Hs, 12.0, 8192, recs, counts, offs, 0, recs, counts, offs, 0)
    got, _, nf = _run(ctx, KEYFRAME_PAIRS, Hs, 12.0, recs, counts, offs, 0)
    # set 2 is the input batch itself: the oracle read the positions and descriptors of `recs`, which the call never
    # writes, so every byte of the shared buffer must equal the restated set 1
    same_bytes(got, exp, "shared batch")
    assert np.array_equal(nf, enf), (nf, enf)


@pytest.mark.parametrize("n1,n2", [(2000, 4100), (33, 129)])
def test_unbounded_radius_identity_equals_exact_full_match(ctx, n1, n2):
    """radius = +inf and the identity H: every record is a candidate, so the call equals misift_match in exact, full mode."""
    f1 = frames([n1], 21, False)
    f2 = frames([n2], 22, False)
    got, _, nf = _run(ctx, [(0, 0)], [np.eye(3, dtype=np.float32)], float("inf"), f1[0], [n1], None, n1,
                      f2[0], [n2], None, n2)
    ctx.set_options(match_full=1, match_exact_top2=1)
    try:
        exp = ctx.match(f1[0].copy(), n1, f2[0].copy(), n2)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    same_bytes(got, exp, "set 1")
    assert nf[0] == (exp["match"] >= 0).sum() == n1


def test_guided_match_rejects_decoys(ctx):
    """Each row's true partner sits at H * x with a perturbed descriptor; an exact copy of the row's descriptor (a higher
    score) sits 3 radii away.  misift_match_batch takes the decoy; the guided call takes the partner for every row."""
    from cudasift_amd import capi
    n, radius = 1024, 8.0
    rng = np.random.default_rng(31)
    H = _homography(2)
    d1 = synth_descriptors(n, 41, l2=True)
    noisy = d1 + rng.normal(0.0, 0.02, d1.shape).astype(np.float32)
    partner = (noisy / np.linalg.norm(noisy, axis=1, keepdims=True)).astype(np.float32)
    s1 = descriptors_to_points(d1, capi.POINT_DTYPE)
    s1["xpos"] = rng.uniform(100, 1800, n).astype(np.float32)
    s1["ypos"] = rng.uniform(100, 1000, n).astype(np.float32)
    q = H.astype(np.float64) @ np.stack([s1["xpos"], s1["ypos"], np.ones(n)]).astype(np.float64)
    px, py = q[0] / q[2], q[1] / q[2]
    s2 = descriptors_to_points(np.concatenate([partner, d1]), capi.POINT_DTYPE)   # partners 0..n-1, decoys n..2n-1
    ang = rng.uniform(0, 2 * np.pi, n)
    s2["xpos"] = np.concatenate([px + rng.uniform(-0.5, 0.5, n), px + 3 * radius * np.cos(ang)]).astype(np.float32)
    s2["ypos"] = np.concatenate([py + rng.uniform(-0.5, 0.5, n), py + 3 * radius * np.sin(ang)]).astype(np.float32)
    c1 = ctx.upload(np.array([n], np.int32))
    c2 = ctx.upload(np.array([2 * n], np.int32))
    d2 = ctx.upload(s2)
    dg = ctx.upload(s1)
    db = ctx.upload(s1)
    dH = ctx.upload(H.reshape(-1))
    nf = ctx.match_guided_batch([(0, 0)], dg, 1, c1, dH, radius, None, n, d2, 1, c2, None, 2 * n)
    ctx.match_batch([(0, 0)], db, 1, c1, None, n, d2, 1, c2, None, 2 * n)
    ctx.sync()
    guided = ctx.download(dg, (n,), capi.POINT_DTYPE)
    glob = ctx.download(db, (n,), capi.POINT_DTYPE)
    assert np.array_equal(glob["match"], np.arange(n) + n)
    assert np.array_equal(guided["match"], np.arange(n))
    assert ctx.download(nf, (1,), np.int32)[0] == n
    exp, enf = _expected([(0, 0)], [H], radius, 8192, s1, [n], None, n, s2, [2 * n], None, 2 * n)
    same_bytes(guided, exp, "guided rows")
    assert enf[0] == n


def test_chain_behind_real_extraction(ctx):
    """extract packed -> match_batch -> find_homography_batch -> match_guided_batch with find's H ->
    improve_homography_batch, with no host read in between."""
    from cudasift_amd import capi
    B, h, w, mp = 6, 480, 640, 4096
    frames = np.stack([synth_frame(f, w, h) for f in range(B)]).astype(np.float32)
    frames[1:] = np.stack([np.roll(frames[0], (2 * f, 3 * f), axis=(0, 1)) for f in range(1, B)])
    d = ctx.upload(frames)
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    pairs = [(f, f + 1) for f in range(B - 1)]
    sel = [f for f, _ in pairs]
    seeds = [100 + f for f in sel]
    find = dict(max_pts=mp, num_loops=1000, min_score=0.0, max_ambiguity=0.80, thresh=5.0)
    ctx.match_batch(pairs, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0)
    dH, dn = ctx.find_homography_batch(sel, seeds, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, **find)
    # the same find once more: improve refines its start in place, and the guided call must be checked against find's H
    dHi, _ = ctx.find_homography_batch(sel, seeds, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, **find)
    dnf = ctx.match_guided_batch(pairs, packed, B, cnt.ptr, dH, 4.0, cnt.ptr + 4 * B, 0, max_pts=mp)
    dfit = ctx.improve_homography_batch(sel, packed, B, cnt.ptr, dHi, cnt.ptr + 4 * B, 0, num_loops=5, **IMPROVE)
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    counts, offs = ci[:B], ci[B:]
    got = ctx.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    H = ctx.download(dH, (len(sel), 3, 3), np.float32)
    Hi = ctx.download(dHi, (len(sel), 3, 3), np.float32)
    nm = ctx.download(dn, (len(sel),), np.int32)
    nf = ctx.download(dnf, (len(sel),), np.int32)
    fit = ctx.download(dfit, (len(sel),), np.int32)
    assert (counts > 100).all(), counts
    assert nm.max() > 50, nm
    # the guided fields: the restatement on the downloaded records and find's H (the frame's other fields were written by
    # the extraction and improve's match_error; the restatement only reads positions and descriptors)
    exp, enf = _expected(pairs, list(H), 4.0, mp, got, counts, offs, 0, got, counts, offs, 0)
    for i, (f1, _) in enumerate(pairs):
        s1 = span(offs, 0, f1, int(counts[f1]))
        for k in MATCH_FIELDS:
            assert np.array_equal(exp[s1][k], got[s1][k]), (f1, k)
    assert np.array_equal(nf, enf), (nf, enf)
    solved = nm > 50
    assert (nf[solved] > 0.3 * counts[:B - 1][solved]).all(), (nf, nm, counts)
    # improve ran on the guided matches: H, num_fit and match_error as the single call from find's H
    for i, (f1, _) in enumerate(pairs):
        n1 = int(counts[f1])
        s1 = span(offs, 0, f1, n1)
        dm = ctx.upload(got[s1].copy())
        He, nfe = ctx.improve_homography(dm.ptr, n1, H[i], 5, **IMPROVE)
        after = ctx.download(dm, (n1,), capi.POINT_DTYPE)
        assert fit[i] == nfe and He.view(np.uint32).tobytes() == Hi[i].view(np.uint32).tobytes(), (i, fit[i], nfe)
        assert after.tobytes() == got[s1].tobytes(), f1


def test_edge_cases(ctx):
    """NaN H and a zero denominator: no candidate, no fault.  A radius whose square underflows: no candidate.  max_pts
    overflow on either side: -1, set 1 untouched.  Two runs: the same bytes."""
    sizes1, sizes2 = [150, 60, 90, 80, 70], [50, 150, 90, 80, 70]
    f1 = frames(sizes1, 51, False)
    f2 = frames(sizes2, 52, False)
    r1, o1, _ = layout(f1, sizes1, False, min_stride=0, pad_error=0.0)
    r2, o2, _ = layout(f2, sizes2, False, min_stride=0, pad_error=0.0)
    nan_h = np.full((3, 3), np.nan, np.float32)
    zero_den = _homography(1)
    zero_den[2] = 0.0
    pairs = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    Hs = [np.eye(3, dtype=np.float32), np.eye(3, dtype=np.float32), nan_h, zero_den, np.eye(3, dtype=np.float32)]
    f2[4]["xpos"] = f1[4]["xpos"][:70]                 # exact coincidences: err = 0, still not < fl(1e-30^2) = 0
    f2[4]["ypos"] = f1[4]["ypos"][:70]
    r2, o2, _ = layout(f2, sizes2, False, min_stride=0, pad_error=0.0)
    for radius in (1e-30, 50.0):
        got1, got2, nf = _run(ctx, pairs, Hs, radius, r1, sizes1, o1, 0, r2, sizes2, o2, 0, max_pts=100)
        again1, _, nf2 = _run(ctx, pairs, Hs, radius, r1, sizes1, o1, 0, r2, sizes2, o2, 0, max_pts=100)
        same_bytes(got1, again1, "two runs")
        assert np.array_equal(nf, nf2)
        exp, enf = _expected(pairs, Hs, radius, 100, r1, sizes1, o1, 0, r2, sizes2, o2, 0)
        same_bytes(got1, exp, "set 1, radius %g" % radius)
        same_bytes(got2, r2, "set 2")
        assert nf[0] == -1 and nf[1] == -1 and nf[2] == 0 and nf[3] == 0, nf
        for f in (0, 1):                               # over max_pts: untouched
            sl = span(o1, 0, f, sizes1[f])
            same_bytes(got1[sl], r1[sl], "frame %d over max_pts" % f)
        for f in (2, 3):                               # NaN H, zero denominator: nothing matched
            sl = span(o1, 0, f, sizes1[f])
            assert (got1["match"][sl] == -1).all() and (got1["score"][sl] == 0).all()
            assert (got1["ambiguity"][sl] == 0).all() and (got1["match_xpos"][sl] == 0).all()
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
    dH = ctx.upload(np.tile(np.eye(3, dtype=np.float32).reshape(-1), 2))
    poison = np.full(4, 0x5EED, np.int32)
    nf = ctx.upload(poison)

    def call(pairs, npairs=None, r=None, c=None, h=None, radius=10.0, max_pts=64):
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        r = recs.ptr if r is None else r
        c = counts.ptr if c is None else c
        h = dH.ptr if h is None else h
        return L.misift_match_guided_batch(ctx.h, len(p) if npairs is None else npairs, p.ctypes.data, r, 2, c, None,
                                           32, r, 2, c, None, 32, h, radius, max_pts, nf.ptr)
    assert call([(0, 1), (0, 0)]) == -1                 # set-1 frame 0 twice
    assert call([(0, 2)]) == -1                         # set-2 index out of range
    assert call([(-1, 0)]) == -1                        # set-1 index out of range
    assert call([(0, 1)], npairs=-1) == -1
    assert call([(0, 1)], r=0) == -1                    # NULL records
    assert call([(0, 1)], c=0) == -1                    # NULL counts
    assert call([(0, 1)], h=0) == -1                    # NULL homography
    assert call([(0, 1)], radius=float("nan")) == -1
    assert call([(0, 1)], radius=0.0) == -1
    assert call([(0, 1)], radius=-1.0) == -1
    assert call([(0, 1)], max_pts=0) == -1
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
    f1, f2, Hs = _parity_case(71)
    r1, o1, s1 = layout(f1, COUNTS1, False, min_stride=0, pad_error=0.0)
    r2, o2, s2 = layout(f2, SIZES2, False, min_stride=0, pad_error=0.0)
    with guarded_context(3) as g:
        got = _run(g, PAIRS, Hs, 10.0, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
        inf = _run(g, [(10, 1)], [np.eye(3, dtype=np.float32)], float("inf"), r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    assert capi.check_guards() >= 0
    again = _run(ctx, PAIRS, Hs, 10.0, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    same_bytes(got[0], again[0], "guarded vs unguarded")
    assert np.array_equal(got[2], again[2])
    again = _run(ctx, [(10, 1)], [np.eye(3, dtype=np.float32)], float("inf"), r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    same_bytes(inf[0], again[0], "guarded vs unguarded, radius inf")
