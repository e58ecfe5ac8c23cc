"""misift_quantize_batch + misift_match_batch_i8: 8-bit descriptors and batched pair matching on the int8 matrix cores.

Integer scores are exact, so every byte is checked against a numpy restatement of the contract (batch_util):
quantisation against np.clip(np.rint(256 d), 0, 127), matching against a float64 matmul of the integer q (exact below
2^53).  Bytes the calls must not write — other fields, frames in no pair, pairs with an empty side, q outside the frames,
set 2 — stay byte-identical."""
import ctypes as C
import os

import numpy as np
import pytest

from batch_util import frames, guarded_context, layout, match_np, num_cus, quantize_np, same_bytes, sequence_case, span
from synth import descriptors_to_points, synth_descriptors, synth_frame

pytestmark = pytest.mark.gpu

SIZES1 = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, 50, 77]   # frame 12: count -1; frame 13: in no pair
COUNTS1 = SIZES1[:12] + [-1, 77]
SIZES2 = [4100, 2000, 129, 128, 127, 64, 33, 32, 31, 20, 1, 0, 300]
PAIRS = [(i, (5 * i + 2) % 13) for i in range(13)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _q_expected(recs, counts, offs, stride, pattern):
    """q after misift_quantize_batch over a buffer that held `pattern`: the frames' records quantised, the rest kept."""
    q = pattern.copy()
    for f, c in enumerate(counts):
        n = max(int(c), 0)
        sl = span(offs, stride, f, n)
        q[sl] = quantize_np(recs["data"][sl])
    return q


def _expected(pairs, recs1, q1, counts1, offs1, stride1, recs2, q2, counts2, offs2, stride2):
    exp = recs1.copy()
    for f1, f2 in pairs:
        n1, n2 = max(int(counts1[f1]), 0), max(int(counts2[f2]), 0)
        if n1 == 0 or n2 == 0:
            continue
        s1, s2 = span(offs1, stride1, f1, n1), span(offs2, stride2, f2, n2)
        exp[s1] = match_np(recs1[s1], q1[s1], recs2[s2], q2[s2])
    return exp


def _pattern(n, seed=9):
    return np.random.default_rng(seed).integers(-128, 128, (max(n, 1), 128)).astype(np.int8)


def _quantize(c, recs, counts, offs, stride, pattern):
    """One misift_quantize_batch into a buffer pre-filled with `pattern`; returns (device records, device q, q)."""
    d = c.upload(recs)
    dc = c.upload(np.asarray(counts, np.int32))
    do = c.upload(offs) if offs is not None else None
    dq = c.upload(pattern)
    c.quantize_batch(d, len(counts), dc, do, stride, dq)
    c.sync()
    return d, dc, do, dq, c.download(dq, pattern.shape, np.int8)


@pytest.mark.parametrize("padded", [False, True])
def test_quantize_bytes(ctx, padded):
    recs, offs, stride = layout(frames(SIZES1, 3, True), COUNTS1, padded, min_stride=0, pad_error=0.0)
    rng = np.random.default_rng(1)
    recs["data"][::7, ::5] = rng.normal(0, 0.4, recs["data"][::7, ::5].shape)     # negatives and saturation too
    recs["data"][3, :4] = [np.nan, np.inf, -np.inf, 127.5 / 256]
    pat = _pattern(len(recs))
    got = _quantize(ctx, recs, COUNTS1, offs, stride, pat)[4]
    assert np.array_equal(got, _q_expected(recs, COUNTS1, offs, stride, pat))
    if padded:                                                # count -1 frame and padding keep the pattern
        f = 12
        assert np.array_equal(got[span(None, stride, f, stride)], pat[span(None, stride, f, stride)])


@pytest.mark.parametrize("padded", [False, True])
def test_match_bytes(ctx, padded):
    from cudasift_amd import capi
    r1, o1, s1 = layout(frames(SIZES1, 3, True), COUNTS1, padded, min_stride=0, pad_error=0.0)
    r2, o2, s2 = layout(frames(SIZES2, 4, True), SIZES2, padded, min_stride=0, pad_error=0.0)
    d1, c1, do1, dq1, q1 = _quantize(ctx, r1, COUNTS1, o1, s1, _pattern(len(r1), 1))
    d2, c2, do2, dq2, q2 = _quantize(ctx, r2, SIZES2, o2, s2, _pattern(len(r2), 2))
    ctx.set_options(match_full=1, match_exact_top2=1)        # ignored by the int8 matcher: every column, exact top 2
    try:
        ctx.match_batch_i8(PAIRS, d1, dq1, len(COUNTS1), c1, do1, s1, d2, dq2, len(SIZES2), c2, do2, s2)
        ctx.sync()
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    got1 = ctx.download(d1, (len(r1),), capi.POINT_DTYPE)
    got2 = ctx.download(d2, (len(r2),), capi.POINT_DTYPE)
    assert np.array_equal(ctx.download(dq1, q1.shape, np.int8), q1)
    same_bytes(got1, _expected(PAIRS, r1, q1, COUNTS1, o1, s1, r2, q2, SIZES2, o2, s2), "set 1")
    same_bytes(got2, r2, "set 2 (read only)")


def test_keyframe_and_same_buffer(ctx):
    """Every frame against keyframe 0 (a set-2 frame in many pairs), then frame f against f + 1 with d_recs1 == d_recs2
    and d_q1 == d_q2."""
    from cudasift_amd import capi
    sizes = [300, 2000, 129, 31, 1, 0, 700]
    recs, offs, _ = layout(frames(sizes, 8, True), sizes, False, min_stride=0, pad_error=0.0)
    d, dc, do, dq, q = _quantize(ctx, recs, sizes, offs, 0, _pattern(len(recs)))
    ref = ctx.upload(recs)
    key = [(f, 0) for f in range(1, len(sizes))]
    ctx.match_batch_i8(key, d, dq, len(sizes), dc, do, 0, ref, dq, len(sizes), dc, do, 0)
    ctx.sync()
    same_bytes(ctx.download(d, (len(recs),), capi.POINT_DTYPE),
                _expected(key, recs, q, sizes, offs, 0, recs, q, sizes, offs, 0), "keyframe")
    d = ctx.upload(recs)
    seq = [(f, f + 1) for f in range(len(sizes) - 1)]
    ctx.match_batch_i8(seq, d, dq, len(sizes), dc, do, 0)
    ctx.sync()
    got = ctx.download(d, (len(recs),), capi.POINT_DTYPE)
    same_bytes(got, _expected(seq, recs, q, sizes, offs, 0, recs, q, sizes, offs, 0), "d_recs1 == d_recs2")


def test_ties_zero_rows_and_single_candidates(ctx):
    from cudasift_amd import capi
    rng = np.random.default_rng(4)
    n2 = 200
    p2 = descriptors_to_points(synth_descriptors(n2, 77, True), capi.POINT_DTYPE)
    p2["xpos"] = np.arange(n2, dtype=np.float32) + 0.25
    p2["ypos"] = np.arange(n2, dtype=np.float32) * 2
    for j in (40, 7, 150, 33, 32):                            # copies of record 5 at larger and smaller-lane indices
        p2["data"][j] = p2["data"][5]
    p1 = descriptors_to_points(synth_descriptors(6, 78, True), capi.POINT_DTYPE)
    p1["data"][0] = p2["data"][5]                             # best = the duplicated record: index 5 wins
    p1["data"][1] = 0                                         # all-zero row: no S > 0
    p1["data"][2] = 0
    p1["data"][2][17] = 0.3                                   # supported on one element only ...
    p2["data"][:, 17] = 0
    p2["data"][123][17] = 0.2                                 # ... which one set-2 record has: one candidate
    p1["data"][3] = -p2["data"][9]                            # quantises to zero
    recs = np.concatenate([p1, p2])
    counts = np.array([6, n2], np.int32)
    offs = np.array([0, 6, 6 + n2], np.int32)
    d, dc, do, dq, q = _quantize(ctx, recs, counts, offs, 0, _pattern(len(recs)))
    ctx.match_batch_i8([(0, 1)], d, dq, 2, dc, do, 0)
    ctx.sync()
    got = ctx.download(d, (len(recs),), capi.POINT_DTYPE)
    same_bytes(got, _expected([(0, 1)], recs, q, counts, offs, 0, recs, q, counts, offs, 0), "ties")
    r = got[:6]
    assert r["match"][0] == 5 and r["match_xpos"][0] == np.float32(5.25)
    assert r["ambiguity"][0] == r["score"][0] / (r["score"][0] + np.float32(1e-6))
    assert r["match"][1] == -1 and r["score"][1] == 0 and r["ambiguity"][1] == 0 and r["match_xpos"][1] == 0
    assert r["match"][2] == 123 and r["score"][2] > 0 and r["ambiguity"][2] == 0
    assert r["match"][3] == -1 and r["score"][3] == 0


def test_column_chunks(ctx):
    """64 rows x 60 000 columns: one row block, columns cut into chunks and merged; every byte exact."""
    from cudasift_amd import capi
    sizes = [64, 60000]
    fr = frames(sizes, 12, True)
    fr[1]["data"][59990] = fr[0]["data"][3]                   # a match in the last chunk
    fr[1]["data"][31] = fr[0]["data"][4]
    fr[1]["data"][40000] = fr[0]["data"][4]
    recs, offs, _ = layout(fr, sizes, False, min_stride=0, pad_error=0.0)
    n1, n2 = np.array([64], np.int32), np.array([60000], np.int32)
    plan, ni, ch, bound = np.zeros(5, np.int32), C.c_int(), C.c_int(), C.c_int()
    capi.lib().misift_test_match_i8_plan(num_cus(), 1, n1.ctypes.data, n2.ctypes.data, plan.ctypes.data, C.byref(ni),
                                         C.byref(ch), C.byref(bound))
    assert ch.value > 1 and plan[3] > 1, (ch.value, plan)
    d, dc, do, dq, q = _quantize(ctx, recs, sizes, offs, 0, _pattern(len(recs)))
    ctx.match_batch_i8([(0, 1)], d, dq, 2, dc, do, 0)
    ctx.sync()
    got = ctx.download(d, (len(recs),), capi.POINT_DTYPE)
    same_bytes(got, _expected([(0, 1)], recs, q, sizes, offs, 0, recs, q, sizes, offs, 0), "64 x 60000")
    assert got["match"][3] == 59990 and got["match"][4] == 31


def test_argument_errors(ctx):
    L = __import__("cudasift_amd.capi", fromlist=["lib"]).lib()
    recs = ctx.zeros(576 * 64)
    q = ctx.zeros(128 * 64 + 16)
    counts = ctx.upload(np.array([32, 32], np.int32))

    def quant(d_recs=True, n=2, d_counts=True, dq=None, stride=32):
        return L.misift_quantize_batch(ctx.h, recs.ptr if d_recs else None, n, counts.ptr if d_counts else None, None,
                                       stride, q.ptr if dq is None else dq)
    assert quant(d_recs=False) == -1
    assert quant(d_counts=False) == -1
    assert quant(dq=0) == -1
    assert quant(dq=q.ptr + 8) == -1                          # not 16-byte aligned
    assert quant(n=-1) == -1
    assert quant(stride=-1) == -1
    assert quant(n=0) == 0

    def call(pairs, npairs=None, q1=None, q2=None):
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        return L.misift_match_batch_i8(ctx.h, len(p) if npairs is None else npairs, p.ctypes.data, recs.ptr,
                                       q.ptr if q1 is None else q1, 2, counts.ptr, None, 32, recs.ptr,
                                       q.ptr if q2 is None else q2, 2, counts.ptr, None, 32)
    assert call([(0, 1), (0, 0)]) == -1                       # set-1 frame 0 twice
    assert call([(0, 2)]) == -1                               # set-2 index out of range
    assert call([(-1, 0)]) == -1
    assert call([(0, 1)], npairs=-1) == -1
    assert call([(0, 1)], q1=0) == -1
    assert call([(0, 1)], q2=q.ptr + 4) == -1
    assert call(np.zeros((0, 2)), npairs=0) == 0
    ctx.sync()
    assert (ctx.download(recs, (64 * 144,), np.float32) == 0).all()   # nothing was enqueued
    assert (ctx.download(q, (128 * 64 + 16,), np.uint8) == 0).all()
    assert quant() == 0 and call([(1, 1), (0, 1)]) == 0
    ctx.sync()


def test_chain_behind_extraction(ctx):
    """extract (packed, async) -> quantize -> match_i8 -> find_homography_batch on one context, no host read between."""
    from cudasift_amd import capi
    B, h, w, mp = 4, 480, 640, 4096
    base = synth_frame(0, w, h)                               # frame f + 1 = frame f shifted: real matches
    frames = np.stack([np.roll(base, (3 * f, 5 * f), axis=(0, 1)) for f in range(B)]).astype(np.float32)
    d = ctx.upload(frames)
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    dq = ctx.zeros(128 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    ctx.quantize_batch(packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, dq)
    pairs = [(f, f + 1) for f in range(B - 1)]
    ctx.match_batch_i8(pairs, packed, dq, B, cnt.ptr, cnt.ptr + 4 * B, 0)
    seeds = np.arange(1, B, dtype=np.uint32)
    H, nm = ctx.find_homography_batch(np.arange(B - 1), seeds, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp)
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    counts, offs = ci[:B], ci[B:]
    assert (counts > 100).all(), counts
    got = ctx.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    q = ctx.download(dq, (int(offs[B]), 128), np.int8)
    assert np.array_equal(q, quantize_np(got["data"]))
    exp = got.copy()
    for f1, f2 in pairs:
        s1, s2 = slice(offs[f1], offs[f1] + counts[f1]), slice(offs[f2], offs[f2] + counts[f2])
        exp[s1] = match_np(got[s1], q[s1], got[s2], q[s2])
    same_bytes(got, exp, "chain")
    # the same find on the same (now final) records gives the same H and counts: find ran behind the match
    H2, nm2 = ctx.find_homography_batch(np.arange(B - 1), seeds, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp)
    ctx.sync()
    assert np.array_equal(ctx.download(nm, (B - 1,), np.int32), ctx.download(nm2, (B - 1,), np.int32))
    assert np.array_equal(ctx.download(H, (B - 1, 9), np.float32), ctx.download(H2, (B - 1, 9), np.float32))
    assert (ctx.download(nm, (B - 1,), np.int32) > 8).all()


def _i8_case(c, n_pairs, seed, lo, hi):
    from cudasift_amd import capi
    pairs, recs, sizes, offs = sequence_case(n_pairs, seed, lo, hi, True)
    d, dc, do, dq, q = _quantize(c, recs, sizes, offs, 0, _pattern(len(recs)))
    c.match_batch_i8(pairs, d, dq, len(sizes), dc, do, 0)
    c.sync()
    return pairs, recs, q, sizes, offs, c.download(d, (len(recs),), capi.POINT_DTYPE)


def test_guard_mode(ctx):
    """Two chunked batches (3 pairs: many chunks per row block; 40 pairs: a few) on a fresh guarded context (plan and
    partials start as 0xFF): no band damaged, every byte as the restatement says.  The unchunked path runs guarded in
    test_unchunked_batch_two_windows."""
    with guarded_context(3) as g:
        cases = [_i8_case(g, 3, 5, 1000, 3000), _i8_case(g, 40, 6, 1500, 2500)]
    for pairs, recs, q, sizes, offs, got in cases:
        same_bytes(got, _expected(pairs, recs, q, sizes, offs, 0, recs, q, sizes, offs, 0), "%d pairs" % len(pairs))


def test_unchunked_batch_two_windows(ctx):
    """At least 16 * num_cus row blocks: one column chunk per row block (C == 1), so the sweep writes the rows itself
    and no merge runs.  Every set-1 frame is matched against one 20 000-column keyframe, so an item sweeps 625 tiles:
    two key windows of 512.  Copies of a record 32 k columns apart lie in one lane's column stream, inside a window and
    across the window boundary; the lane's own top-2 must keep the earliest.  Run plain and on a guarded context."""
    from cudasift_amd import capi
    cus = num_cus()
    nf, n2 = 16 * cus + 6, 20000
    rng = np.random.default_rng(31)
    sizes = rng.integers(1, 9, nf)
    counts = sizes.copy()
    counts[11] = -1                                           # no records: one row block fewer, still a full target
    p2 = frames([n2], 32, True)[0]
    dup = {100: (196, 19204, 101), 16400: (16560, 19600), 16359: (16391,), 5000: (5032, 16392)}
    for j, copies in dup.items():                             # column j % 32 is the lane; tile 512 opens window 1
        for k in copies:
            p2["data"][k] = p2["data"][j]
    fr = frames(sizes, 33, True)
    for f, j in zip((0, 1, 2, 3), dup):
        fr[f]["data"][0] = p2["data"][j]
    recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    n1, n2s = np.maximum(counts, 0).astype(np.int32), np.full(nf, n2, np.int32)
    plan = np.zeros((nf, 5), np.int32)
    ni, ch, bound = C.c_int(), C.c_int(), C.c_int()
    assert capi.lib().misift_test_match_i8_plan(cus, nf, n1.ctypes.data, n2s.ctypes.data, plan.ctypes.data,
                                                C.byref(ni), C.byref(ch), C.byref(bound)) == 0
    assert ch.value == 1 and (plan[n1 > 0, 3] == 1).all() and (plan[n1 > 0, 4] == 625).all(), (ch.value, plan[:3])
    pairs = [(f, 0) for f in range(nf)]
    q2 = quantize_np(p2["data"])
    q1 = quantize_np(recs["data"])
    exp = recs.copy()
    for r0 in range(0, len(recs), 512):                       # every record of set 1 is in a pair
        exp[r0:r0 + 512] = match_np(recs[r0:r0 + 512], q1[r0:r0 + 512], p2, q2)
    first = offs[:4]
    assert list(exp["match"][first]) == list(dup), exp["match"][first]

    def run(c):
        d, dc, do, dq, q = _quantize(c, recs, counts, offs, 0, _pattern(len(recs)))
        d2, dq2 = c.upload(p2), c.upload(q2)
        c2 = c.upload(np.array([n2], np.int32))
        c.match_batch_i8(pairs, d, dq, nf, dc, do, 0, d2, dq2, 1, c2, None, 0)
        c.sync()
        assert np.array_equal(q, q1)
        return c.download(d, (len(recs),), capi.POINT_DTYPE)

    same_bytes(run(ctx), exp, "unchunked, two windows")
    with guarded_context(3) as g:
        got = run(g)
    same_bytes(got, exp, "unchunked, guarded")
    sc = got["score"][first]
    assert (got["ambiguity"][first] == sc / (sc + np.float32(1e-6))).all()


def test_quality_on_golden_pair(ctx):
    """The reference's own stereo records: rows the fp32 oracle (exact + full) passes through FindHomography's gates match
    the same index, and find_homography_batch keeps >= 0.95 of the inliers it finds on misift_match_batch's matches."""
    from cudasift_amd import capi
    from oracle import pyoracle as orc
    z = np.load(os.path.join(ROOT, "tests", "golden", "refemul_golden.npz"))
    left, right = z["left_records"].copy(), z["righ_records"].copy()
    ex = left.copy()
    orc.match(ex, len(left), right, len(right), full=True, exact=True)
    recs = np.concatenate([left, right])
    counts = np.array([len(left), len(right)], np.int32)
    offs = np.array([0, len(left), len(recs)], np.int32)
    d, dc, do, dq, q = _quantize(ctx, recs, counts, offs, 0, _pattern(len(recs)))
    ctx.match_batch_i8([(0, 1)], d, dq, 2, dc, do, 0)
    d32 = ctx.upload(recs)
    ctx.match_batch([(0, 1)], d32, 2, dc, do, 0)
    seeds = np.array([1, 2, 3], np.uint32)
    res = {}
    for name, buf in (("i8", d), ("fp32", d32)):
        nms = []
        for s in seeds:
            _, nm = ctx.find_homography_batch([0], [s], buf, 2, dc, do, 0, max_pts=4096)
            nms.append(nm)
        ctx.sync()
        res[name] = [int(ctx.download(nm, (1,), np.int32)[0]) for nm in nms]
    got = ctx.download(d, (len(recs),), capi.POINT_DTYPE)[:len(left)]
    same_bytes(got, _expected([(0, 1)], recs, q, counts, offs, 0, recs, q, counts, offs, 0)[:len(left)], "golden")
    gate = (ex["score"] > 0.85) & (ex["ambiguity"] < 0.95)
    assert gate.sum() > 300
    assert (got["match"][gate] == ex["match"][gate]).mean() >= 0.99
    for a, b in zip(res["i8"], res["fp32"]):
        assert a >= 0.95 * b, res
