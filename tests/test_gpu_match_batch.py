"""misift_match_batch: many (frame of set 1, frame of set 2) pairs of device-resident batches in one stream-ordered call.

Every pair must come out bit-identical to misift_match on that pair (all bytes of set 1: the five match fields written,
everything else — other fields, frames in no pair, pairs with an empty side, padding — untouched) and to the oracle."""
import numpy as np
import pytest

from batch_util import MATCH_FIELDS, frames, guarded_context, layout, num_cus, orc, same_bytes, sequence_case, span
from synth import synth_frame

pytestmark = pytest.mark.gpu

SIZES1 = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, 50, 77]   # frame 12: count -1; frame 13: in no pair
COUNTS1 = SIZES1[:12] + [-1, 77]
SIZES2 = [4100, 2000, 129, 128, 127, 64, 33, 32, 31, 20, 1, 0, 300]
PAIRS = [(i, (5 * i + 2) % 13) for i in range(13)]


def _run_batch(c, pairs, recs1, counts1, offs1, stride1, recs2=None, counts2=None, offs2=None, stride2=0):
    """One misift_match_batch; returns (set-1 records after, set-2 records after or None)."""
    from cudasift_amd import capi
    d1, c1 = c.upload(recs1), c.upload(np.asarray(counts1, np.int32))
    o1 = c.upload(offs1) if offs1 is not None else None
    if recs2 is None:
        c.match_batch(pairs, d1, len(counts1), c1, o1, stride1)
        c.sync()
        return c.download(d1, (len(recs1),), capi.POINT_DTYPE), None
    d2, c2 = c.upload(recs2), c.upload(np.asarray(counts2, np.int32))
    o2 = c.upload(offs2) if offs2 is not None else None
    c.match_batch(pairs, d1, len(counts1), c1, o1, stride1, d2, len(counts2), c2, o2, stride2)
    c.sync()
    return c.download(d1, (len(recs1),), capi.POINT_DTYPE), c.download(d2, (len(recs2),), capi.POINT_DTYPE)


def _expected(ctx, pairs, recs1, counts1, offs1, stride1, recs2, counts2, offs2, stride2, full, exact, oracle=True):
    """Set 1 after one misift_match per pair (and the same rows from the oracle)."""
    o = orc()
    exp = recs1.copy()
    ctx.set_options(match_full=int(full), match_exact_top2=int(exact))
    try:
        for f1, f2 in pairs:
            n1, n2 = max(int(counts1[f1]), 0), max(int(counts2[f2]), 0)
            if n1 == 0 or n2 == 0:
                continue
            s1, s2 = span(offs1, stride1, f1, n1), span(offs2, stride2, f2, n2)
            p1, p2 = recs1[s1].copy(), recs2[s2].copy()
            got = ctx.match(p1, n1, p2, n2)
            if oracle:
                ref = p1.copy()
                o.match(ref, n1, p2, n2, full=full, exact=exact)
                for k in MATCH_FIELDS:
                    assert np.array_equal(ref[k], got[k]), (f1, f2, n1, n2, k)
            exp[s1] = got
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    return exp


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("full,exact", [(False, False), (True, False), (False, True)])
def test_parity_with_single_pair_matching(ctx, full, exact, padded):
    f1 = frames(SIZES1, 3, exact)
    f2 = frames(SIZES2, 4, exact)
    r1, o1, s1 = layout(f1, COUNTS1, padded, min_stride=0, pad_error=0.0)
    r2, o2, s2 = layout(f2, SIZES2, padded, min_stride=0, pad_error=0.0)
    exp = _expected(ctx, PAIRS, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2, full, exact)
    ctx.set_options(match_full=int(full), match_exact_top2=int(exact))
    try:
        got1, got2 = _run_batch(ctx, PAIRS, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    same_bytes(got1, exp, "set 1")
    same_bytes(got2, r2, "set 2 (read only)")
    # the n2 < 32 pair of reference mode: no column takes part -> match -1, score 0
    f = SIZES1.index(129)
    n2 = SIZES2[dict(PAIRS)[f]]
    sl = span(o1, s1, f, 129)
    if n2 < 32 and not full:
        assert (got1["match"][sl] == -1).all() and (got1["score"][sl] == 0).all()


def test_behind_real_extraction(ctx):
    """misift_extract_batch_packed_async, then misift_match_batch (f, f + 1) on its packed records (d_recs1 == d_recs2)
    with no synchronisation in between."""
    from cudasift_amd import capi
    B, h, w, mp = 6, 480, 640, 4096
    frames = np.stack([synth_frame(f, w, h) for f in range(B)]).astype(np.float32)
    d = ctx.upload(frames)
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    pairs = [(f, f + 1) for f in range(B - 1)]
    ctx.match_batch(pairs, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0)
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    counts, offs = ci[:B], ci[B:]
    got = ctx.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    assert (counts > 100).all(), counts
    # misift_match on host copies of each pair recomputes the five fields from the same descriptors: frame f is set 1 of
    # pair f and set 2 of pair f - 1, and the batch wrote nothing but the match fields of set-1 rows
    exp = _expected(ctx, pairs, got, counts, offs, 0, got, counts, offs, 0, False, False, oracle=False)
    same_bytes(got, exp, "packed batch")


def test_argument_errors(ctx):
    from cudasift_amd import capi
    L = capi.lib()
    recs = ctx.zeros(576 * 64)
    counts = ctx.upload(np.array([32, 32], np.int32))

    def call(pairs, npairs=None):
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        return L.misift_match_batch(ctx.h, len(p) if npairs is None else npairs, p.ctypes.data, recs.ptr, 2, counts.ptr,
                                    None, 32, recs.ptr, 2, counts.ptr, None, 32)
    assert call([(0, 1), (0, 0)]) == -1                 # set-1 frame 0 twice
    assert call([(0, 2)]) == -1                         # set-2 index out of range
    assert call([(-1, 0)]) == -1                        # set-1 index out of range
    assert call([(0, 1)], npairs=-1) == -1
    assert call(np.zeros((0, 2)), npairs=0) == 0        # no-op
    assert call([(1, 1), (0, 1)]) == 0
    ctx.sync()


def _batch_case(c, n_pairs, seed, sizes_lo, sizes_hi):
    pairs, recs, sizes, offs = sequence_case(n_pairs, seed, sizes_lo, sizes_hi, False)
    got, _ = _run_batch(c, pairs, recs, sizes, offs, 0)
    return pairs, recs, sizes, offs, got


@pytest.mark.parametrize("n_pairs,lo,hi", [(256, 1500, 2500), (3, 1800, 4200)])
def test_large_and_small_batches(ctx, n_pairs, lo, hi):
    """Many pairs (one chunk per row block, rows written by the sweep) and few (columns cut, merge launch)."""
    import ctypes as C
    from cudasift_amd import capi
    pairs, recs, sizes, offs, got = _batch_case(ctx, n_pairs, 21 + n_pairs, lo, hi)
    n1 = np.array([sizes[a] for a, _ in pairs], np.int32)
    n2 = np.array([sizes[b] for _, b in pairs], np.int32)
    plan = np.zeros((n_pairs, 5), np.int32)
    ni, ch, bound = C.c_int(), C.c_int(), C.c_int()
    capi.lib().misift_test_match_batch_plan(num_cus(), 0, n_pairs, n1.ctypes.data, n2.ctypes.data, plan.ctypes.data,
                                            C.byref(ni), C.byref(ch), C.byref(bound))
    assert (ch.value == 1) == (n_pairs >= 64), (n_pairs, ch.value)
    exp = _expected(ctx, pairs, recs, sizes, offs, 0, recs, sizes, offs, 0, False, False, oracle=n_pairs < 8)
    same_bytes(got, exp, "%d pairs" % n_pairs)


def test_guard_mode(ctx):
    """One chunked and one unchunked batch on a fresh guarded context (plan and partials buffers start as 0xFF): no band
    damaged, same bytes as the unguarded context."""
    from cudasift_amd import capi
    with guarded_context(3) as g:
        small = _batch_case(g, 3, 5, 1000, 3000)
        large = _batch_case(g, 80, 6, 1500, 2500)
    assert capi.check_guards() >= 0
    for (pairs, recs, sizes, offs, got), seed, lo, hi in ((small, 5, 1000, 3000), (large, 6, 1500, 2500)):
        again = _batch_case(ctx, len(pairs), seed, lo, hi)[4]
        same_bytes(got, again, "guarded vs unguarded")
