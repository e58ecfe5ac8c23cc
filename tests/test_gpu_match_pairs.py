"""misift_match_pairs_batch: batch matching into pair-indexed output rows, frames repeated freely, with an optional mutual
nearest-neighbour check.

Every output row must carry set-1 record r's xpos / ypos and the five match fields misift_match on that pair writes
(the oracle's, too); with mutual = 1 a row keeps its match only if the oracle's reversed match (sets swapped, full +
exact) of that column names it.  Every other byte of the output, the inputs, and oversized pairs stay untouched."""
import ctypes as C

import numpy as np
import pytest

from batch_util import (POISON, POISON_WORD, expected_pair, fields_equal, frames, guarded_context, layout,
                        no_match_rows, num_cus, orc, span, untouched)
from synth import descriptors_to_points, synth_descriptors, synth_frame

pytestmark = pytest.mark.gpu

SIZES1 = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, 50, 77]   # frame 12: count -1; frame 13: in no pair
COUNTS1 = SIZES1[:12] + [-1, 77]
SIZES2 = [4100, 2000, 129, 128, 127, 64, 33, 32, 31, 20, 1, 0, 300]
PAIRS = [(i, (5 * i + 2) % 13) for i in range(13)]
MISIFT_OK, MISIFT_EINVAL = 0, -1


def _run(ctx, pairs, r1, c1, o1, s1, r2=None, c2=None, o2=None, s2=0, max_pts=4100, mutual=0, same=False):
    """One misift_match_pairs_batch on poisoned output; returns (out records, counts, num_matched, set 1 after, set 2
    after)."""
    from cudasift_amd import capi
    npairs = len(pairs)
    d1, dc1 = ctx.upload(r1), ctx.upload(np.asarray(c1, np.int32))
    do1 = ctx.upload(o1) if o1 is not None else None
    if same:
        d2, dc2, do2, nf2, s2 = d1, dc1, do1, len(c1), s1
    else:
        d2, dc2 = ctx.upload(r2), ctx.upload(np.asarray(c2, np.int32))
        do2 = ctx.upload(o2) if o2 is not None else None
        nf2 = len(c2)
    out = ctx.upload(np.full(npairs * max_pts * 576, POISON, np.uint8))
    oc = ctx.upload(np.full(npairs, POISON_WORD, np.int32))
    nm = ctx.upload(np.full(npairs, POISON_WORD, np.int32))
    ctx.match_pairs_batch(pairs, d1, len(c1), dc1, do1, s1, d2, nf2, dc2, do2, s2, max_pts=max_pts, mutual=mutual,
                          out=out, out_counts=oc, num_matched=nm)
    ctx.sync()
    got = ctx.download(out, (npairs * max_pts,), capi.POINT_DTYPE)
    a1 = ctx.download(d1, (len(r1),), capi.POINT_DTYPE)
    a2 = None if same else ctx.download(d2, (len(r2),), capi.POINT_DTYPE)
    return got, ctx.download(oc, (npairs,), np.int32), ctx.download(nm, (npairs,), np.int32), a1, a2


def _check(ctx, pairs, r1, c1, o1, s1, r2, c2, o2, s2, full, exact, mutual, max_pts=4100, same=False):
    ctx.set_options(match_full=int(full), match_exact_top2=int(exact))
    try:
        got, oc, nm, a1, a2 = _run(ctx, pairs, r1, c1, o1, s1, r2, c2, o2, s2, max_pts, mutual, same)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    assert a1.tobytes() == r1.tobytes(), "set 1 written"
    if not same:
        assert a2.tobytes() == r2.tobytes(), "set 2 written"
    if same:
        r2, c2, o2, s2 = r1, c1, o1, s1
    exp_counts = []
    for i, (f1, f2) in enumerate(pairs):
        n1, n2 = max(int(c1[f1]), 0), max(int(c2[f2]), 0)
        if n1 > max_pts or n2 > max_pts:
            assert oc[i] == -1 and nm[i] == -1, (i, oc[i], nm[i])
            exp_counts.append(-1)
            continue
        assert oc[i] == n1, (i, oc[i], n1)
        exp_counts.append(n1)
        p1, p2 = r1[span(o1, s1, f1, n1)], r2[span(o2, s2, f2, n2)]
        e, k = expected_pair(p1, p2, full, exact, mutual)
        fields_equal(got[i * max_pts:i * max_pts + n1], e, "pair %d (%d x %d)" % (i, n1, n2))
        assert nm[i] == k, (i, nm[i], k)
    untouched(got, exp_counts, max_pts)
    return got, oc, nm


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("full,exact", [(False, False), (True, False), (False, True), (True, True)])
def test_same_answer_as_match_batch(ctx, full, exact, padded):
    """Each set-1 frame in one pair: the seven fields equal misift_match_batch's set-1 rows byte for byte, and the oracle."""
    from cudasift_amd import capi
    f1 = frames(SIZES1, 3, exact)
    f2 = frames(SIZES2, 4, exact)
    r1, o1, s1 = layout(f1, COUNTS1, padded, min_stride=1, pad_error=0.0)
    r2, o2, s2 = layout(f2, SIZES2, padded, min_stride=1, pad_error=0.0)
    got, oc, _ = _check(ctx, PAIRS, r1, COUNTS1, o1, s1, r2, SIZES2, o2, s2, full, exact, 0)
    ctx.set_options(match_full=int(full), match_exact_top2=int(exact))
    try:
        d1, dc1 = ctx.upload(r1), ctx.upload(np.asarray(COUNTS1, np.int32))
        d2, dc2 = ctx.upload(r2), ctx.upload(np.asarray(SIZES2, np.int32))
        ctx.match_batch(PAIRS, d1, len(COUNTS1), dc1, ctx.upload(o1) if o1 is not None else None, s1, d2, len(SIZES2),
                        dc2, ctx.upload(o2) if o2 is not None else None, s2)
        ctx.sync()
        mb = ctx.download(d1, (len(r1),), capi.POINT_DTYPE)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    for i, (a, b) in enumerate(PAIRS):
        n1, n2 = max(COUNTS1[a], 0), SIZES2[b]
        if n1 == 0:
            assert oc[i] == 0
            continue
        rows = got[i * 4100:i * 4100 + n1]
        if n2 == 0:
            fields_equal(rows, no_match_rows(r1[span(o1, s1, a, n1)]), "empty set 2")
            continue
        fields_equal(rows, mb[span(o1, s1, a, n1)], "pair %d against misift_match_batch" % i)


def _chunked(n1, n2):
    """Whether misift_match_batch's planner (the one misift_match_pairs_batch runs) cuts the columns into chunks."""
    from cudasift_amd import capi
    L = capi.lib()
    n1 = np.asarray(n1, np.int32)
    n2 = np.asarray(n2, np.int32)
    plan5 = np.zeros(5 * len(n1), np.int32)
    ni, ch, pb = C.c_int(), C.c_int(), C.c_int()
    capi.check(L.misift_test_match_batch_plan(num_cus(), 0, len(n1), n1.ctypes.data, n2.ctypes.data,
                                              plan5.ctypes.data, C.byref(ni), C.byref(ch), C.byref(pb)),
               "misift_test_match_batch_plan")
    return ch.value > 1


@pytest.mark.parametrize("mutual", [0, 1])
def test_many_to_many(ctx, mutual):
    """Windowed, keyframe (both directions), self pairs and d_recs1 == d_recs2, in a chunked and an unchunked plan."""
    small = [1300 + 13 * f for f in range(16)]                 # 11-12 row blocks each: the call fills a round
    fr = frames(small, 7, False)
    r, o, s = layout(fr, small, False, min_stride=1, pad_error=0.0)
    window = [(f, g) for f in range(16) for g in range(f + 1, min(f + 4, 16))]
    keyframe = [(15, k) for k in (0, 5, 10)] + [(k, 15) for k in (0, 5, 10)]
    selfp = [(3, 3), (9, 9)]
    pairs = window + keyframe + selfp
    assert not _chunked([small[a] for a, _ in pairs], [small[b] for _, b in pairs])
    _check(ctx, pairs, r, small, o, s, None, None, None, 0, False, False, mutual, max_pts=1500, same=True)
    _check(ctx, pairs, r, small, o, s, r.copy(), small, o, s, True, True, mutual, max_pts=1500)
    big = [3000, 2500, 2800]
    fr = frames(big, 8, False)
    r, o, s = layout(fr, big, True, min_stride=1, pad_error=0.0)
    pairs = [(0, 1), (0, 2), (1, 0), (2, 2)]
    assert _chunked([big[a] for a, _ in pairs], [big[b] for _, b in pairs])
    _check(ctx, pairs, r, big, o, s, None, None, None, 0, False, True, mutual, max_pts=3000, same=True)


def _tie_frames():
    """Set 1 with duplicate rows, all-zero and negative rows, a NaN row; set 2 with duplicate columns."""
    from cudasift_amd import capi
    d1 = synth_descriptors(300, 71)
    d2 = synth_descriptors(260, 72)
    d1[10] = d1[3]
    d1[11] = d1[3]                                   # three equal rows: the smallest (3) must win their column
    d1[200] = d2[40]
    d1[201] = d2[40]                                 # two rows equal to a column
    d1[50] = 0.0                                     # all-zero row: every score 0, never a match
    d1[51] = -d1[52]                                 # negative scores only
    d1[60, 7] = np.nan                               # a NaN descriptor
    d2[100] = d2[40]                                 # duplicate columns: the smaller column wins the row
    d2[101] = d1[3]
    d2[102] = d1[3]
    p1 = descriptors_to_points(d1, capi.POINT_DTYPE)
    p2 = descriptors_to_points(d2, capi.POINT_DTYPE)
    p1["xpos"] += 0.25
    p2["ypos"] += 0.5
    return p1, p2


@pytest.mark.parametrize("full,exact", [(False, False), (True, True)])
def test_mutual_rule_with_ties(ctx, full, exact):
    p1, p2 = _tie_frames()
    r1 = np.concatenate([p1, p1])
    r2 = np.concatenate([p2, p2[:130]])
    c1, o1 = [300, 300], np.array([0, 300, 600], np.int32)
    c2, o2 = [260, 130], np.array([0, 260, 390], np.int32)
    pairs = [(0, 0), (1, 0), (0, 1), (1, 1)]
    got, _, nm = _check(ctx, pairs, r1, c1, o1, 0, r2, c2, o2, 0, full, exact, 1, max_pts=300)
    rows = got[:300]
    assert rows["match"][50] == -1 and rows["match"][51] == -1 and rows["match"][60] == -1
    assert rows["match"][10] == -1 and rows["match"][11] == -1 and rows["match"][3] >= 0
    # rows 200 / 201 tie on columns 40 and 100: the exact merge keeps the smaller column, the reference's class merge the
    # smaller class (column 100); either way row 200 wins the column and row 201 loses it
    assert rows["match"][201] == -1 and rows["match"][200] == (40 if exact else 100)
    assert 0 < nm[0] < 300


def test_oversized_pairs_and_argument_errors(ctx):
    from cudasift_amd import capi
    sizes = [100, 700, 40]
    fr = frames(sizes, 9, False)
    r, o, s = layout(fr, sizes, False, min_stride=1, pad_error=0.0)
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
    got, oc, nm = _check(ctx, pairs, r, sizes, o, s, None, None, None, 0, False, False, 1, max_pts=512, same=True)
    assert list(oc) == [-1, -1, 100, 40, -1] and nm[0] == -1 and nm[1] == -1 and nm[4] == -1
    L = capi.lib()
    d, dc, do = ctx.upload(r), ctx.upload(np.asarray(sizes, np.int32)), ctx.upload(o)
    out = ctx.upload(np.full(2 * 512 * 576, POISON, np.uint8))
    oc = ctx.upload(np.full(2, 7, np.int32))
    nmb = ctx.upload(np.full(2, 7, np.int32))

    def call(pl, npairs=None, recs1=d.ptr, counts1=dc.ptr, recs2=d.ptr, counts2=dc.ptr, max_pts=512, mutual=1,
             o_=out.ptr, oc_=oc.ptr, nm_=nmb.ptr):
        pl = np.ascontiguousarray(pl, np.int32).reshape(-1, 2)
        return L.misift_match_pairs_batch(ctx.h, len(pl) if npairs is None else npairs, pl.ctypes.data, recs1, 3,
                                          counts1, do.ptr, 0, recs2, 3, counts2, do.ptr, 0, max_pts, mutual, o_, oc_,
                                          nm_)
    ok = [(0, 2), (2, 2)]
    bad = [dict(npairs=-1), dict(pl=[(0, 3), (1, 1)]), dict(pl=[(-1, 0), (1, 1)]), dict(recs1=None), dict(recs2=None),
           dict(counts1=None), dict(counts2=None), dict(o_=None), dict(oc_=None), dict(max_pts=0), dict(mutual=2),
           dict(mutual=-1), dict(o_=d.ptr)]
    for kw in bad:
        pl = kw.pop("pl", ok)
        assert call(pl, **kw) == MISIFT_EINVAL, kw
    assert call(ok, npairs=0) == MISIFT_OK
    ctx.sync()
    assert (ctx.download(out, (2 * 512 * 576,), np.uint8) == POISON).all(), "an argument error enqueued work"
    assert list(ctx.download(oc, (2,), np.int32)) == [7, 7] and list(ctx.download(nmb, (2,), np.int32)) == [7, 7]
    assert call(ok, nm_=None) == MISIFT_OK                  # d_num_matched may be NULL
    ctx.sync()
    assert list(ctx.download(oc, (2,), np.int32)) == [100, 40]


def test_mutual_output_feeds_find_homography(ctx):
    """Extracted frames -> mutual pairs -> misift_find_homography_batch on the output as it is: H and inlier counts equal
    srand(seed) + misift_find_homography on the downloaded rows."""
    from cudasift_amd import capi
    o = orc()
    B, h, w, mp = 4, 480, 640, 4096
    base = synth_frame(0, w, h).astype(np.float32)
    frames = np.stack([np.roll(base, (2 * f, 3 * f), axis=(0, 1)) for f in range(B)]).astype(np.float32)
    d = ctx.upload(frames)
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (3, 0)]
    npairs = len(pairs)
    out, oc, nm = ctx.match_pairs_batch(pairs, packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp, mutual=True)
    seeds = [200 + i for i in range(npairs)]
    FIND = dict(num_loops=1000, min_score=0.0, max_ambiguity=0.80, thresh=5.0)
    dH, dn = ctx.find_homography_batch(list(range(npairs)), seeds, out, npairs, oc, None, mp, max_pts=mp, **FIND)
    ctx.sync()
    counts = ctx.download(oc, (npairs,), np.int32)
    nmatch = ctx.download(nm, (npairs,), np.int32)
    H = ctx.download(dH, (npairs, 3, 3), np.float32)
    num = ctx.download(dn, (npairs,), np.int32)
    rows = ctx.download(out, (npairs * mp,), capi.POINT_DTYPE)
    assert (counts > 100).all(), counts
    for i in range(npairs):
        n = int(counts[i])
        sel = rows[i * mp:i * mp + n].copy()
        assert nmatch[i] == int((sel["match"] >= 0).sum()) and 0 < nmatch[i] < n, (i, nmatch[i], n)
        dm = ctx.upload(sel)
        o.srand(seeds[i])
        He, ne = ctx.find_homography(dm.ptr, n, **FIND)
        assert num[i] == ne and np.array_equal(H[i].view(np.uint32), np.asarray(He, np.float32).view(np.uint32)), i
    assert num.max() > 50, num


def test_guard_mode(ctx):
    """One mutual call with every allocation guarded: no band damaged."""
    from cudasift_amd import capi
    with guarded_context(None) as g:
        sizes = [500, 130, 2000]
        fr = frames(sizes, 11, False)
        r, o, s = layout(fr, sizes, False, min_stride=1, pad_error=0.0)
        pairs = [(0, 1), (1, 2), (2, 0), (2, 2)]
        _check(g, pairs, r, sizes, o, s, None, None, None, 0, False, False, 1, max_pts=2000, same=True)
    capi.check_guards()
