"""What the device-batch tests share (match_batch, match_pairs_batch, match_batch_i8, match_guided_batch, the homography
batches and the full-size checks): the batch scaffolding, the numpy restatements that define the expected answers, and
the coverage check of a pair plan.  A plain module: no fixtures, no hooks.  cudasift_amd.capi is imported inside the
functions, so collecting the tests needs no built library."""
import contextlib
import ctypes as C

import numpy as np

from synth import descriptors_to_points, synth_descriptors, synth_matches

MATCH_FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
# the pair-indexed matchers: the fields of an output row, and what their output, counts and num_matched are filled with
OUT_FIELDS = ("xpos", "ypos") + MATCH_FIELDS
POISON = 0xA5
POISON_WORD = 0x5A5A5A5A


# ---- batch scaffolding

def orc():
    from oracle import pyoracle
    return pyoracle


def num_cus():
    from cudasift_amd import capi
    cus, i = C.c_int(), [C.c_int() for _ in range(3)]
    capi.check(capi.lib().misift_device_info(0, C.create_string_buffer(64), 64, C.byref(i[0]), C.byref(i[1]),
                                             C.byref(C.c_size_t()), C.byref(cus), C.byref(i[2])), "misift_device_info")
    return cus.value


def frames(sizes, seed, l2):
    """Records with random descriptors, positions and (poisoned) other fields, so untouched bytes show."""
    from cudasift_amd import capi
    rng = np.random.default_rng(seed)
    out = []
    for f, n in enumerate(sizes):
        p = descriptors_to_points(synth_descriptors(n, seed * 100 + f, l2), capi.POINT_DTYPE)
        for k in ("xpos", "ypos", "scale", "orientation", "score", "ambiguity", "match_xpos", "match_ypos", "match_error"):
            p[k] = rng.random(n, dtype=np.float32) * 500
        p["match"] = rng.integers(-5, 5000, n)
        out.append(p)
    return out


def layout(frames, counts, padded, *, min_stride, pad_error):
    """(records, offsets or None, stride): packed like misift_extract_batch_packed_async leaves it (a frame of count
    -1 holds no records), or padded to a common stride of at least min_stride with offsets = None; the padding is zero
    bytes but for match_error = pad_error."""
    from cudasift_amd import capi
    if padded:
        stride = max(max(len(p) for p in frames), min_stride)
        recs = np.zeros(stride * len(frames), capi.POINT_DTYPE)
        recs["match_error"] = pad_error
        for f, p in enumerate(frames):
            recs[f * stride:f * stride + len(p)] = p
        return recs, None, stride
    kept = [p if c >= 0 else p[:0] for p, c in zip(frames, counts)]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in kept])]).astype(np.int32)
    return np.concatenate(kept), offs, 0


def sequence_case(n_pairs, seed, lo, hi, l2):
    """(pairs, records, sizes, offsets): pairs (f, f + 1) over n_pairs + 1 packed frames of lo <= size < hi records."""
    sizes = np.random.default_rng(seed).integers(lo, hi, n_pairs + 1)
    recs, offs, _ = layout(frames(sizes, seed, l2), sizes, False, min_stride=0, pad_error=0.0)
    return [(f, f + 1) for f in range(n_pairs)], recs, sizes, offs


def span(offs, stride, f, n):
    b = int(offs[f]) if offs is not None else f * stride
    return slice(b, b + n)


def same_bytes(a, b, what):
    if a.tobytes() != b.tobytes():
        av = a.view(np.uint8).reshape(len(a), -1)
        bv = b.view(np.uint8).reshape(len(b), -1)
        bad = np.nonzero((av != bv).any(1))[0]
        raise AssertionError("%s: %d records differ, first %s" % (what, len(bad), bad[:8]))


def same_rows(got, exp, what, fields=None):
    """Byte equality of whole records (fields None) or of the named fields, with the first differing rows on failure."""
    if fields is None:
        a, b = got.view(np.uint8).reshape(len(got), -1), exp.view(np.uint8).reshape(len(exp), -1)
    else:
        a = np.stack([np.ascontiguousarray(got[k]).view(np.uint32) for k in fields], 1)
        b = np.stack([np.ascontiguousarray(exp[k]).view(np.uint32) for k in fields], 1)
    bad = np.nonzero((a != b).any(1))[0]
    assert len(bad) == 0, "%s: %d rows differ, first %s" % (what, len(bad), bad[:8])


@contextlib.contextmanager
def guarded_context(min_checked, stream=None):
    """A fresh context on device 0 (on `stream`, a raw hipStream_t value; None: the NULL stream) with every allocation
    guarded.  When the body ends, check_guards() must find no band damaged and, with min_checked not None, at least that
    many allocations; then the context is closed and the previous guard mode restored."""
    from cudasift_amd import capi
    old = capi.set_guard(True)
    try:
        g = capi.Context(0, stream)
        try:
            yield g
            n = capi.check_guards()
            if min_checked is not None:
                assert n >= min_checked, n
        finally:
            g.close()
    finally:
        capi.set_guard(old)


# ---- fabricated tracks and records (misift_link_tracks_batch, misift_export_tracks_batch)

def planted_members(sizes, usable, lengths, rng):
    """Planted tracks: track t visits lengths[t] consecutive usable frames from a random start, taking one record nobody
    else has in each frame that still has one."""
    free = {f: list(rng.permutation(sizes[f])) for f in usable}
    out = []
    for L in lengths:
        a = int(rng.integers(0, max(len(usable) - L, 0) + 1))
        t = {}
        for f in usable[a:a + L]:
            if free[f]:
                t[f] = int(free[f].pop())
        out.append(t)
    return out


def fabricated_records(n, seed):
    """n records whose xpos / ypos are random bit patterns (NaN payloads, infinities, denormals); the rest zero."""
    from cudasift_amd import capi
    recs = np.zeros(max(n, 1), capi.POINT_DTYPE)
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, (2, len(recs)), dtype=np.uint64).astype(np.uint32)
    recs["xpos"], recs["ypos"] = bits[0].view(np.float32), bits[1].view(np.float32)
    return recs


def xy_bits(recs):
    """What expected_export takes: the bits of xpos / ypos per record, as they sit in the array that is uploaded."""
    return np.stack([np.ascontiguousarray(recs[k]).view(np.uint32) for k in ("xpos", "ypos")], 1)


# ---- frames of stored matches (the homography batches)

def matched_frames(sizes, seed):
    from cudasift_amd import capi
    out = []
    for f, n in enumerate(sizes):
        out.append(synth_matches(n, seed=seed * 100 + f)[0] if n else np.zeros(0, capi.POINT_DTYPE))
    return out


def gated_frame(n, seed, valid):
    """n records of which exactly `valid` pass the gate 0.85 / 0.95; the others (spread over the frame) have score 0."""
    p = synth_matches(n, seed=seed)[0]
    p["score"], p["ambiguity"] = 0.99, 0.5
    p["score"][np.linspace(0, n - 1, n - valid).astype(int)] = 0.0
    return p


# ---- expected answers, restated in numpy

def quantize_np(d):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip(np.rint(np.float32(256) * np.asarray(d, np.float32)), 0, 127)
    return np.where(np.isnan(v), 0, v).astype(np.int8)


def match_np(p1, q1, p2, q2):
    """The five match fields of set-1 rows p1 (q1: their int8 descriptors) against set 2 (p2, q2)."""
    out = p1.copy()
    S = q1.astype(np.float64) @ q2.astype(np.float64).T
    S = np.where(S > 0, S, 0.0)
    best = S.max(1)
    m = np.where(best > 0, S.argmax(1), -1)                  # argmax: the first (smallest) index of the maximum
    S[np.arange(len(S)), np.maximum(m, 0)] = 0
    sec = np.where(m >= 0, S.max(1) if S.shape[1] else 0, 0)
    score = best.astype(np.float32) * np.float32(2.0 ** -16)
    out["score"] = score
    out["ambiguity"] = (sec.astype(np.float32) * np.float32(2.0 ** -16)) / (score + np.float32(1e-6))
    out["match"] = m
    mm = np.maximum(m, 0)
    out["match_xpos"] = np.where(m >= 0, p2["xpos"][mm], np.float32(0))
    out["match_ypos"] = np.where(m >= 0, p2["ypos"][mm], np.float32(0))
    return out


def i8_records(p1, p2, core):
    """misift_match_batch_i8's five fields from the oracle's exact integer top-2 (match_np's contract: scores scaled by
    2^-16)."""
    out = p1.copy()
    sc = np.float32(2.0 ** -16)
    best, idx = core["ex_best"] * sc, core["ex_idx"]
    out["score"], out["match"] = best, idx
    out["ambiguity"] = (core["ex_sec"] * sc) / (best + np.float32(1e-6))
    mm = np.maximum(idx, 0)
    out["match_xpos"] = np.where(idx >= 0, p2["xpos"][mm], np.float32(0))
    out["match_ypos"] = np.where(idx >= 0, p2["ypos"][mm], np.float32(0))
    return out


def fields_equal(got, exp, what):
    for k in OUT_FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        if a.tobytes() != b.tobytes():
            diff = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
            raise AssertionError("%s: field %s differs in %d rows, first %s" % (what, k, len(diff), diff[:8]))


def untouched(got, counts, max_pts):
    """Every byte outside the seven fields of rows < count stays poisoned; all bytes of an oversized pair too."""
    from cudasift_amd import capi
    raw = got.view(np.uint8).reshape(len(got), 576).copy()
    mask = np.zeros(576, bool)
    for k in OUT_FIELDS:
        off = capi.POINT_DTYPE.fields[k][1]
        mask[off:off + 4] = True
    for i, n in enumerate(counts):
        rows = raw[i * max_pts:(i + 1) * max_pts]
        if n > 0:
            rows[:n, mask] = POISON
        assert (rows == POISON).all(), ("bytes outside the output fields written", i, n)


def no_match_rows(p1):
    """The rows a pair with no column (or a rejected row) gets: xpos / ypos of set 1, no match."""
    e = np.zeros(len(p1), p1.dtype)
    e["xpos"], e["ypos"] = p1["xpos"], p1["ypos"]
    e["match"] = -1
    return e


def expected_pair(p1, p2, full, exact, mutual):
    """The seven output fields of one pair from the oracle: forward MatchSiftData under (full, exact); with mutual, a row
    r with match m >= 0 keeps it only if the reversed match (set 2 against set 1, full + exact) of m is r.  Returns the
    rows (structured, only xpos, ypos and MATCH_FIELDS meaningful) and the number with match >= 0."""
    o = orc()
    n1, n2 = len(p1), len(p2)
    e = no_match_rows(p1)
    if n1 == 0 or n2 == 0:
        return e, 0
    fw = p1.copy()
    o.match(fw, n1, p2.copy(), n2, full=full, exact=exact)
    for k in MATCH_FIELDS:
        e[k] = fw[k]
    if mutual:
        rv = p2.copy()
        o.match(rv, n2, p1.copy(), n1, full=True, exact=True)
        m = e["match"]
        bad = (m >= 0) & (rv["match"][np.clip(m, 0, n2 - 1)] != np.arange(n1))
        e[bad] = no_match_rows(p1[bad])
    return e, int((e["match"] >= 0).sum())


# ---- pair plans

def check_pair_plan(plan, nitems, chunks, n1, n2, tiles_of):
    """The work list of a pair planner (rows of item0, row blocks, tiles, chunks, tiles per chunk) covers every (pair,
    128-row block, column tile) exactly once, where a pair of n1 x n2 records has tiles_of(n2) tiles.  Returns the row
    blocks of the call; how they bound the chunks and the partials is the caller's rule."""
    covered = np.zeros(nitems, np.int32)
    rows_total = 0
    for p, (item0, nrb, ntiles, nch, tpc) in enumerate(plan):
        a, b = max(int(n1[p]), 0), max(int(n2[p]), 0)
        assert nrb == ((a + 127) // 128 if a and b else 0), (p, a, b, nrb)
        assert ntiles == (tiles_of(b) if a and b else 0)
        assert nch >= 1 and tpc >= 1
        if ntiles:
            assert nch * tpc >= ntiles and (nch - 1) * tpc < ntiles          # no empty chunk
            if chunks == 1:
                assert nch == 1 and tpc == ntiles
        # the items of the pair: row block major, chunk minor; together they cover every (row block, tile) once
        tiles = np.zeros((nrb, max(ntiles, 1)), np.int32)
        for i in range(nrb * nch):
            rb, c = divmod(i, nch)
            covered[item0 + i] += 1
            t0, t1 = c * tpc, min(c * tpc + tpc, ntiles)
            tiles[rb, t0:t1] += 1
        if nrb and ntiles:
            assert (tiles[:, :ntiles] == 1).all(), p
        rows_total += nrb
    assert (covered == 1).all()                               # items are a partition of [0, nitems)
    return rows_total
