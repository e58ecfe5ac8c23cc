"""Extraction at record capacity: the case tables and the checker of the capacity tests (test_extract_capacity_cpu.py
checks the premises on the oracle and the checker on doctored outputs, test_gpu_extract_capacity.py runs the HIP paths).
No GPU in here.

The rule (include/misift.h, misift_extract).  For one frame let c be the 17 counters of the oracle's UNCAPPED run, noct
the number of octaves (the coarsest is k = 1), detection segment k the rows [c[2k-1], c[2k]), duplicate segment k (second
orientations) the rows [c[2k], c[2k+1]), and M = max_pts.
  1. numPts = min(c[2 noct], M); with fix_numpts min(c[2 noct + 1], M).
  2. Rows [0, min(c[2 noct + 1], M)) hold records, nothing behind them is written.  A segment that ends at or below M holds
     exactly the oracle's records of that segment; the one segment that contains row M holds M - start DISTINCT members of
     the oracle's same segment (which ones is the append order's business).
  3. Records are paired on the bits of (subsampling, xpos, ypos, scale, orientation): unique within each uncapped set
     (util.associate pairs a keypoint's two orientations by their order, which a subset does not keep).  The paired
     records agree as compare_points asks: sharpness and edgeness bit-identical too, every descriptor element within
     DESC_ATOL, no outlier budget.
  4. Counters: every word whose uncapped value is below M is equal, every other word is >= M; the per-octave detection
     counts c[2k] - c[2k-1] equal the uncapped ones (a dropped detection is still counted: refine_all / refine_kernel add
     to the counter before they look at the capacity, on the fused and on the dense path alike).

Frames: extract_cases.frames6(), 483 x 270, 4 octaves.  Uncapped counters c[2 .. 9] (test_extract_capacity_cpu.py pins
them):
    frame 0:  22  27  89  98 245 274 448  486        frame 3:  32  34 104 118 332 379 648  717
    frame 1:  40  44 147 162 414 454 904 1050        frame 4:  23  31 112 126 291 327 567  648
    frame 2:  26  32 122 138 362 402 719  806        frame 5:  21  27  79  89 267 313 486  554
"""
import numpy as np

from util import DESC_ATOL

NOCT = 4
POISON_BYTE = 0xA5                         # every output buffer starts as this byte
POISON_U32 = 0xA5A5A5A5                    # (as a float -2.9e-16: no field of a record is ever that)
RECORD_WORDS = 144
# the words of a record an extraction writes wherever it writes a record (the rest are the matcher's: a packed record
# has them cleared, a row of d_pts keeps what was there)
EXTRACT_WORDS = np.array([0, 1, 2, 3, 4, 5, 12] + list(range(16, 144)))
KEY_FIELDS = ("subsampling", "xpos", "ypos", "scale", "orientation")
EXACT_FIELDS = ("sharpness", "edgeness")

UNCAPPED = np.array([[22, 27, 89, 98, 245, 274, 448, 486], [40, 44, 147, 162, 414, 454, 904, 1050],
                     [26, 32, 122, 138, 362, 402, 719, 806], [32, 34, 104, 118, 332, 379, 648, 717],
                     [23, 31, 112, 126, 291, 327, 567, 648], [21, 27, 79, 89, 267, 313, 486, 554]])

# a single call on frame 1 (segments end at 40, 44, 147, 162, 414, 454, 904 and 1050)
SINGLE_CAPS = (1, 41, 44, 150, 454, 455, 700, 903, 904, 905, 1000)
# a batch of the six frames.  1 ... 1000 put frame 1 into the classes of the single-call table and the other five into
# others; no frame's numPts is one off any of them, so 718 (frame 2: total - 1) and 649 (frame 3: total + 1, and one past
# the end of frame 4) are there for those two classes.
BATCH_CAPS = (1, 44, 150, 455, 700, 904, 1000, 718, 649)
BIG_CAPS = (150, 700)                      # patch_reach 9: most keypoints through descr_big
# deterministic = 1 (rule 7).  The fused path stages every octave's detections in a list of M entries and orders the list:
# byte-identical wherever no octave's detection count exceeds M (lists_fit).  The dense kernels have no staging list, the
# record array itself is the list and is ordered afterwards: byte-identical wherever nothing inside numPts is cut
# (nothing_cut).  Frames for which that holds, per capacity (asserted on the oracle's counters by the CPU test):
DETERMINISTIC_CAPS = (150, 455, 700)
LISTS_FIT = {150: (), 455: (0, 1, 2, 3, 4, 5), 700: (0, 1, 2, 3, 4, 5)}
NOTHING_CUT = {150: (), 455: (0,), 700: (0, 3, 4, 5)}
ALTERNATING = (4096, 150, 4096, 1, 4096)   # one context, the same buffers
PIPE_CAP = 150
OVERFLOW_CAP = 700                         # the batch with a noise frame that floods its candidate list
OVERFLOW_THRESH = 0.05
OVERFLOW_UNCAPPED = 16384                  # room for the oracle's uncapped run at that threshold (frame 0: 3130 records)

CLASSES = ("M = 1", "inside a detection segment", "inside a duplicate segment", "at a segment end", "one past",
           "total - 1", "total", "total + 1", "inside the finest duplicates")


def noise_frame(seed=5):
    """483 x 270 white noise, 8-bit values as float32."""
    return np.random.default_rng(seed).integers(0, 256, (270, 483), dtype=np.uint8).astype(np.float32)


def segments(c, noct=NOCT):
    """[(kind, k, start, end)] of one frame's uncapped counters, in row order: kind 'det' or 'dup', octave k."""
    c = [int(v) for v in c]
    out = []
    for k in range(1, noct + 1):
        out.append(("det", k, c[2 * k - 1], c[2 * k]))
        out.append(("dup", k, c[2 * k], c[2 * k + 1]))
    return out


def classify(c, M, noct=NOCT):
    """(class, segment) of capacity M against one frame's uncapped counters c.  segment = (kind, k) of the segment that
    contains row M, or None.  'total' is the uncapped numPts c[2 noct].  The first rule that applies names the class:
    M = 1; total - 1, total, total + 1; 'above all' (M beyond the last record: nothing is capped); at a segment end (a
    non-empty segment ends exactly at M); one past (one ends at M - 1); else the segment that contains row M — 'inside
    the finest duplicates', 'inside a duplicate segment' or 'inside a detection segment'."""
    segs = [s for s in segments(c, noct) if s[3] > s[2]]
    total, last = int(c[2 * noct]), int(c[2 * noct + 1])
    inside = next(((kind, k) for kind, k, s, e in segs if s <= M < e), None)
    if M == 1:
        return "M = 1", inside
    for d, name in ((-1, "total - 1"), (0, "total"), (1, "total + 1")):
        if M == total + d:
            return name, inside
    if M > last:
        return "above all", None
    ends = {e for _, _, _, e in segs}
    if M in ends:
        return "at a segment end", inside
    if M - 1 in ends:
        return "one past", inside
    assert inside is not None, (c, M)
    if inside == ("dup", noct):
        return "inside the finest duplicates", inside
    return ("inside a duplicate segment" if inside[0] == "dup" else "inside a detection segment"), inside


def detection_counts(c, noct=NOCT):
    c = np.asarray(c, np.int64)
    return [int(c[2 * k] - c[2 * k - 1]) for k in range(1, noct + 1)]


def lists_fit(c, M, noct=NOCT):
    """No octave's detection count exceeds M: the fused path's staging lists hold every detection."""
    return max(detection_counts(c, noct)) <= M


def nothing_cut(c, M, fix_numpts=0, noct=NOCT):
    """No segment inside numPts is cut by M."""
    return int(c[2 * noct + (1 if fix_numpts else 0)]) <= M


def words(recs):
    """[n, 144] uint32 view of n records."""
    recs = np.ascontiguousarray(recs)
    return recs.view(np.uint32).reshape(len(recs), RECORD_WORDS)


def poisoned_records(n, dtype):
    return np.frombuffer(np.full(576 * n, POISON_BYTE, np.uint8).tobytes(), dtype).copy()


def key5(recs):
    """[n, 5] uint32: the bits of (subsampling, xpos, ypos, scale, orientation)."""
    return np.stack([np.ascontiguousarray(recs[f]).view(np.uint32) for f in KEY_FIELDS], axis=1)


def key_index(recs):
    """{key bytes: row} of an uncapped record set; the key must be unique in it."""
    k = key5(recs)
    out = {k[i].tobytes(): i for i in range(len(k))}
    assert len(out) == len(k), "the five-field key repeats: %d keys for %d records" % (len(out), len(k))
    return out


def check_frame(ref, c, M, rows, fix_numpts=0, noct=NOCT, num_pts=None, packed=False, name=""):
    """Rules 1 - 3 and the hole check for one frame.
    ref: the oracle's uncapped records (at least c[2 noct + 1] of them), c its 17 counters.
    rows: the frame's M rows of a poisoned d_pts — or, packed, its `count` packed records.
    num_pts: the count the call returned (None: not checked; packed: len(rows) is checked against rule 1 anyway).
    Returns (class, records checked)."""
    total = int(c[2 * noct + 1])
    want = min(int(c[2 * noct + (1 if fix_numpts else 0)]), M)
    if num_pts is not None:
        assert int(num_pts) == want, "%s: numPts %d, rule 1 says %d (M = %d)" % (name, num_pts, want, M)
    valid = want if packed else min(total, M)
    assert len(rows) == (want if packed else M), "%s: %d rows for M = %d (count %d)" % (name, len(rows), M, want)
    w = words(rows)
    cols = np.arange(RECORD_WORDS) if packed else EXTRACT_WORDS
    hole = np.nonzero((w[:valid][:, cols] == POISON_U32).any(axis=1))[0]
    assert len(hole) == 0, "%s: %d rows inside [0, %d) keep a poison word, first %s" % (name, len(hole), valid, hole[:8])
    stray = np.nonzero((w[valid:] != POISON_U32).any(axis=1))[0]
    assert len(stray) == 0, "%s: %d rows behind row %d were written, first %s" % (name, len(stray), valid,
                                                                                  (stray[:8] + valid))
    index = key_index(ref[:total])
    got_keys = key5(rows[:valid])
    for kind, k, s, e in segments(c, noct):
        if s >= valid:
            break
        hi = min(e, valid)
        src = np.empty(hi - s, np.int64)
        for j in range(s, hi):
            i = index.get(got_keys[j].tobytes(), -1)
            assert i >= 0, "%s: row %d (%s %d) is no record of the oracle's uncapped set" % (name, j, kind, k)
            assert s <= i < e, "%s: row %d lies in %s segment %d [%d, %d) but is the oracle's row %d" % (name, j, kind, k,
                                                                                                    s, e, i)
            src[j - s] = i
        assert len(np.unique(src)) == len(src), "%s: %s segment %d holds a record twice" % (name, kind, k)
        # (hi == e: hi - s distinct members of a segment of e - s records are all of them: nothing is missing)
        a, b = ref[src], rows[s:hi]
        for f in EXACT_FIELDS:
            assert np.array_equal(a[f].view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)), \
                "%s: %s differs in %s segment %d" % (name, f, kind, k)
        assert not np.isnan(b["data"]).any(), "%s: NaN descriptor in %s segment %d" % (name, kind, k)
        dd = np.abs(a["data"].astype(np.float64) - b["data"]).max() if len(src) else 0.0
        assert dd <= DESC_ATOL, "%s: descriptor element off by %g in %s segment %d" % (name, dd, kind, k)
    return classify(c, M, noct)[0], valid


def check_counters(got, c, M, noct=NOCT, name=""):
    """Rule 4 for one frame's 17 device counters against the uncapped oracle's."""
    got, c = np.asarray(got, np.int64), np.asarray(c, np.int64)
    assert len(got) == 17 and len(c) == 17, (name, len(got), len(c))
    below = c < M
    assert np.array_equal(got[below], c[below]) and (got[~below] >= M).all(), (name, M, got, c)
    assert detection_counts(got, noct) == detection_counts(c, noct), (name, M, got, c)


def check_packed_layout(counts, offsets, packed_rows, want_counts, name=""):
    """Rules 1 and 5 for a packed call: counts as rule 1 says (want_counts; -1 where the candidate list overflows),
    offsets the exclusive prefix sum of the non-negative counts, and nothing written behind offsets[B] of the poisoned
    packed array (packed_rows: all its records).  The records themselves: check_frame(..., packed=True) per frame."""
    counts, offsets = np.asarray(counts, np.int64), np.asarray(offsets, np.int64)
    assert np.array_equal(counts, np.asarray(want_counts, np.int64)), (name, counts, want_counts)
    prefix = np.concatenate([[0], np.cumsum(np.maximum(counts, 0))])
    assert np.array_equal(offsets, prefix), "%s: offsets %s are not the prefix sum %s" % (name, offsets, prefix)
    stray = np.nonzero((words(packed_rows[int(offsets[-1]):]) != POISON_U32).any(axis=1))[0]
    assert len(stray) == 0, "%s: %d packed records written behind offsets[B] = %d, first %s" % (
        name, len(stray), offsets[-1], stray[:8] + int(offsets[-1]))
