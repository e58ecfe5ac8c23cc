"""Premises of the capacity tests (extract_capacity_cases.py), on the oracle alone, and the checker's own test: every
doctoring of a correct output that a wrong bound in a kernel would produce must be rejected.  No GPU."""
import numpy as np
import pytest

import extract_capacity_cases as cc
import extract_cases as xc
from extract_capacity_cases import check_counters, check_frame, check_packed_layout, classify
from extract_cases import expected, frames6, small6
from util import DESC_ATOL

B = 6


def orc():
    from oracle import pyoracle
    return pyoracle


def uncapped():
    return expected(frames6())


_at = {}


def oracle_at(f, M, **kw):
    """The oracle's capped run of frame f as a poisoned array of M rows would hold it: (rows, numPts, counters)."""
    key = (f, M, tuple(sorted(kw.items())))
    if key not in _at:
        src = small6()[f] if kw.get("scale_up") else frames6()[f]
        pts, n, cnt = orc().extract(src, **dict(xc.ARGS, max_pts=M, **kw))
        c = expected(small6(), **kw)[2][f] if kw.get("scale_up") else uncapped()[2][f]
        rows = cc.poisoned_records(M, pts.dtype)
        valid = min(int(c[2 * cc.NOCT + 1]), M)
        rows[:valid] = pts[:valid]
        # the oracle leaves the matcher's fields zero; a row of d_pts keeps what was there
        w = cc.words(rows)
        other = np.setdiff1d(np.arange(cc.RECORD_WORDS), cc.EXTRACT_WORDS)
        w[:valid][:, other] = cc.POISON_U32
        rows.setflags(write=False)
        _at[key] = (rows, n, cnt)
    return _at[key]


def test_uncapped_counters_are_the_ones_the_tables_were_chosen_for():
    _, n, cnt = uncapped()
    assert np.array_equal(cnt[:, 2:10], cc.UNCAPPED), cnt[:, :10]
    assert np.array_equal(n, cc.UNCAPPED[:, 6]) and (cnt[:, :2] == 0).all()
    assert int(cnt[:, 9].max()) < xc.ARGS["max_pts"]


def test_every_class_occurs_in_both_tables():
    _, _, cnt = uncapped()
    single = {classify(cnt[xc.SINGLE], M)[0] for M in cc.SINGLE_CAPS}
    batch = {classify(cnt[f], M)[0] for f in range(B) for M in cc.BATCH_CAPS}
    assert set(cc.CLASSES) <= single, sorted(set(cc.CLASSES) - single)
    assert set(cc.CLASSES) <= batch and "above all" in batch, sorted(set(cc.CLASSES) - batch)
    # the segment that contains row M: every detection segment, and the duplicates of a coarse and of the finest octave
    inside = {classify(cnt[f], M)[1] for f in range(B) for M in cc.BATCH_CAPS}
    assert {("det", k) for k in range(1, 5)} | {("dup", 2), ("dup", 4)} <= inside, inside
    # what the single-call table was written down as
    want = {1: "M = 1", 41: "one past", 44: "at a segment end", 150: "inside a duplicate segment", 454: "at a segment end",
            455: "one past", 700: "inside a detection segment", 903: "total - 1", 904: "total", 905: "total + 1",
            1000: "inside the finest duplicates"}
    assert {M: classify(cnt[xc.SINGLE], M)[0] for M in cc.SINGLE_CAPS} == want
    assert cc.PIPE_CAP == 150 and 150 in cc.BIG_CAPS and 150 in cc.DETERMINISTIC_CAPS and 150 in cc.ALTERNATING
    assert all(150 < cnt[f][2 * k] - cnt[f][2 * k - 1] for f in range(B) for k in (4,))    # 150 cuts every frame (and its finest list)
    assert [f for f in range(B) if 700 < cnt[f][8]] == [1, 2]


def test_five_field_key_is_unique_and_the_order_pairing_is_not_enough():
    from util import associate
    ref, _, cnt = uncapped()
    for f in range(B):
        cc.key_index(ref[f, :cnt[f][9]])
    for kw in (dict(scale_up=True), dict(scale_up=True, fix_numpts=True)):
        r, _, c = expected(small6(), **kw)
        for f in range(B):
            cc.key_index(r[f, :c[f][9]])
    # associate() pairs a keypoint's orientations by their order: wrong for a subset that keeps only the second one
    rows, n, _ = oracle_at(1, 700)
    ia, ib, _, _ = associate(ref[1, :cnt[1][9]], rows[:700])
    wrong = int((ref[1]["orientation"][ia] != rows["orientation"][ib]).sum())
    assert wrong > 0, wrong


@pytest.mark.parametrize("fix", [0, 1])
def test_oracle_at_capacity_obeys_the_rule(fix):
    """Rules 1 - 3 on the oracle's own capped runs: byte-equal members of its uncapped set, numPts by rule 1."""
    ref, _, cnt = uncapped()
    for f in range(B):
        for M in sorted(set(cc.BATCH_CAPS) | (set(cc.SINGLE_CAPS) if f == xc.SINGLE else set())):
            rows, n, _ = oracle_at(f, M, fix_numpts=bool(fix))
            check_frame(ref[f], cnt[f], M, rows, fix, num_pts=n, name="oracle/f%d/M%d" % (f, M))
            valid = min(int(cnt[f][9]), M)
            idx = cc.key_index(ref[f, :cnt[f][9]])
            src = [idx[k.tobytes()] for k in cc.key5(rows[:valid])]
            assert np.array_equal(cc.words(ref[f][src])[:, cc.EXTRACT_WORDS], cc.words(rows[:valid])[:, cc.EXTRACT_WORDS])


@pytest.mark.parametrize("fix", [0, 1])
def test_oracle_with_scale_up_at_capacity_obeys_the_rule(fix):
    """The kept records are halved exactly once and the finest octave's second orientations behind numPts are not: both
    as in the uncapped run, whose records the capped ones must be."""
    ref, nref, cnt = expected(small6(), scale_up=True, fix_numpts=bool(fix))
    met = set()
    for f in range(B):
        for M in cc.BATCH_CAPS:
            rows, n, _ = oracle_at(f, M, scale_up=True, fix_numpts=bool(fix))
            met.add(check_frame(ref[f], cnt[f], M, rows, fix, num_pts=n, name="oracle/up/f%d/M%d" % (f, M))[0])
    assert {"inside a detection segment", "inside a duplicate segment", "inside the finest duplicates",
            "above all"} <= met, met
    if not fix:                       # the premise of the test: unhalved rows behind numPts exist and differ from halved ones
        f = 1
        tail = ref[f, nref[f]:cnt[f][9]]
        assert len(tail) > 50 and (tail["xpos"] / tail["subsampling"]).max() > 0.75 * small6().shape[2]


def test_counters_rule_on_the_oracle_and_where_it_ends():
    """The oracle counts dropped detections too, so rule 4 holds for its capped counters — and the duplicate words of a
    capped run differ from the uncapped ones, which is why the device is held to the uncapped counters only."""
    _, _, cnt = uncapped()
    differ = []
    for M in cc.SINGLE_CAPS:
        _, _, c = oracle_at(xc.SINGLE, M)
        check_counters(c, cnt[xc.SINGLE], M, name="oracle/M%d" % M)
        if not np.array_equal(c, cnt[xc.SINGLE]):
            differ.append(M)
    assert 1 in differ and 150 in differ and 700 in differ, differ


def test_emulated_reference_returns_the_same_count():
    from oracle import pyrefemul
    if not pyrefemul.available("fast"):
        pytest.skip("the emulated reference is not built")
    _, _, cnt = uncapped()
    for M in cc.SINGLE_CAPS:
        _, n, _ = pyrefemul.extract(frames6()[xc.SINGLE], num_octaves=4, thresh=3.0, max_pts=M, flavour="fast")
        assert n == min(int(cnt[xc.SINGLE][8]), M), (M, n)


def test_deterministic_premises():
    _, _, cnt = uncapped()
    for M in cc.DETERMINISTIC_CAPS:
        assert tuple(f for f in range(B) if cc.lists_fit(cnt[f], M)) == cc.LISTS_FIT[M], M
        assert tuple(f for f in range(B) if cc.nothing_cut(cnt[f], M)) == cc.NOTHING_CUT[M], M
    assert any(cc.LISTS_FIT[M] for M in cc.DETERMINISTIC_CAPS) and any(cc.NOTHING_CUT[M] for M in cc.DETERMINISTIC_CAPS)
    assert any(len(cc.LISTS_FIT[M]) < B for M in cc.DETERMINISTIC_CAPS)


def test_overflow_batch_premises():
    """The frames around the noise frame hold more records than the capacity at the low threshold, and the oracle's
    uncapped run of them fits its array."""
    for f in (0, 1, 3, 4, 5):
        _, n, c = expected(frames6()[f], thresh=cc.OVERFLOW_THRESH, max_pts=cc.OVERFLOW_UNCAPPED)
        assert cc.OVERFLOW_CAP < n and c[9] < cc.OVERFLOW_UNCAPPED, (f, n, c)
    _, n, _ = expected(cc.noise_frame(), thresh=cc.OVERFLOW_THRESH, max_pts=cc.OVERFLOW_UNCAPPED)
    assert n > 5000, n


# ------------------------------------------------------------------ the checker's own test
F, M = 1, 700                     # frame 1 at 700: five complete segments, the finest detections cut


def correct():
    ref, _, cnt = uncapped()
    rows, n, _ = oracle_at(F, M)
    return ref[F], cnt[F], rows.copy(), n


def rejected(rows, match, n=None, **kw):
    ref, c, _, n0 = correct()
    with pytest.raises(AssertionError, match=match):
        check_frame(ref, c, M, rows, 0, num_pts=n0 if n is None else n, name="doctored", **kw)


def test_checker_accepts_the_correct_output():
    ref, c, rows, n = correct()
    assert check_frame(ref, c, M, rows, 0, num_pts=n) == ("inside a detection segment", M)
    # any other choice of the cut segment's members is as good: the LAST 246 finest detections instead of the first
    rows[454:700] = ref[904 - 246:904]
    cc.words(rows)[454:700, 6:12] = cc.POISON_U32
    cc.words(rows)[454:700, 13:16] = cc.POISON_U32
    check_frame(ref, c, M, rows, 0, num_pts=n)


def test_checker_rejects_a_descriptor_element_off_by_ten_tolerances():
    _, _, rows, _ = correct()
    rows["data"][333, 77] += 10 * DESC_ATOL
    rejected(rows, "descriptor element off")
    _, _, rows, _ = correct()
    rows["data"][333, 77] += 0.5 * DESC_ATOL                        # within the tolerance: accepted
    ref, c, _, n = correct()
    check_frame(ref, c, M, rows, 0, num_pts=n)


def test_checker_rejects_an_orientation_one_ulp_off():
    _, _, rows, _ = correct()
    rows["orientation"][10] = np.nextafter(rows["orientation"][10], np.float32(1000.0))
    rejected(rows, "no record of the oracle")
    for f in cc.EXACT_FIELDS:
        _, _, rows, _ = correct()
        rows[f][10] = np.nextafter(rows[f][10], np.float32(1000.0))
        rejected(rows, f + " differs")


def test_checker_rejects_a_repeated_record():
    _, _, rows, _ = correct()
    rows[500] = rows[501]
    rejected(rows, "holds a record twice")
    _, _, rows, _ = correct()
    rows[20] = rows[21]                                             # in a complete segment: a member is missing as well
    rejected(rows, "holds a record twice")


def test_checker_rejects_a_record_of_the_wrong_octave():
    _, _, rows, _ = correct()
    rows[100] = rows[300]
    rejected(rows, r"row 100 lies in det segment 2 \[44, 147\) but is the oracle's row 300")
    _, _, rows, _ = correct()
    rows[[150, 20]] = rows[[20, 150]]                               # a second orientation among the detections, and back
    rejected(rows, "row 20 lies in det segment 1")


def test_checker_rejects_a_missing_member_of_a_complete_segment():
    ref, c, rows, _ = correct()
    rows[60:146] = rows[61:147].copy()                              # record 60 is gone, the segment is one short:
    rejected(rows, "holds a record twice")                          # row 146 still holds its old record
    ref, c, rows, _ = correct()
    rows[60:413] = rows[61:414].copy()                              # ... or everything behind it moved up by one
    rejected(rows, "row 146 lies in det segment 2")
    ref, c, rows, _ = correct()
    rows["xpos"][60] += 1.0                                         # ... or something else stands in its place
    rejected(rows, "row 60 .* is no record")


def test_checker_rejects_a_poison_row_inside_the_count():
    for row in (0, 453, 699):
        _, _, rows, _ = correct()
        cc.words(rows)[row] = cc.POISON_U32
        rejected(rows, "keep a poison word")
    _, _, rows, _ = correct()
    cc.words(rows)[12, 16 + 127] = cc.POISON_U32                    # one element of one descriptor
    rejected(rows, "keep a poison word")


def test_checker_rejects_a_count_off_by_one():
    _, _, rows, n = correct()
    for d in (-1, 1):
        rejected(rows, "rule 1 says 700", n=n + d)
    ref, c, _, _ = correct()
    full, nf, _ = oracle_at(F, 1000)                                 # numPts is 904 here, not 1000 and not 1050
    check_frame(ref, c, 1000, full, 0, num_pts=904)
    for bad in (903, 905, 1000):
        with pytest.raises(AssertionError, match="rule 1 says 904"):
            check_frame(ref, c, 1000, full, 0, num_pts=bad)
    with pytest.raises(AssertionError, match="rule 1 says 1000"):
        check_frame(ref, c, 1000, full, 1, num_pts=904)


def packed_case():
    """A correct packed output of the six frames at M = 455 in a poisoned array of B * M records."""
    ref, _, cnt = uncapped()
    cap = 455
    counts = np.array([min(int(cnt[f][8]), cap) for f in range(B)])
    offs = np.concatenate([[0], np.cumsum(counts)])
    packed = cc.poisoned_records(B * cap, ref.dtype)
    for f in range(B):
        packed[offs[f]:offs[f + 1]] = orc().extract(frames6()[f], **dict(xc.ARGS, max_pts=cap))[0][:counts[f]]
    return ref, cnt, cap, counts, offs, packed


def test_checker_rejects_a_wrong_offset_table_and_a_record_behind_the_last():
    ref, cnt, cap, counts, offs, packed = packed_case()
    check_packed_layout(counts, offs, packed, counts)
    for f in range(B):
        check_frame(ref[f], cnt[f], cap, packed[offs[f]:offs[f + 1]], 0, packed=True, name="packed/f%d" % f)
    bad = offs.copy()
    bad[3] += 1
    with pytest.raises(AssertionError, match="not the prefix sum"):
        check_packed_layout(counts, bad, packed, counts)
    with pytest.raises(AssertionError, match="not the prefix sum"):
        check_packed_layout(counts, offs + 1, packed, counts)
    with pytest.raises(AssertionError):                              # a count off by one
        check_packed_layout(counts - np.eye(B, dtype=np.int64)[2], offs, packed, counts)
    # a frame whose candidate list overflowed: count -1, width 0
    c2 = counts.copy()
    c2[2] = -1
    o2 = np.concatenate([[0], np.cumsum(np.maximum(c2, 0))])
    check_packed_layout(c2, o2, cc.poisoned_records(B * cap, ref.dtype), c2)
    with pytest.raises(AssertionError, match="not the prefix sum"):
        check_packed_layout(c2, np.concatenate([[0], np.cumsum(c2)]), packed, c2)
    stray = packed.copy()
    stray[offs[B]] = ref[0][0]
    with pytest.raises(AssertionError, match=r"written behind offsets\[B\]"):
        check_packed_layout(counts, offs, stray, counts)
    # a packed record with a hole, and one that is another frame's
    holed = packed.copy()
    cc.words(holed)[offs[1] + 3, 8] = cc.POISON_U32                 # the match index: a packed record is complete
    with pytest.raises(AssertionError, match="keep a poison word"):
        check_frame(ref[1], cnt[1], cap, holed[offs[1]:offs[2]], 0, packed=True)
    with pytest.raises(AssertionError, match="no record of the oracle"):
        check_frame(ref[1], cnt[1], cap, packed[offs[2]:offs[2] + counts[1]], 0, packed=True)
    with pytest.raises(AssertionError, match="rows for M"):
        check_frame(ref[1], cnt[1], cap, packed[offs[1]:offs[2] - 1], 0, packed=True)


def test_checker_rejects_a_record_in_the_next_frames_rows():
    """Frame 0 holds 486 records: at M = 700 its rows 486 ... 699 must keep their poison, and a record of frame 5 that
    landed there (or in row 0 of the frame behind it) is found."""
    ref, _, cnt = uncapped()
    rows0, n0, _ = oracle_at(0, 700)
    check_frame(ref[0], cnt[0], 700, rows0, 0, num_pts=n0)
    for row in (486, 699):
        bad = rows0.copy()
        bad[row] = ref[5][3]
        with pytest.raises(AssertionError, match="behind row 486 were written"):
            check_frame(ref[0], cnt[0], 700, bad, 0, num_pts=n0)
    bad = rows0.copy()
    cc.words(bad)[600, 130] = 0                                      # a single word
    with pytest.raises(AssertionError, match="behind row 486 were written"):
        check_frame(ref[0], cnt[0], 700, bad, 0, num_pts=n0)
    rows1, n1, _ = oracle_at(1, 700)                                 # a full frame: the stray record replaces one of its own
    bad = rows1.copy()
    bad[0] = ref[0][699 % 486]
    with pytest.raises(AssertionError, match="row 0 .* is no record"):
        check_frame(ref[1], cnt[1], 700, bad, 0, num_pts=n1)


def test_checker_rejects_wrong_counters():
    _, _, cnt = uncapped()
    c = cnt[F].astype(np.int64)
    check_counters(c, c, M)
    low = c.copy()
    low[8:10] = M - 1                                                # a word that must be >= M
    with pytest.raises(AssertionError):
        check_counters(low, c, M)
    moved = c.copy()
    moved[6] += 1                                                    # a word below M
    with pytest.raises(AssertionError):
        check_counters(moved, c, M)
    drop = c.copy()
    drop[8:10] = M                                                   # dropped detections not counted
    with pytest.raises(AssertionError):
        check_counters(drop, c, M)
