"""The expected output tests/test_gpu_match_pairs.py holds misift_match_pairs_batch to (batch_util.expected_pair: the
oracle's forward match and, with mutual, the oracle's reversed match) against brute force on small hand-made cases with ties.  Descriptors
are small integers, so every score is exact in fp32 whatever the summation order."""
import numpy as np
import pytest

from batch_util import expected_pair
from synth import descriptors_to_points


def _points(d):
    from cudasift_amd import capi
    p = descriptors_to_points(np.asarray(d, np.float32), capi.POINT_DTYPE)
    p["xpos"] = np.arange(len(d), dtype=np.float32) + 0.5
    p["ypos"] = -np.arange(len(d), dtype=np.float32)
    return p


def _brute(d1, d2, full, mutual):
    """match per row: the first column of the largest score > 0 among the columns that take part (all with full, else
    32 * floor(n2 / 32)); with mutual, kept only when that row is the first row of the largest score > 0 of its column."""
    S = np.asarray(d1, np.float64) @ np.asarray(d2, np.float64).T
    ncols = len(d2) if full else 32 * (len(d2) // 32)
    m = np.full(len(d1), -1)
    for r in range(len(d1)):
        row = S[r, :ncols]
        if ncols and row.max() > 0:
            m[r] = int(np.argmax(row))
    if mutual:
        for r in range(len(d1)):
            if m[r] >= 0:
                col = S[:, m[r]]
                if int(np.argmax(col)) != r:
                    m[r] = -1
    return m


def _case(seed, n1, n2):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 3, (n1, 128)).astype(np.float32)
    d2 = rng.integers(0, 3, (n2, 128)).astype(np.float32)
    d1[1] = d1[0]                      # duplicate rows: row 0 wins their column
    d1[5] = d2[2]
    d1[6] = d2[2]                      # two rows equal to a column
    d2[7] = d2[2]                      # and a duplicate of that column: the smaller column wins the row
    d1[3] = 0                          # all-zero row: scores 0, no match
    d1[4] = -d1[8]                     # negative scores only
    d2[9] = d1[10] * 2                 # a column far ahead for one row
    d2[11] = d2[9]
    return d1, d2


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("n1,n2", [(12, 40), (40, 12), (33, 64), (20, 20)])
def test_expected_rule_matches_brute_force(full, n1, n2):
    d1, d2 = _case(n1 * 100 + n2, n1, n2)
    p1, p2 = _points(d1), _points(d2)
    for mutual in (0, 1):
        e, k = expected_pair(p1, p2, full, True, mutual)
        want = _brute(d1, d2, full, mutual)
        assert np.array_equal(e["match"], want), (mutual, e["match"], want)
        assert k == int((want >= 0).sum())
        assert np.array_equal(e["xpos"], p1["xpos"]) and np.array_equal(e["ypos"], p1["ypos"])
        gone = want < 0
        assert (e["score"][gone & (_brute(d1, d2, full, 0) >= 0)] == 0).all()
        assert (e["match_xpos"][gone] == 0).all() and (e["ambiguity"][gone & (_brute(d1, d2, full, 0) >= 0)] == 0).all()
        kept = ~gone
        assert np.array_equal(e["match_xpos"][kept], p2["xpos"][want[kept]])


def test_ties_resolve_to_the_smallest_index():
    d1, d2 = _case(1, 16, 40)
    p1, p2 = _points(d1), _points(d2)
    e, _ = expected_pair(p1, p2, True, True, 1)
    S = d1.astype(np.float64) @ d2.astype(np.float64).T
    if S[5].max() == S[5, 2]:
        assert e["match"][5] == 2 and e["match"][6] == -1     # rows 5 and 6 tie on column 2: row 5 keeps it
    assert e["match"][3] == -1 and e["match"][4] == -1
    if S[10].max() == S[10, 9]:
        assert e["match"][10] == 9                           # columns 9 and 11 tie: the smaller


def test_empty_sides():
    d1, d2 = _case(2, 16, 16)
    p1, p2 = _points(d1), _points(d2)
    e, k = expected_pair(p1, p2[:0], True, True, 1)
    assert k == 0 and (e["match"] == -1).all() and (e["score"] == 0).all() and np.array_equal(e["xpos"], p1["xpos"])
    e, k = expected_pair(p1[:0], p2, True, True, 1)
    assert k == 0 and len(e) == 0
