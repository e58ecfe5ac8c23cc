"""misift_match_pairs_batch_i8 without a GPU: the export, and the expected output the GPU tests hold it to.

expected_pair_i8 restates the contract for one pair in numpy (forward = batch_util.match_np, the mutual filter by
match_np with the sets swapped).  It is pinned here to two independent restatements: a plain-loop brute force on small
hand-made int8 cases with ties, and the oracle's blocked core on the same q as float32 (products of integers <= 127 sum
to < 2^24, so fp32 is exact)."""
import numpy as np
import pytest

from batch_util import MATCH_FIELDS, match_np, no_match_rows, orc
from synth import descriptors_to_points


def expected_pair_i8(p1, q1, p2, q2, mutual):
    """The seven output fields of one pair: forward misift_match_batch_i8 (match_np); with mutual, a row r with match
    m >= 0 keeps it only if misift_match_batch_i8 with the sets swapped gives set-2 record m the match r.  Returns the
    rows (structured, only xpos, ypos and MATCH_FIELDS meaningful) and the number with match >= 0."""
    n1, n2 = len(p1), len(p2)
    e = no_match_rows(p1)
    if n1 == 0 or n2 == 0:
        return e, 0
    fw = match_np(p1, q1, p2, q2)
    for k in MATCH_FIELDS:
        e[k] = fw[k]
    if mutual:
        rv = match_np(p2, q2, p1, q1)["match"]
        m = e["match"]
        bad = (m >= 0) & (rv[np.clip(m, 0, n2 - 1)] != np.arange(n1))
        e[bad] = no_match_rows(p1[bad])
    return e, int((e["match"] >= 0).sum())


def _points(n):
    from cudasift_amd import capi
    p = descriptors_to_points(np.zeros((n, 128), np.float32), capi.POINT_DTYPE)
    p["xpos"] = np.arange(n, dtype=np.float32) + 0.5
    p["ypos"] = -np.arange(n, dtype=np.float32)
    return p


def _brute(q1, q2, mutual):
    """Plain loops: per row the first column of the largest S > 0 and the largest S of any other column; with mutual
    the row keeps its match only when it is the first row of the largest S > 0 of that column."""
    n1, n2 = len(q1), len(q2)
    S = [[int(sum(int(a) * int(b) for a, b in zip(q1[r], q2[j]))) for j in range(n2)] for r in range(n1)]
    m, best, sec = [-1] * n1, [0] * n1, [0] * n1
    for r in range(n1):
        for j in range(n2):
            if S[r][j] > best[r]:
                best[r], m[r] = S[r][j], j
        for j in range(n2):
            if j != m[r] and S[r][j] > sec[r] and m[r] >= 0:
                sec[r] = S[r][j]
    if mutual:
        for r in range(n1):
            if m[r] >= 0:
                top, row = 0, -1
                for i in range(n1):
                    if S[i][m[r]] > top:
                        top, row = S[i][m[r]], i
                if row != r:
                    m[r], best[r], sec[r] = -1, 0, 0
    return np.array(m), np.array(best), np.array(sec)


def _case(seed, n1, n2):
    rng = np.random.default_rng(seed)
    q1 = rng.integers(0, 4, (n1, 128)).astype(np.int8)
    q2 = rng.integers(0, 4, (n2, 128)).astype(np.int8)
    q1[1] = q1[0]                      # duplicate rows: row 0 wins their column
    q1[5] = q2[2]
    q1[6] = q2[2]                      # two rows equal to a column
    q2[7] = q2[2]                      # and a duplicate of that column: the smaller column wins the row
    q1[3] = 0                          # all-zero row: scores 0, no match
    q1[4] = -q1[8]                     # negative scores only
    q2[9] = q1[10] * 2                 # a column far ahead for one row
    q2[11] = q2[9]
    return q1, q2


def test_library_exports_the_call():
    """Fails without the feature: the symbol, its row in capi.SIGNATURES, and the NULL-context check."""
    from cudasift_amd import capi
    assert "misift_match_pairs_batch_i8" in capi.SIGNATURES
    L = capi.lib()
    assert hasattr(L, "misift_match_pairs_batch_i8")
    pairs = np.zeros(2, np.int32)
    rc = L.misift_match_pairs_batch_i8(None, 1, pairs.ctypes.data, None, None, 1, None, None, 0, None, None, 1, None,
                                       None, 0, 16, 0, None, None, None)
    assert rc == -1                                             # MISIFT_EINVAL


@pytest.mark.parametrize("n1,n2", [(12, 40), (40, 12), (33, 64), (20, 20), (16, 33)])
def test_expected_rule_matches_brute_force(n1, n2):
    q1, q2 = _case(n1 * 100 + n2, n1, n2)
    p1, p2 = _points(n1), _points(n2)
    sc = np.float32(2.0 ** -16)
    for mutual in (0, 1):
        e, k = expected_pair_i8(p1, q1, p2, q2, mutual)
        m, best, sec = _brute(q1, q2, mutual)
        assert np.array_equal(e["match"], m), (mutual, e["match"], m)
        assert k == int((m >= 0).sum())
        assert np.array_equal(e["xpos"], p1["xpos"]) and np.array_equal(e["ypos"], p1["ypos"])
        score = best.astype(np.float32) * sc
        assert np.array_equal(e["score"], score)
        assert np.array_equal(e["ambiguity"], (sec.astype(np.float32) * sc) / (score + np.float32(1e-6)))
        kept = m >= 0
        assert np.array_equal(e["match_xpos"][kept], p2["xpos"][m[kept]])
        assert np.array_equal(e["match_ypos"][kept], p2["ypos"][m[kept]])
        assert (e["match_xpos"][~kept] == 0).all() and (e["match_ypos"][~kept] == 0).all()
    fw = _brute(q1, q2, 0)[0]
    assert ((fw >= 0) & (m < 0)).any() and (m >= 0).any()       # the filter both rejects and keeps rows here


def test_ties_resolve_to_the_smallest_index():
    q2 = np.zeros((8, 128), np.int8)
    for j in range(8):
        q2[j, 16 * j:16 * j + 16] = 3 + j                       # disjoint supports: S is 0 off the copies
    q2[7] = q2[2]                                               # duplicate columns 2 and 7
    q1 = np.zeros((7, 128), np.int8)
    q1[0], q1[1] = q2[0], q2[0]                                 # duplicate rows
    q1[2] = q2[3]
    q1[4] = -q2[1]                                              # negative scores only; row 3 stays all-zero
    q1[5], q1[6] = q2[2], q2[2]                                 # two rows equal to the duplicated column
    p1, p2 = _points(7), _points(8)
    f, kf = expected_pair_i8(p1, q1, p2, q2, 0)
    assert list(f["match"]) == [0, 0, 3, -1, -1, 2, 2] and kf == 5      # columns 2 and 7 tie: the smaller
    assert f["ambiguity"][5] == f["score"][5] / (f["score"][5] + np.float32(1e-6)) and f["ambiguity"][2] == 0
    e, ke = expected_pair_i8(p1, q1, p2, q2, 1)
    assert list(e["match"]) == [0, -1, 3, -1, -1, 2, -1] and ke == 3    # rows tie on a column: the smaller keeps it
    assert np.array_equal(e["match"], _brute(q1, q2, 1)[0])


def test_empty_sides():
    q1, q2 = _case(2, 16, 16)
    p1, p2 = _points(16), _points(16)
    e, k = expected_pair_i8(p1, q1, p2[:0], q2[:0], 1)
    assert k == 0 and (e["match"] == -1).all() and (e["score"] == 0).all() and np.array_equal(e["xpos"], p1["xpos"])
    assert (e["ambiguity"] == 0).all() and (e["match_xpos"] == 0).all() and (e["match_ypos"] == 0).all()
    e, k = expected_pair_i8(p1[:0], q1[:0], p2, q2, 1)
    assert k == 0 and len(e) == 0


@pytest.mark.parametrize("n1,n2,seed", [(40, 33, 3), (200, 300, 4), (257, 129, 5)])
def test_expected_rule_matches_the_oracle_core(n1, n2, seed):
    """The oracle's blocked core on q as float32: its exact top-2 is the forward rule, its col_row the reversed match."""
    rng = np.random.default_rng(seed)
    if n1 == 40:
        q1, q2 = _case(seed, n1, n2)
    else:
        q1 = rng.integers(0, 128, (n1, 128)).astype(np.int8)
        q2 = rng.integers(0, 128, (n2, 128)).astype(np.int8)
        q1[7] = q1[2]
        q2[9] = q2[4]
        q1[11] = q2[4]
        q1[20] = 0
    p1, p2 = _points(n1), _points(n2)
    core = orc().match_core(q1.astype(np.float32), q2.astype(np.float32), columns=True)
    sc = np.float32(2.0 ** -16)
    f, _ = expected_pair_i8(p1, q1, p2, q2, 0)
    assert np.array_equal(f["match"], core["ex_idx"])
    assert np.array_equal(f["score"], core["ex_best"] * sc)
    assert np.array_equal(f["ambiguity"], (core["ex_sec"] * sc) / (core["ex_best"] * sc + np.float32(1e-6)))
    e, k = expected_pair_i8(p1, q1, p2, q2, 1)
    m = core["ex_idx"]
    keep = (m >= 0) & (core["col_row"][np.maximum(m, 0)] == np.arange(n1))
    assert np.array_equal(e["match"], np.where(keep, m, -1)) and k == int(keep.sum())
    assert (e["score"][~keep] == 0).all() and np.array_equal(e["score"][keep], f["score"][keep])
    assert np.array_equal(match_np(p2, q2, p1, q1)["match"], core["col_row"])
