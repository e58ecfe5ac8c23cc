"""orc_match_core, the blocked oracle matcher tests/test_gpu_match_full_size.py checks the 100 000 x 100 000 calls
against: bit-identical to a plain loop over orc_dot128 with a restated top-2 and class merge (ragged and tiny shapes,
zero and negative rows, ties inside a 32-column slab and across slabs), its per-column best equal to the reversed
MatchSiftData, its integer top-2 equal to the int8 contract, and within a rigorous fp32 bound of float64 at full size.
The GPU module's comparison (batch_util.same_rows) must reject a single wrong index, a score one ulp off and a tie
resolved the wrong way."""
import numpy as np
import pytest

from batch_util import i8_records, match_np, orc, quantize_np, same_rows
from synth import descriptors_to_points, synth_descriptors


def _plain(a, b):
    """The score matrix pair by pair through orc_dot128, then the two modes restated row by row."""
    import ctypes as C
    o = orc()
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    n1, n2 = len(a), len(b)
    S = np.zeros((n1, n2), np.float32)
    for i in range(n1):
        for j in range(n2):
            S[i, j] = o.lib().orc_dot128(a[i].ctypes.data_as(C.c_void_p), b[j].ctypes.data_as(C.c_void_p))
    r = {k: np.zeros(n1, np.int32 if k.endswith("idx") else np.float32)
         for k in ("cls_best", "cls_idx", "cls_sec", "ex_best", "ex_idx", "ex_sec")}
    ncls = 32 * (n2 // 32)
    for i in range(n1):
        em, es, ei = np.float32(0), np.float32(0), -1
        cm, cs, ci = [np.float32(0)] * 8, [np.float32(0)] * 8, [-1] * 8
        for j in range(n2):
            s = S[i, j]
            if s > em:
                em, es, ei = s, em, j
            elif s > es:
                es = s
            if j < ncls:
                c = (j % 32) // 4
                if s > cm[c]:
                    cm[c], cs[c], ci[c] = s, cm[c], j
                elif s > cs[c]:
                    cs[c] = s
        m, sec, idx = cm[0], cs[0], ci[0]
        for y in range(8):
            if idx != ci[y]:
                if cm[y] > m:
                    sec, m, idx = max(m, sec), cm[y], ci[y]
                elif cm[y] > sec:
                    sec = cm[y]
        r["ex_best"][i], r["ex_sec"][i], r["ex_idx"][i] = em, es, ei
        r["cls_best"][i], r["cls_sec"][i], r["cls_idx"][i] = m, sec, idx
    pos = np.where(S > 0, S, 0)
    col_best = pos.max(0) if n1 else np.zeros(n2, np.float32)
    col_row = np.where(col_best > 0, pos.argmax(0), -1) if n1 else np.full(n2, -1)
    return r, S, col_best.astype(np.float32), col_row.astype(np.int32)


def _tie_sets(n1, n2, seed):
    """Descriptors with zero and negative rows, and duplicate columns inside one slab, across a slab edge and far apart."""
    rng = np.random.default_rng(seed)
    a = synth_descriptors(n1, seed)
    b = synth_descriptors(n2, seed + 1)
    if n1 > 3:
        a[1] = 0
        a[2] = -a[2]
        a[3] = b[min(5, n2 - 1)]                   # row 3's best: column 5 or a copy of it
    if n2 > 40:
        b[7] = b[5]                                 # one slab, another class
        b[6] = b[5]                                 # one slab, the same class
        b[33] = b[31]                               # across a slab edge
        b[32] = b[31]
        b[n2 - 1] = b[31]                           # the ragged tail
    if n1 > 6 and n2 > 40:
        a[6] = b[31]
        a[5] = a[6]                                 # a column's best row is a tie too
    b[rng.integers(0, n2, 2)] *= -1                 # negative columns
    return a, b


def _cmp(got, exp):
    for k in exp:
        assert np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes(), k


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 31), (3, 32), (9, 33), (40, 95), (70, 130), (261, 67), (5, 300)])
def test_core_equals_plain_loop(n1, n2):
    a, b = _tie_sets(n1, n2, 7 + n1 + n2)
    exp, _, col_best, col_row = _plain(a, b)
    got = orc().match_core(a, b)
    _cmp({k: got[k] for k in exp}, exp)
    assert np.array_equal(got["col_best"].view(np.uint32), col_best.view(np.uint32))
    assert np.array_equal(got["col_row"], col_row)
    if n1 > 6 and n2 > 40:                          # the planted ties are ties
        assert got["ex_idx"][6] == 31 and got["ex_sec"][6] == got["ex_best"][6]
        assert got["col_row"][31] == got["col_row"][32] == 5
        assert got["ex_idx"][1] == -1 and got["ex_best"][1] == 0 and got["cls_idx"][1] == -1


@pytest.mark.parametrize("threads", [1, 3])
def test_core_does_not_depend_on_threads(threads):
    """The row ranges per thread and the merge of the per-thread column states leave no trace in the result."""
    import ctypes as C
    a, b = _tie_sets(600, 250, 3)
    a[300:] = a[:300]                               # every column's best row has a twin in another thread's range
    ref = orc().match_core(a, b)
    set_threads = C.CDLL("libgomp.so.1").omp_set_num_threads      # the runtime liboracle.so is linked against
    set_threads(threads)
    try:
        got = orc().match_core(a, b)
    finally:
        set_threads(orc().cpu_budget())
    _cmp(got, ref)
    assert (ref["col_row"][ref["col_row"] >= 0] < 300).all()


@pytest.mark.parametrize("n1,n2", [(50, 97), (300, 64), (33, 1)])
def test_core_rows_match_reference_matcher(n1, n2):
    """orc_match_rows runs on the core: the records equal match_records of one core pass in both modes, and the
    per-column best is the reversed full + exact match."""
    from cudasift_amd.capi import POINT_DTYPE
    o = orc()
    a, b = _tie_sets(n1, n2, 11)
    p1, p2 = descriptors_to_points(a, POINT_DTYPE), descriptors_to_points(b, POINT_DTYPE)
    core = o.match_core(a, b)
    for exact in (False, True):
        m = p1.copy()
        o.match(m, n1, p2, n2, full=exact, exact=exact)
        assert m.tobytes() == o.match_records(p1, p2, core, exact).tobytes(), exact
    rv = p2.copy()
    o.match(rv, n2, p1, n1, full=True, exact=True)
    assert np.array_equal(rv["match"], core["col_row"])
    assert np.array_equal(rv["score"].view(np.uint32), core["col_best"].view(np.uint32))


def test_core_integer_top2_equals_int8_contract():
    """q as float32: every partial sum is an exact integer, so the exact top-2 is the int8 matcher's (match_np)."""
    from cudasift_amd.capi import POINT_DTYPE
    o = orc()
    rng = np.random.default_rng(5)
    d1, d2 = synth_descriptors(300, 21, l2=True), synth_descriptors(700, 22, l2=True)
    d1[0] = 0                                       # all-zero row
    d2[40] = d2[700 - 1] = d2[9]                    # ties (q equal too)
    d1[1] = d2[9]
    q1, q2 = quantize_np(d1), quantize_np(d2)
    q1[2] = 127                                     # the largest score: 128 * 127^2 < 2^24
    q2[3] = q2[50] = 127                            # every row's best: a tie of columns 3 and 50
    p1, p2 = descriptors_to_points(d1, POINT_DTYPE), descriptors_to_points(d2, POINT_DTYPE)
    p2["xpos"] = rng.random(700, dtype=np.float32) * 500
    exp = match_np(p1, q1, p2, q2)
    core = o.match_core(q1.astype(np.float32), q2.astype(np.float32), columns=False)
    got = i8_records(p1, p2, core)
    assert got.tobytes() == exp.tobytes()
    assert core["ex_idx"][0] == -1 and (core["ex_idx"][1:] == 3).all() and (core["ex_best"] == core["ex_sec"]).all()
    assert core["ex_best"][2] == 128 * 127 * 127


def test_core_within_fp32_bound_of_float64_at_scale():
    """2048 rows of bench.py's sets against all 100 000 columns: every score lies within the fp32 chain's bound
    gamma_128 * sum |a_k b_k| of its pair's float64 dot, and every chosen column within twice the bound of the row's
    float64 maximum."""
    o = orc()
    a, b = synth_descriptors(100000, 12345)[:2048], synth_descriptors(100000, 12346)
    core = o.match_core(a, b, columns=False)
    u = 2.0 ** -24
    gamma = 128 * u / (1 - 128 * u) + 256 * 2.0 ** -53           # the fp32 chain + the float64 reference's own error
    b64 = b.astype(np.float64)
    for r0 in range(0, 2048, 256):
        S = a[r0:r0 + 256].astype(np.float64) @ b64.T              # descriptors are >= 0: sum |a_k b_k| = S
        rows = np.arange(len(S))
        idx, best = core["ex_idx"][r0:r0 + 256], core["ex_best"][r0:r0 + 256].astype(np.float64)
        assert (idx >= 0).all()
        s_idx, s_max = S[rows, idx], S.max(1)
        assert (np.abs(best - s_idx) <= gamma * s_idx).all()
        assert (s_idx >= s_max - 2 * gamma * s_max).all()
        cidx = core["cls_idx"][r0:r0 + 256]
        assert (np.abs(core["cls_best"][r0:r0 + 256] - S[rows, cidx]) <= gamma * S[rows, cidx]).all()


def test_comparison_rejects_single_faults():
    """What the GPU module compares with: one wrong index, one score one ulp off, one tie resolved to the larger
    column — each alone fails the comparison."""
    from cudasift_amd.capi import POINT_DTYPE
    o = orc()
    a, b = _tie_sets(70, 130, 4)
    p1, p2 = descriptors_to_points(a, POINT_DTYPE), descriptors_to_points(b, POINT_DTYPE)
    core = o.match_core(a, b)
    exp = o.match_records(p1, p2, core, True)
    same_rows(exp.copy(), exp, "unchanged")
    bad = exp.copy()
    bad["match"][10] += 1
    with pytest.raises(AssertionError):
        same_rows(bad, exp, "index")
    bad = exp.copy()
    bad["score"][11] = np.nextafter(bad["score"][11], np.float32(np.inf))
    with pytest.raises(AssertionError):
        same_rows(bad, exp, "score")
    r = 6                                           # its best is the tie of columns 31 and 32: the smaller must win
    assert exp["match"][r] == 31 and core["ex_sec"][r] == core["ex_best"][r]
    bad = exp.copy()
    bad["match"][r], bad["match_xpos"][r], bad["match_ypos"][r] = 32, p2["xpos"][32], p2["ypos"][32]
    with pytest.raises(AssertionError):
        same_rows(bad, exp, "tie")
    with pytest.raises(AssertionError):
        same_rows(bad, exp, "tie", ("match",))
