"""8-bit descriptors, host-only: misift_test_quantize runs the rule misift_quantize_batch's kernel runs (quantize_i8.hpp)
and must equal its numpy restatement; misift_test_match_i8_plan is the work list of misift_match_batch_i8's plan kernel,
which must cover every (pair, 128-row block, 32-column tile) exactly once and stay within the partials bound."""
import ctypes as C

import numpy as np

from batch_util import check_pair_plan, quantize_np


def _quantize(d):
    from cudasift_amd import capi
    d = np.ascontiguousarray(d, np.float32)
    out = np.full(d.shape, 99, np.int8)
    assert capi.lib().misift_test_quantize(d.ctypes.data, d.size, out.ctypes.data) == 0
    return out


def test_quantize_random_matches_numpy():
    rng = np.random.default_rng(5)
    d = np.concatenate([rng.random(200000, dtype=np.float32) * 0.6,             # SIFT range and past saturation
                        rng.normal(0, 1, 50000).astype(np.float32),
                        (rng.integers(0, 256, 20000) / np.float32(512)).astype(np.float32)])   # exact halves
    assert np.array_equal(_quantize(d), quantize_np(d))


def test_quantize_edges():
    f32 = np.float32
    cases = {126.5 / 256: 126, 127.5 / 256: 127, 125.5 / 256: 126, 0.5 / 256: 0, 1.5 / 256: 2, 2.5 / 256: 2,
             0.5: 127, 1.0: 127, -0.0: 0, 0.0: 0, -1e-30: 0, -0.5: 0, -1.0: 0, float("inf"): 127, float("-inf"): 0,
             float("nan"): 0, 1e-45: 0, 1e-39: 0, -1e-39: 0, 0.49609375: 127, 0.4921875: 126, 3e38: 127}
    d = np.array(list(cases), f32)
    want = np.array(list(cases.values()), np.int8)
    got = _quantize(d)
    assert np.array_equal(got, want), [(float(a), int(b), int(c)) for a, b, c in zip(d, got, want) if b != c]
    assert np.array_equal(got, quantize_np(d))
    # every NaN payload and sign
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FBFFFFF], np.uint32).view(f32)
    assert (_quantize(nans) == 0).all()


def test_quantize_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    assert L.misift_test_quantize(None, 0, None) == 0
    assert L.misift_test_quantize(None, -1, None) == -1
    assert L.misift_test_quantize(None, 4, None) == -1


def _plan(L, cus, n1, n2):
    n1 = np.ascontiguousarray(n1, np.int32)
    n2 = np.ascontiguousarray(n2, np.int32)
    out = np.zeros((max(len(n1), 1), 5), np.int32)
    ni, ch, bound = C.c_int(), C.c_int(), C.c_int()
    assert L.misift_test_match_i8_plan(cus, len(n1), n1.ctypes.data, n2.ctypes.data, out.ctypes.data, C.byref(ni),
                                       C.byref(ch), C.byref(bound)) == 0
    return out[:len(n1)], ni.value, ch.value, bound.value


def _check_i8_plan(L, cus, n1, n2):
    plan, nitems, chunks, bound = _plan(L, cus, n1, n2)
    rows_total = check_pair_plan(plan, nitems, chunks, n1, n2, lambda b: (b + 31) // 32)    # every column takes part
    target = 16 * cus                                         # 4 rounds of a grid of 4 workgroups per CU
    assert bound == 2 * target
    if rows_total >= target:
        assert chunks == 1                                    # enough row blocks: no partials at all
    else:
        assert nitems <= bound                                # the partials buffer the host allocates holds them all
    return nitems, chunks


def test_match_i8_plan_covers_every_block_once():
    from cudasift_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(12)
    sizes = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, -1]
    cases = [(sizes, sizes[::-1]), ([2000] * 64, [2000] * 64), ([2000] * 8, [2000] * 8), ([2000] * 256, [2100] * 256),
             ([0] * 10, [5] * 10), ([], []), ([1], [1]), ([100000], [100000]), ([64], [60000]), ([20] * 3, [20] * 3)]
    cases += [(rng.integers(-1, 5000, n), rng.integers(-1, 5000, n)) for n in (1, 3, 8, 40, 300, 1500)]
    for cus in (256, 304, 80, 1):
        for n1, n2 in cases:
            _check_i8_plan(L, cus, n1, n2)


def test_match_i8_plan_chunks_only_small_calls():
    from cudasift_amd import capi
    L = capi.lib()
    _, _, chunks, _ = _plan(L, 256, [2000] * 256, [2000] * 256)     # 4096 row blocks: a full target
    assert chunks == 1
    _, nitems, chunks, bound = _plan(L, 256, [100000], [100000])    # 782 row blocks: columns cut
    assert chunks > 1 and nitems <= bound
    _, nitems, chunks, bound = _plan(L, 256, [64], [60000])         # one row block, 1875 tiles
    assert chunks > 1 and nitems <= bound
