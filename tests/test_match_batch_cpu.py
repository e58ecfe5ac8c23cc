"""misift_test_match_batch_plan (host-only): the work list of misift_match_batch covers every (pair, 128-row block,
64-column super-tile) exactly once, cuts columns only when the row blocks of the call do not fill one round of two
workgroups per CU, and then stays within the partials bound the host allocates."""
import ctypes as C

import numpy as np

from batch_util import check_pair_plan


def _plan(L, cus, full, n1, n2):
    n1 = np.ascontiguousarray(n1, np.int32)
    n2 = np.ascontiguousarray(n2, np.int32)
    out = np.zeros((max(len(n1), 1), 5), np.int32)
    ni, ch, bound = C.c_int(), C.c_int(), C.c_int()
    assert L.misift_test_match_batch_plan(cus, full, len(n1), n1.ctypes.data, n2.ctypes.data, out.ctypes.data,
                                          C.byref(ni), C.byref(ch), C.byref(bound)) == 0
    return out[:len(n1)], ni.value, ch.value, bound.value


def _check_batch_plan(L, cus, full, n1, n2):
    plan, nitems, chunks, bound = _plan(L, cus, full, n1, n2)
    rows_total = check_pair_plan(plan, nitems, chunks, n1, n2, lambda b: ((b if full else 32 * (b // 32)) + 63) // 64)
    assert chunks >= 1
    if rows_total >= 2 * cus:
        assert chunks == 1                                    # a full round of row blocks: no partials at all
    else:
        assert nitems <= bound == 4 * cus                      # the partials buffer the host allocates holds them all
    return nitems, chunks


def test_match_batch_plan_covers_every_block_once():
    from cudasift_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(11)
    sizes = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, -1]
    cases = [(sizes, sizes[::-1]), ([2000] * 64, [2000] * 64), ([2000] * 4, [2000] * 4), ([2000] * 256, [2100] * 256),
             ([0] * 10, [5] * 10), ([], []), ([1], [1]), ([100000], [100000]), ([20] * 3, [20] * 3)]
    cases += [(rng.integers(-1, 5000, n), rng.integers(-1, 5000, n)) for n in (1, 3, 8, 40, 300, 1500)]
    for n1, n2 in cases:
        for cus in (256, 64, 304):
            for full in (0, 1):
                _check_batch_plan(L, cus, full, n1, n2)


def test_match_batch_plan_splits_small_batches_only():
    from cudasift_amd import capi
    L = capi.lib()
    _, chunks = _check_batch_plan(L, 256, 0, [2000] * 64, [2000] * 64)     # 64 x 16 row blocks: two full rounds
    assert chunks == 1
    nitems, chunks = _check_batch_plan(L, 256, 0, [2000] * 4, [2000] * 4)  # 64 row blocks: columns cut to fill 512 slots
    assert chunks == 8 and nitems == 4 * 16 * 8
    assert _check_batch_plan(L, 256, 0, [], [])[0] == 0


def test_match_batch_plan_rejects_bad_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    ni, ch, bound = C.c_int(), C.c_int(), C.c_int()
    assert L.misift_test_match_batch_plan(256, 0, -1, None, None, None, C.byref(ni), C.byref(ch), C.byref(bound)) != 0
    assert L.misift_test_match_batch_plan(256, 0, 2, None, None, None, C.byref(ni), C.byref(ch), C.byref(bound)) != 0
