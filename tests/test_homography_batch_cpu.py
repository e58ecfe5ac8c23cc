"""misift_find_homography_batch draws each entry's RANSAC samples on the device from glibc's rand() restated
(cudasift_amd/csrc/libc_rand.hpp).  The host hooks run that same header code: its stream must equal this process's libc
rand() after srand, and its sample positions the reference's rejection loop (matching.cu:1041-1053) drawn from libc."""
import ctypes as C

import numpy as np
import pytest

from cudasift_amd import capi

LIBC = C.CDLL(None)
SEEDS = [0, 1, 2, 12345, 2**31 - 1, 2**31, 2**32 - 1]


def _libc_stream(seed, n):
    LIBC.srand(C.c_uint(seed))
    return np.array([LIBC.rand() for _ in range(n)], np.int32)


@pytest.mark.parametrize("seed", SEEDS)
def test_libc_rand_restated(seed):
    n = 5000
    got = np.zeros(n, np.int32)
    assert capi.lib().misift_test_libc_rand(seed, n, got.ctypes.data) == 0
    assert np.array_equal(got, _libc_stream(seed, n)), np.nonzero(got != _libc_stream(seed, n))[0][:8]


def _reference_samples(seed, num_valid, num_loops):
    """matching.cu:1041-1053 in Python, drawn from libc rand()."""
    LIBC.srand(C.c_uint(seed))
    r = LIBC.rand
    out = np.zeros((num_loops, 4), np.int32)
    for i in range(num_loops):
        p1, p2, p3, p4 = r() % num_valid, r() % num_valid, r() % num_valid, r() % num_valid
        while p2 == p1:
            p2 = r() % num_valid
        while p3 == p1 or p3 == p2:
            p3 = r() % num_valid
        while p4 == p1 or p4 == p2 or p4 == p3:
            p4 = r() % num_valid
        out[i] = (p1, p2, p3, p4)
    return out


@pytest.mark.parametrize("seed", [0, 7, 2**32 - 1])
@pytest.mark.parametrize("num_valid", [8, 9, 1000])
@pytest.mark.parametrize("num_loops", [16, 1000])
def test_homography_samples(seed, num_valid, num_loops):
    got = np.zeros((num_loops, 4), np.int32)
    assert capi.lib().misift_test_homography_samples(seed, num_valid, num_loops, got.ctypes.data) == 0
    assert np.array_equal(got, _reference_samples(seed, num_valid, num_loops))


def test_sample_modulus_large_divisors():
    """The magic-number modulus the draw uses, at divisors far from the small cases above (2^k, 2^k + 1, 2^31 - 1)."""
    for num_valid in (2**10, 2**10 + 1, 3 * 2**20 - 1, 2**30 + 1, 2**31 - 1):
        got = np.zeros((200, 4), np.int32)
        assert capi.lib().misift_test_homography_samples(99, num_valid, 200, got.ctypes.data) == 0
        assert np.array_equal(got, _reference_samples(99, num_valid, 200)), num_valid


def test_sample_hook_arguments():
    out = np.zeros(64, np.int32)
    assert capi.lib().misift_test_homography_samples(1, 7, 4, out.ctypes.data) == -1      # fewer than 8 valid points
    assert capi.lib().misift_test_homography_samples(1, 8, -1, out.ctypes.data) == -1
    assert capi.lib().misift_test_libc_rand(1, -1, out.ctypes.data) == -1
