"""The sampling rules of SPEC.md 10 as the library's C++ states them (cluster_hash, cluster_keep0, cluster_keep1 of gsearch_amd/csrc/gs_spec.hpp),
compiled for the host alone and held to known answers and to the numpy restatement: the C++ side of the coreset is pinned without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyref_cluster as R

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cluster_spec") / "libcluster_spec.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(_HERE, "cluster_spec_shim.cpp")])
    L = C.CDLL(so)
    L.cs_hash.restype, L.cs_hash.argtypes = C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint64]
    L.cs_keep0.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.cs_keep1.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    return L


def test_hash_known_answers(cs):
    """state 0 gives the published first output of SplitMix64(0); seed, round and node enter by XOR"""
    assert cs.cs_hash(0, 0, 0) == 0xE220A8397B1DCDAF
    assert cs.cs_hash(5, 0, 5) == 0xE220A8397B1DCDAF
    assert cs.cs_hash(0, 1, 1 << 56) == 0xE220A8397B1DCDAF
    assert cs.cs_hash(1 << 56, 1, 0) == 0xE220A8397B1DCDAF


def test_hash_equals_the_restatement(cs):
    rng = np.random.default_rng(3)
    for seed in (0, 0x5eed, 2 ** 64 - 1, int(rng.integers(0, 2 ** 63))):
        i = np.concatenate([np.arange(64, dtype=np.uint64), rng.integers(0, 2 ** 32, 64, dtype=np.uint64)])
        for r in (0, 1):
            want = R.h(seed, r, i)
            assert [cs.cs_hash(seed, r, int(x)) for x in i] == want.tolist()


def test_keep_rules_at_their_boundaries(cs):
    """round 0: (h >> 32) n < t0 << 32; round 1: (h >> 40) D < (t1 d0) << 24 - in integers, at the largest operands SPEC 10 admits"""
    n, t0 = 300000, 15000
    edge = (t0 << 32) // n                                   # the smallest h >> 32 that is NOT kept is ceil((t0 << 32) / n)
    first_out = -((-(t0 << 32)) // n)
    assert cs.cs_keep0((first_out - 1) << 32 | 0xFFFFFFFF, n, t0) == 1 and cs.cs_keep0(first_out << 32, n, t0) == 0 and edge <= first_out
    assert cs.cs_keep0(2 ** 64 - 1, n, n) == 1 and cs.cs_keep0(0, n, 0) == 0
    # n m just below 2^40: D and t1 d0 just below 2^40, h >> 40 up to 2^24 - 1
    D, t1, d0 = 2 ** 40 - 1, 2 ** 24 - 1, 65535
    for top in (0, 1, 2 ** 23, 2 ** 24 - 1):
        assert cs.cs_keep1(top << 40, D, t1, d0) == int(top * D < (t1 * d0) << 24)
    assert cs.cs_keep1(0, 5, 5, 0) == 0 and cs.cs_keep1(1 << 40, 0, 5, 0) == 0
    # D = 0 means every d0 is 0: nothing is drawn
    assert cs.cs_keep1(123 << 40, 0, 5, 0) == 0


def test_round_0_equals_the_restatement(cs):
    """the members of round 0 that the probability rule picks, for the shapes of the tests: C++ against numpy"""
    for n, t0, seed in ((400, 50, 0), (1000, 125, 11), (9, 5, 2)):
        i = np.arange(n, dtype=np.uint64)
        want = (R.h(seed, 0, i) >> np.uint64(32)) * np.uint64(n) < (np.uint64(t0) << np.uint64(32))
        got = [cs.cs_keep0(cs.cs_hash(seed, 0, int(x)), n, t0) for x in i]
        assert got == want.astype(int).tolist()
