"""The rule by which the two host drivers of the DistHamming kernels split the row words of a small problem over blockIdx.z
(gsearch_amd/csrc/gs_hamming_split.hpp), compiled with the host compiler alone and held against its restatement in tests/hamming_cases.py: every
row-word count 1..131072 x 1..512 tiles (items) x n_cu in {1, 64, 256, 304}, both forms. Where the rule splits, a part is a positive number of whole
K-chunks and none is empty - part z owns the words [z * ksplit, min((z + 1) * ksplit, roww)), and in the work-list form a part takes
(its words' elements - its mismatches) off a counter, so an empty part would wrap that subtraction - and it splits only under the conditions the
header's comment documents."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hamming_cases as HC

_HERE = os.path.dirname(os.path.abspath(__file__))
ROWW_MAX, UNITS_MAX, N_CUS = 131072, 512, (1, 64, 256, 304)


@pytest.fixture(scope="module")
def hs(tmp_path_factory):
    cxx = shutil.which("g++") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("hs") / "libhs.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(_HERE, "hamming_split_shim.cpp")])
    L = C.CDLL(so)
    L.hs_geometry.restype = None
    L.hs_geometry.argtypes = [C.c_void_p]
    L.hs_fill.restype = None
    L.hs_fill.argtypes = [C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    return L


def test_geometry(hs):
    g = np.zeros(4, np.int32)
    hs.hs_geometry(g.ctypes.data)
    assert g.tolist() == [HC.HT, HC.HKW, HC.HTQ, HC.HTR] == [128, 32, 16, 4]


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n_cu", N_CUS)
def test_split_rule_everywhere(hs, n_cu, form):
    roww = np.arange(1, ROWW_MAX + 1, dtype=np.int64)
    ks, parts = np.zeros(ROWW_MAX, np.uint32), np.zeros(ROWW_MAX, np.uint32)
    n_split = 0
    for units in range(1, UNITS_MAX + 1):
        hs.hs_fill(n_cu, form, units, ROWW_MAX, ks.ctypes.data, parts.ctypes.data)
        k, p = ks.astype(np.int64), parts.astype(np.int64)
        want_k, want_p = HC.split_rule(n_cu, units, roww, form)
        assert np.array_equal(k, want_k) and np.array_equal(p, want_p), (n_cu, form, units)
        split = p > 1
        assert np.array_equal(split, k > 0), (n_cu, form, units)                      # one part = no split, and the other way round
        # only under the documented conditions
        a, b, f = HC.SPLIT_FORMS[form]
        allowed = (units * a <= n_cu * b) and (n_cu * f // units > 1)
        assert not split.any() or allowed, (n_cu, form, units)
        assert not (split & ((roww < 8 * HC.HKW) | (roww // (4 * HC.HKW) < 2))).any(), (n_cu, form, units)
        if allowed:
            assert split[roww >= 8 * HC.HKW].all(), (n_cu, form, units)                 # ... and always under them
        ksp, psp, rsp = k[split], p[split], roww[split]
        assert (ksp > 0).all() and (ksp % HC.HKW == 0).all(), (n_cu, form, units)
        assert ((psp - 1) * ksp < rsp).all() and (rsp <= psp * ksp).all(), (n_cu, form, units)   # no part is empty, the parts cover the row
        assert (ksp >= 4 * HC.HKW).all(), (n_cu, form, units)                           # a part is at least 128 words
        n_split += int(split.sum())
    assert (n_split > 0) == (n_cu > 1 or form == 1)        # one compute unit: the dense form never splits (2 tiles' worth of units at most), the work-list form does at one item


def test_shorter_last_part_exists(hs):
    """the cases of the GPU table rely on it: a split whose last part is shorter than the others, and one whose parts are all equal"""
    for roww, units, form in ((257, 1, 0), (300, 4, 0), (515, 1, 1), (256, 1, 0)):
        k, p = HC.split_rule(256, units, np.array([roww]), form)
        assert p[0] > 1 and ((roww % k[0] != 0) == (roww != 256)), (roww, units, form)
