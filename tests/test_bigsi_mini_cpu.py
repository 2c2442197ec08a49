"""bigsig minimizers (SPEC.md 11, "Minimizer indexes and the coverage filter") without a device: gs_bigsi_minimizers, the host form of the selection rule
the device kernel shares (gs_spec.hpp), against the numpy restatement tests/pyref_bigsi_mini.py - values and positions, ==. The restatement's naive
definition (sort every window) is the yardstick: minimizers_checked asserts that its sequential definition agrees before the library is compared."""
import numpy as np
import pytest

import gsearch_amd as G
import pyref_bigsi_mini as RM

KM = [(2, 1), (22, 21), (31, 15), (32, 1), (32, 31)]


def _seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def _same(text, k, m, data_t, qual=None, min_phred=15):
    want_v, want_p = RM.minimizers_checked(text, k, m, qual, min_phred, fwd_only=data_t == "dna_fwd")
    v, p = G.bigsi_minimizers(text, k, m, qual=qual, min_phred=min_phred, data_t=data_t)
    assert v.dtype == np.uint64 and p.dtype == np.uint64
    assert np.array_equal(v, want_v) and np.array_equal(p, want_p), (k, m, data_t, text[:40])
    return v, p


@pytest.mark.parametrize("data_t", ["dna", "dna_fwd"])
@pytest.mark.parametrize("k,m", KM)
def test_minimizers_equal_the_restatement(k, m, data_t):
    rng = np.random.default_rng(1000 * k + m)
    w = k - m + 1
    # segment lengths k - 1 (none), k (one), k + 1
    for n, lo, hi in ((k - 1, 0, 0), (k, 1, 1), (k + 1, 1, 2)):
        v, _ = _same(_seq(rng, n), k, m, data_t)
        assert lo <= len(v) <= hi
    # poly-A: every key ties, each window selects its left end
    v, p = _same(b"A" * (k + 40), k, m, data_t)
    assert len(v) == 41 and p.tolist() == list(range(41)) and (v == 0).all()
    # period 2 and period 3
    _same(b"AC" * (k + 9), k, m, data_t)
    _same(b"ACG" * (k + 5) + b"A", k, m, data_t)
    # an N in the middle; the two sides are segments of their own
    left, right = _seq(rng, k + 17), _seq(rng, k + 3)
    v, p = _same(left + b"N" + right, k, m, data_t)
    vl, pl = _same(left, k, m, data_t)
    vr, pr = _same(right, k, m, data_t)
    assert np.array_equal(v, np.concatenate([vl, vr])) and np.array_equal(p, np.concatenate([pl, pr + np.uint64(len(left) + 1)]))
    # a base below min_phred ends a segment, one at the threshold does not
    text = _seq(rng, 2 * k + 30)
    qual = bytearray(b"I" * len(text))
    qual[k + 11] = 33 + 14
    qual[5] = 33 + 15
    v, p = _same(text, k, m, data_t, qual=bytes(qual))
    assert all(not (int(x) <= k + 11 < int(x) + m) for x in p)
    # line breaks inside a window end nothing; positions are offsets in the text with the breaks
    plain = _seq(rng, 3 * k + 7)
    broken = plain[:k // 2] + b"\n" + plain[k // 2:k + 3] + b"\r\n" + plain[k + 3:]
    vb, pb = _same(broken, k, m, data_t)
    vp, _ = _same(plain, k, m, data_t)
    assert np.array_equal(vb, vp) and all(broken[int(x)] not in (10, 13) for x in pb)
    # a random 2 kbp text: about 2 / (w + 1) of the positions are selected
    v, p = _same(_seq(rng, 2000), k, m, data_t)
    assert 0.5 * 2 / (w + 1) < len(v) / (2000 - k + 1) <= 1.0


def test_count_only_calls_return_the_same_n():
    import ctypes as C
    L = G.load()
    rng = np.random.default_rng(5)
    for k, m in KM:
        for text in (_seq(rng, 2000), _seq(rng, k - 1), b"", b"A" * 50 + b"N" + _seq(rng, 64)):
            v, _ = G.bigsi_minimizers(text, k, m)
            t = np.frombuffer(text, np.uint8)
            n = C.c_uint64(12345)
            rc = L.gs_bigsi_minimizers(t.ctypes.data_as(C.c_void_p) if len(t) else None, None, len(t), 15, k, m, 0, 0, None, None, C.byref(n))
            assert rc == 0 and n.value == len(v)
            # a short buffer is filled as far as it goes and the full count comes back
            cap = len(v) // 2
            vo, po = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint64)
            rc = L.gs_bigsi_minimizers(t.ctypes.data_as(C.c_void_p) if len(t) else None, None, len(t), 15, k, m, 0, cap, vo.ctypes.data_as(C.c_void_p),
                                       po.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == 0 and n.value == len(v) and np.array_equal(vo[:cap], v[:cap])


def test_minimizer_parameters_are_checked():
    for k, m in ((21, 0), (21, 21), (21, 22), (33, 5), (0, 0)):
        with pytest.raises(G.GsError) as e:
            G.bigsi_minimizers(b"ACGT" * 20, k, m)
        assert e.value.code == -1, (k, m)
    with pytest.raises(G.GsError) as e:
        G.bigsi_minimizers(b"ACGT" * 20, 21, 11, data_t="aa")
    assert e.value.code == -1


def test_the_filter_of_the_restatement():
    v = np.array([5, 7, 5, 9, 7, 5, 1], np.uint64)
    for f in (0, 1):
        got, nk = RM.filtered(v, f)
        assert np.array_equal(got, v) and nk == 7
    got, nk = RM.filtered(v, 2)
    assert got.tolist() == [5, 7] and nk == 5
    got, nk = RM.filtered(v, 3)
    assert got.tolist() == [5] and nk == 3
    got, nk = RM.filtered(v, 4)
    assert got.tolist() == [] and nk == 0


def test_the_tile_constant_is_the_header_s():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gsearch_amd.h")).read()
    assert int(re.search(r"#define GS_BIGSI_MINI_TILE (\d+)u", hdr).group(1)) == G.BIGSI_MINI_TILE
