"""The three device primitives of gs_radix.hip against numpy (tests/pyref_radix.py), == on every array: the stable radix sort of 64-bit keys
(gs_debug_radix_sort_u64), the run lengths of a sorted array (gs_debug_run_lengths_u64) and the one-workgroup prefix sum (gs_debug_scan_u32). Six
operations stand on them (the sorted ProbMinHash form, FracMinHash sketches, superani's seed order, bigsig's coverage filter, the embedding's adjacency,
the gene caller's candidate order) and reach them only at the shapes their own tests happen to have. The shapes here are the kernels' own edges, built
and held to their names in tests/radix_cases.py / tests/test_radix_cases_cpu.py: a wavefront's tile of 16384 keys (n on either side of it, runs on and
across it), the 64-key step of the scatter (n % 64 in {0, 1, 63}, one digit in all lanes, 64 digits in 64 lanes), 1, 3, 4, 5 and 8 passes (the result in
either buffer), keys that tie on the sorted bits (stability), the ragged and the longer stretches of the scan. Every table runs with the fill off and on
scratch filled with 0x00 and 0xFF: the entry points size the radix scratch exactly, so a count that the histogram or the head pass does not write is read
as poison."""
import ctypes as C

import numpy as np
import pytest

import pyref_radix as R
import radix_cases as RC

pytestmark = pytest.mark.gpu
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3
FILLS = [None, 0x00, 0xFF]
CANARY64, CANARY32 = np.uint64(0xC5C5C5C5C5C5C5C5), np.uint32(0xC5C5C5C5)


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d entries differ, the first at %d (got %#x, want %#x)" % (tag, len(bad), len(want), bad[0], int(got[bad[0]]), int(want[bad[0]])))


@pytest.fixture(scope="module")
def sort_table():
    return [(c, R.sort(c["keys"], c["endbit"])) for c in RC.sort_cases()]


@pytest.fixture(scope="module")
def rle_table():
    return [(c,) + R.run_lengths(c["a"]) for c in RC.rle_cases()]


@pytest.fixture(scope="module")
def scan_table():
    return [(c,) + R.scan(c["v"]) for c in RC.scan_cases()]


@pytest.mark.parametrize("fill", FILLS)
def test_radix_sort_cases(gpu_ctx, sort_table, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for case, want in sort_table:
            keys = case["keys"].copy()
            got = G.debug_radix_sort(keys, case["endbit"], ctx=gpu_ctx)
            _same(got, want, case["name"])
            assert np.array_equal(keys, case["keys"]), case["name"]                   # the input is left alone
    finally:
        G.debug_mem_fill(None)


@pytest.mark.parametrize("fill", FILLS)
def test_run_length_cases(gpu_ctx, rle_table, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for case, want_u, want_l in rle_table:
            n, r = len(case["a"]), len(want_u)
            uniq, lens = np.full(n, CANARY64, np.uint64), np.full(n, CANARY32, np.uint32)
            got_u, got_l = G.debug_run_lengths(case["a"], ctx=gpu_ctx, out=(uniq, lens))
            assert len(got_u) == len(got_l) == r, (case["name"], len(got_u), r)
            _same(got_u, want_u, case["name"] + " keys")
            _same(got_l, want_l, case["name"] + " lengths")
            assert (uniq[r:] == CANARY64).all() and (lens[r:] == CANARY32).all(), case["name"]      # nothing from r on
    finally:
        G.debug_mem_fill(None)


@pytest.mark.parametrize("fill", FILLS)
def test_scan_cases(gpu_ctx, scan_table, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for case, want, want_total in scan_table:
            got, total = G.debug_scan(case["v"], ctx=gpu_ctx)
            _same(got, want, case["name"])
            assert total == want_total, (case["name"], total, want_total)
    finally:
        G.debug_mem_fill(None)


def test_error_codes_and_the_smallest_calls(gpu_ctx):
    L, h = gpu_ctx.L, gpu_ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    keys = np.array([9, 3, 7], np.uint64)
    out = np.full(3, CANARY64, np.uint64)
    for endbit in (0, -1, 65, 1 << 20):
        assert L.gs_debug_radix_sort_u64(h, p(keys), 3, endbit, p(out)) == GS_ERR_INVALID, endbit
    assert (out == CANARY64).all()
    for endbit in (1, 64):
        assert L.gs_debug_radix_sort_u64(h, p(keys), 3, endbit, p(out)) == 0 and out.tolist() == [3, 7, 9]
    assert L.gs_debug_radix_sort_u64(h, None, 3, 8, p(out)) == GS_ERR_INVALID and L.gs_debug_radix_sort_u64(h, p(keys), 3, 8, None) == GS_ERR_INVALID
    assert L.gs_debug_radix_sort_u64(None, p(keys), 3, 8, p(out)) == GS_ERR_INVALID
    # n = 0 writes nothing (null pointers will do), n = 1 returns the key
    out[:] = CANARY64
    assert L.gs_debug_radix_sort_u64(h, None, 0, 8, None) == 0 and L.gs_debug_radix_sort_u64(h, p(keys), 0, 64, p(out)) == 0 and (out == CANARY64).all()
    assert L.gs_debug_radix_sort_u64(h, p(keys), 1, 24, p(out)) == 0 and out[0] == 9 and (out[1:] == CANARY64).all()
    # run lengths: the primitive refuses an empty array
    uniq, lens, r = np.full(3, CANARY64, np.uint64), np.full(3, CANARY32, np.uint32), C.c_uint64(77)
    assert L.gs_debug_run_lengths_u64(h, p(keys), 0, p(uniq), p(lens), C.byref(r)) == GS_ERR_UNSUPPORTED
    assert L.gs_debug_run_lengths_u64(h, None, 0, None, None, C.byref(r)) == GS_ERR_UNSUPPORTED
    assert r.value == 77 and (uniq == CANARY64).all() and (lens == CANARY32).all()
    assert L.gs_debug_run_lengths_u64(h, p(keys), 3, p(uniq), p(lens), None) == GS_ERR_INVALID
    assert L.gs_debug_run_lengths_u64(h, None, 3, p(uniq), p(lens), C.byref(r)) == GS_ERR_INVALID
    # scan: n = 0 gives the total 0 and writes nothing
    v, s, total = np.array([5, 6, 7], np.uint32), np.full(3, CANARY32, np.uint32), C.c_uint32(77)
    assert L.gs_debug_scan_u32(h, p(v), 0, p(s), C.byref(total)) == 0 and total.value == 0 and (s == CANARY32).all()
    total.value = 77
    assert L.gs_debug_scan_u32(h, None, 0, None, C.byref(total)) == 0 and total.value == 0
    assert L.gs_debug_scan_u32(h, p(v), 3, p(s), None) == GS_ERR_INVALID and L.gs_debug_scan_u32(h, None, 3, p(s), C.byref(total)) == GS_ERR_INVALID
    assert L.gs_debug_scan_u32(h, p(v), 3, p(s), C.byref(total)) == 0 and s.tolist() == [0, 5, 11] and total.value == 18
