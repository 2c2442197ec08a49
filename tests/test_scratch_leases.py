"""The lease bookkeeping of the per-context scratch pool (gsearch_amd/csrc/gs_scratch.hpp), driven directly: a few lines of host C++ compiled with g++,
no HIP and no device. PoolBuf (gs_internal.hpp) is this lease plus the device allocation of the slot."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
GS_OK, GS_ERR_STATE = 0, -4


@pytest.fixture(scope="module")
def sl(tmp_path_factory):
    cxx = shutil.which("g++") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("leases") / "libscratch_leases.so")
    # -Bsymbolic: the shim's own gs::set_error, not the one of a libgsearch_amd.so that another test of the session has loaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", so, os.path.join(_HERE, "scratch_leases_shim.cpp")])
    L = C.CDLL(so)
    L.sl_name.restype = L.sl_last_error.restype = C.c_char_p
    L.sl_pool_new.restype = L.sl_lease_new.restype = C.c_void_p
    for f in (L.sl_pool_delete, L.sl_lease_give, L.sl_lease_delete):
        f.argtypes, f.restype = [C.c_void_p], None
    L.sl_pool_held.argtypes = [C.c_void_p, C.c_int]
    L.sl_lease_take.argtypes = [C.c_void_p, C.c_void_p]
    L.sl_lease_take_fresh.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    return L


def _slot(sl, name):
    names = [sl.sl_name(i).decode() for i in range(sl.sl_count())]
    assert len(set(names)) == len(names) and "?" not in names
    return names.index(name)


def test_take_hold_give(sl):
    s = _slot(sl, "PROB_Q")
    pool, a, b = sl.sl_pool_new(), sl.sl_lease_new(s), sl.sl_lease_new(s)
    assert sl.sl_lease_take(a, pool) == GS_OK and sl.sl_pool_held(pool, s) == 1          # a free slot
    assert sl.sl_lease_take(a, pool) == GS_OK                                            # again through the same object: allowed
    assert sl.sl_lease_take(b, pool) == GS_ERR_STATE                                     # held by another
    assert "PROB_Q" in sl.sl_last_error().decode()
    other = sl.sl_lease_new(s + 1)
    assert sl.sl_lease_take(other, pool) == GS_OK                                        # the neighbour is not affected
    sl.sl_lease_give(a)
    assert sl.sl_pool_held(pool, s) == 0
    assert sl.sl_lease_take(b, pool) == GS_OK and sl.sl_pool_held(pool, s) == 1          # given back = free again
    sl.sl_lease_delete(b)                                                                # the end of a scope gives back too
    assert sl.sl_pool_held(pool, s) == 0 and sl.sl_pool_held(pool, s + 1) == 1
    for l in (a, other):
        sl.sl_lease_delete(l)
    sl.sl_pool_delete(pool)


def test_pools_are_independent(sl):
    s = _slot(sl, "SK_REC_UNITS")
    p1, p2 = sl.sl_pool_new(), sl.sl_pool_new()
    a, b = sl.sl_lease_new(s), sl.sl_lease_new(s)
    assert sl.sl_lease_take(a, p1) == GS_OK
    assert sl.sl_lease_take(b, p2) == GS_OK                                              # a second context's pool
    assert sl.sl_pool_held(p1, s) == 1 and sl.sl_pool_held(p2, s) == 1
    sl.sl_lease_delete(a)
    assert sl.sl_pool_held(p1, s) == 0 and sl.sl_pool_held(p2, s) == 1
    sl.sl_lease_delete(b)
    for p in (p1, p2):
        sl.sl_pool_delete(p)


def test_give_back_after_the_pool_is_deleted(sl):
    s = _slot(sl, "HMH_LIST_REL")
    old, a = sl.sl_pool_new(), sl.sl_lease_new(s)
    assert sl.sl_lease_take(a, old) == GS_OK
    sl.sl_pool_delete(old)                                                               # gs_ctx_release_scratch / on_worker_failed under a live lease
    new, b = sl.sl_pool_new(), sl.sl_lease_new(s)                                        # the next call of the context makes a new pool
    assert sl.sl_pool_held(new, s) == 0
    assert sl.sl_lease_take(b, new) == GS_OK
    sl.sl_lease_give(a)                                                                  # does nothing: not to the deleted pool, not to the new one
    assert sl.sl_pool_held(new, s) == 1
    assert sl.sl_lease_take(a, new) == GS_ERR_STATE and "HMH_LIST_REL" in sl.sl_last_error().decode()
    sl.sl_lease_delete(a)
    assert sl.sl_pool_held(new, s) == 1
    sl.sl_lease_delete(b)
    assert sl.sl_pool_held(new, s) == 0
    sl.sl_pool_delete(new)


def test_take_reports_whether_the_lease_is_new(sl):
    """PoolBuf::alloc fills a slot for gs_debug_mem_fill when its call is the one that took the lease, and only then: a second alloc through the same
    object keeps its content"""
    s = _slot(sl, "BIGSI_BITMAP")
    pool, a, b = sl.sl_pool_new(), sl.sl_lease_new(s), sl.sl_lease_new(s)
    fresh = C.c_int(-1)
    assert sl.sl_lease_take_fresh(a, pool, C.byref(fresh)) == GS_OK and fresh.value == 1       # the first take
    assert sl.sl_lease_take_fresh(a, pool, C.byref(fresh)) == GS_OK and fresh.value == 0       # again through the same object: not new
    assert sl.sl_lease_take(a, pool) == GS_OK and sl.sl_pool_held(pool, s) == 1                # (the plain form is unchanged)
    fresh.value = -1
    assert sl.sl_lease_take_fresh(b, pool, C.byref(fresh)) == GS_ERR_STATE and fresh.value == 0   # refused: nothing was taken
    sl.sl_lease_give(a)
    assert sl.sl_lease_take_fresh(a, pool, C.byref(fresh)) == GS_OK and fresh.value == 1       # given back and taken again: new
    sl.sl_lease_give(a)
    assert sl.sl_lease_take_fresh(b, pool, C.byref(fresh)) == GS_OK and fresh.value == 1       # another object after it
    other_pool = sl.sl_pool_new()
    assert sl.sl_lease_take_fresh(b, other_pool, C.byref(fresh)) == GS_OK and fresh.value == 1  # moved to another pool's table: new there
    assert sl.sl_pool_held(pool, s) == 0 and sl.sl_pool_held(other_pool, s) == 1
    for l in (a, b):
        sl.sl_lease_delete(l)
    for p in (pool, other_pool):
        sl.sl_pool_delete(p)
