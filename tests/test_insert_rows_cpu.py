"""The row planner of parallel_insert (gsearch_amd/csrc/gs_insert_rows.hpp: where the count rows of a dense insert batch go, and which join fills them),
driven directly: a few lines of host C++ compiled with g++, no HIP and no device. Every answer over 12 000 random insert calls is compared with
`_old_loop` below, a restatement of the batch loop insert_common had before the planner existed (the variables grp_b0, grp_end, can_group, slab,
slab_first and the condition `b0 >= grp_b0 && b0 < grp_end`, spelled four times there). `_old_loop` does not call into the header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
DENSE, HAVE_SLAB, CAN_GROUP, SLAB_TAKEN, RESET_AFTER = 1, 2, 4, 8, 16
JOIN_GROUP, JOIN_RANGE, JOIN_ALONE = 0, 1, 2
N_PLANS = 12000


@pytest.fixture(scope="module")
def ir(tmp_path_factory):
    cxx = shutil.which("g++") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("insert_rows") / "libinsert_rows.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(_HERE, "insert_rows_shim.cpp")])
    L = C.CDLL(so)
    L.ir_run.restype = C.c_longlong
    L.ir_run.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    return L


def _plan(rng):
    """One insert call: nodes [first, first + n) in batches of B, and what every batch meets."""
    B = int(rng.choice([1, 16, 64, 256]))
    nbatch = int(rng.integers(1, 41))
    n = (nbatch - 1) * B + int(rng.integers(1, B + 1))                 # a short last batch more often than not
    first = int(rng.choice([0, 1, 4095, 4096, 4097, int(rng.integers(0, 1 << 20)), (1 << 32) - 2 - n - int(rng.integers(0, 1000))]))
    grp_n = int(rng.integers(1, 13))
    kind = rng.integers(0, 4)                                           # all batches dense / dense from some batch on / dense at random (the cost model's verdict)
    dense = np.ones(nbatch, bool) if kind == 0 else np.arange(nbatch) >= rng.integers(0, nbatch) if kind < 3 else rng.random(nbatch) < 0.7
    allowed = bool(rng.integers(0, 2))                                  # GS_INSERT_GROUP > 1 and the join in use
    can_group = np.full(nbatch, allowed) if rng.random() < 0.8 else rng.random(nbatch) < 0.5
    slab = bool(rng.integers(0, 2))                                     # the call gets a slab of the pair cache at its first dense batch
    # the pair cache is given back at one batch (or never): before the batch's rows are placed (ensure_cols), or while its join runs (dense_counts)
    evict_at = int(rng.integers(0, nbatch)) if rng.random() < 0.6 else -1
    evict_in_join = bool(rng.integers(0, 2))
    return dict(first=first, n=n, B=B, grp_n=grp_n, dense=dense, can_group=can_group, slab=slab, evict_at=evict_at, evict_in_join=evict_in_join)


def _old_loop(p):
    """The part of the old batch loop that placed a batch's count rows and chose its join, statement for statement. Returns, per dense batch,
    (row offset of out16 in the slab or in ix->mat, rows the buffer may grow to or 0, join, rows joined, node0, nodes) and whether the batch's
    counts were produced again after an eviction."""
    first, n, B, grp_n = p["first"], p["n"], p["B"], p["grp_n"]
    grp_b0 = grp_end = 0
    slab, slab_first, slab_tried, slabs = False, 0, False, 0            # slabs: len(ix->slabs)
    out = {}
    for i, b0 in enumerate(range(first, first + n, B)):
        nb = min(B, first + n - b0)
        if not p["dense"][i]:
            continue
        if i == p["evict_at"] and not p["evict_in_join"]:
            slabs = 0                                                   # drop_pair_cache under ensure_cols
        if slab and slabs == 0:
            slab = False
        if not slab_tried:
            slab_tried = True
            if p["slab"]:
                slab, slab_first, slabs = True, b0, slabs + 1
        can_group = bool(p["can_group"][i])
        grow = 0
        if slab:
            off = b0 - slab_first
        else:
            rows_wanted = grp_n * B if can_group else B
            if not (b0 >= grp_b0 and b0 < grp_end):
                grow = rows_wanted
            off = b0 - grp_b0 if (b0 >= grp_b0 and b0 < grp_end) else 0
        if can_group and b0 >= grp_b0 and b0 < grp_end:
            join = (JOIN_RANGE, nb, grp_b0, b0 - grp_b0)
        elif can_group:
            grp_b0, grp_end = b0, min(first + n, b0 + grp_n * B)
            join = (JOIN_GROUP, grp_end - grp_b0, 0, 0)
        else:
            grp_b0 = grp_end = 0
            join = (JOIN_ALONE, nb, 0, 0)
        if i == p["evict_at"] and p["evict_in_join"]:
            slabs = 0                                                   # drop_pair_cache under dense_counts
        again = slab and slabs == 0
        if again:
            slab = False
            grp_b0 = grp_end = 0
        out[i] = ((off, grow) + join, again)
    return out


def _drive(ir, p):
    """What InsertCall feeds the planner for the same call: the environment of every batch, worked out here (not taken from _old_loop)."""
    nbatch = len(p["dense"])
    flags = np.zeros(nbatch, np.uint8)
    taken = gone = False                                                # this call took a slab; the cache was given back since
    for i in range(nbatch):
        if not p["dense"][i]:
            continue
        f = DENSE | (CAN_GROUP if p["can_group"][i] else 0)
        if i == p["evict_at"] and not p["evict_in_join"] and taken:
            gone = True
        if p["slab"] and not taken and not np.any(p["dense"][:i]):
            taken, f = True, f | SLAB_TAKEN
        if taken and not gone:
            f |= HAVE_SLAB
            if i == p["evict_at"] and p["evict_in_join"]:
                gone, f = True, f | RESET_AFTER                         # ix->call_slab went null under the join: batch_counts resets the planner
        flags[i] = f
    out = np.full((nbatch, 6), -1, np.int64)
    assert ir.ir_run(p["first"], p["n"], p["B"], p["grp_n"], flags.ctypes.data, out.ctypes.data) == nbatch
    return flags, out


def test_planner_answers_what_the_old_loop_did(ir):
    rng = np.random.default_rng(20240611)
    seen = {JOIN_GROUP: 0, JOIN_RANGE: 0, JOIN_ALONE: 0, "again": 0, "slab": 0, "grow": 0}
    mismatches = []
    for k in range(N_PLANS):
        p = _plan(rng)
        want = _old_loop(p)
        flags, got = _drive(ir, p)
        for i in range(len(p["dense"])):
            if i not in want:
                if tuple(got[i]) != (-1,) * 6:
                    mismatches.append((k, i, "not dense", tuple(got[i])))
                continue
            (ans, again) = want[i]
            if tuple(int(v) for v in got[i]) != ans or bool(flags[i] & RESET_AFTER) != again:
                mismatches.append((k, i, ans, again, tuple(got[i]), int(flags[i])))
            seen[ans[2]] += 1
            seen["again"] += again
            seen["slab"] += bool(flags[i] & HAVE_SLAB)
            seen["grow"] += ans[1] > 0
    assert not mismatches, "%d mismatches, the first: %r" % (len(mismatches), mismatches[:5])
    assert all(v > 1000 for v in seen.values()), seen                  # every kind of answer was exercised


def test_a_group_and_its_tail(ir):
    """3 batches to a group, 7 batches of 64 (the last one short), no slab: rows 0 / 64 / 128 of the rolling buffer, one whole-group join then the
    columns the group added; the third group is cut at the end of the call."""
    p = dict(first=4096, n=6 * 64 + 10, B=64, grp_n=3, dense=np.ones(7, bool), can_group=np.ones(7, bool), slab=False, evict_at=-1, evict_in_join=False)
    _, got = _drive(ir, p)
    assert got.tolist() == [[0, 192, JOIN_GROUP, 192, 0, 0], [64, 0, JOIN_RANGE, 64, 4096, 64], [128, 0, JOIN_RANGE, 64, 4096, 128],
                            [0, 192, JOIN_GROUP, 192, 0, 0], [64, 0, JOIN_RANGE, 64, 4288, 64], [128, 0, JOIN_RANGE, 64, 4288, 128],
                            [0, 192, JOIN_GROUP, 10, 0, 0]]
