"""The cursor of walk_genome's two-stage loop (gsearch_amd/csrc/gs_walk_span.hpp: which record owns a flat unit, and which packed words the walk of that
unit loads), driven directly: a few lines of host C++ compiled with g++, no HIP and no device. tests/walk_span_shim.cpp takes every lane of every
workgroup through the loop's schedule; for every unit the lane reaches, what its cursor says is compared here with a restatement of the one-stage walk
(`_one_stage` below: numpy's searchsorted for "the last r with rec_upre[r] <= f", then the arithmetic walk_unit had), which does not call into the header.

Held for every lane and every trip: the record, its bounds, the word, a0 and first_valid equal the binary search's, field by field; the words a lane
loads - ahead of the walk before, or where it had to look the record up - are words the one-stage walk loads for that unit (u, and u - 1 only where the
unit has a halo); none is negative, none lies past the genome's last word, and nothing is loaded for a unit the genome does not have."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 16, 17, 21, 32)
PARTS = (1, 2, 3)
PROLOGUE, LOOKED_UP, INSIDE = 0, 1, 2
COLS = 9


@pytest.fixture(scope="module")
def ws(tmp_path_factory):
    cxx = shutil.which("g++") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("walk_span") / "libwalk_span.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(_HERE, "walk_span_shim.cpp")])
    L = C.CDLL(so)
    L.ws_run.restype = C.c_longlong
    L.ws_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    L.ws_probe.restype = None
    L.ws_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_ulonglong] * 5 + [C.c_void_p]
    return L


def _table(rng, case):
    """One genome's record table inside a larger one (records of other genomes in front and behind): starts at every offset mod 32 over the cases, records
    shorter than every k, runs of them, 1 to 200 records, the first record at base 0 in every fourth case."""
    n = int(rng.choice([1, 2, 3, 7, 40, 200])) if case % 3 else int(rng.integers(1, 201))
    before = 0 if case % 4 == 0 else int(rng.integers(1, 4))
    after = int(rng.integers(0, 3))
    kind = rng.integers(0, 5, size=before + n + after)
    lens = np.where(kind == 0, rng.integers(1, 34, size=kind.size),                       # around k and around one word
           np.where(kind == 1, rng.integers(1, 12, size=kind.size),                        # shorter than most k
           np.where(kind == 2, rng.integers(34, 200, size=kind.size),
           np.where(kind == 3, rng.integers(200, 6000, size=kind.size), rng.integers(16_000, 70_000, size=kind.size)))))
    if case % 5 == 0 and n > 6:                                                            # a run of records too short for any k > 1, in the middle
        lens[before + n // 2: before + n // 2 + 5] = 1
    gaps = np.where(rng.random(kind.size) < 0.5, 0, rng.integers(0, 70, size=kind.size))   # records back to back share a word
    first = 0 if case % 4 == 0 else (case % 32) + 32 * int(rng.integers(0, 5))
    starts = first + np.concatenate([[0], np.cumsum(lens + gaps)[:-1]])
    return starts.astype(np.uint64), lens.astype(np.uint64), before, before + n


def _prefix(rs, rl, r0, r1, k):
    """k_unit_prefix: units per record (0 for a record shorter than k), exclusive prefix inside the genome"""
    s, ln = rs[r0:r1].astype(np.int64), rl[r0:r1].astype(np.int64)
    u = np.where(ln >= k, ((s + ln - 1) >> 5) - (s >> 5) + 1, 0)
    upre = np.zeros(len(rs), np.uint64)
    upre[r0:r1] = np.concatenate([[0], np.cumsum(u)[:-1]])
    return upre, int(u.sum())


def _one_stage(rs, rl, upre, r0, r1, units, k):
    """walk_unit of the one-stage loop for every f < units: record, rb, re, u, a0, first_valid, halo"""
    f = np.arange(units, dtype=np.int64)
    lo = r0 + np.searchsorted(upre[r0:r1].astype(np.int64), f, side="right") - 1
    rb = rs[lo].astype(np.int64)
    re = rb + rl[lo].astype(np.int64)
    u = (rb >> 5) + (f - upre[lo].astype(np.int64))
    a0 = u << 5
    return lo, rb, re, u, a0, rb + k - 1, (a0 > rb) & (k > 1)


def test_cursor_equals_the_binary_search_and_loads_no_new_word(ws):
    rng = np.random.default_rng(20241019)
    seen = {PROLOGUE: 0, LOOKED_UP: 0, INSIDE: 0, "short": 0, "hop_many": 0, "no_halo": 0, "start_mod": set()}
    bad = []
    for case in range(48):
        rs, rl, r0, r1 = _table(rng, case)
        block = 64 if case % 2 else 512                               # 64: a lane changes record on most trips of the small tables
        for k in KS:
            upre, units = _prefix(rs, rl, r0, r1, k)
            if units == 0:
                continue
            lo, rb, re, u, a0, fv, halo = _one_stage(rs, rl, upre, r0, r1, units, k)
            last_word = int((re.max() - 1) >> 5)
            for parts in PARTS:
                out = np.zeros((units, COLS), np.int64)
                ahead = ws.ws_run(rs.ctypes.data, rl.ctypes.data, upre.ctypes.data, r0, r1, units, k, block, parts, out.ctypes.data)
                how = out[:, 6] >> 4
                tag = (case, k, parts)
                if ahead < 0 or ahead != int((how == INSIDE).sum()):
                    bad.append((tag, "loads ahead", ahead))
                    continue
                if not np.all((out[:, 6] & 15) == 1):
                    bad.append((tag, "units not reached exactly once", np.flatnonzero((out[:, 6] & 15) != 1)[:5].tolist()))
                    continue
                for name, col, want in (("lo", 0, lo), ("rb", 1, rb), ("re", 2, re), ("u", 3, u), ("a0", 4, a0), ("first_valid", 5, fv)):
                    if not np.array_equal(out[:, col], want):
                        i = int(np.flatnonzero(out[:, col] != want)[0])
                        bad.append((tag, name, i, int(out[i, col]), int(want[i]), int(how[i])))
                w, pw = out[:, 7], out[:, 8]
                if not np.array_equal(w, u):
                    bad.append((tag, "w is not the unit's word", int(np.flatnonzero(w != u)[0])))
                if not np.all((pw == u) | ((pw == u - 1) & halo)):
                    bad.append((tag, "pw is a word the one-stage walk does not load", int(np.flatnonzero(~((pw == u) | ((pw == u - 1) & halo)))[0])))
                if min(w.min(), pw.min()) < 0 or max(w.max(), pw.max()) > last_word or pw.min() < int(rs[r0] >> 5):
                    bad.append((tag, "a word outside the genome", int(w.min()), int(pw.min()), int(w.max()), last_word))
                # a unit with a halo reads the word in front of it: loading u in its place would be wrong where it is legal
                if not np.all(pw[halo] == u[halo] - 1):
                    bad.append((tag, "halo word not loaded", int(np.flatnonzero(halo & (pw != u - 1))[0])))
                for h in (PROLOGUE, LOOKED_UP, INSIDE):
                    seen[h] += int((how == h).sum())
                seen["no_halo"] += int((~halo).sum())
                stride = parts * block
                if units > stride:
                    seen["hop_many"] += int((lo[stride:] - lo[:-stride] > 1).sum())
            seen["short"] += int((rl[r0:r1] < k).sum())
        seen["start_mod"] |= set(int(x) & 31 for x in rs[r0:r1])
    assert not bad, "%d failures, the first: %r" % (len(bad), bad[:5])
    assert seen["start_mod"] == set(range(32)), sorted(seen["start_mod"])
    assert all(seen[x] > 1000 for x in (PROLOGUE, LOOKED_UP, INSIDE, "short", "hop_many", "no_halo")), seen


def test_counts_beyond_32_bits_only_make_the_cursor_look_again(ws):
    """The cursor holds the units left in its span, and the stride, in 32 bits. Record tables are only numbers: a record of 2^38 bases (2^33 units) next to
    a small one, probed one lane at a time. Where the cursor says `inside`, the unit is inside and the word is u + stride; where count and stride fit 32
    bits it says so exactly; where they do not it may only say `not inside`."""
    k = 21
    rs = np.array([7, 7 + (1 << 38) + 40, 7 + (1 << 38) + 40 + 5000], np.uint64)
    rl = np.array([1 << 38, 5000, 333], np.uint64)
    upre, units = _prefix(rs, rl, 0, 3, k)
    ends = np.concatenate([upre[1:], [units]]).astype(object)
    out = np.zeros(3, np.int64)
    said_inside = said_saturated = 0
    for f in (0, 1, 511, (1 << 32) - 1, (1 << 32), (1 << 33) - 600, int(upre[1]) - 513, int(upre[1]) - 512, int(upre[1]) - 1, int(upre[1]), int(upre[1]) + 100, units - 1):
        for stride in (1, 64, 512, 1536, (1 << 32) - 2, (1 << 32) - 1, (1 << 32), (1 << 32) + 5, (1 << 33) - 700):
            ws.ws_probe(rs.ctypes.data, rl.ctypes.data, upre.ctypes.data, 0, 3, units, f, stride, out.ctypes.data)
            lo = int(np.searchsorted(upre.astype(object), f, side="right")) - 1
            left = int(ends[lo]) - f
            truly = stride < left
            u = (int(rs[lo]) >> 5) + f - int(upre[lo])
            assert int(out[2]) == min(left, 0xFFFFFFFF), (f, stride)
            if out[0]:
                assert truly and int(out[1]) == u + stride, (f, stride, left)
                said_inside += 1
            elif left <= 0xFFFFFFFF and stride < 0xFFFFFFFF:
                assert not truly, (f, stride, left)
            said_saturated += left > 0xFFFFFFFF
    assert said_inside > 20 and said_saturated > 20
