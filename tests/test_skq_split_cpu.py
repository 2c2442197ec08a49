"""The fill count of the filtered sketcher's survivor queue (gsearch_amd/csrc/gs_skq.hpp), compiled with the host compiler alone and held against a
queue written down as a plain list: the new entries are appended, and once 64 are pending the first 64 leave and the rest move to the front. For every
qn in 0..64 pending entries (64 itself never stands between two pushes; the helper must answer there all the same) and every cnt in 0..64 new ones:
whether the wave flushes, how many entries are pending afterwards, and that the queue's 128 entries are never exceeded."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def skq(tmp_path_factory):
    cxx = shutil.which("g++") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("skq") / "libskq.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(_HERE, "skq_split_shim.cpp")])
    L = C.CDLL(so)
    L.skq_capacity.restype = C.c_uint
    L.skq_flush_at.restype = C.c_uint
    L.skq_probe.restype = None
    L.skq_probe.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
    return L


def test_geometry(skq):
    """one flush feeds each of the 64 lanes; fewer than 64 pending and at most 64 new entries fit"""
    assert skq.skq_flush_at() == 64 and skq.skq_capacity() == 128


def test_fill_count_matches_the_plain_queue(skq):
    cap, at = skq.skq_capacity(), skq.skq_flush_at()
    out = np.zeros(2, np.uint32)
    for qn in range(at + 1):
        for cnt in range(65):
            queue = list(range(qn)) + list(range(1000, 1000 + cnt))
            assert len(queue) <= cap, (qn, cnt)                  # every slot a push writes (qn + rank) lies inside the queue
            flushed = len(queue) >= at
            if flushed:
                queue = queue[at:]                               # the entries at.. move to the front
            assert len(queue) < at or qn == at
            skq.skq_probe(qn, cnt, out.ctypes.data)
            assert (int(out[0]), bool(out[1])) == (len(queue), flushed), (qn, cnt)


def test_pending_stays_below_a_flush_between_pushes(skq):
    """a run of pushes of every size: the count the helper hands back is always a legal qn for the next push"""
    rng = np.random.default_rng(2053)
    out = np.zeros(2, np.uint32)
    qn = 0
    for cnt in rng.integers(0, 65, size=5000):
        skq.skq_probe(qn, int(cnt), out.ctypes.data)
        qn = int(out[0])
        assert qn < 64
