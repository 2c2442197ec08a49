"""The claim rule that deals the .gz files of a gs_sketch_files call between the host pipeline (front of the list) and the device pipeline (back of the
list): gsearch_amd/csrc/gs_gzdeal.hpp, compiled with the host compiler alone and held against a plain model written here. The model is the header's
documented rule: avail = n_gz - front - back; the front side gets min(cnt, avail); the back side gets min(cnt, avail, floor(share)) when its share is
at least the smallest claim, else nothing; the share is fixed (GS_GZIP_DEAL_SHARE) or, from the priors,
((avail + pa) / ra - pb / rb - (LAT until the back side has finished a file)) / (1 / rb + 1 / ra) with pa, pb the members claimed and not finished.
Every case stays below the number of finished files at which measured rates replace the priors, so the clock plays no part. The constants come
from the header through the shim; the model evaluates the formula with them in the header's order of operations (IEEE doubles on both sides)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
BIG = 10 ** 6                      # a group larger than any list here: the claim is bounded by avail and the share alone
SHARES = (-1, 0, 127, 128, 300, 5000)          # -1: from the priors; the others: fixed-share mode


@pytest.fixture(scope="module")
def gzd(tmp_path_factory):
    cxx = shutil.which("g++") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("gzdeal") / "libgzdeal.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(_HERE, "gzdeal_shim.cpp")])
    L = C.CDLL(so)
    L.gzdeal_constants.restype = None
    L.gzdeal_constants.argtypes = [C.c_void_p]
    L.gzdeal_new.restype = C.c_void_p
    L.gzdeal_new.argtypes = [C.c_ulonglong, C.c_longlong]
    L.gzdeal_free.restype = None
    L.gzdeal_free.argtypes = [C.c_void_p]
    L.gzdeal_claim.restype = C.c_ulonglong
    L.gzdeal_claim.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong]
    L.gzdeal_finished.restype = None
    L.gzdeal_finished.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong]
    L.gzdeal_state.restype = None
    L.gzdeal_state.argtypes = [C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def consts(gzd):
    out = np.zeros(5, np.float64)
    gzd.gzdeal_constants(out.ctypes.data)
    lat, ra, rb, after, least = (float(x) for x in out)
    assert lat > 0 and ra > 0 and rb > 0 and after == int(after) > 0 and least == int(least) > 0
    return dict(lat=lat, ra=ra, rb=rb, after=int(after), least=int(least))


class Model:
    """the documented rule, with the priors as the rates"""
    def __init__(self, n_gz, share, k):
        self.n, self.share, self.k = n_gz, share, k
        self.front = self.back = self.done_front = self.done_back = 0

    def device_share(self, avail):
        if self.share >= 0:
            return float(self.share)
        assert self.done_front < self.k["after"] and self.done_back < self.k["after"]       # priors only
        ra, rb = self.k["ra"], self.k["rb"]
        pa, pb = float(self.front - self.done_front), float(self.back - self.done_back)
        return ((float(avail) + pa) / ra - pb / rb - (0.0 if self.done_back else self.k["lat"])) / (1.0 / rb + 1.0 / ra)

    def claim(self, from_back, cnt):
        avail = self.n - self.front - self.back
        take = min(cnt, avail)
        if from_back:
            share = self.device_share(avail)
            take = 0 if share < self.k["least"] else min(take, int(share))
            self.back += take
        else:
            self.front += take
        return take

    def finished(self, from_back, n):
        if from_back:
            self.done_back += n
        else:
            self.done_front += n


class Deal:
    """one GzDeal of the header and the model beside it: every call goes to both and must agree"""
    def __init__(self, L, n_gz, share, k):
        self.L, self.h, self.model = L, L.gzdeal_new(n_gz, share), Model(n_gz, share, k)

    def close(self):
        self.L.gzdeal_free(self.h)

    def state(self):
        out = np.zeros(4, np.uint64)
        self.L.gzdeal_state(self.h, out.ctypes.data)
        return tuple(int(x) for x in out)

    def claim(self, from_back, cnt):
        got, want = int(self.L.gzdeal_claim(self.h, int(from_back), cnt)), self.model.claim(from_back, cnt)
        m = self.model
        assert got == want, (m.n, m.share, from_back, cnt, got, want)
        assert self.state() == (m.front, m.back, m.done_front, m.done_back)
        return got

    def finished(self, from_back, n):
        self.L.gzdeal_finished(self.h, int(from_back), n)
        self.model.finished(from_back, n)


def _first_back_claim(L, n_gz, share=-1, cnt=BIG):
    h = L.gzdeal_new(n_gz, share)
    try:
        return int(L.gzdeal_claim(h, 1, cnt))
    finally:
        L.gzdeal_free(h)


def test_first_device_claim_under_the_priors(gzd, consts):
    """nothing claimed, nothing done: the device side declines every list up to a boundary and takes at least the smallest claim beyond it. The two
    boundary values (the last list length declined, the first taken) are read off the header's behaviour and must be those of the formula"""
    first = [_first_back_claim(gzd, n) for n in range(0, 6001)]
    taken = [n for n in range(64, 6001) if first[n]]
    assert taken, "the device side never takes a member under the priors"
    n_take = taken[0]
    n_decline = n_take - 1
    print("priors: the device side declines a list of up to %d .gz files and takes its first claim from %d on" % (n_decline, n_take))
    assert n_decline >= 64
    assert all(first[n] == 0 for n in range(0, n_take))
    assert all(first[n] >= consts["least"] for n in range(n_take, 6001))
    # the model's own evaluation of ((avail + 0) / ra - LAT) / (1 / rb + 1 / ra)
    share = lambda n: (float(n) / consts["ra"] - consts["lat"]) / (1.0 / consts["rb"] + 1.0 / consts["ra"])
    assert share(n_decline) < consts["least"] <= share(n_take)
    assert all(first[n] == (0 if share(n) < consts["least"] else min(n, int(share(n)))) for n in range(0, 6001))


@pytest.mark.parametrize("share", SHARES)
def test_claim_grows_with_avail_and_stays_within_cnt_and_avail(gzd, consts, share):
    for cnt in (1, 16, consts["least"] - 1, consts["least"], consts["least"] + 1, 300, 1536, BIG):
        last = 0
        for avail in range(0, 4001, 1 if cnt == BIG else 7):
            got = _first_back_claim(gzd, avail, share, cnt)
            assert got <= cnt and got <= avail, (share, cnt, avail, got)
            assert got >= last, (share, cnt, avail, got, last)
            last = got
    # the same with members of the host side pending (pa > 0): the front claims first, the back side sees what is left
    for pending in (1, 64, 768):
        last = 0
        for avail in range(0, 4001, 13):
            d = Deal(gzd, avail + pending, share, consts)
            try:
                assert d.claim(False, pending) == pending
                got = d.claim(True, BIG)
            finally:
                d.close()
            assert got <= avail and got >= last, (share, pending, avail, got, last)
            last = got


def test_fixed_share_is_what_the_device_side_is_offered(gzd, consts):
    least = consts["least"]
    for share in (0, 1, least - 1):
        assert all(_first_back_claim(gzd, n, share) == 0 for n in (0, 1, 64, 83, least, 5000))
    for share in (least, least + 1, 300, 5000):
        for n in (0, 1, 64, 83, least, 299, 300, 301, 5000, 20000):
            assert _first_back_claim(gzd, n, share) == min(n, share)
            assert _first_back_claim(gzd, n, share, 16) == min(n, 16)


@pytest.mark.parametrize("share", SHARES)
def test_random_interleavings_of_front_and_back_claims(gzd, consts, share):
    """seeded runs of claims from both ends, cnt in 1..300, a few files reported finished now and then (fewer than the priors' lifetime). After every
    claim: the header and the model agree, the two sides never overlap, the front side got min(cnt, avail), and a side that came up short was the back
    side or left nothing unclaimed - which is what makes "a short group is the last one" safe. Then the front side claims until it comes up short:
    every member is claimed exactly once, [0, front) by the front side and [n_gz - back, n_gz) by the back side."""
    rng = np.random.default_rng(4100 + share)
    steps = 0
    for run in range(12):
        n_gz = int(rng.choice([64, 83, 500, 1247, 1248, 1400, 3000, 9000, 40000])) + int(rng.integers(0, 3))
        d = Deal(gzd, n_gz, share, consts)
        owner = np.zeros(n_gz, np.int8)                      # 1: claimed by the front side, 2: by the back side
        done = [0, 0]

        def claim(from_back, cnt):
            front0, back0, _, _ = d.state()
            avail = n_gz - front0 - back0
            take = d.claim(from_back, cnt)
            front1, back1, _, _ = d.state()
            assert front1 + back1 <= n_gz
            assert take <= cnt and take <= avail
            if from_back:
                assert (front1, back1) == (front0, back0 + take)
                assert not owner[n_gz - back1:n_gz - back0].any()
                owner[n_gz - back1:n_gz - back0] = 2
            else:
                assert take == min(cnt, avail), (n_gz, share, cnt, avail, take)
                assert (front1, back1) == (front0 + take, back0)
                assert not owner[front0:front1].any()
                owner[front0:front1] = 1
            if take < cnt:
                assert from_back or n_gz - front1 - back1 == 0, (n_gz, share, from_back, cnt, take)
            return take
        try:
            for _ in range(70):
                from_back = bool(rng.integers(0, 2))
                take = claim(from_back, int(rng.integers(1, 301)))
                steps += 1
                if take and rng.random() < 0.2:              # a few of them finished: the latency term goes, the priors stay
                    fin = min(take, int(rng.integers(1, 20)), consts["after"] - 1 - done[from_back])
                    d.finished(from_back, fin)
                    done[from_back] += fin
            while True:
                cnt = int(rng.integers(1, 301))
                steps += 1
                if claim(False, cnt) < cnt:
                    break
            front, back, _, _ = d.state()
            assert front + back == n_gz
            assert (owner[:front] == 1).all() and (owner[front:] == 2).all() and n_gz - back == front
            assert claim(True, 300) == 0 and claim(False, 300) == 0
        finally:
            d.close()
    assert steps >= 840
