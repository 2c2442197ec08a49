"""SPEC 13.8 without a device: gs_hmm_hit_records, the host twin of the device step, `==` the numpy restatement (tests/pyref_hit_records.py) on the
constructed cases of tests/hit_records_cases.py - every output word and byte, and nothing written behind them -, the four refusals with their code, and
the counts-first rule of the capacity refusal. The cases' own promises are checked first. gs_hmm_hit_records_dev is held to the same restatement by
tests/test_gpu_hit_records.py."""
import numpy as np
import pytest

import gsearch_amd as G
import hit_records_cases as HC
import pyref_hit_records as R

PATTERN = 0xA5


@pytest.fixture(scope="module", autouse=True)
def the_library_has_the_feature():
    assert all(s in G.SYMBOLS for s in ("gs_hmm_hit_records", "gs_hmm_hit_records_dev"))
    assert (HC.WIDTHS["dom"], HC.WIDTHS["env"], HC.WIDTHS["ali"]) == (G._lib.HMM_DOM_WORDS, G._lib.HMM_ENV_WORDS, G._lib.HMM_ALI_WORDS)
    assert R.NO_HIT == G._lib.HMM_NO_HIT and R.GS_ERR_INVALID == G._lib.GS_ERR_INVALID


def outputs(case, room_rec, room_aa):
    """pre-filled output arrays: the residues to a multiple of 8 bytes and a word more, as the sketcher wants its buffer"""
    ng = case["best_rec"].shape[0]
    words = lambda n: np.full(8 * n, PATTERN, np.uint8).view(np.uint64)      # noqa: E731
    return np.full((room_aa + 7) // 8 * 8 + 8, PATTERN, np.uint8), words(room_rec + 2), words(room_rec + 2), words(ng + 1)


def test_the_cases_keep_their_promises():
    cases = HC.all_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    shapes = {c["best_rec"].shape for c in cases if c["name"].startswith("shape")}
    assert shapes == {(g, p) for g in (1, 3, 70) for p in (1, 2, 120, 130)}
    by = {c["name"]: c for c in cases}
    assert (by["all NO_HIT"]["best_rec"] == HC.NO_HIT).all()
    for where, g0 in (("first", 0), ("middle", 2), ("last", 4)):
        rec = by["empty genome %s" % where]["best_rec"]
        assert [bool((row != HC.NO_HIT).any()) for row in rec] == [g != g0 for g in range(5)]
    # every edge length at every (source, destination) offset mod 8, as whole records and as spans of each slot width
    for name in ["record lengths x offsets"] + ["span lengths x offsets, %s slots" % w for w in HC.WIDTHS]:
        c = by[name]
        got = R.hit_records(c["best_rec"], c["aa"], c["rec_start"], c["rec_len"], c["n_item"], c["item"])
        flat = c["best_rec"].reshape(-1)
        src = c["rec_start"][flat].astype(np.int64) + (2 if c["item"] is not None else 0)
        seen = {(int(n), int(s) % 8, int(d) % 8) for n, s, d, r in zip(got[2], src, got[1], flat) if r >= 8}
        assert seen == {(n, s, d) for n in HC.EDGE_LENGTHS for s in range(8) for d in range(8)}, name
    for w in HC.WIDTHS:
        for m in (1, 3):
            c = by["spans %s max_item %d" % (w, m)]
            hit = c["best_rec"].reshape(-1) != HC.NO_HIT
            assert c["item"].shape[1:] == (m, HC.WIDTHS[w]) and {0, 1, m} <= set(int(v) for v in c["n_item"][hit])


@pytest.mark.parametrize("case", HC.all_cases(), ids=lambda c: c["name"])
def test_host_form_is_the_restatement(case):
    want = R.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"])
    n_hit, n_aa = len(want[1]), len(want[0])
    out = outputs(case, n_hit, n_aa)
    got = G.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"], cap_rec=n_hit, cap_aa=n_aa, out=out)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert (out[0][n_aa:] == PATTERN).all() and (out[1][n_hit:] == out[1][-1]).all() and (out[2][n_hit:] == out[2][-1]).all()
    assert int(want[3][-1]) == n_hit and (np.diff(want[3].astype(np.int64)) >= 0).all()
    # the arrays the wrapper makes itself hold the same
    again = G.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"])
    assert all(np.array_equal(g, w) for g, w in zip(again, want))


def test_a_record_chosen_twice_appears_twice():
    c = {x["name"]: x for x in HC.layout_cases()}["record chosen twice"]
    aa, start, ln, goff = G.hit_records(c["best_rec"], c["aa"], c["rec_start"], c["rec_len"])
    assert list(goff) == [0, 2, 5] and len(set(int(v) for v in ln[:2])) == 1
    rec5 = c["aa"][int(c["rec_start"][5]):int(c["rec_start"][5]) + int(c["rec_len"][5])]
    assert np.array_equal(aa[:2 * len(rec5)], np.concatenate([rec5, rec5]))


@pytest.mark.parametrize("err", HC.error_cases(), ids=lambda e: e[0])
def test_refusals(err):
    what, case, cap_rec, cap_aa = err
    with pytest.raises(R.Refused) as want:
        R.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"], cap_rec, cap_aa)
    out = outputs(case, 64, 4096)
    with pytest.raises(G.GsError) as got:
        G.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"], cap_rec=cap_rec, cap_aa=cap_aa, out=out)
    assert got.value.code == want.value.code == G._lib.GS_ERR_INVALID
    assert got.value.counts == want.value.counts and (want.value.counts is not None) == what.startswith("room")
    assert all((a.view(np.uint8) == PATTERN).all() for a in out), "a refusal writes nothing"


def test_the_counts_size_a_second_call():
    what, case, cap_rec, cap_aa = HC.error_cases()[-1]
    with pytest.raises(G.GsError) as e:
        G.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], cap_rec=0, cap_aa=0)
    n_hit, n_aa = e.value.counts
    got = G.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], cap_rec=n_hit, cap_aa=n_aa)
    want = R.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"])
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_arguments():
    c = HC.layout_cases()[0]
    with pytest.raises(ValueError):
        G.hit_records(c["best_rec"], c["aa"], c["rec_start"], c["rec_len"], n_item=np.zeros(15, np.uint32))
    L = G.load()
    n = (np.zeros(2, np.uint64))
    goff = np.zeros(4, np.uint64)
    ni, it = np.zeros(15, np.uint32), np.zeros((15, 1, 1), np.int32)
    args = (None, c["best_rec"].ctypes.data, 3, 5, c["aa"].ctypes.data, c["rec_start"].ctypes.data, c["rec_len"].ctypes.data, len(c["rec_len"]))
    assert L.gs_hmm_hit_records(*args, ni.ctypes.data, it.ctypes.data, 1, 1, 0, 0, None, None, None, goff.ctypes.data, n.ctypes.data) == G._lib.GS_ERR_INVALID      # one word a slot
    assert L.gs_hmm_hit_records(*args, ni.ctypes.data, None, 4, 1, 0, 0, None, None, None, goff.ctypes.data, n.ctypes.data) == G._lib.GS_ERR_INVALID               # half of the spans
    assert L.gs_hmm_hit_records(*args, None, None, 0, 0, 0, 0, None, None, None, goff.ctypes.data, n.ctypes.data) == G._lib.GS_OK and list(goff) == [0, 0, 0, 0]
