"""Forward scores without a GPU (SPEC 13.1): the library's table of lse, STATS reader, Viterbi floor and E-value against the numpy restatement
(tests/pyref_hmm_forward.py), the restatement against a cell-by-cell f64 Forward, `fwd >= vit` on the integers, and the score held to the
reference's own data: the STATS LOCAL FORWARD tau lambda lines of the two profile files under tests/golden/hmm."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import gsearch_amd as G
import pyref_hmm as R
import pyref_hmm_forward as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
SYN_M = (1, 2, 65, 129)
GS_ERR_INVALID = -1
BOUND_UNITS = 64                      # |restatement - f64| at most, in units of 2^-10 bit


def fixture(name):
    return open(os.path.join(HERE, "golden", "hmm", name), "rb").read()


@pytest.fixture(scope="module")
def case():
    """the profiles, their records, and the integer Forward, the Viterbi and the f64 Forward score of every pair, once"""
    rng = np.random.default_rng(131)
    texts = [fixture(n) for n in FIXTURES] + [R.write_hmm(R.synth_model(rng, M)) for M in SYN_M]
    models = [m for t in texts for m in R.parse_hmm(t)]
    pairs = []
    for m in models:
        tab, M = m["tables"], m["M"]
        c = R.consensus(tab)
        recs = [R.background(rng, L) for L in (1, 64, 200)]
        recs += [c, c + R.background(rng, 20) + c, R.background(rng, 125) + c[:max(M // 2, 1)] + R.background(rng, 125)]
        if M == 129:
            recs.append(c[:30] + c[100:])                                        # nodes 31..100 deleted: a D run across 23 groups of 3
        fwd, vit = F.forward_batch(tab, recs), R.viterbi_batch(tab, recs)
        pairs += [(M, rec, int(fwd[r]), int(vit[r]), F.forward_f64(tab, rec)) for r, rec in enumerate(recs)]
    return {"texts": texts, "models": models, "pairs": pairs}


def test_logsum_table_is_the_restatements():
    t = G.hmm_logsum_table()
    assert t.dtype == np.uint16 and t.shape == (F.LSE_N,) == (5903,)
    assert np.array_equal(t.astype(np.int64), F.T[:F.LSE_N]) and F.T[F.LSE_N] == 0
    assert t[0] == 1024 and t[-1] == 1
    step = np.diff(t.astype(np.int64))
    assert (step <= 0).all() and (step >= -1).all()
    # the entry that would follow rounds to 0, and no entry is near a rounding boundary
    exact = [1024.0 * math.log2(1.0 + 2.0 ** (-2.0 * j / 1024.0)) for j in range(F.LSE_N + 1)]
    assert math.floor(exact[F.LSE_N] + 0.5) == 0
    assert min(abs(v - math.floor(v) - 0.5) for v in exact) > 3e-6
    short = np.zeros(F.LSE_N - 1, np.uint16)
    L = G.load()
    assert L.gs_hmm_logsum_table(short.ctypes.data, short.size) == GS_ERR_INVALID and not short.any()
    assert L.gs_hmm_logsum_table(None, 5903) == GS_ERR_INVALID


def test_lse_is_symmetric_monotone_and_at_least_the_max():
    rng = np.random.default_rng(3)
    a = rng.integers(-20000, 20000, 4000)
    b = a + rng.integers(-13000, 13000, 4000)
    s = F.lse(a, b)
    assert np.array_equal(s, F.lse(b, a)) and (s >= np.maximum(a, b)).all()
    assert (F.lse(a + 1, b) >= s).all() and (F.lse(a, b + 1) >= s).all()
    assert np.array_equal(F.lse(a + 777, b + 777), s + 777)
    assert F.lse(0, 0) == 1024 and F.lse(0, -11804) == 1 and F.lse(0, -11805) == 0 and F.lse(5, R.NEG) == 5
    exact = np.maximum(a, b) + 1024.0 * np.log2(1.0 + 2.0 ** (-np.abs(a - b) / 1024.0))
    assert np.abs(s - exact).max() <= 1.0


def test_restatement_against_the_f64_forward(case):
    worst = max(abs(fwd - f64) for _, _, fwd, _, f64 in case["pairs"])
    bad = [(M, len(rec), fwd, round(f64, 2)) for M, rec, fwd, _, f64 in case["pairs"] if not abs(fwd - f64) <= BOUND_UNITS]
    assert len(case["pairs"]) == 37
    assert not bad and 0 < worst <= BOUND_UNITS, "worst |int - f64| = %.2f units of %d; %s" % (worst, BOUND_UNITS, bad[:8])
    print("worst |int - f64| = %.2f units" % worst)


def test_forward_is_at_least_viterbi_on_the_integers(case):
    low = [(M, len(rec), fwd, vit) for M, rec, fwd, vit, _ in case["pairs"] if not fwd >= vit]
    assert not low, low
    # one node, one residue: nothing to sum, the two are equal; copies and fragments gain the most
    assert any(fwd == vit for M, rec, fwd, vit, _ in case["pairs"] if M == 1 and len(rec) == 1)
    assert max(fwd - vit for _, _, fwd, vit, _ in case["pairs"]) > 4 * 1024


def test_single_and_batch_agree_and_empty_records_have_no_score(case):
    m = case["models"][1]
    recs = [b"", R.consensus(m["tables"]), b"ACDEFGHIKL", b""]
    got = F.forward_batch(m["tables"], recs)
    assert got[0] == got[3] == R.NO_SCORE and [int(got[1]), int(got[2])] == [F.forward(m["tables"], recs[1]), F.forward(m["tables"], recs[2])]
    vit, fwd = F.search_forward(case["models"][:2], recs, floor=[R.threshold_units(0.0), F.FLOOR_ALL])
    assert (fwd[[0, 3]] == R.NO_SCORE).all() and fwd[1, 1] == got[1] and fwd[2, 1] == got[2]
    assert fwd[2, 0] == R.NO_SCORE and vit[2, 0] < 0 and fwd[1, 0] == R.NO_SCORE and vit[1, 0] < 0


@pytest.mark.parametrize("name,measured_seed_values", [("PF00380.20.HMM", (0.893, 0.706)), ("TIGR00964.HMM", (0.823, 0.134))])
def test_held_to_the_files_forward_statistics(name, measured_seed_values):
    """HMMER fits tau of STATS LOCAL FORWARD at tail mass 0.04 on L = 100, so the 0.96 quantile of the Forward bits of background records of 100
    residues lies at tau + ln(25) / lambda. 400 records, seed 977: measured / predicted bits are (0.893, 0.706) for PF00380.20 and (0.823, 0.134)
    for TIGR00964; sixteen tail samples are noisy, hence 1.5 bits."""
    text = fixture(name)
    (st, has), = F.stats_lines(text)
    assert has == 7
    tau, lam = st[4], st[5]
    rng = np.random.default_rng(977)
    recs = [R.background(rng, 100) for _ in range(400)]
    bits = np.sort(F.forward_batch(R.parse_hmm(text)[0]["tables"], recs) / 1024.0)
    measured = float(bits[int(0.96 * 400) - 1])
    predicted = tau + math.log(25.0) / lam
    assert abs(measured - predicted) <= 1.5, (measured, predicted)
    assert (round(measured, 3), round(predicted, 3)) == measured_seed_values


def test_parse_stats():
    for name, want in ((FIXTURES[0], [-9.6946, 0.71333, -10.5953, 0.71333, -3.8068, 0.71333]), (FIXTURES[1], [-8.4992, 0.71900, -8.6216, 0.71900, -4.3433, 0.71900])):
        st, has = G.hmm_parse_stats(fixture(name))
        (rst, rhas), = F.stats_lines(fixture(name))
        assert has == rhas == 7 and st.tolist() == rst == want
    both = fixture(FIXTURES[0]) + fixture(FIXTURES[1])
    assert G.hmm_parse_stats(both, 1)[0][4] == -4.3433 and G.hmm_parse_stats(both, 0)[0][4] == -3.8068
    s = R.synth_model(np.random.default_rng(5), 7)
    text = R.write_hmm(s)
    assert G.hmm_parse_stats(text)[1] == 7 and G.hmm_parse_stats(text)[0][4] == float("%.4f" % (s["mu"] + 4))
    bare = b"\n".join(ln for ln in text.split(b"\n") if not ln.startswith(b"STATS"))
    st, has = G.hmm_parse_stats(bare)
    assert has == 0 and not st.any() and F.stats_lines(bare) == [([0.0] * 6, 0)]
    only_fwd = b"\n".join(ln for ln in text.split(b"\n") if not ln.startswith(b"STATS LOCAL MSV") and not ln.startswith(b"STATS LOCAL VIT"))
    assert G.hmm_parse_stats(only_fwd)[1] == 4 and G.hmm_parse(only_fwd)[0]["mu"] is None
    out, has = np.zeros(6), C.c_uint32()
    L = G.load()
    buf = np.frombuffer(text, np.uint8)
    assert L.gs_hmm_parse_stats_mem(buf.ctypes.data, len(buf), 1, out.ctypes.data, C.byref(has)) == GS_ERR_INVALID          # one model in the text
    assert L.gs_hmm_parse_stats_mem(buf.ctypes.data, len(buf) // 2, 0, out.ctypes.data, C.byref(has)) == GS_ERR_INVALID     # truncated


def test_viterbi_floor_and_forward_evalue():
    for mu, lam in ((-10.5953, 0.71333), (-8.6216, 0.719), (-8.5, 0.7), (3.25, 1.1)):
        for p in (1e-3, 0.02, 0.5, 1e-9, 0.999):
            assert G.hmm_viterbi_floor(mu, lam, p) == F.viterbi_floor(mu, lam, p), (mu, lam, p)
    # P = 1e-3 on the S9 profile: mu + 6.9073 / lambda bits
    assert G.hmm_viterbi_floor(-10.5953, 0.71333) == R.threshold_units(-10.5953 + 6.907255 / 0.71333) == -934
    out = C.c_int32(77)
    L = G.load()
    for mu, lam, p in ((0.0, 0.0, 1e-3), (0.0, -1.0, 1e-3), (0.0, 0.7, 0.0), (0.0, 0.7, 1.0), (float("nan"), 0.7, 0.5)):
        assert L.gs_hmm_viterbi_floor(mu, lam, p, C.byref(out)) == GS_ERR_INVALID and out.value == 77
    assert G.hmm_viterbi_floor(1e12, 0.7) == (1 << 31) - 1 and G.hmm_viterbi_floor(-1e12, 0.7) == F.FLOOR_ALL
    tau, lam = -3.8068, 0.71333
    assert G.hmm_forward_evalue(tau - 0.01, tau, lam, 250.0) == 250.0 and G.hmm_forward_evalue(-50.0, tau, lam, 3.0) == 3.0
    assert G.hmm_forward_evalue(tau, tau, lam, 250.0) == 250.0
    for bits in (-3.0, 0.0, 10.0, 22.1, 300.0):
        assert G.hmm_forward_evalue(bits, tau, lam, 40.0) == pytest.approx(40.0 * F.forward_pvalue(bits, tau, lam), rel=1e-12)
    assert L.gs_hmm_forward_evalue(C.c_double(25.0), C.c_double(tau), C.c_double(lam), C.c_double(1.0)) < 1e-8
