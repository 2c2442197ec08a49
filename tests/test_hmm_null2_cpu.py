"""SPEC 13.5 on the CPU: the restatement tests/pyref_hmm_null2.py (Forward and Backward over an envelope with the folds of expected state usage, the
null2 vector, corr, the two biases) against its own cell-by-cell f64 yardstick with full matrices, on the identities that hold on the integers, and held
to what the committed profile files say: their cutoffs and their STATS LOCAL FORWARD lines. No kernel runs; the library is asked for its constants and
symbols only, so that without gs_hmm_null2 every test here fails.

The inputs are the world of tests/test_hmm_posterior_cpu.py (same recipe, same seed) and, for both committed profiles, the record kinds of the issue's
table: a homopolymer, the consensus, 200 background residues, the shuffled consensus, the consensus with 40 x K / F planted in its middle. Every
envelope of every pair is a segment; a pair without an envelope contributes its whole record as one. Each bound is four times the measurement rounded
up to a power of two, and must not be more than 16 times the measurement:

    largest |n2[a] - f64|             13.95 units   asserted  64
    largest |corr - f64| / Ld         13.04 units   asserted  64
    largest |mass|                    13    units   asserted  64
    largest bias among the 48 best of 400 background records of 100 residues: 77 units (0.075 bit) for PF00380.20, asserted 512;
                                      3 937 units (3.845 bits) for TIGR00964, asserted 16 384

The 0.96 quantile of the corrected scores of those 400 records: 0.886 bits (uncorrected 0.893, predicted 0.706) for PF00380.20, 0.421 bits (0.823, 0.134)
for TIGR00964 - the correction moves both towards the files' own figures. The yardstick's corrected score is the integer Forward raw (within 14 units of
the f64 Forward, SPEC 13.1) minus the f64 bias.

corr itself drifts by MORE than a quarter bit: the per-residue deviation adds up over the segment, 1 577 units (1.54 bits) on `K` x 121 against
PF00380.20, of a bias of 126.8 bits; 433 units on the consensus with 40 x `K` planted, 351 units on the consensus alone."""
import math
import os

import numpy as np
import pytest

import gsearch_amd as G
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_null2 as N
import pyref_hmm_posterior as P
import test_hmm_posterior_cpu as W

FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
HOMOPOLYMER = {"PF00380.20.HMM": b"K" * 121, "TIGR00964.HMM": b"F" * 57}
N2_BOUND, CORR_PER_RESIDUE_BOUND, MASS_BOUND = 64, 64, 64
BG_BIAS_BOUND_UNITS = {"PF00380.20.HMM": 512, "TIGR00964.HMM": 16384}         # measured 77 and 3 937 units


@pytest.fixture(scope="module", autouse=True)
def the_library_has_the_feature():
    assert "gs_hmm_null2" in G.SYMBOLS and "gs_hmm_null2_dev" in G.SYMBOLS and hasattr(G.HmmDb, "null2") and hasattr(G.HmmDb, "null2_packed") and hasattr(G.HmmDb, "null2_dev")
    assert (G._lib.HMM_N2_WORDS, G._lib.HMM_N2_OMEGA) == (N.N2_WORDS, N.OMEGA)


def model(name):
    return R.parse_hmm(open(W.fixture_path(name), "rb").read())[0]


def record_kinds(name, tab):
    """the record kinds of the issue's table for one committed profile"""
    rng = np.random.default_rng(1351)
    c = R.consensus(tab)
    h = HOMOPOLYMER[name]
    mid = len(c) // 2
    return {"homopolymer": h, "consensus": c, "background": R.background(rng, 200), "shuffled": bytes(np.frombuffer(c, np.uint8)[rng.permutation(len(c))]),
            "planted": c[:mid] + h[:1] * 40 + c[mid:]}


@pytest.fixture(scope="module")
def world():
    """every pair with its envelopes, its segments on the integers and in f64, once"""
    rng = np.random.default_rng(1349)                                                       # the recipe of test_hmm_posterior_cpu.world
    models = [model(n) for n in FIXTURES]
    models += [R.parse_hmm(R.write_hmm(R.synth_model(rng, M)))[0] for M in W.SYN_M]
    pairs = []
    for m in models:
        tab, M = m["tables"], m["M"]
        c = R.consensus(tab)
        recs = [R.background(rng, 1), R.background(rng, 64), R.background(rng, 200), c, c + c, R.background(rng, 30) + c[:max(M // 2, 1)] + R.background(rng, 30)]
        if M > 100:
            recs.append(c[:30] + c[100:])
        pairs += [{"tab": tab, "rec": rec, "kind": None, "model": m} for rec in recs]
    pairs += [{"tab": tab, "rec": rec, "kind": None, "model": None} for tab, rec, _ in W.hand_cases()]
    for name, m in zip(FIXTURES, models[:2]):
        pairs += [{"tab": m["tables"], "rec": rec, "kind": kind, "model": m, "name": name} for kind, rec in record_kinds(name, m["tables"]).items()]
    for w in pairs:
        x = R.encode(w["rec"])
        w["int"] = N.pair(w["tab"], w["rec"], whole_if_none=True)
        w["f64"] = [N.segment_f64(w["tab"], x[a - 1:b], len(x)) for a, b, _, _ in w["int"]["env"]]
    return pairs


def test_deviations_from_the_yardstick(world):
    n2_dev = per_res = mass = drift = 0.0
    n_seg = 0
    for w in world:
        for (a, b, _, _), s, y in zip(w["int"]["env"], w["int"]["seg"], w["f64"]):
            Ld = b - a + 1
            assert abs(y["mass"]) < 1e-4 and abs(y["total_f"] - y["total_b"]) < 1e-6          # the decomposition is sound in f64
            n2_dev = max(n2_dev, float(np.abs(s["n2"] - y["n2"]).max()))
            per_res = max(per_res, abs(s["corr"] - y["corr"]) / Ld)
            mass = max(mass, abs(s["mass"]))
            if abs(s["corr"] - y["corr"]) > drift:
                drift, where = abs(s["corr"] - y["corr"]), (w["kind"], Ld, s["corr"])
            n_seg += 1
    print("segments %d; largest |n2 - f64| %.2f units, |corr - f64| / Ld %.2f units, |mass| %d units; largest drift of corr %.0f units at %s" % (
        n_seg, n2_dev, per_res, mass, drift, where))
    assert n_seg >= 60
    for got, bound in ((n2_dev, N2_BOUND), (per_res, CORR_PER_RESIDUE_BOUND), (mass, MASS_BOUND)):
        assert bound / 16 < got <= bound, (got, bound)
    assert drift > 256                                                                        # said in SPEC 13.5: more than a quarter bit


def test_identities_on_the_integers(world):
    n_whole = 0
    for w in world:
        p = w["int"]
        for (a, b, env_raw, _), s in zip(p["env"], p["seg"]):
            assert s["seg_raw"] == env_raw and s["dom_bias"] >= 0 and s["dom_bias"] == N.lse(0, N.OMEGA + s["corr"])
            if (a, b) == (1, len(w["rec"])):
                assert s["seg_raw"] == p["fwd"]
                n_whole += 1
            assert s["occI"][-1] == R.NEG and len(s["occM"]) == w["tab"].shape[1] - 1
        assert p["seq_bias"] >= 0 and p["seq_bias"] == N.seq_bias([s["corr"] for s in p["seg"]])
        if len(p["seg"]) == 1:
            assert p["seq_bias"] == p["seg"][0]["dom_bias"]
    assert n_whole >= 12
    assert N.seq_bias([]) == 6 == N.lse(0, N.OMEGA)                                           # a pair without an envelope: 1 / 256 of null2, 0.006 bit
    assert N.seq_bias([1 << 40]) == N.OMEGA + N.CORR_MAX and N.seq_bias([-(1 << 40), -5]) == 0 and N.lg(1) == 0 and N.lg(64) == 6144


def test_held_to_the_files_cutoffs(world):
    """the consensus keeps TC1 after correction, the homopolymer reaches GA1 without it and falls below with it - in the integers and in the yardstick"""
    seen = 0
    for w in world:
        if w["kind"] not in ("consensus", "homopolymer", "planted"):
            continue
        m, p = w["model"], w["int"]
        ga, tc = m["ga_units"], R.bits_units("%.2f" % m["tc"][0])
        corrected = p["fwd"] - p["seq_bias"]
        corrected_f64 = p["fwd"] - N.bias_f64([y["corr"] for y in w["f64"]])
        print("%-14s %-11s fwd %7.2f bits, seq_bias %6.2f (f64 %6.2f), corrected %7.2f; GA1 %.2f TC1 %.2f; envelopes %s%s" % (
            w["name"], w["kind"], p["fwd"] / 1024, p["seq_bias"] / 1024, (p["fwd"] - corrected_f64) / 1024, corrected / 1024, ga / 1024, tc / 1024,
            [e[:2] for e in p["env"]], " (the whole record: no envelope)" if p["whole"] else ""))
        if w["kind"] == "homopolymer":
            assert not p["whole"] and [e[:2] for e in p["env"]] == [(1, len(w["rec"]))]       # envelope detection lists the whole homopolymer
            assert p["fwd"] >= ga and corrected < ga and corrected_f64 < ga
        else:
            assert corrected >= tc and corrected_f64 >= tc
            assert w["kind"] != "planted" or p["seq_bias"] > 20 * 1024                        # the planted run costs bits and the hit stays a hit
        seen += 1
    assert seen == 6


@pytest.mark.parametrize("name", FIXTURES)
def test_held_to_the_files_forward_statistics(name):
    """the check of tests/test_hmm_forward_cpu.py (400 background records of 100 residues, seed 977, the 0.96 quantile within 1.5 bits of
    tau + ln(25) / lambda) on corrected scores. The bias is never negative, so the 17th largest corrected score is decided among the records with the
    largest uncorrected scores: the 48 best get their envelopes and their bias, and the 17th largest corrected score of those must be at least the
    49th uncorrected score, else more would have to be computed."""
    m = model(name)
    (st, has), = F.stats_lines(open(W.fixture_path(name), "rb").read())
    tau, lam = st[4], st[5]
    rng = np.random.default_rng(977)
    recs = [R.background(rng, 100) for _ in range(400)]
    fwd = F.forward_batch(m["tables"], recs).astype(np.int64)
    order = np.argsort(-fwd, kind="stable")
    best = order[:48]
    bias = np.array([N.pair(m["tables"], recs[r])["seq_bias"] for r in best], np.int64)
    corrected = np.sort(fwd[best] - bias)[::-1]
    assert (bias >= 0).all() and corrected[16] >= fwd[order[48]]
    measured, plain = corrected[16] / 1024.0, float(np.sort(fwd)[int(0.96 * 400) - 1]) / 1024.0
    predicted = tau + math.log(25.0) / lam
    print("%s: 0.96 quantile %.3f bits corrected, %.3f uncorrected, predicted %.3f; largest bias of the 48 best %.3f bits" % (name, measured, plain, predicted, bias.max() / 1024.0))
    assert abs(measured - predicted) <= 1.5
    assert BG_BIAS_BOUND_UNITS[name] / 16 < int(bias.max()) <= BG_BIAS_BOUND_UNITS[name]


def test_writers():
    models = [model(n) for n in FIXTURES]
    stats = [F.stats_lines(open(W.fixture_path(n), "rb").read())[0] for n in FIXTURES]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    seqs = [c0[:60] + b"K" * 40 + c0[60:], c1 + c1, b"K" * 121, c0]
    ids = ["a", "b", "k", "c"]
    fwd = F.search_forward(models, seqs)[1]
    cand = [(r, p) for r in range(len(seqs)) for p in range(2) if fwd[r, p] != R.NO_SCORE and fwd[r, p] >= 0]
    pr, pp = np.array([r for r, _ in cand], np.uint32), np.array([p for _, p in cand], np.uint32)
    _, _, ne, env = P.envelope_pairs(models, seqs, pr, pp, 8)
    slots, sb, n2, occM, occI = N.null2_pairs(models, seqs, pr, pp, ne, env, 8)
    sbias = np.zeros(fwd.shape, np.int64)
    sbias[pr, pp] = sb
    text = N.table_bytes(models, stats, ids, fwd, sbias)
    print(text.decode())
    assert text == TABLE
    listed = N.listed_pairs(models, fwd, sbias)
    at = {rp: j for j, rp in enumerate(cand)}
    j = [at[rp] for rp in listed]
    etext = N.envelope_table_bytes(models, ids, listed, ne[j], env[j], slots[j])
    print(etext.decode())
    assert etext == ENV_TABLE
    assert n2.shape == (len(cand), 8, 20) and len(occM[at[1, 1]]) == 2 and occM[at[1, 1]][0].shape == (57,) and not slots[at[1, 1], 2:].any()


TABLE = (b"target\tprofile\tacc\tbits\tevalue\tpass_ga\tbias\n"
         b"c\tRibosomal_S9\tPF00380.20\t192.82\t4.884E-61\t1\t2.45\n"
         b"a\tRibosomal_S9\tPF00380.20\t155.65\t1.599E-49\t1\t32.27\n"
         b"k\tRibosomal_S9\tPF00380.20\t-87.18\t4.000E+00\t0\t126.83\n"
         b"b\tTIGR00964\tTIGR00964\t181.03\t5.224E-58\t1\t28.21\n")
ENV_TABLE = (b"target\tprofile\tacc\tenv\tn_env\ti_from\ti_to\tenv_bits\tpeak_occ\tenv_bias\n"
             b"c\tRibosomal_S9\tPF00380.20\t1\t1\t1\t121\t192.82\t1.000\t2.45\n"
             b"a\tRibosomal_S9\tPF00380.20\t1\t1\t1\t161\t155.65\t1.000\t32.27\n"
             b"k\tRibosomal_S9\tPF00380.20\t1\t1\t1\t121\t-87.18\t0.951\t126.83\n"
             b"b\tTIGR00964\tTIGR00964\t1\t2\t1\t57\t93.90\t1.000\t10.11\n"
             b"b\tTIGR00964\tTIGR00964\t2\t2\t58\t114\t93.90\t1.000\t10.11\n")
