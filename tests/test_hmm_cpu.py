"""hmmsearch without a GPU (SPEC 13): the library's parser, integer tables and length model against the numpy restatement, the restatement against
its naive yardstick, the refusals, and the model held to the reference's own data: the two profile files under tests/golden/hmm carry their
cutoffs (TC) and their calibrated score distribution (STATS LOCAL VITERBI mu lambda)."""
import math
import os

import numpy as np
import pytest

import gsearch_amd as G
import pyref_hmm as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")


def fixture(name):
    return open(os.path.join(HERE, "golden", "hmm", name), "rb").read()


def without_compo(text):
    lines = text.split(b"\n")
    out = [ln for ln in lines if not ln.strip().startswith(b"COMPO")]
    assert len(out) == len(lines) - text.count(b"  COMPO ")
    return b"\n".join(out)


def check_against_restatement(text):
    ref = R.parse_hmm(text)
    for i, m in enumerate(ref):
        info, tab, n = G.hmm_parse(text, i)
        assert n == len(ref)
        assert tab.dtype == np.int32 and tab.shape == m["tables"].shape and np.array_equal(tab, m["tables"])
        for key in ("name", "acc", "M", "ga", "tc", "nc", "mu", "lam", "ga_units"):
            assert info[key] == m[key], (key, info[key], m[key])
        assert info["tbm"] == R.specials(1, m["M"])[3]
    return ref


def test_fixtures_parse_like_the_restatement():
    a, b = fixture(FIXTURES[0]), fixture(FIXTURES[1])
    assert a.startswith(b"HMMER3/f") and b.startswith(b"HMMER3/b") and b"COMPO" in a and b"COMPO" in b
    for text in (a, b, a + b, b + b"\n\n" + a):
        assert len(check_against_restatement(text)) == text.count(b"\n//")
        check_against_restatement(without_compo(text))
    m = R.parse_hmm(a)[0]
    assert (m["name"], m["acc"], m["M"], m["ga"], m["tc"]) == ("Ribosomal_S9", "PF00380.20", 121, (22.1, 22.1), (22.6, 22.1))
    assert R.parse_hmm(b)[0]["ga"] == (27.55, 27.55)                          # `GA    27.55 27.55;`


@pytest.mark.parametrize("M,dialect", [(1, "f"), (2, "b"), (63, "f"), (65, "b"), (300, "f"), (R.MAX_M, "b")])
def test_synthetic_models_parse_like_the_restatement(M, dialect):
    s = R.synth_model(np.random.default_rng(M), M)
    for compo in (True, False):
        text = R.write_hmm(s, dialect, compo)
        (m,) = check_against_restatement(text)
        assert m["M"] == M and m["tables"][:20, 1:].max() > 0 and (m["tables"][20:] <= 0).all()
    none = R.write_hmm(dict(s, ga=None, acc=""), dialect)
    info, _, _ = G.hmm_parse(none)
    assert info["ga"] is None and info["ga_units"] is None and info["acc"] == "" and R.parse_hmm(none)[0]["ga_units"] is None


def test_file_units_edges():
    """the conversion of SPEC 13 "Units": C and s literal, half-up rounding of the magnitude, `*`, and the refusals of the number format"""
    assert R.file_units("0.00000") == 0 and R.file_units("*") == R.STAR == -(1 << 18)
    assert R.file_units("0.69315") == -1024                                    # ln 2 nats = one bit
    assert R.file_units("99.99999") == -147732 and R.file_units("99.99999") > R.STAR
    for tok in ("2.43118", "0.00956", "10.5", "3"):
        exact = float(tok) / math.log(2) * 1024
        assert abs(-R.file_units(tok) - exact) <= 0.5 + 1e-3
    for bad in ("1.234567", "100.00000", "-0.5", "1e-3", "abc", "1."):
        with pytest.raises(R.HmmError):
            R.file_units(bad)
    assert R.bits_units("22.10") == 22630 and R.bits_units("27.55") == 28211 and R.bits_units("-1.5") == -1536 and R.bits_units("25") == 25600
    assert abs(sum(2.0 ** (b / 1024.0) for b in R.BG) - 1.0) < 2e-4             # the 20 literal background scores are a distribution


def test_specials_match_the_restatement_and_numpy():
    Ls = list(range(1, 4097))
    k = 13
    while (1 << k) <= R.MAX_L:
        Ls += [x for x in ((1 << k) - 1, 1 << k, (1 << k) + 1) if x <= R.MAX_L]
        k += 1
    assert Ls[-1] == R.MAX_L
    for L in Ls:
        M = 1 + (L * 7) % R.MAX_M
        got = G.hmm_specials(L, M)
        assert got == R.specials(L, M), (L, M)
        tloop, tmove, null, tbm, nloop, nmove = got
        # every logarithm within one unit of numpy's
        for mine, num, den in ((tloop, L, L + 3), (tmove, 3, L + 3), (nloop, L, L + 1), (nmove, 1, L + 1), (tbm, 2, M * (M + 1))):
            assert abs(mine - 1024.0 * (np.log2(float(num)) - np.log2(float(den)))) <= 1.0, (L, M, mine, num, den)
        assert null == L * nloop + nmove
    for n in [1, 2, 3, 5, 1000, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]:
        assert abs(R.lgq(n) / float(1 << 20) - np.log2(float(n))) < 4.0 / (1 << 20)
    for L, M in ((0, 5), (5, 0)):
        with pytest.raises(G.GsError) as e:
            G.hmm_specials(L, M)
        assert e.value.code == -1
    for L, M in ((R.MAX_L + 1, 5), (5, R.MAX_M + 1)):
        with pytest.raises(G.GsError) as e:
            G.hmm_specials(L, M)
        assert e.value.code == -3


def test_restatement_equals_its_naive_yardstick():
    rng = np.random.default_rng(5)
    for M in (1, 2, 3, 4, 5):
        s = R.synth_model(rng, M)
        tab = R.parse_hmm(R.write_hmm(s, "b" if M % 2 else "f"))[0]["tables"]
        recs = [R.background(rng, L) for L in range(0, 9)] + [R.consensus(tab), R.consensus(tab) * 2, R.consensus(tab)[:1] + R.consensus(tab)[2:], b"W" * 8]
        for rec in recs:
            if len(rec) <= 8:
                assert R.viterbi(tab, rec) == R.viterbi_naive(tab, rec), (M, rec)
    assert R.viterbi(tab, b"") == R.NO_SCORE


def refused(text, code=-1):
    with pytest.raises(G.GsError) as e:
        G.hmm_parse(text)
    assert e.value.code == code, e.value
    with pytest.raises(R.HmmError):
        R.parse_hmm(text)


def test_refusals():
    good = fixture("TIGR00964.HMM")
    G.hmm_parse(good)
    refused(good.replace(b"ALPH  amino", b"ALPH  DNA"))
    refused(good[: len(good) // 2])                                              # truncated inside a node
    refused(good[: good.rindex(b"//")])                                          # the closing line is missing
    refused(good[: good.rindex(b"//")] + good)                                   # ... and the next model starts instead
    lines = good.split(b"\n")
    at = [i for i, ln in enumerate(lines) if ln.split()[:1] == [b"7"]][0]
    swapped = list(lines)
    swapped[at] = swapped[at].replace(b"      7 ", b"      8 ", 1)
    assert swapped != lines
    refused(b"\n".join(swapped))                                                 # a node number out of order
    refused(good.replace(b"2.87956", b"2.879561", 1))                            # six decimals
    refused(good.replace(b"LENG  57", b"LENG  58"))                              # LENG says more nodes than the file has
    s = R.synth_model(np.random.default_rng(3), 4)
    big = R.write_hmm(s).replace(b"LENG  4", b"LENG  %d" % (R.MAX_M + 1))
    refused(big, code=-3)                                                        # M > GS_HMM_MAX_M: unsupported, not invalid
    refused(b"")
    refused(b"NAME x\n")


@pytest.fixture(scope="module")
def models():
    return {n: R.parse_hmm(fixture(n))[0] for n in FIXTURES}


@pytest.mark.parametrize("name", FIXTURES)
def test_consensus_clears_the_trusted_cutoff(models, name):
    m = models[name]
    cons = R.consensus(m["tables"])
    one = R.viterbi(m["tables"], cons)
    print(name, "consensus", one / 1024.0, "bits, TC1", m["tc"][0])
    assert one / 1024.0 >= m["tc"][0]
    if name == "PF00380.20.HMM":
        assert abs(one / 1024.0 - 194.7) < 0.5                                   # the figure a float model of the same profile gives
    two = R.viterbi(m["tables"], cons + R.background(np.random.default_rng(7), 50) + cons)
    print(name, "two copies", two / 1024.0)
    assert two > one                                                             # the second copy is reached through J


@pytest.mark.parametrize("name", FIXTURES)
def test_background_scores_follow_the_files_gumbel(models, name):
    """200 iid background sequences of length 200: their median within 0.75 bit of mu - ln(ln 2) / lambda of the file's STATS LOCAL VITERBI line
    (0.33 bit measured offset of a float model + 3 standard errors of 0.144 of a Gumbel median at n = 200, lambda = 0.71)"""
    m = models[name]
    rng = np.random.default_rng(20261018)
    sc = sorted(R.viterbi(m["tables"], R.background(rng, 200)) / 1024.0 for _ in range(200))
    median = (sc[99] + sc[100]) / 2
    want = m["mu"] - math.log(math.log(2)) / m["lam"]
    print(name, "sample median", median, "file's Gumbel median", want)
    assert abs(median - want) <= 0.75


def test_evalue_is_the_double_formula():
    for bits in (-20.0, -9.8, 0.0, 5.5, 22.1, 60.0, 194.67, 400.0):
        for mu, lam in ((-10.5953, 0.71333), (-8.6216, 0.719)):
            for Z in (1.0, 4000.0):
                want = Z * R.pvalue(bits, mu, lam)
                got = G.hmm_evalue(bits, mu, lam, Z)
                assert got == want or abs(got - want) <= 1e-9 * abs(want), (bits, mu, lam, Z, got, want)
    assert G.hmm_evalue(-20.0, -10.0, 0.7, 3.0) == pytest.approx(3.0) and 0 < G.hmm_evalue(300.0, -10.0, 0.7, 1.0) < 1e-80
    assert G.hmm_bits(22630) == 22630 / 1024.0 and G.hmm_bits(-1) == -1 / 1024.0
    assert G.hmm_threshold_units(22.1) == R.threshold_units(22.1) == 22630 and G.hmm_threshold_units(-0.5) == R.threshold_units(-0.5) == -512


def test_batched_restatement_equals_the_single_one(models):
    """tests/test_gpu_hmm.py takes its expected scores from search(): many records of mixed lengths at once"""
    rng = np.random.default_rng(11)
    tabs = [models[n]["tables"] for n in FIXTURES] + [R.parse_hmm(R.write_hmm(R.synth_model(rng, M)))[0]["tables"] for M in (1, 2, 65)]
    for tab in tabs:
        cons = R.consensus(tab)
        recs = [b"", R.background(rng, 1), R.background(rng, 70), cons, cons + R.background(rng, 9) + cons, b"", b"K" * 33, cons[: len(cons) // 2]]
        got = R.viterbi_batch(tab, recs)
        assert got.dtype == np.int32 and [int(v) for v in got] == [R.viterbi(tab, r) for r in recs]
