"""SPEC 13.4 on the CPU: the restatement tests/pyref_hmm_posterior.py (blocked integer Backward, occupancy, runs, envelopes, envelope scores) against its
own cell-by-cell f64 yardstick, against the hand cases the issue and the spec give, and on the identities that hold on the integers. No library call.

The two bounds are measured over the inputs below and asserted at four times the measurement rounded up to a power of two, the margin SPEC 13.1 takes
for Forward (another seed must not trip it): the largest deviation of a kept Backward row from the f64 one is 13.6 units (asserted 64), the largest
|bN[0] - total_f| on the integers is 9 units (asserted 64; in f64 the two agree to 1e-6 unit). Both maxima are reached on the hand cases, which are
measured with the other inputs."""
import os

import numpy as np
import pytest

import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_posterior as P

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture_path(name):
    return os.path.join(HERE, "golden", "hmm", name)


ROW_MEASURED = 14         # 13.6 units, rounded up
ROW_BOUND = 64            # 4 * 13.6 = 54.4 -> 64
TOTAL_BOUND = 64          # measured 9: 36 -> 64
SYN_M = (1, 2, 65, 129)


@pytest.fixture(scope="module")
def world():
    """the profiles, the records of each and both computations of every pair, once"""
    rng = np.random.default_rng(1349)
    models = [R.parse_hmm(open(fixture_path(n), "rb").read())[0] for n in ("PF00380.20.HMM", "TIGR00964.HMM")]
    models += [R.parse_hmm(R.write_hmm(R.synth_model(rng, M)))[0] for M in SYN_M]
    pairs = []
    for m in models:
        tab, M = m["tables"], m["M"]
        c = R.consensus(tab)
        recs = [R.background(rng, 1), R.background(rng, 64), R.background(rng, 200), c, c + c, R.background(rng, 30) + c[:max(M // 2, 1)] + R.background(rng, 30)]
        if M > 100:
            recs.append(c[:30] + c[100:])                                              # a 70-node deletion
        for rec in recs:
            pairs.append({"M": M, "tab": tab, "rec": rec, "planted": None})
    pairs += [{"M": tab.shape[1] - 1, "tab": tab, "rec": rec, "planted": planted} for tab, rec, planted in hand_cases()]
    for w in pairs:
        w["int"], w["f64"] = P.posterior(w["tab"], w["rec"], rows=True), P.posterior_f64(w["tab"], w["rec"])
    return pairs


def test_backward_rows_against_the_yardstick(world):
    worst = 0.0
    for w in world:
        for name in ("bN", "bJ"):
            got, ref = w["int"][name], w["f64"][name]
            fin = np.isfinite(ref)
            assert (got[~fin] == R.NEG).all() and not fin[-1] and fin[:-1].all()          # row L alone holds no probability
            worst = max(worst, float(np.abs(got[fin] - ref[fin]).max()))
    print("largest deviation of a kept Backward row: %.2f units" % worst)
    assert worst <= ROW_BOUND
    assert worst > ROW_BOUND / 16, "the bound is more than 16 times the measurement: measure again and lower it"


def test_backward_total_is_forward_total(world):
    worst_int, worst_f64 = 0, 0.0
    for w in world:
        assert w["int"]["fwd"] == F.forward(w["tab"], w["rec"])                          # the rows come from Forward as SPEC 13.1 orders it
        worst_int = max(worst_int, abs(w["int"]["bck"] - w["int"]["fwd"]))
        worst_f64 = max(worst_f64, abs(w["f64"]["total_b"] - w["f64"]["total_f"]))
    print("largest |bN[0] - total_f|: %d units on the integers, %.2e in f64" % (worst_int, worst_f64))
    assert worst_f64 < 1e-6 and worst_int <= TOTAL_BOUND
    assert worst_int > TOTAL_BOUND / 16


def hand_cases():
    """(table, record, the planted copies): the background draws are seeded, the coordinates follow from the lengths. The seed is the first from 5 on
    under which every case keeps the margin test_hand_cases asserts (with 5, 7 and 8 a background row comes within 13 units of LO; with 6 chance puts
    more than the planted copies into the background)"""
    rng = np.random.default_rng(9)
    cases = []
    for p, name in enumerate(("PF00380.20.HMM", "TIGR00964.HMM")):
        tab = R.parse_hmm(open(fixture_path(name), "rb").read())[0]["tables"]
        c, M = R.consensus(tab), tab.shape[1] - 1
        bg = lambda n: R.background(rng, n)                                            # noqa: E731
        cases += [(tab, c, [(1, M)]), (tab, c + c, [(1, M), (M + 1, 2 * M)]),
                  (tab, bg(40) + c + bg(60) + c + bg(30), [(41, 40 + M), (101 + M, 100 + 2 * M)]),
                  (tab, bg(5) + c + bg(3) + c, [(6, 5 + M), (9 + M, 8 + 2 * M)])]
        if p == 0:
            cases.append((tab, c + c + c[:60], [(1, 121), (122, 242), (243, 302)]))
    return cases


def test_hand_cases(world):
    got = []
    for w in world:
        if w["planted"] is None:
            continue
        p, y, planted = w["int"], w["f64"], w["planted"]
        assert [(a, b) for a, b, _ in P.runs(y["out"], y["cont"])] == planted              # the yardstick finds exactly the planted copies
        assert [e[:2] for e in p["env"]] == planted                                        # and so do the integers
        got.append(planted)
        # the condition under which both must agree: no row decides within twice the measured Backward deviation of a threshold, and no row of
        # the integers is as far from the f64 one as it is from a threshold
        for rows, ref in ((p["out"][1:], y["out"][1:]), (p["cont"][1:], y["cont"][1:])):
            for thr in (P.LO, P.HI):
                assert np.abs(rows - thr).min() > 2 * ROW_MEASURED, (planted, thr, int(np.abs(rows - thr).min()))
                assert (np.abs(rows - ref) < np.abs(rows - thr)).all()
    assert len(got) == 9 and got[1] == [(1, 121), (122, 242)] and got[2] == [(41, 161), (222, 342)] and got[3] == [(6, 126), (130, 250)] and got[4] == [(1, 121), (122, 242), (243, 302)]
    assert got[5:] == [[(1, 57)], [(1, 57), (58, 114)], [(41, 97), (158, 214)], [(6, 62), (66, 122)]]


def test_the_cont_rule_is_what_separates_touching_copies():
    tab, rec, planted = hand_cases()[1]
    p = P.posterior(tab, rec, rows=True)
    assert [(a, b) for a, b, _ in P.runs(p["out"], p["cont"], use_cont=False)] == [(1, 242)] and len(planted) == 2


def test_identities_on_the_integers(world):
    n_whole = 0
    for w in world:
        env, L = w["int"]["env"], len(w["rec"])
        for a, b, raw, peak in env:
            assert 1 <= a <= b <= L and peak <= P.HI and peak == w["int"]["out"][a:b + 1].min()
            if (a, b) == (1, L):
                assert raw == w["int"]["fwd"]
                n_whole += 1
        assert all(env[d][1] < env[d + 1][0] for d in range(len(env) - 1))                # disjoint and ascending
    assert n_whole >= 6                                                                    # the consensus alone, in every profile
    assert sum(len(w["int"]["env"]) >= 2 for w in world) >= 4


def test_pair_lists_and_the_table_of_hmmsearch():
    models = [R.parse_hmm(open(fixture_path(n), "rb").read())[0] for n in ("PF00380.20.HMM", "TIGR00964.HMM")]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    rng = np.random.default_rng(7)
    seqs = [R.background(rng, 20) + c0, c1 + R.background(rng, 10) + c1, b"", b"ACDX"]
    pr, pp = np.array([0, 1, 1, R.NO_HIT, 2, 3], np.uint32), np.array([0, 1, 1, 0, 0, 1], np.uint32)
    fwd, bck, ne, env, outs, conts = P.envelope_pairs(models, seqs, pr, pp, 1, rows=True)
    assert ne.tolist() == [1, 2, 2, 0, 0, 0] and (fwd[3:] == R.NO_SCORE).all() and (bck[3:] == R.NO_SCORE).all() and not env[3:].any()
    assert env[:, 0, :2].tolist()[:3] == [[21, 141], [1, 57], [1, 57]] and outs[3] is None and len(outs[1]) == 124 == len(conts[2])
    _, _, ne, env = P.envelope_pairs(models, seqs, pr[:2], pp[:2], 8)
    text = P.envelope_table_bytes(models, ["a", "b"], [(0, 0), (1, 1)], ne, env)
    assert text == (b"target\tprofile\tacc\tenv\tn_env\ti_from\ti_to\tenv_bits\tpeak_occ\n"
                    b"a\tRibosomal_S9\tPF00380.20\t1\t1\t21\t141\t194.41\t1.000\n"
                    b"b\tTIGR00964\tTIGR00964\t1\t2\t1\t57\t103.72\t1.000\n"
                    b"b\tTIGR00964\tTIGR00964\t2\t2\t68\t124\t103.72\t1.000\n")
    assert P.listed_pairs(models, np.array([[5, R.NO_SCORE], [-1, 9], [7, 9]], np.int32)) == [(2, 0), (0, 0), (1, 1), (2, 1)]
