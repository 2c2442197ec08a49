"""The inputs of tests/test_gpu_hmm_classes.py held to their purpose, without a GPU. That file runs every kernel class of gs_hmm.hip (Q = 1, 2, 3, 4,
6, 8, 12, 16, 20 nodes per lane) and wants each of the six steps of the lane scan to carry weight in an expected score. Whether it does is a
property of the profiles and records (tests/hmm_classes_case.py), so it is measured here on the restatement: the blocked row step with the scan cut
off after NS steps must give another score than the whole scan, for Viterbi (join = max) and for Forward (join = lse). Beside that: the blocked form
with max is SPEC 13's Viterbi, the integer Forward against the cell-by-cell f64 one at the group sizes test_hmm_forward_cpu.py does not reach, the
library's parser on the new sizes, and a spot check that tests/golden/hmm_limits.json is the restatement's."""
import json
import os

import numpy as np
import pytest

import gsearch_amd as G
import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_forward as F

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND_UNITS = 64                      # |restatement - f64| at most, in units of 2^-10 bit: the bound of test_hmm_forward_cpu.py


def profile(M):
    (m,) = R.parse_hmm(K.model_text(M))
    return m


@pytest.mark.parametrize("M", K.CLASS_M)
def test_every_scan_step_carries_an_expected_score(M):
    """Step s of the scan hands lane l what left lane l - 2^s, and lane l + 1 takes it as c_in: it can show only in a profile with a node in lane
    2^s + 1 or above. M = 65 has two nodes per lane in lanes 0 .. 32, so its step 5 reaches no node and cutting it changes nothing, which is asserted
    as such; everywhere else every cut must show in one of the six records."""
    m = profile(M)
    tab = m["tables"]
    recs = K.deletion_records(R.consensus(tab), M)
    assert len(recs) == 6 and max(len(r) for r in recs) <= 50
    lanes = -(-M // F.group_size(M))
    vit = F.blocked_batch(tab, recs, join=np.maximum)
    assert np.array_equal(vit, R.viterbi_batch(tab, recs))
    fwd = F.forward_batch(tab, recs)
    assert np.array_equal(fwd, F.blocked_batch(tab, recs, scan_steps=6, join=F.lse))
    assert vit[0] > m["ga_units"] and (fwd >= vit).all()
    for ns in range(6):
        cut_v = F.blocked_batch(tab, recs, scan_steps=ns, join=np.maximum)
        cut_f = F.blocked_batch(tab, recs, scan_steps=ns)
        changed = (int((cut_v != vit).sum()), int((cut_f != fwd).sum()))
        print("M = %d, scan cut after %d steps: %d Viterbi and %d Forward scores of 6 change" % ((M, ns) + changed))
        if lanes >= (1 << ns) + 2:
            assert changed[0] >= 1 and changed[1] >= 1, (M, ns, changed)
        else:
            assert (M, ns, lanes) == (65, 5, 33) and changed == (0, 0)
        assert (cut_v <= vit).all() and (cut_f <= fwd).all()                    # a cut only takes paths away


@pytest.mark.parametrize("M", [193, 257, 385, 513, 769, 1025])
def test_restatement_against_the_f64_forward_at_the_larger_groups(M):
    """G = 4, 6, 8, 12, 16 and 20 nodes per group, an ordinary and a deletion-friendly profile each, two records of 24 residues that leave out most
    of the profile. Measured: at most 4.3 units on the ordinary profiles and 6.0 on the deletion-friendly ones, of the 64 allowed."""
    assert F.group_size(M) == {193: 4, 257: 6, 385: 8, 513: 12, 769: 16, 1025: 20}[M]
    for s in (R.synth_model(np.random.default_rng(M), M), K.deletion_model(M)):
        tab = R.parse_hmm(R.write_hmm(s))[0]["tables"]
        c = R.consensus(tab)
        recs = [c[:12] + c[M - 12:], c[5:17] + c[M // 2:M // 2 + 12]]
        fwd = F.forward_batch(tab, recs)
        for rec, got in zip(recs, fwd):
            f64 = F.forward_f64(tab, rec)
            print("M = %d %s: int - f64 = %.2f units" % (M, s["name"], got - f64))
            assert abs(got - f64) <= BOUND_UNITS, (M, s["name"], int(got), f64)
            assert got > 30 * 1024                                               # a hit, not noise


@pytest.mark.parametrize("M", K.SET_ORDER)
def test_the_sets_profiles_parse_like_the_restatement(M):
    text = K.model_text(M)
    (m,) = R.parse_hmm(text)
    info, tab, n = G.hmm_parse(text)
    assert n == 1 and info["M"] == m["M"] == M and info["name"] == m["name"] and info["ga_units"] == m["ga_units"]
    assert tab.dtype == np.int32 and tab.shape == m["tables"].shape and np.array_equal(tab, m["tables"])
    assert info["tbm"] == R.specials(1, M)[3]
    if M in K.CLASS_M:
        dd = m["tables"][R.ROW_DD, 1:M]
        assert (dd >= -3).all() and (dd <= 0).all()                             # 0.998 .. 0.9995: at most 3 units a node


def test_set_covers_both_sides_of_every_class_edge():
    assert sorted(K.SET_ORDER) == sorted(K.CLASS_M + K.ORDINARY_M) and list(K.SET_ORDER) != sorted(K.SET_ORDER)
    assert {F.group_size(M) for M in K.SET_ORDER} == set(F.CLASS_G)
    for g in F.CLASS_G[:-1]:
        assert 64 * g in K.CLASS_M and 64 * g + 1 in K.CLASS_M and F.group_size(64 * g) == g < F.group_size(64 * g + 1)
    assert R.MAX_M in K.CLASS_M


@pytest.fixture(scope="module")
def limits():
    with open(os.path.join(HERE, "golden", "hmm_limits.json")) as f:
        return json.load(f)["cases"]


def test_limit_profiles_are_what_they_are_called(limits):
    assert [(c["score"], c["kind"], c["M"], c["L"]) for c in limits] == list(K.LIMIT_CASES)
    for kind, M in {(c["kind"], c["M"]) for c in limits}:
        text = K.limit_text(kind, M)
        assert [c["sha256"] for c in limits if (c["kind"], c["M"]) == (kind, M)][0] == K.sha256(text)
        (m,) = R.parse_hmm(text)
        info, tab, _ = G.hmm_parse(text)
        assert np.array_equal(tab, m["tables"]) and info["M"] == M
        t = m["tables"]
        w = R.AA.index("W")
        if kind == "zero":
            assert (t[20:] == 0).all() and np.array_equal(t[:20, 1:], np.tile(-np.array(R.BG)[:, None], (1, M)))
        else:
            assert (t[w, 1:] == -R.BG[w]).all() and (np.delete(t[:20, 1:], w, axis=0) == R.STAR - np.delete(np.array(R.BG), w)[:, None]).all()
            assert (t[[R.ROW_MM, R.ROW_IM, R.ROW_DM]] == 0).all() and (t[[R.ROW_MI, R.ROW_MD, R.ROW_II, R.ROW_DD]] == R.STAR).all()
    # the cases reach where the range proofs of SPEC 13 and 13.1 matter, and stay inside them
    for c in limits:
        assert 0 < c["raw"] < (1 << 31)
        if c["score"] == "viterbi" and c["L"] >= (1 << 18) - 1:
            assert c["raw"] > (1 << 30)
        if c["score"] == "forward":
            assert (1 << 29) < c["raw"] <= c["max_cell"] + 22000 and c["max_cell"] < 1400000000 and c["max_hi_lo"] > (1 << 30)


def test_golden_limits_file_is_the_restatements(limits):
    """the 2^16 Viterbi case again, about two seconds; all seven take the generator three and a half minutes"""
    (c,) = [c for c in limits if c["score"] == "viterbi" and c["L"] == 1 << 16]
    (m,) = R.parse_hmm(K.limit_text(c["kind"], c["M"]))
    assert R.viterbi(m["tables"], b"W" * c["L"]) == c["raw"]
