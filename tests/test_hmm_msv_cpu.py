"""The MSV prefilter without a GPU (SPEC 13.3): the restatement (tests/pyref_hmm_msv.py) against its naive yardstick, the model held to the
reference's data - the STATS LOCAL MSV lines of the two profile files under tests/golden/hmm - the floor arithmetic of the library, and the condition
the device tests lean on: no pair of the planted inputs at or above the gathering cutoff falls below the MSV floor of P = 0.02."""
import math

import numpy as np
import pytest

import gsearch_amd as G
import hmm_msv_case as MC
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_msv as V

INT32_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def fx():
    return MC.fixtures()


@pytest.fixture(scope="module")
def background_msv(fx):
    """MSV bits of 2 000 iid background records of 200 residues against each committed profile, once"""
    rng = np.random.default_rng(11)
    recs = [R.background(rng, 200) for _ in range(2000)]
    return [V.msv_batch(m["tables"], recs) / 1024.0 for m in fx["models"]]


def test_restatement_equals_its_naive_yardstick(fx):
    rng = np.random.default_rng(5)
    tabs = [R.parse_hmm(R.write_hmm(R.synth_model(np.random.default_rng(M), M)))[0]["tables"] for M in (1, 2, 65, 129)] + [m["tables"] for m in fx["models"]]
    for tab in tabs:
        c = R.consensus(tab)
        recs = [R.background(rng, n) for n in (1, 2, 63, 64, 65)] + [R.background(rng, 60) + c[:80] + R.background(rng, 200 - 60 - len(c[:80]))]
        assert [len(r) for r in recs] == [1, 2, 63, 64, 65, 200]
        want = [V.msv_naive(tab, r) for r in recs]
        assert [V.msv(tab, r) for r in recs] == want
        assert V.msv_batch(tab, recs).tolist() == want
    assert V.msv(tabs[0], b"") == V.msv_naive(tabs[0], b"") == R.NO_SCORE and V.msv(tabs[0], b"AC*D") == V.msv_naive(tabs[0], b"AC*D") == R.NO_SCORE
    assert V.msv_batch(tabs[2], [b"", b"ACD", b"A-C"]).tolist()[::2] == [R.NO_SCORE, R.NO_SCORE]


@pytest.mark.parametrize("p", [0, 1])
def test_background_scores_follow_the_files_msv_gumbel(fx, background_msv, p):
    """the first 200 of the background records: their median within 0.75 bit of mu - ln(ln 2) / lambda of the file's STATS LOCAL MSV line - the bound
    test_background_scores_follow_the_files_gumbel holds Viterbi to, for the same reason. Measured offsets (sample median - the file's): +0.01 and
    -0.03 bit at n = 200, +0.16 and +0.22 bit over all 2 000 (SPEC 13.3)."""
    (mu, lam), has = fx["stats"][p][0][:2], fx["stats"][p][1]
    assert has & 1
    want = mu - math.log(math.log(2)) / lam
    sc = np.sort(background_msv[p][:200])
    median = (sc[99] + sc[100]) / 2
    print(MC.FIXTURES[p], "MSV sample median", median, "file's Gumbel median", want, "offset", median - want, "offset at n = 2000", np.median(background_msv[p]) - want)
    assert abs(median - want) <= 0.75


@pytest.mark.parametrize("p", [0, 1])
def test_the_gate_passes_what_it_says(fx, background_msv, p):
    """of 2 000 background records the number at or above msv_floor(0.02) lies within a factor of 2 of 0.02 * 2 000 = 40: one bit either way at
    lambda ~ ln 2, the slack of the median test plus sampling. Measured: 52 and 70 (SPEC 13.3)."""
    floor = V.floors(fx["stats"])[p]
    n = int((np.round(background_msv[p] * 1024).astype(np.int64) >= floor).sum())
    print(MC.FIXTURES[p], "floor (bits)", floor / 1024.0, "passing of 2000", n)
    assert 20 <= n <= 80


def test_consensus_is_far_above_the_floor(fx):
    floors = V.floors(fx["stats"])
    for p, m in enumerate(fx["models"]):
        s = V.msv(m["tables"], fx["cons"][p])
        print(MC.FIXTURES[p], "consensus MSV bits", s / 1024.0, "floor bits", floors[p] / 1024.0)
        assert s - floors[p] > 50 * 1024


def test_msv_bounds_viterbi_without_gap_states():
    """a profile whose m->i and m->d are all `*`: Viterbi is MSV's model plus non-positive tMM, so msv >= vit on the integers"""
    rng = np.random.default_rng(9)
    for M in (5, 70, 150):
        s = R.synth_model(np.random.default_rng(M), M)
        for k in range(M + 1):
            mm = s["tr"][k][0]
            s["tr"][k] = [mm, 0.0, 0.0, s["tr"][k][3], s["tr"][k][4], s["tr"][k][5], s["tr"][k][6]]
        m = R.parse_hmm(R.write_hmm(s))[0]
        tab = m["tables"]
        assert (tab[R.ROW_MI] == R.STAR).all() and (tab[R.ROW_MD] == R.STAR).all() and (tab[R.ROW_MM, :M] < 0).any()
        c = R.consensus(tab)
        recs = [R.background(rng, n) for n in (1, 30, 64, 200)] + [c, R.background(rng, 20) + c[:M // 2 + 1] + R.background(rng, 20) + c[M // 2:], c + c]
        msv, vit = V.msv_batch(tab, recs).astype(np.int64), R.viterbi_batch(tab, recs).astype(np.int64)
        assert (msv >= vit).all() and (msv > vit).any(), (M, msv, vit)


def test_msv_is_no_bound_of_viterbi_in_general(fx):
    """SPEC 13.3 says so: it drops the gap states (below Viterbi where a gap pays) and the cost of m->m (above it on an ungapped match)"""
    tab, c = fx["models"][0]["tables"], fx["cons"][0]
    assert V.msv(tab, c) > R.viterbi(tab, c)
    gapped = c[:60] + b"W" + c[60:]                                              # one inserted residue: an insert is cheaper than leaving and entering again
    assert V.msv(tab, gapped) < R.viterbi(tab, gapped)


def test_planted_inputs_lose_nothing_at_the_gathering_cutoff(fx):
    """the condition the end-to-end device tests lean on, on the restatement alone: every pair of the planted inputs with vit >= GA1 - or
    fwd >= GA1, the score="forward" runs - has msv >= msv_floor(0.02)"""
    models, floors = fx["models"], V.floors(fx["stats"])
    ga = np.array([m["ga_units"] for m in models], np.int64)
    _, seqs = MC.faa_case()
    _, proteins = MC.genome_case()
    for name, recs in (("faa", list(seqs)), ("genome", list(proteins))):
        msv = V.search(models, recs)
        vit = R.search(models, recs)
        _, fwd = F.search_forward(models, recs, floor=F.floors(models), vit=vit)
        passed = V.passes(msv, floors)
        hit_v, hit_f = vit.astype(np.int64) >= ga[None, :], (fwd != R.NO_SCORE) & (fwd.astype(np.int64) >= ga[None, :])
        print(name, "pairs", msv.size, "pass the MSV floor", int(passed.sum()), "Viterbi hits", int(hit_v.sum()), "Forward hits", int(hit_f.sum()))
        assert hit_v.sum() >= 2 and hit_f.sum() >= hit_v.sum()
        assert passed[hit_v].all() and passed[hit_f].all()
        assert 0 < passed.sum() < msv.size                                     # the filter does filter on these inputs


def test_floor_arithmetic_equals_the_double_formula(fx):
    for mu, lam in [tuple(fx["stats"][p][0][:2]) for p in (0, 1)] + [(-8.5, 0.7), (-11.25, 0.69314)]:
        for P in (0.02, 1e-3):
            want = int(math.floor((mu - math.log(-math.log1p(-P)) / lam) * 1024.0 + 0.5))
            assert G.hmm_viterbi_floor(mu, lam, P) == V.msv_floor(mu, lam, P) == want
    text = fx["texts"][0]
    assert V.floors(F.stats_lines(text)).tolist() == [V.msv_floor(*fx["stats"][0][0][:2])]
    bare = b"\n".join(ln for ln in text.split(b"\n") if not ln.startswith(b"STATS LOCAL MSV"))
    assert bare != text and V.floors(F.stats_lines(bare)).tolist() == [INT32_MIN + 1] == [V.FLOOR_ALL]
    st, has = G.hmm_parse_stats(bare)
    assert not has & 1 and has & 2 and G.hmm_parse_stats(text)[1] & 1
