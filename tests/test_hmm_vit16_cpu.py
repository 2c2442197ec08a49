"""The packed int16 Viterbi filter without a GPU (SPEC 13.7): the restatement (tests/pyref_hmm_vit16.py) against its naive yardstick, the properties the
filter rests on - vf >= vit, a measured excess, a lower clamp that is not sticky, a D scan whose form does not reach a score -, the overflow edge, the
inputs of the device tests, and on the reference's two profiles the claim itself: the pairs at or above a Viterbi floor are among those whose vf is.
The device inherits all of it through `==` with the restatement (tests/test_gpu_hmm_vit16.py)."""
import numpy as np
import pytest

import hmm_classes_case as HC
import hmm_msv_case as MC
import hmm_vit16_case as VC
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_trace as T
import pyref_hmm_vit16 as W

# vf - vit in units over the pairs of this file that do not overflow, measured (printed by the tests) and the bound asserted: the next power of two at
# or above twice the maximum, per family of records since the excess grows with what the path holds - half a unit of rounding a table word
#   300 background records of 200 residues, both committed profiles:   max 64, mean 19.9 and 14.4      -> 128
#   the 2 000 background records of the losslessness test:              max 96                          -> held to the 128 of the 300
#   consensus prefixes of 5, 10, .. residues up to the overflow:        max 65 (1.3 a residue)          -> 256
#   the deletion pairs of hmm_vit16_case, deletions of up to 1 257 nodes: max 706 (at most 1 a node)    -> 2048
EXCESS_BACKGROUND, EXCESS_PREFIX, EXCESS_DELETION = 128, 256, 2048


@pytest.fixture(scope="module")
def fx():
    return MC.fixtures()


def _pow2_at_or_above(x):
    return 1 << int(x - 1).bit_length()


def test_restatement_equals_its_naive_yardstick(fx):
    rng = np.random.default_rng(5)
    tabs = [R.parse_hmm(R.write_hmm(R.synth_model(np.random.default_rng(M), M)))[0]["tables"] for M in (1, 2, 3, 65, 129)] + [m["tables"] for m in fx["models"]]
    seen_over = 0
    for tab in tabs:
        c = R.consensus(tab)
        recs = [R.background(rng, n) for n in (1, 2, 63, 64, 65)] + [R.background(rng, 30) + c[:30] + R.background(rng, 40), c[:70]]
        want = [W.vit16_naive(tab, r) for r in recs]
        assert [W.vit16(tab, r) for r in recs] == want
        assert W.vit16_batch(tab, recs).tolist() == want
        seen_over += want.count(W.VF_OVER)
    assert seen_over >= 3                                                       # 70 consensus nodes are past 64 bits
    assert W.vit16(tabs[0], b"") == W.vit16_naive(tabs[0], b"") == R.NO_SCORE
    assert W.vit16_batch(tabs[3], [b"", b"ACD", b"A-C"]).tolist()[::2] == [R.NO_SCORE, R.NO_SCORE]
    bad = bytearray(R.consensus(tabs[3]) + R.consensus(tabs[3]))                # a byte that is no residue goes before the overflow in front of it
    bad[-1] = ord("*")
    assert W.vit16(tabs[3], bytes(bad[:-1])) == W.VF_OVER and W.vit16(tabs[3], bytes(bad)) == R.NO_SCORE


def test_half_units_of_the_committed_tables(fx):
    for m in fx["models"]:
        tab = m["tables"].astype(np.int64)
        t16 = W.tables16(m["tables"]).astype(np.int64)
        assert t16.dtype == np.int64 and W.tables16(m["tables"]).dtype == np.int16 and t16.shape == tab.shape
        star = tab == R.STAR
        assert star.any() and (t16[star] == W.NEG16).all()
        assert (t16[~star] == -((-tab[~star]) // 2)).all()                      # the ceiling of x / 2
        assert ((2 * t16 - tab)[~star] >= 0).all() and ((2 * t16 - tab)[~star] <= 1).all() and (2 * t16 >= tab).all()
    assert W.h(-65537) == W.NEG16 and W.h(-65536) == W.NEG16 and W.h(-65535) == -32767 and W.h(3) == 2 and W.h(-3) == -1 and W.h(R.NEG) == W.NEG16


def test_vf_bounds_viterbi_and_the_excess_is_what_was_measured(fx):
    rng = np.random.default_rng(17)
    bgs = [R.background(rng, 200) for _ in range(300)]
    worst = {"background": 0, "prefix": 0, "deletion": 0}
    for p, m in enumerate(fx["models"]):
        tab, c = m["tables"], fx["cons"][p]
        d = W.vit16_batch(tab, bgs).astype(np.int64) - R.viterbi_batch(tab, bgs).astype(np.int64)
        print(m["name"], "background: vf - vit min", d.min(), "max", d.max(), "mean", d.mean())
        assert (d >= 0).all()
        worst["background"] = max(worst["background"], int(d.max()))
        pre = [c[:n] for n in range(5, len(c) + 1, 5)]
        vf, vit = W.vit16_batch(tab, pre).astype(np.int64), R.viterbi_batch(tab, pre).astype(np.int64)
        ok = vf != W.VF_OVER
        assert ok[:6].all() and not ok[-1] and (np.diff(ok.astype(int)) <= 0).all()        # a prefix overflows, and then every longer one
        assert (vit[~ok] > 50 * 1024).all()                                                # only far above every floor
        print(m["name"], "consensus prefixes that do not overflow:", [len(r) for r, o in zip(pre, ok) if o], "vf - vit", (vf - vit)[ok].tolist())
        assert ((vf - vit)[ok] >= 0).all()
        worst["prefix"] = max(worst["prefix"], int((vf - vit)[ok].max()))
    ps = VC.profile_set()
    for m in ps["models"]:
        pair = VC.deletion_pair(ps["cons"][m["M"]], m["M"])
        vf, vit = W.vit16_batch(m["tables"], pair).astype(np.int64), R.viterbi_batch(m["tables"], pair).astype(np.int64)
        assert (vf != W.VF_OVER).all() and (vf >= vit).all()
        worst["deletion"] = max(worst["deletion"], int((vf - vit).max()))
    print("largest vf - vit:", worst)
    assert _pow2_at_or_above(2 * worst["background"]) <= EXCESS_BACKGROUND and _pow2_at_or_above(2 * worst["prefix"]) <= EXCESS_PREFIX
    assert _pow2_at_or_above(2 * worst["deletion"]) <= EXCESS_DELETION


def test_the_lower_clamp_is_not_sticky():
    """a node that cannot emit W (`*`, so msc16 = NEG16): behind a hit of 18 consensus nodes B + tBM is positive, and the cell of that node in a row of W is
    NEG16 plus it, above NEG16 - which is why the padding nodes of the device, NEG16 in every row, have to be kept out of E16 by a mask"""
    s = R.synth_model(np.random.default_rng(40), 40)
    s["mat"][20, R.AA.index("W")] = 0.0
    s["mat"][20] /= s["mat"][20].sum()
    tab = R.parse_hmm(R.write_hmm(s))[0]["tables"]
    assert tab[R.AA.index("W"), 20] == R.STAR - R.BG[R.AA.index("W")] and W.tables16(tab)[R.AA.index("W"), 20] == W.NEG16
    rec = R.consensus(tab)[:18] + b"W"
    vf, Mm, Im, Dm, E16 = W.vit16_naive(tab, rec, cells=True)
    assert vf != W.VF_OVER and E16[18] > 16 * 512
    assert W.NEG16 < Mm[19][20] < 0 and Mm[19][20] - W.NEG16 > 8 * 512          # NEG16 + max(.., ent), ent some bits above 0
    keep = []
    assert W.vit16_batch(tab, [rec], keep=keep)[0] == vf and keep[18][0][0, 20] == Mm[19][20]
    assert W.sat(W.NEG16 + 5) == W.NEG16 + 5 and W.sat(W.NEG16 - 5) == W.NEG16 and W.sat(W.MAX16 + 5) == W.MAX16


def test_the_form_of_the_d_scan_does_not_reach_a_score():
    """the definition (every step of the D recurrence saturates; equal to wide sums of tDD16, which a lane scan with int32 group sums computes) against a
    scan whose sums over 2^s groups saturate in int16. A saturated sum is -32768 where the wide one is lower, so a D cell of that scan can be larger - but
    then it is 64 bits or more below the row's E16, and the cell's own node is fed from B at E -> J -> B -> M, at most 1 024 + 16 810 + 20 120 units below
    E of the row before: no score differs. Measured on these records: 0 cells differ at all, the local term wins everywhere (SPEC 13.7)"""
    ps = VC.profile_set()
    differing = 0
    for M, group in ((1280, 20), (900, 16), (513, 12), (300, 6), (129, 3), (65, 2)):
        m = ps["models"][VC.SET_M.index(M)]
        tab, c = m["tables"], ps["cons"][M]
        recs = (VC.deletion_pair(c, M) if M in VC.CASE_M else [c[:20], c[5:25]]) + [c[:12] + c[-10:], R.background(np.random.default_rng(M), 60)]
        ka, kb = [], []
        a = W.vit16_batch(tab, recs, keep=ka)
        b = W.vit16_batch(tab, recs, d_form="sat_groups", group=group, keep=kb)
        assert a.tolist() == b.tolist() and (a != W.VF_OVER).all()
        assert [W.vit16_naive(tab, r) for r in recs[:2]] == a[:2].tolist() or M > 300          # the definition itself, where the naive loop is affordable
        for (Ma, Ia, Da, Ea), (Mb, Ib, Db, Eb) in zip(ka, kb):
            assert np.array_equal(Ea, Eb)
            diff = Da != Db
            differing += int(diff.sum())
            assert (Db >= Da).all()
            if diff.any():
                r = np.nonzero(diff)[0]
                assert (Db[diff] <= Ea[r] - 32768).all() and (Ea[r] > 0).all()
    print("D cells that differ between the two scans:", differing)


def test_the_overflow_edge_of_the_w_only_profile():
    """every node emits W with probability 1 and no transition costs anything: a row adds 3 304 half units. The yardstick decides where E16 reaches
    32767; measured: W x 11 scores 60 916, W x 12 overflows"""
    tab = R.parse_hmm(HC.limit_text("w_only", 64))[0]["tables"]
    naive = [W.vit16_naive(tab, b"W" * n) for n in range(1, 15)]
    n = 1 + next(i for i, v in enumerate(naive) if v == W.VF_OVER)
    print("W x", n - 1, "scores", naive[n - 2], "W x", n, "overflows; the int32 score of W x", n - 1, "is", R.viterbi(tab, b"W" * (n - 1)))
    assert all(v == W.VF_OVER for v in naive[n - 1:]) and all(v != W.VF_OVER for v in naive[:n - 1]) and 2 <= n <= 14
    assert W.vit16_batch(tab, [b"W" * k for k in range(1, 15)]).tolist() == naive
    assert 0 <= naive[n - 2] - R.viterbi(tab, b"W" * (n - 1)) <= EXCESS_PREFIX
    assert (n, naive[n - 2]) == (12, 60916)


def test_the_case_records_delete_and_do_not_overflow():
    ps = VC.profile_set()
    assert sorted(set(F.group_size(m["M"]) for m in ps["models"])) == list(F.CLASS_G) and set(HC.CLASS_M) | {1, 2, 3, 1280} <= set(VC.SET_M)
    for m in ps["models"]:
        M = m["M"]
        if M not in VC.CASE_M:
            continue
        pair = VC.deletion_pair(ps["cons"][M], M)
        vf = W.vit16_batch(m["tables"], pair)
        assert (vf != W.VF_OVER).all() and (vf != R.NO_SCORE).all() and (vf > 4 * 1024).all(), M
        if M >= 64:
            assert [8 <= len(r) - k <= 10 for r in pair for k in (9, 8)] and len(pair) == 2
            for r, span in zip(pair, (M - 23, M // 2 - 8)):
                raw, doms = T.trace(m["tables"], r)
                assert len(doms) == 1 and doms[0][7] >= span - 2 and doms[0][7] > 0.35 * M, (M, doms)       # one domain, the deletion in it
    recs = VC.set_records()
    own = W.vit16(ps["models"][VC.SET_M.index(300)]["tables"], recs[VC.OVER_RECORD])
    assert own == W.VF_OVER and len(recs[VC.OVER_RECORD]) == len(recs[VC.AFTER_OVER]) and b"*" in recs[VC.BAD_RECORD] and recs[0] == b""
    reuse = VC.wave_reuse_records()
    lens = [len(r) for r in reuse]
    assert len(reuse) == 528 and lens == sorted(lens, reverse=True) and min(lens[:8]) > max(lens[8:])
    tab = ps["models"][VC.SET_M.index(300)]["tables"]
    vf = W.vit16_batch(tab, list(reuse[:8]) + list(reuse[512:520]))
    assert (vf[:8] == W.VF_OVER).all() and (vf[8:] != W.VF_OVER).all()


def test_no_hit_is_lost_on_the_reference_profiles(fx):
    """the 2 000 background records of test_hmm_msv_cpu against both committed profiles, at the Viterbi floor of P = 1e-3: the pairs with vf >= floor
    contain the pairs with vit >= floor, and the extra ones are no more than the records whose vit lies within the asserted excess below the floor -
    a number taken from the int32 restatement alone. Measured: 0 and 0 extra pairs beside 1 and 4 that pass (SPEC 13.7)."""
    rng = np.random.default_rng(11)
    recs = [R.background(rng, 200) for _ in range(2000)]
    floors = F.floors(fx["models"])
    for p, m in enumerate(fx["models"]):
        vit = R.viterbi_batch(m["tables"], recs).astype(np.int64)
        vf = W.vit16_batch(m["tables"], recs).astype(np.int64)
        fl = int(floors[p])
        hit, kept = vit >= fl, vf >= fl
        near = (vit < fl) & (vit >= fl - EXCESS_BACKGROUND)
        extra = int((kept & ~hit).sum())
        print(m["name"], "floor", fl, "vit >= floor:", int(hit.sum()), "vf >= floor:", int(kept.sum()), "extra:", extra, "vit within", EXCESS_BACKGROUND, "below the floor:",
              int(near.sum()), "largest vf - vit:", int((vf - vit).max()))
        assert (vf != W.VF_OVER).all() and (vf >= vit).all() and (vf - vit).max() <= EXCESS_BACKGROUND
        assert kept[hit].all() and hit.sum() >= 1
        assert extra <= near.sum()
