"""genes (SPEC 15) without a device: the restatement tests/pyref_gene.py held to second definitions (math.log2, an exhaustive search over subsets, planted
genomes), the host functions of the library (gs_gene_log2_q16, gs_gene_train_host, gs_gene_score_host) held to the restatement with ==, and every case of
tests/gene_cases.py held to the property its name promises."""
import math
import os
import re

import numpy as np
import pytest

import gsearch_amd as G
import gene_cases as GC
import pyref_gene as R
import pyref_orf as RO


# ---- the integer logarithm --------------------------------------------------------------------------------------------------------------------------
def _log2_sample():
    rng = np.random.default_rng(15)
    xs = [1, 2, 3, 5, 6, 7, 2 ** 64 - 1]
    for e in range(1, 64):
        xs += [2 ** e - 1, 2 ** e, 2 ** e + 1]
    xs += [int(v) >> int(s) for v, s in zip(rng.integers(1, 2 ** 63, 3000), rng.integers(0, 62, 3000))]
    return [x for x in xs if x >= 1]


def test_log2_against_math_log2():
    """Bound, from the recurrence: the result is floor(65536 y) of a y that lies at most d below log2 x. Cutting the mantissa to 32 bits loses a factor
    below 1 + 2^-31, i.e. at most 1.45 * 2^-31 in the logarithm; a cut after a squaring at step k (and the cut of the halving) loses at most 2 * 1.45 * 2^-31
    in log2 m_k, which enters the result with weight 2^-k. Sum: d < 1.45 * 2^-31 * (1 + 2 * sum 2^-k) < 2^-28. Every cut goes down, so the result never
    exceeds log2 x: 0 <= log2 x - r / 65536 < 2^-16 + 2^-28 = LOG2_ERR. (math.log2 itself is within 2^-50 here.)"""
    for x in _log2_sample():
        r = R.log2_q16(x)
        d = math.log2(x) - r / 65536.0
        assert -2.0 ** -40 <= d < R.LOG2_ERR + 2.0 ** -40, (x, r, d)
    for e in range(64):
        assert R.log2_q16(2 ** e) == e << 16                                # exact at the powers of two
    assert R.log2_q16(0) == 0


def test_host_log2_equals_the_restatement():
    for x in _log2_sample() + [0]:
        assert G.gene_log2_q16(x) == R.log2_q16(x), x


def test_table_entry_rounds_half_up_and_stays_in_range():
    """S = floor((d + 32) / 64) of the Q16 difference d; an unseen dicodon scores log2(A / (Nc + A)) < 0 whatever Nb; |S| <= 32768"""
    assert R.table_entry(0, 7, 4096, 10 ** 6) == -1024 and R.table_entry(0, 123, 3 * 4096, 10 ** 9) == -2048
    for cod, b, Nc, Nb in ((0, 1, 2 ** 32 - 4096, 2 ** 31 + 4096), (2 ** 32 - 4096, 1, 2 ** 32 - 4096, 2 ** 31 + 4096), (5, 2 ** 31, 5, 2 ** 31 + 4096)):
        assert abs(R.table_entry(cod, b, Nc, Nb)) <= 32768
        assert cod * Nb + 4096 * b < 2 ** 64 and (Nc + 4096) * b < 2 ** 64      # the products stay inside 64 bits at the documented limits


# ---- the selection, against all subsets ----------------------------------------------------------------------------------------------------------------
def _exhaustive(cands, mo):
    """the largest total of a non-empty pairwise compatible subset: every compatible subset is visited (grown one candidate at a time)"""
    best = [None]

    def grow(sub, total, nxt):
        if sub and (best[0] is None or total > best[0]):
            best[0] = total
        for i in range(nxt, len(cands)):
            if all(R.compatible(cands[i], cands[m], mo) for m in sub):
                grow(sub + [i], total + cands[i][2], i + 1)
    grow([], 0, 0)
    return best[0]


def test_selection_equals_exhaustive_search():
    rng = np.random.default_rng(4)
    for trial in range(400):
        mo = int(rng.integers(0, 90))
        n = int(rng.integers(1, 13))
        ends = np.sort(rng.choice(np.arange(100, 1200), n, replace=False))
        cands = []
        for e in ends:
            length = int(rng.integers(mo + 1, 500))                            # a gene is longer than max_overlap (3 * min_aa > max_overlap)
            cands.append((int(e) - length, int(e), int(rng.integers(-3000, 9000)) if trial % 3 else int(rng.integers(1, 4)) * 1000))
        want = _exhaustive(cands, mo)
        if n <= 8:
            assert want == R.select_exhaustive(cands, mo)                       # the pruned search visits what the plain one visits
        sel = R.select(cands, mo)
        assert sel == sorted(sel) and len(sel) >= 1
        assert all(R.compatible(cands[a], cands[b], mo) for a in sel for b in sel if a < b), (trial, cands, sel)
        assert sum(cands[i][2] for i in sel) == want, (trial, cands, sel, want)


def test_selection_tie_rules():
    # equal f at the end: the smaller index; equal f at a predecessor: the smaller index
    c = [(0, 100, 5), (10, 110, 5), (200, 300, 7)]
    assert R.select(c, 0) == [0, 2]
    assert R.select(c[:2], 0) == [0]
    assert R.select([], 10) == []


# ---- the host forms of the stage entries == the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GC.scoring_cases(), ids=lambda c: c["name"])
def test_scoring_case_property_and_host_form(case):
    want = R.score(case["records"], case["goff"], case["tables"], case["orfs"], case["min_aa"], case["min_score"])
    assert case["check"](*want), case["name"]
    seq, rs, rl = GC.packed(case)
    orf = np.array([(b, r, s) for r, b, n, s in case["orfs"]], G.ORF_DTYPE)
    got = G.gene_score(seq, rs, rl, case["goff"], case["tables"], orf, [n for _, _, n, _ in case["orfs"]], host=True, min_aa=case["min_aa"], min_score=case["min_score"],
                       max_overlap=min(60, 3 * case["min_aa"] - 1))
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), case["name"]


def test_train_host_form_equals_the_restatement():
    records, goff, iv = GC.training_input()
    want_t, want_i = R.train(records, goff, iv, min_train_codons=18000)
    assert [int(x) for x in want_i[:, 1]] == [1, 0] and (want_t[0] != want_t[1]).any()
    seq, rs, rl = G.pack_dna_records([RO.ascii_of(b) for b in records])
    got_t, got_i = G.gene_train(seq, rs, rl, goff, np.array([(b, n, r, s) for r, b, n, s in iv], G.GENE_INTERVAL_DTYPE), host=True, min_train_codons=18000)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_t, want_t)
    assert np.abs(got_t).max() <= 32768


def test_host_forms_check_their_arguments():
    records, goff, iv = GC.training_input()
    seq, rs, rl = G.pack_dna_records([RO.ascii_of(b) for b in records])
    ivs = np.array([(b, n, r, s) for r, b, n, s in iv], G.GENE_INTERVAL_DTYPE)
    bad = [dict(max_overlap=90), dict(min_aa=0), dict(rounds=0)]
    for kw in bad:
        with pytest.raises(G.GsError) as e:
            G.gene_train(seq, rs, rl, goff, ivs, host=True, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(table=1), dict(flags=1)):
        with pytest.raises(G.GsError) as e:
            G.gene_train(seq, rs, rl, goff, ivs, host=True, **kw)
        assert e.value.code == -3, kw
    G.gene_train(seq, rs, rl, goff, ivs, host=True, max_overlap=89)
    for wrong in ([(0, 7000, 0, 0)], [(19999, 1, 0, 0)], [(0, 5, 0, 2)], [(0, 5, 9, 0)], [(0, 5, 1, 0), (0, 5, 0, 0)]):        # too long, past the end, strand, record, order
        with pytest.raises(G.GsError) as e:
            G.gene_train(seq, rs, rl, goff, np.array(wrong, G.GENE_INTERVAL_DTYPE), host=True)
        assert e.value.code == -1, wrong
    for g in ([0, 4, 3], [1, 3, 4], [0, 3, 5]):
        with pytest.raises(G.GsError) as e:
            G.gene_train(seq, rs, rl, g, ivs[:0], host=True)
        assert e.value.code == -1, g
    tables = np.zeros((2, 4096), np.int32)
    orf = np.array([(0, 0, 0)], G.ORF_DTYPE)
    G.gene_score(seq, rs, rl, goff, tables, orf, [40], host=True)
    tables[1, 77] = 32769
    with pytest.raises(G.GsError) as e:
        G.gene_score(seq, rs, rl, goff, tables, orf, [40], host=True)
    assert e.value.code == -1
    tables[1, 77] = -32768
    for o, n in (((0, 0, 0), 0), ((0, 0, 0), 6667), ((19999, 0, 0), 1), ((0, 4, 0), 1), ((0, 0, 2), 5)):
        with pytest.raises(G.GsError) as e:
            G.gene_score(seq, rs, rl, goff, tables, np.array([o], G.ORF_DTYPE), [n], host=True)
        assert e.value.code == -1, (o, n)


# ---- the method, on planted genomes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,size,train_min_aa", [(7, 100000, 150), (11, 100000, 150), (7, 300000, 250)])
def test_planted_genes_are_found(seed, size, train_min_aa):
    """conditions of the issue, after round 2: the 3' end exactly right for >= 0.95 of the planted genes, both ends for >= 0.85, <= 0.05 of the calls at no
    planted 3' end"""
    g, planted = GC.planted_genome(seed, size)
    res = R.call([g], [0, 1], train_min_aa=train_min_aa)
    assert int(res["info"][0, 1]) == 1
    end3, both, false = GC.accuracy(planted, res["gene"])
    print("seed %d size %d: %d planted, %d called, Nc %d: 3' %.3f both %.3f false %.3f" % (seed, size, len(planted), len(res["gene"]), int(res["info"][0, 0]), end3, both, false))
    assert end3 >= 0.95 and both >= 0.85 and false <= 0.05
    # every called protein starts with M or at the record's edge, holds no stop, and is what its coordinates translate to
    for gn, prot in zip(res["gene"], res["proteins"]):
        b, e, s = int(gn["begin"]), int(gn["end"]), int(gn["flags"]) & 1
        stop = 0 if int(gn["flags"]) & R.F_OPEN3 else 3
        body = RO.protein(g, b + (stop if s else 0), (e - b - stop) // 3, s)
        assert b"*" not in prot and prot[1:] == body[1:] and (prot[:1] == b"M" or (int(gn["flags"]) >> 1) & 3 == R.EDGE)


def test_a_small_genome_stays_untrained():
    g, _ = GC.planted_genome(7, 20000)
    res = R.call([g], [0, 1], train_min_aa=150)
    assert int(res["info"][0, 1]) == 0 and len(res["gene"]) == 0 and res["rec_gene_off"].tolist() == [0, 0]


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GC.pipeline_cases(), ids=lambda c: c["name"])
def test_pipeline_case_has_the_property_of_its_name(case):
    res = GC.pipeline_result(case)
    assert case["check"](res, case["records"]), case["name"]
    assert res["rec_gene_off"][-1] == len(res["gene"]) == len(res["aa_len"]) and int(res["aa_len"].sum()) == len(res["aa"])


def test_the_constants_are_the_header_s():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    spec = open(os.path.join(root, "gsearch_amd", "csrc", "gs_spec.hpp")).read()

    def const(name):
        return int(re.search(r"#define %s \(?(-?\d+)" % name, spec).group(1))
    prm = G.gene_params()
    assert (prm.min_aa, prm.table, prm.train_min_aa, prm.min_train_codons, prm.min_score, prm.max_overlap, prm.rounds, prm.flags) == (
        R.DEFAULTS["min_aa"], 11, const("GS_GENE_TRAIN_MIN_AA"), const("GS_GENE_MIN_TRAIN_CODONS"), const("GS_GENE_MIN_SCORE"), const("GS_GENE_MAX_OVERLAP"),
        const("GS_GENE_ROUNDS"), 0)
    assert (prm.train_min_aa, prm.min_train_codons, prm.min_score, prm.max_overlap, prm.rounds) == tuple(
        R.DEFAULTS[k] for k in ("train_min_aa", "min_train_codons", "min_score", "max_overlap", "rounds"))
    assert const("GS_GENE_PRIOR") == R.PRIOR and const("GS_GENE_BONUS_GTG") == R.BONUS[R.GTG] and const("GS_GENE_BONUS_TTG") == R.BONUS[R.TTG]
    assert G.GENE_DTYPE.itemsize == 32 and G.GENE_INTERVAL_DTYPE.itemsize == 24 and G.GENE_DTYPE == R.GENE_DTYPE and G.GENE_INTERVAL_DTYPE == R.INTERVAL_DTYPE
