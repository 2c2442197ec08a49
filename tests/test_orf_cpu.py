"""SPEC 14 (orfs) without a device: the codon tables of the library (gs_orf_codon_table is host code), the two definitions of the restatement
(tests/pyref_orf.py) against each other, and the planted-gene property the device tests build on - a consensus gene planted in random bases is
found by stop-to-stop translation as exactly one ORF, which is the only one that reaches the profile's GA cutoff - and that every constructed
case of tests/orf_cases.py has the shape its name promises."""
import collections
import os

import numpy as np
import pytest

import pyref_hmm as R
import pyref_orf as P
from orf_cases import SMALL, TILE

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3


def test_codon_tables():
    import gsearch_amd as G
    t11, t4 = G.orf_codon_table(11), G.orf_codon_table(4)
    assert t11 == P.TABLES[11] and t4 == P.TABLES[4] and G.orf_codon_table() == t11
    cnt = collections.Counter(t11)
    assert len(t11) == 64 and cnt["*"] == 3 and cnt["L"] == cnt["S"] == cnt["R"] == 6 and cnt["M"] == 1 and cnt["W"] == 1 and len(cnt) == 21
    assert [i for i in range(64) if t11[i] != t4[i]] == [56] and t4[56] == "W"
    # TAA TAG TGA by the index rule 16 b0 + 4 b1 + b2, ATG the one M
    assert [i for i, ch in enumerate(t11) if ch == "*"] == [48, 50, 56] and t11.index("M") == 14
    for bad in (1, 0, 25):
        with pytest.raises(G.GsError) as e:
            G.orf_codon_table(bad)
        assert e.value.code == GS_ERR_UNSUPPORTED
    import ctypes as C
    assert G.load().gs_orf_codon_table(11, None) == GS_ERR_INVALID
    buf = C.create_string_buffer(64)
    assert G.load().gs_orf_codon_table(4, buf) == 0 and buf.raw.decode() == t4


def _same(b, **kw):
    scan, nl_s = P.orfs_scan(b, **kw)
    naive, nl_n = P.orfs_naive(b, **kw)
    assert nl_s == nl_n
    assert scan == [(bg, n, s) for bg, n, s, _ in naive]
    for (bg, n, s), (_, _, _, prot) in zip(scan, naive):
        assert P.protein(b, bg, n, s, kw.get("table", 11)) == prot and b"*" not in prot and len(prot) == n
    return scan


def test_definitions_agree():
    rng = np.random.default_rng(3)
    total = 0
    for L in range(0, 201):
        b = rng.integers(0, 4, L).astype(np.uint8)
        for kw in ({"min_aa": 1}, {"min_aa": 5, "max_aa": 12}, {"min_aa": 3, "table": 4}):
            total += len(_same(b, **kw))
    assert total > 3000
    taa = P.codes(b"TAA" * 40)                               # forward class 0 is stops only; the other frames read AAT / ATA and their reverses
    assert all(not (s == 0 and bg % 3 == 0) for bg, n, s in _same(taa, min_aa=1))
    stops = P.codes(b"TTATCACTA" * 12 + b"TAATAGTGA" * 12)   # both strands' stops
    _same(stops, min_aa=1)
    nostop = P.codes(b"ACG" * 50 + b"AC")                    # no stop in any frame: six ORFs that end at the virtual ends
    got = _same(nostop, min_aa=1)
    L = len(nostop)
    assert sorted(got) == sorted((c, (L - c) // 3, s) for c in range(3) for s in (0, 1))
    assert P.orfs_scan(nostop, min_aa=1, max_aa=40) == ([], 6)


def test_order_is_end_then_strand():
    rng = np.random.default_rng(5)
    b = rng.integers(0, 4, 5000).astype(np.uint8)
    lst, _ = P.orfs_scan(b, min_aa=1)
    keys = [(bg + 3 * n, s) for bg, n, s in lst]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.fixture(scope="module")
def models():
    return [R.parse_hmm(open(os.path.join(HERE, "golden", "hmm", n), "rb").read())[0] for n in FIXTURES]


def test_planted_gene_is_the_one_orf_above_ga(models):
    cases = P.planted_cases(models, seed=7)
    assert len(cases) == 12
    for cs in cases:
        m, g, cons = models[cs["model"]], cs["genome"], cs["cons"]
        assert P.protein(g, cs["at"], len(cons), cs["strand"]) == cons                      # the plant reads back as the consensus on its strand
        lst, _ = P.orfs_scan(g, min_aa=P.MIN_AA)
        prots = [P.protein(g, bg, n, s) for bg, n, s in lst]
        holds = [i for i, p in enumerate(prots) if cons in p]
        assert len(holds) == 1
        bg, n, s = lst[holds[0]]
        assert s == cs["strand"] and bg <= cs["at"] and cs["at"] + 3 * len(cons) <= bg + 3 * n and (cs["at"] - bg) % 3 == 0
        raw = [int(R.viterbi(m["tables"], p)) for p in prots]
        best = int(np.argmax(raw))
        print("model %s strand %d f %d: %d ORFs, planted raw %d, GA %d, runner-up %d" % (m["name"], s, cs["f"], len(lst), raw[holds[0]], m["ga_units"],
                                                                                        max(r for i, r in enumerate(raw) if i != holds[0])))
        assert best == holds[0] and raw[best] >= m["ga_units"]
        assert all(r < m["ga_units"] for i, r in enumerate(raw) if i != best)


def test_split_and_names():
    ctg = b"ACGTNNACGTACGTRYacgtN"
    assert P.split_contig(ctg) == [(0, b"ACGT"), (6, b"ACGTACGT"), (16, b"acgt")]
    import gsearch_amd as G
    assert G.bigsi_split(ctg) == [(o, len(s)) for o, s in P.split_contig(ctg)]
    assert P.orf_name("c1", 0, 90, 0) == "c1_1_90_+" and P.orf_name("c1", 5, 95, 1) == "c1_6_95_-"


def test_cases_hold_what_they_claim():
    """the restatement's answers on the constructed cases have the shapes the names promise (so that the `==` of tests/test_gpu_orf.py compares something)"""
    by = {name: P.translate_records(records, **{"min_aa": P.MIN_AA, **kw}) for name, records, kw in SMALL}
    w = by["3 min_aa + {-1, 0, 1, 2} bases without a stop"]
    assert [int(w["rec_orf_off"][i + 1] - w["rec_orf_off"][i]) for i in range(4)] == [0, 2, 4, 6]          # 29 codons in every frame, then one frame after the other reaches 30
    w = by["ORFs of min_aa - 1, min_aa, max_aa, max_aa + 1 codons"]
    fr0 = [[int(n) for o, n in zip(w["orf"], w["aa_len"]) if o["rec"] == r and o["strand"] == 0 and o["begin"] == 3] for r in range(4)]
    assert fr0 == [[], [10], [40], []] and w["n_long"] >= 1
    w = by["no stop: six ORFs at the virtual ends"]
    assert list(w["rec_orf_off"]) == [0, 6, 12, 18]
    w = by["an ORF through a whole tile: the carry crosses two boundaries"]
    assert any(int(n) * 3 > 2 * TILE for n in w["aa_len"])
    t11, t4 = by["table 11 on a sequence rich in TGA"], by["table 4 on a sequence rich in TGA"]
    assert len(t4["aa"]) > len(t11["aa"]) and b"W" in t4["aa"].tobytes()
