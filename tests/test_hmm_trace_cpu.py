"""SPEC 13.2 on the CPU: the restatement tests/pyref_hmm_trace.py against its own cell-by-cell yardstick, against the hand cases the spec gives as
numbers, and on the tie rules. No GPU, no library call. trace() and trace_naive() themselves assert the two identities of the spec, raw ==
pyref_hmm.viterbi and that every traced cell lies above -2^19, so every call below checks those too."""
import numpy as np
import pytest

import hmm_classes_case as K
import hmm_trace_case as TC
import pyref_hmm as R
import pyref_hmm_trace as T


def both(tab, rec):
    got = T.trace(tab, rec)
    assert got == T.trace_naive(tab, rec), rec
    return got


def test_hand_cases_of_the_spec():
    for text, rec, raw, doms in TC.hand_cases():
        tab = R.parse_hmm(text)[0]["tables"]
        assert T.trace(tab, rec) == (raw, doms)
        if tab.shape[1] <= 4:
            assert T.trace_naive(tab, rec) == (raw, doms)


@pytest.mark.parametrize("kind", ["ordinary", "deletion", "insertion"])
def test_trace_is_its_naive_form(kind):
    rng = np.random.default_rng(41)
    for M in (1, 2, 7, 24):
        s = {"ordinary": lambda: R.synth_model(np.random.default_rng(M), M), "deletion": lambda: K.deletion_model(M),
             "insertion": lambda: TC.insertion_model(M)}[kind]()
        tab = TC.tables(s)
        c = R.consensus(tab)
        recs = [c, c + R.background(rng, 9) + c, R.background(rng, 30), c[:M // 3] + c[2 * M // 3:], c[:M // 2] + R.background(rng, 12) + c[M // 2:], c[:1]]
        for rec in recs:
            if len(rec):
                raw, doms = both(tab, rec)
                assert len(doms) >= 1
    assert T.trace(tab, b"") == (R.NO_SCORE, []) == T.trace_naive(tab, b"")


def test_long_deletions_and_insertions_are_one_domain():
    tab = TC.tables(K.deletion_model(64))
    c = R.consensus(tab)
    raw, doms = both(tab, c[:12] + c[52:])
    assert doms == [(1, 24, 1, 64, doms[0][4], 24, 0, 40)]
    for M in (40, 65):
        tab = TC.tables(TC.insertion_model(M))
        raw, doms = T.trace(tab, TC.insertion_record(R.consensus(tab)))
        assert doms == [(1, M + 30, 1, M, doms[0][4], M, 30, 0)]
    raw, doms = both(TC.tables(TC.insertion_model(40)), TC.insertion_record(R.consensus(TC.tables(TC.insertion_model(40)))))
    assert doms[0][6] == 30


def test_tie_rules_where_nearly_every_cell_ties():
    """all_zero_model: no transition costs anything and a residue scores the same at every node, so M, I, D and B tie in most cells and the order of
    the alternatives decides the path"""
    for M in (1, 2, 3, 5):
        tab = TC.tables(K.all_zero_model(M))
        for rec in (b"W", b"WW", b"W" * 7, b"A" * 7, b"WAWWC", b"AWAAWWA", b"ACDEFGHIKLMNPQRSTVWY"):
            raw, doms = both(tab, rec)
            for d in doms:
                assert d[2] == 1                               # equal entries: B is listed last, so a domain reaches back to node 1 through M
    raw, doms = both(TC.tables(K.all_zero_model(1)), b"WWW")
    assert [d[:4] for d in doms] == [(1, 1, 1, 1), (2, 2, 1, 1), (3, 3, 1, 1)]          # one node: every residue is a domain of its own
    # w_only_model on residues other than W: the domains are the runs of W
    tab = TC.tables(K.w_only_model(5))
    raw, doms = both(tab, b"AWWWAAWWA")
    assert [d[:2] for d in doms] == [(2, 4), (7, 8)]


def test_fixtures_consensus_and_copies():
    rng = np.random.default_rng(43)
    for name in TC.FIXTURES:
        tab = R.parse_hmm(TC.fixture_text(name))[0]["tables"]
        M = tab.shape[1] - 1
        c = R.consensus(tab)
        raw, doms = T.trace(tab, c)
        assert doms == [(1, M, 1, M, doms[0][4], M, 0, 0)]
        for n in (2, 3):
            rec = R.background(rng, 10).join([c] * n)
            raw, doms = T.trace(tab, rec)
            assert [(d[0], d[1], d[2], d[3]) for d in doms] == [(1 + j * (M + 10), M + j * (M + 10), 1, M) for j in range(n)]


def test_domain_table_writer():
    models = R.parse_hmm(TC.fixture_text(TC.FIXTURES[0]))
    c = R.consensus(models[0]["tables"])
    recs = [c + c, b"A" * 5]
    scores = R.search(models, recs)
    pr, pp = np.array([0], np.uint32), np.array([0], np.uint32)
    raw, nd, dom = T.trace_pairs(models, recs, pr, pp, 4)
    assert raw[0] == scores[0, 0] and nd[0] == 2 and (dom[0, 2:] == 0).all()
    text = T.domain_table_bytes(models, ["x", "y"], scores, raw, nd, dom, pr, pp)
    lines = text.split(b"\n")
    assert lines[0] + b"\n" == T.DOMAIN_HEADER and len(lines) == 4
    f = lines[2].split(b"\t")
    assert f[:10] == [b"x", b"Ribosomal_S9", b"PF00380.20", b"2", b"2", b"122", b"242", b"1", b"121", b"121"] and f[11:] == [b"121", b"0", b"0"]
    assert f[10] == b"%.2f" % (dom[0, 1, 4] / 1024.0)
