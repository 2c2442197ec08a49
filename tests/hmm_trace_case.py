"""Inputs shared by tests/test_hmm_trace_cpu.py and tests/test_gpu_hmm_trace.py (SPEC 13.2): the insertion-friendly sibling of
hmm_classes_case.deletion_model, the three hand cases of the spec as literals, and the records of the tie and class cases. Nothing here calls the library."""
import os

import numpy as np

import hmm_classes_case as K
import pyref_hmm as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")


def fixture_text(name):
    with open(os.path.join(HERE, "golden", "hmm", name), "rb") as f:
        return f.read()


def insertion_model(M):
    """synth_model(default_rng(M), M) with the transitions of nodes 1 .. M - 1 drawn again: m->i 0.05 .. 0.15, m->d 0.005 .. 0.02, i->i 0.99 .. 0.998, i->m
    the rest: a long insertion costs 3 to 4 bits to open and next to nothing per residue, so it beats leaving through E and J and entering again"""
    rng = np.random.default_rng(M)
    s = R.synth_model(rng, M, name="INS%d" % M)
    for k in range(1, M):
        mi = rng.uniform(0.05, 0.15)
        md = rng.uniform(0.005, 0.02)
        ii = rng.uniform(0.99, 0.998)
        s["tr"][k] = [1 - mi - md, mi, md, 1 - ii, ii, s["tr"][k][5], s["tr"][k][6]]
    return s


def insertion_record(c, n=30, at=20, seed=5):
    """the consensus c with n background residues inserted after node `at`"""
    return c[:at] + R.background(np.random.default_rng(seed), n) + c[at:]


def tables(s):
    return R.parse_hmm(R.write_hmm(s))[0]["tables"]


def hand_cases():
    """(profile text, record, raw, domains) of the three cases SPEC 13.2 gives as numbers: none depends on a random draw"""
    pf = fixture_text("PF00380.20.HMM")
    c = R.consensus(R.parse_hmm(pf)[0]["tables"])
    return [(R.write_hmm(K.all_zero_model(2)), b"WAWWC", 20364, [(1, 3, 1, 2, 11593, 2, 1, 0), (4, 5, 1, 2, 11174, 2, 0, 0)]),
            (R.write_hmm(K.all_zero_model(3)), b"AAAAAAA", 14296, [(1, 4, 1, 3, 8615, 3, 1, 0), (5, 7, 1, 3, 8615, 3, 0, 0)]),
            (pf, c[:30] + c[70:], 118992, [(1, 30, 1, 30, 45483, 30, 0, 0), (31, 81, 71, 121, 82358, 51, 0, 0)])]


TIE_M = (1, 64, 65, 129)
TIE_RECORDS = [b"W" * n for n in (1, 63, 64, 65, 200)] + [b"A" * 7]
INSERTION_M = (64, 65, 1280)
