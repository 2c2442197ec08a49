"""Inputs of tests/test_hmm_classes_cpu.py and tests/test_gpu_hmm_classes.py: synthetic profiles in which a long deletion is the best path, so that the
lane scan of the D states (gs_hmm.hip, SPEC 13 and 13.1) carries the expected scores, at sizes on both sides of every edge between two kernel
classes; and the two profiles whose cells grow as fast as the tables allow, for the length limits. Nothing here calls the library.

Why the ordinary synth_model does not do: its tDD comes from probabilities 0.3 to 0.6, about a bit per deleted node, so past some fifteen nodes leaving
through E and J and entering again is cheaper than the deletion, and no expected score travels through more than the first scan steps. Here a D run
costs 0.001 to 0.003 bit per node and entering it 3 to 4 bits, against 1 bit for E -> J plus -tBM (11 to 20 bits) for the way round."""
import hashlib

import numpy as np

import pyref_hmm as R
import pyref_hmm_forward as F

# both sides of every class edge (64 Q nodes, Q = 1, 2, 3, 4, 6, 8, 12, 16, 20) and GS_HMM_MAX_M. An upper edge fills all 64 lanes; one node more
# is the next class with about 48 lanes in use, then a lane that holds a single node, then lanes of padding only
CLASS_M = (64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025, 1280)
# the order of the profiles in the device's set: not by M, so that the set's list of profiles by class is a real permutation
SET_ORDER = (513, 64, 1280, 193, 65, 1025, 128, 769, 300, 129, 1024, 192, 385, 256, 900, 768, 257, 384, 512)
ORDINARY_M = (300, 900)


def deletion_model(M):
    """synth_model(default_rng(M), M) with the transitions of nodes 1 .. M - 1 drawn again: m->d 0.05 .. 0.15, m->i 0.005 .. 0.02, d->d 0.998 .. 0.9995"""
    rng = np.random.default_rng(M)
    s = R.synth_model(rng, M, name="DEL%d" % M)
    for k in range(1, M):
        md = rng.uniform(0.05, 0.15)
        mi = rng.uniform(0.005, 0.02)
        dd = rng.uniform(0.998, 0.9995)
        s["tr"][k] = [1 - mi - md, mi, md, s["tr"][k][3], s["tr"][k][4], 1 - dd, dd]
    return s


def deletion_records(c, M):
    """six pieces of the consensus c with nodes left out between them: deletions over a few lanes up to most of the wavefront. From M = 193 on every
    class has about 48 lanes or more in use and pieces of 12 to 25 nodes fit; below, the pieces are 8 to 12 nodes so that they stay inside the
    profile and apart, and the first record still deletes across more than 32 lanes where the profile has them (M = 64, 128, 129)."""
    G = F.group_size(M)
    if M >= 193:
        recs = [c[:25] + c[M - 25:],
                c[:12] + c[M // 2 - 6:M // 2 + 6] + c[M - 12:],
                c[:20] + c[M // 3:M // 3 + 20],
                c[3 * G:3 * G + 15] + c[5 * G + 2:5 * G + 17],
                c[:15] + c[9 * G:9 * G + 15],
                c[G:G + 15] + c[18 * G:18 * G + 15]]
    else:
        recs = [c[:12] + c[M - 12:],
                c[:8] + c[M // 2 - 4:M // 2 + 4] + c[M - 8:],
                c[:10] + c[M // 3:M // 3 + 10],
                c[3 * G:3 * G + 8] + c[5 * G + 8:5 * G + 16],
                c[:8] + c[8 + 5 * G:16 + 5 * G],
                c[G:G + 8] + c[18 * G + 8:18 * G + 16]]
    assert all(len(r) >= 16 for r in recs) and 18 * G + 16 <= M
    return recs


def model_text(M):
    """the HMMER3 text of the profile of M nodes in the set: deletion-friendly for CLASS_M, ordinary for ORDINARY_M; the dialects alternate"""
    if M in ORDINARY_M:
        s = R.synth_model(np.random.default_rng(M), M)
    else:
        s = deletion_model(M)
    return R.write_hmm(s, "b" if M % 2 else "f", compo=bool(M % 3))


def all_zero_model(M):
    """every number of the file 0.00000: each probability 1, which the parser accepts. A match scores -BG[a], up to 6 608 units for W, and no
    transition costs anything: cells grow as fast as the tables allow"""
    s = R.synth_model(np.random.default_rng(M), M, name="ZERO%d" % M)
    s["mat"][:] = 1.0
    s["ins"][:] = 1.0
    s["tr"][:] = 1.0
    return s


def w_only_model(M):
    """W with probability 1 at every node, m->m = i->m = d->m = 1, everything else `*`"""
    s = R.synth_model(np.random.default_rng(M), M, name="WONLY%d" % M)
    s["mat"][:] = 0.0
    s["mat"][:, R.AA.index("W")] = 1.0
    s["tr"][:] = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    return s


LIMIT_MODELS = {"zero": all_zero_model, "w_only": w_only_model}
# (score, profile kind, M, L of the record b"W" * L): the two limits, one residue below each, and 2^16 for Viterbi
LIMIT_CASES = (("viterbi", "zero", 64, 1 << 18), ("viterbi", "w_only", 64, 1 << 18), ("viterbi", "zero", 64, (1 << 18) - 1), ("viterbi", "zero", 64, 1 << 16),
               ("forward", "zero", 64, 65536), ("forward", "zero", 1280, 65536), ("forward", "zero", 64, 65535))


def limit_text(kind, M):
    return R.write_hmm(LIMIT_MODELS[kind](M))


def sha256(text):
    return hashlib.sha256(text).hexdigest()
