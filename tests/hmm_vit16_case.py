"""Inputs of tests/test_hmm_vit16_cpu.py and tests/test_gpu_hmm_vit16.py (SPEC 13.7, the packed int16 Viterbi filter). Nothing here calls the library.

The six records of hmm_classes_case.deletion_records() carry 30 to 50 consensus residues: from M = 193 on their int16 cells pass 32767 half units (64 bits)
and the record ends with VF_OVER at its first piece, so the lane scan of D would carry no expected score in the large classes. Here every profile of
M >= 64 gets two records of two short consensus pieces (8 to 10 nodes) with one deletion between them that spans most of the lanes the profile uses;
they stay below 64 bits. k_hmm_vit16 runs a class of Q nodes a lane with ceil(Q / 2) registers of two node slots, so its class edges are those of
hmm_classes_case.CLASS_M and it adds none; M = 1, 2, 3 are the profiles with one lane in use, and with a high run that holds padding only."""
import functools

import numpy as np

import hmm_classes_case as HC
import pyref_hmm as R
import pyref_hmm_forward as F

SMALL_M = (1, 2, 3)
CASE_M = SMALL_M + HC.CLASS_M
# the device's set: the order of hmm_classes_case (a real permutation of the classes, two ordinary profiles) with the small profiles in between
SET_M = HC.SET_ORDER[:5] + (3,) + HC.SET_ORDER[5:12] + (1,) + HC.SET_ORDER[12:] + (2,)


def model_text(M):
    if M in SMALL_M:
        return R.write_hmm(R.synth_model(np.random.default_rng(M), M), "f" if M % 2 else "b")
    return HC.model_text(M)


def deletion_pair(c, M):
    """the records of a profile of M nodes with consensus c: for M >= 64 two pieces of 8 to 10 nodes around one long deletion - from the first lanes
    to the last, and from the first quarter to the last; for M = 3 the consensus and its ends around the deleted middle node; below, the consensus"""
    if M >= 64:
        return [c[2:11] + c[M - 12:M - 2], c[M // 4:M // 4 + 8] + c[3 * M // 4:3 * M // 4 + 10]]
    return [c, c[:1] + c[2:]] if M == 3 else [c]


@functools.lru_cache(maxsize=None)
def profile_set():
    texts = [model_text(M) for M in SET_M]
    models = [R.parse_hmm(t)[0] for t in texts]
    assert [m["M"] for m in models] == list(SET_M) and set(CASE_M) <= set(SET_M)
    stats = [F.stats_lines(t)[0] for t in texts]
    return {"texts": texts, "models": models, "stats": stats, "cons": {m["M"]: R.consensus(m["tables"]) for m in models}}


BAD_RECORD = 6                                        # the record of set_records() that holds a byte that is no residue
OVER_RECORD, AFTER_OVER = 7, 8                        # a record whose cells overflow, and the ordinary one of the same length that follows it


@functools.lru_cache(maxsize=None)
def set_records():
    """the records of the kernel tests, as raw bytes: an empty one, background of 1, 63, 64, 65 and 130 residues, a byte that is no residue, a record
    that overflows against its own profile and an ordinary one of its length, a consensus piece twice (J carries the score), and the deletion pairs
    of every profile of CASE_M"""
    rng = np.random.default_rng(47)
    cons = profile_set()["cons"]
    bg = lambda n: R.background(rng, n)                                         # noqa: E731
    recs = [bg(n) for n in (0, 1, 63, 64, 65, 130)]
    bad = bytearray(bg(20) + cons[300][40:80] + bg(20))
    bad[50] = ord("*")
    recs.append(bytes(bad))
    assert len(recs) - 1 == BAD_RECORD
    recs.append(bg(10) + cons[300][:80] + bg(10))                               # 80 consensus nodes: past 64 bits
    recs.append(bg(100))
    recs.append(bg(20) + cons[900][100:112] + bg(30) + cons[900][100:112] + bg(15))
    for M in CASE_M:
        recs += deletion_pair(cons[M], M)
    return tuple(recs)


REUSE_M = (300, 65)


@functools.lru_cache(maxsize=None)
def wave_reuse_records():
    """528 records for a set of the profiles REUSE_M. A launch has at most 64 workgroups of eight wavefronts a profile, and wavefront w of workgroup b
    takes the entries b 8 + w, b 8 + w + 512, .. of the records by length, longest first: the eight longest overflow against the profile of 300 nodes
    (80 of its consensus nodes), and entries 512 .. 519, ordinary records, follow them in the same eight wavefronts"""
    rng = np.random.default_rng(53)
    c = profile_set()["cons"][300]
    over = [R.background(rng, 15) + c[10 * j:10 * j + 80] + R.background(rng, 15) for j in range(8)]
    return tuple(over + [R.background(rng, 100 - j // 8) for j in range(8, 528)])
