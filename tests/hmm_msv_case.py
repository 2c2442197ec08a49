"""Inputs of tests/test_hmm_msv_cpu.py and tests/test_gpu_hmm_msv.py (SPEC 13.3, the MSV prefilter): the profile set and the records of the kernel
parity tests, and the planted-gene inputs of the end-to-end tests. The CPU tests assert on the restatement alone that no pair of the planted inputs
at or above the gathering cutoff falls below the MSV floor of P = 0.02; the device tests lean on that. Nothing here calls the library."""
import functools
import os

import numpy as np

import hmm_classes_case as HC
import pyref_hmm as R
import pyref_hmm_forward as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
# the set of the kernel tests: every class, both sides of every class edge, lanes of padding only, a set order that is a real permutation - and the
# two smallest profiles, where 63 and 62 lanes of class 1 hold padding only
SET_M = HC.SET_ORDER + (1, 2)
CLASS_Q = F.CLASS_G
Q_PROFILE = {2: 128, 3: 192, 4: 256, 6: 384, 8: 512, 12: 768, 16: 1024, 20: 1280}      # a profile of the set in each class above 1


def fixture_path(name):
    return os.path.join(HERE, "golden", "hmm", name)


@functools.lru_cache(maxsize=None)
def fixtures():
    """texts, models, STATS lines and consensus of the two committed profiles"""
    texts = [open(fixture_path(n), "rb").read() for n in FIXTURES]
    models = [R.parse_hmm(t)[0] for t in texts]
    stats = [F.stats_lines(t)[0] for t in texts]
    return {"texts": texts, "models": models, "stats": stats, "cons": [R.consensus(m["tables"]) for m in models]}


def set_text(M):
    if M in (1, 2):
        return R.write_hmm(R.synth_model(np.random.default_rng(M), M), "f" if M == 1 else "b")
    return HC.model_text(M)


@functools.lru_cache(maxsize=None)
def profile_set():
    texts = [set_text(M) for M in SET_M]
    models = [R.parse_hmm(t)[0] for t in texts]
    assert [m["M"] for m in models] == list(SET_M)
    stats = [F.stats_lines(t)[0] for t in texts]
    return {"texts": texts, "models": models, "stats": stats, "cons": {m["M"]: R.consensus(m["tables"]) for m in models}}


BAD_RECORD = 7                                        # the record of set_records() that holds a byte that is no residue


@functools.lru_cache(maxsize=None)
def set_records():
    """about 24 records, as raw bytes (one of them is not a protein): lengths on both sides of the 64-residue block, a byte that is no residue, two
    consensus copies apart (J carries the score), a consensus piece across a lane edge of every class, one that enters at node 1 and one that leaves
    at node M, and whole small profiles"""
    rng = np.random.default_rng(41)
    cons = profile_set()["cons"]
    bg = lambda n: R.background(rng, n)                                         # noqa: E731
    recs = [bg(n) for n in (0, 1, 63, 64, 65, 129, 200)]
    bad = bytearray(bg(20) + cons[300][40:80] + bg(20))
    bad[50] = ord("*")
    recs.append(bytes(bad))
    assert len(recs) - 1 == BAD_RECORD
    recs.append(bg(20) + cons[300][:60] + bg(30) + cons[300][:60] + bg(15))      # two copies apart
    for q in CLASS_Q[1:]:                                                       # nodes 6 q - 11 .. 6 q + 12: lanes 5 and 6 of class q
        recs.append(bg(10) + cons[Q_PROFILE[q]][6 * q - 12:6 * q + 12] + bg(10))
    recs.append(cons[513][:30] + bg(25))                                        # enters at node 1
    recs.append(bg(25) + cons[513][-30:])                                       # leaves at node M
    recs.append(cons[65])                                                       # all of a profile: every lane edge of class 2, the partial lane last
    recs.append(bg(5) + cons[129] + bg(5))
    recs.append(cons[1280][1080:])                                              # 200 nodes up to M = GS_HMM_MAX_M, the last lanes of class 20
    recs.append(cons[64] + cons[64])                                            # class 1: a node a lane, twice through the wavefront
    dele = HC.deletion_records(cons[385], 385)                                  # built to score through long deletions: parity only, they may fail the floor
    recs += [dele[0], dele[3]]
    recs.append(b"")
    return tuple(recs)


def pack(records):
    """aa, rec_start, rec_len of records taken as they are (no byte is dropped)"""
    aa = np.frombuffer(b"".join(records), np.uint8)
    rl = np.array([len(r) for r in records], np.uint64)
    rs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64)
    return aa, rs, rl


def substituted(rng, c, n):
    """c with n residues replaced by other ones"""
    out = bytearray(c)
    for i in rng.choice(len(c), size=n, replace=False):
        out[i] = ord(rng.choice([a for a in R.AA if ord(a) != out[i]]))
    return bytes(out)


@functools.lru_cache(maxsize=None)
def faa_case():
    """(ids, sequences) of the hmmsearch end-to-end test: consensus copies of the committed profiles with a few substitutions, in background"""
    rng = np.random.default_rng(43)
    c0, c1 = fixtures()["cons"]
    bg = lambda n: R.background(rng, n)                                         # noqa: E731
    seqs = [bg(150), substituted(rng, c0, 3), bg(40) + substituted(rng, c1, 4) + bg(30), c0[:80], bg(90) + c1[10:], bg(200),
            substituted(rng, c1, 2) + bg(50) + substituted(rng, c0, 5), bg(60), c0[:12], bg(120)]
    return ["prot%d" % i for i in range(len(seqs))], seqs


@functools.lru_cache(maxsize=None)
def genome_case():
    """one genome of three contigs with sixteen genes of 450 codons each, enough coding sequence to train the gene caller; gene 7 of contigs 1 and 2 is
    M + the consensus of a committed profile -> (contigs as ASCII, the planted proteins in contig order)"""
    import gene_cases as GC
    import pyref_orf as RO
    rng = np.random.default_rng(47)
    cons = fixtures()["cons"]
    aas = R.AA.encode()
    contigs, proteins = [], []
    for ci in range(3):
        parts = [rng.integers(0, 4, 300).astype(np.uint8)]
        for k in range(16):
            prof = ci - 1 if k == 7 and ci in (1, 2) else None
            prot = b"M" + (cons[prof] if prof is not None else bytes(aas[i] for i in rng.integers(0, 20, 450)))
            gene = np.concatenate([RO.back_translate(prot), GC.bases([48])])
            strand = int(rng.integers(0, 2)) if prof is None else prof
            parts.append(GC.revcomp(gene) if strand else gene)
            parts.append(rng.integers(0, 4, int(rng.integers(30, 200))).astype(np.uint8))
            proteins.append(prot)
        contigs.append(RO.ascii_of(np.concatenate(parts)))
    return contigs, proteins
