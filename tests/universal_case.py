"""Planted genomes for the universal-gene tests (tests/test_gpu_universal.py, tests/test_gpu_commands_universal.py), after the recipe of
tests/test_gpu_gene.py::test_universal_genes_from_called_genes: three contigs of 16 genes of 450 residues each - enough coding sequence of one codon choice
for the gene caller to train - in which chosen genes are a committed profile's consensus with a fraction of its residues replaced, back-translated. A genome is
written three ways: its proteins (.faa), its contigs (.fna) and those compressed (.fna.gz). Seeded; no library call."""
import gzip
import os

import numpy as np

import gene_cases as GC
import pyref_hmm as RH
import pyref_orf as RO

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
AAS = b"ACDEFGHIKLMNPQRSTVWY"


def profile_paths():
    return [os.path.join(HERE, "golden", "hmm", n) for n in FIXTURES]


def models():
    return [RH.parse_hmm(open(p, "rb").read())[0] for p in profile_paths()]


def variant(rng, cons, fraction):
    """the consensus with `fraction` of its residues replaced by uniform ones"""
    c = bytearray(cons)
    for i in np.flatnonzero(rng.random(len(c)) < fraction):
        c[i] = AAS[int(rng.integers(0, 20))]
    return bytes(c)


def genome(seed, cons, planted, fraction=0.0):
    """planted: the profiles (indices into cons) whose gene the genome holds, profile p as gene 7 of contig p + 1
    -> (contigs as ASCII bytes, proteins in contig order, {profile: its protein})"""
    rng = np.random.default_rng(seed)
    contigs, proteins, where = [], [], {}
    for ci in range(3):
        parts = [rng.integers(0, 4, 300).astype(np.uint8)]
        for k in range(16):
            prof = ci - 1 if k == 7 and ci in (1, 2) and ci - 1 in planted else None
            if prof is None:
                prot = b"M" + bytes(AAS[i] for i in rng.integers(0, 20, 450))
                strand = int(rng.integers(0, 2))
            else:
                prot = b"M" + variant(rng, cons[prof], fraction)
                strand = (seed + prof) % 2
                where[prof] = prot
            gene = np.concatenate([RO.back_translate(prot), GC.bases([48])])
            parts.append(GC.revcomp(gene) if strand else gene)
            parts.append(rng.integers(0, 4, int(rng.integers(30, 200))).astype(np.uint8))
            proteins.append(prot)
        contigs.append(RO.ascii_of(np.concatenate(parts)))
    return contigs, proteins, where


def mutate(seed, contigs, rate):
    """every base replaced with probability `rate` by one of the other three"""
    rng = np.random.default_rng(seed)
    out = []
    for c in contigs:
        code = np.frombuffer(c.translate(bytes.maketrans(b"ACGT", bytes(range(4)))), np.uint8).copy()
        hit = np.flatnonzero(rng.random(len(code)) < rate)
        code[hit] = (code[hit] + rng.integers(1, 4, len(hit))) % 4
        out.append(RO.ascii_of(code))
    return out


def write_fasta(path, ids, seqs, width=70):
    text = b"".join(b">" + i.encode() + b" planted\n" + b"\n".join(s[j:j + width] for j in range(0, len(s), width)) + b"\n" for i, s in zip(ids, seqs))
    with (gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(text)


def write_genome(directory, stem, contigs, proteins, forms=("faa", "fna", "fna.gz")):
    """-> {form: path}"""
    out = {}
    for form in forms:
        path = os.path.join(str(directory), "%s.%s" % (stem, form))
        if form == "faa":
            write_fasta(path, ["%s_p%d" % (stem, i) for i in range(len(proteins))], proteins)
        else:
            write_fasta(path, ["%s_c%d" % (stem, i) for i in range(len(contigs))], contigs)
        out[form] = path
    return out
