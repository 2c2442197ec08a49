"""Python-integer / numpy restatement of SPEC 15 (genes: a self-trained gene caller), written from the SPEC text on top of pyref_orf.py and sharing no
code with gs_gene.hip. Bases are codes A C G T = 0 1 2 3, a codon b0 b1 b2 has index 16 b0 + 4 b1 + b2, a hexamer the index sum b[i] 4^(5 - i).
The selection has two definitions here: select() is the recurrence of the SPEC, select_exhaustive() searches all subsets (small lists only)."""
import bisect
import itertools

import numpy as np

import pyref_orf as RO

PRIOR = 4096
DEFAULTS = dict(min_aa=30, table=11, train_min_aa=250, min_train_codons=15000, min_score=5120, max_overlap=60, rounds=2)
ATG, GTG, TTG = 14, 46, 62
BONUS = {ATG: 0, GTG: -2048, TTG: -3072}
TYPE = {ATG: 0, GTG: 1, TTG: 2}
EDGE = 3
F_STRAND, F_OPEN3, F_HAS_START, F_CANDIDATE, F_OPEN5 = 1, 8, 16, 32, 64
NO_START = 0xFFFFFFFFFFFFFFFF
GENE_DTYPE = np.dtype([("begin", np.uint64), ("end", np.uint64), ("score", np.int64), ("rec", np.uint32), ("flags", np.uint32)])
INTERVAL_DTYPE = np.dtype([("begin", np.uint64), ("n", np.uint64), ("rec", np.uint32), ("strand", np.uint32)])
LOG2_ERR = 2.0 ** -16 + 2.0 ** -28          # 0 <= log2 x - log2_q16(x) / 65536 < LOG2_ERR (derivation: SPEC 15, test_gene_cpu.py)


# ---- the integer logarithm and the table ------------------------------------------------------------------------------------------------------
def log2_q16(x):
    """floor(65536 log2 x) by normalise, then square-and-compare: m is the mantissa in [2^31, 2^32) with the bits below cut; sixteen times m <- m^2 / 2^31
    (cut), and when that reached 2^32 the next fraction bit is 1 and m is halved (cut)"""
    x = int(x)
    if x == 0:
        return 0
    e = x.bit_length() - 1
    m = x >> (e - 31) if e >= 31 else x << (31 - e)
    r = e
    for _ in range(16):
        m = (m * m) >> 31
        r <<= 1
        if m >> 32:
            m >>= 1
            r |= 1
    return r


def table_entry(cod, b, Nc, Nb):
    d = log2_q16(cod * Nb + PRIOR * b) - log2_q16((Nc + PRIOR) * b)
    return (d + 32) >> 6                                               # Python's >> floors: round half up to 10 fraction bits


_REV_HEX = np.array([sum((3 - ((h >> (2 * i)) & 3)) << (2 * (5 - i)) for i in range(6)) for h in range(4096)])     # base i from the right becomes base i from the left


def background(records):
    """bg[h]: the hexamers at every position of every record, on both strands"""
    fwd = np.zeros(4096, np.int64)
    for b in records:
        b = np.asarray(b, np.int64)
        if len(b) >= 6:
            h = sum(b[i:len(b) - 5 + i] << (2 * (5 - i)) for i in range(6))
            fwd += np.bincount(h, minlength=4096)
    return fwd + fwd[_REV_HEX]


def codons_of(b, begin, n, strand):
    """the n codons of bases [begin, begin + 3 n) in reading direction"""
    b = np.asarray(b, np.int64)
    seg = b[begin:begin + 3 * n]
    if strand:
        seg = (3 - seg)[::-1]
    return 16 * seg[0::3] + 4 * seg[1::3] + seg[2::3]


def dicodons(records, intervals):
    """cod[64 c_i + c_{i+1}] over the intervals (rec, begin, n, strand) of one genome's records"""
    cod = np.zeros(4096, np.int64)
    for rec, begin, n, strand in intervals:
        if n >= 2:
            c = codons_of(records[rec], begin, n, strand)
            cod += np.bincount(64 * c[:-1] + c[1:], minlength=4096)
    return cod


def make_table(bg, cod):
    """-> (S as a list of 4096 Python ints, Nc)"""
    b = [int(v) + 1 for v in bg]
    Nb, Nc = sum(b), int(sum(int(v) for v in cod))
    return [table_entry(int(cod[h]), b[h], Nc, Nb) for h in range(4096)], Nc


def train(records, genome_rec_off, intervals, min_train_codons=DEFAULTS["min_train_codons"]):
    """intervals: (rec, begin, n, strand) with rec an index into all records -> (int32 [n_genomes, 4096], uint64 [n_genomes, 2] = (Nc, trained))"""
    ng = len(genome_rec_off) - 1
    tables, info = np.zeros((ng, 4096), np.int32), np.zeros((ng, 2), np.uint64)
    for g in range(ng):
        r0, r1 = int(genome_rec_off[g]), int(genome_rec_off[g + 1])
        recs = records[r0:r1]
        S, Nc = make_table(background(recs), dicodons(recs, [(r - r0, b, n, s) for r, b, n, s in intervals if r0 <= r < r1]))
        tables[g], info[g] = S, (Nc, 1 if Nc >= min_train_codons else 0)
    return tables, info


# ---- the start of an ORF -------------------------------------------------------------------------------------------------------------------------
def open_ends(L, begin, n, strand):
    """(5'-open, 3'-open): no room for a stop codon in front of / behind the ORF inside the record"""
    low, high = begin < 3, begin + 3 * n + 3 > L
    return (high, low) if strand else (low, high)


def best_start(c, S, open5, min_aa):
    """c: the ORF's codons in reading direction -> (j, score, type) of the best start or None. x_i = S[64 c_i + c_{i+1}], T_j = sum of x_i over i >= j."""
    n = len(c)
    S = np.asarray(S, np.int64)
    x = S[64 * c[:-1] + c[1:]] if n >= 2 else np.zeros(0, np.int64)
    T = np.concatenate([np.cumsum(x[::-1])[::-1], [0]]).astype(np.int64)
    best = None
    cand = [j for j in np.flatnonzero((c == ATG) | (c == GTG) | (c == TTG)) if n - j >= min_aa]
    if open5 and (not cand or cand[0] != 0):
        cand = [0] + cand
    for j in cand:
        cj = int(c[j])
        if j == 0 and open5:
            s, t = int(T[0]), (0 if cj == ATG else EDGE)               # the record's edge: bonus 0; the type is ATG when the first codon is one
        else:
            s, t = int(T[j]) + BONUS[cj], TYPE[cj]
        if best is None or s > best[1]:                                # ascending j: among equals the smallest stays
            best = (int(j), s, t)
    return best


def score_flags(strand, open5, open3, best, min_score):
    f = (F_STRAND if strand else 0) | (F_OPEN3 if open3 else 0) | (F_OPEN5 if open5 else 0)
    if best is not None:
        f |= F_HAS_START | (best[2] << 1) | (F_CANDIDATE if best[1] >= min_score else 0)
    return f


def score(records, genome_rec_off, tables, orfs, min_aa=DEFAULTS["min_aa"], min_score=DEFAULTS["min_score"]):
    """orfs: (rec, begin, n, strand) -> (uint64 best j or NO_START, int64 score, uint32 flags)"""
    goff = [int(v) for v in genome_rec_off]
    bj, sc, fl = np.zeros(len(orfs), np.uint64), np.zeros(len(orfs), np.int64), np.zeros(len(orfs), np.uint32)
    for o, (rec, begin, n, strand) in enumerate(orfs):
        g = bisect.bisect_right(goff, rec) - 1
        o5, o3 = open_ends(len(records[rec]), begin, n, strand)
        best = best_start(codons_of(records[rec], begin, n, strand), tables[g], o5, min_aa)
        bj[o], sc[o] = (best[0], best[1]) if best else (NO_START, 0)
        fl[o] = score_flags(strand, o5, o3, best, min_score)
    return bj, sc, fl


def gene_coords(begin, n, strand, j, open3):
    """forward coordinates of the gene of ORF (begin, n, strand) that starts at codon j, the stop codon included where there is one"""
    stop = 0 if open3 else 3
    return (begin - stop, begin + 3 * n - 3 * j) if strand else (begin + 3 * j, begin + 3 * n + stop)


# ---- the selection -------------------------------------------------------------------------------------------------------------------------------
def select(cands, max_overlap, values=None):
    """cands: (begin, end, score) of one record in (end, strand) order -> the chosen indices, ascending. k(i) = the candidates m < i with
    end_m <= begin_i + max_overlap; P_k = max(0, max f_m over m < k); f_i = score_i + P_k(i); predecessor = the smallest m < k(i) with f_m = P_k(i) > 0;
    the chain ends at the smallest i with the largest f. values (a dict): receives f and k."""
    n = len(cands)
    if n == 0:
        return []
    ks = []
    ends = [c[1] for c in cands]
    f, pred = [0] * n, [None] * n
    pmax, parg = [0], [None]                                            # P_k and the smallest m that reaches it, for k = 0 .. i
    for i, (b, e, s) in enumerate(cands):
        k = bisect.bisect_right(ends, b + max_overlap, 0, i)
        ks.append(k)
        f[i] = s + pmax[k]
        pred[i] = parg[k] if pmax[k] > 0 else None
        if f[i] > pmax[-1]:
            pmax.append(f[i]); parg.append(i)
        else:
            pmax.append(pmax[-1]); parg.append(parg[-1])
    if values is not None:
        values["f"], values["k"] = f, ks
    i = max(range(n), key=lambda t: (f[t], -t))
    out = []
    while i is not None:
        out.append(i)
        i = pred[i]
    return out[::-1]


def compatible(a, b, max_overlap):
    """two candidates (begin, end, ...) share at most max_overlap bases"""
    return min(a[1], b[1]) - max(a[0], b[0]) <= max_overlap


def select_exhaustive(cands, max_overlap):
    """the largest total score of a non-empty pairwise compatible subset, by trying them all"""
    best = None
    for r in range(1, len(cands) + 1):
        for sub in itertools.combinations(range(len(cands)), r):
            if all(compatible(cands[a], cands[b], max_overlap) for a, b in itertools.combinations(sub, 2)):
                t = sum(cands[i][2] for i in sub)
                if best is None or t > best:
                    best = t
    return best


# ---- the whole call ------------------------------------------------------------------------------------------------------------------------------
def call(records, genome_rec_off, **params):
    """records: code arrays; genome g = records [genome_rec_off[g], genome_rec_off[g + 1]) -> the arrays gs_gene_call writes: dict of gene, aa, aa_start,
    aa_len, rec_gene_off, info, tables (+ `proteins`, a list of bytes, and `cands`, per record the last round's candidates (begin, end, score))"""
    p = dict(DEFAULTS, **params)
    assert p["max_overlap"] < 3 * p["min_aa"] and p["rounds"] >= 1
    tab = RO.TABLES[p["table"]]
    goff = [int(v) for v in genome_rec_off]
    ng = len(goff) - 1
    orfs = [RO.orfs_scan(b, p["min_aa"], 0, p["table"])[0] for b in records]                     # per record (begin, n, strand) in (end, strand) order
    tables, info = np.zeros((ng, 4096), np.int32), np.zeros((ng, 2), np.uint64)
    chosen_by_rec, cands_by_rec = {}, {}
    for g in range(ng):
        r0, r1 = goff[g], goff[g + 1]
        recs = records[r0:r1]
        bg = background(recs)
        intervals = [(r - r0, begin, n, s) for r in range(r0, r1) for begin, n, s in orfs[r] if n >= p["train_min_aa"]]
        for rnd in range(p["rounds"]):
            S, Nc = make_table(bg, dicodons(recs, intervals))
            trained = Nc >= p["min_train_codons"]
            tables[g], info[g] = S, (Nc, 1 if trained else 0)
            intervals = []
            for r in range(r0, r1):
                cands = []
                for begin, n, s in (orfs[r] if trained else []):
                    o5, o3 = open_ends(len(records[r]), begin, n, s)
                    c = codons_of(records[r], begin, n, s)
                    best = best_start(c, S, o5, p["min_aa"])
                    if best is not None and best[1] >= p["min_score"]:
                        gb, ge = gene_coords(begin, n, s, best[0], o3)
                        cands.append((gb, ge, best[1], s, best[2], o3, begin, n, best[0]))
                cands.sort(key=lambda t: (t[1], t[3]))
                assert len({(t[1], t[3]) for t in cands}) == len(cands)              # (end, strand) is a total order on a record's candidates
                cands_by_rec[r] = [(t[0], t[1], t[2]) for t in cands]                # (of the last round, once the loop is through)
                chosen_by_rec[r] = [cands[i] for i in select(cands_by_rec[r], p["max_overlap"])]
                for gb, ge, sc, s, t, o3, begin, n, j in chosen_by_rec[r]:
                    intervals.append((r - r0, begin if s else begin + 3 * j, n - j, s))
    gene, prots, off = [], [], [0]
    for r, b in enumerate(records):
        for gb, ge, sc, s, t, o3, begin, n, j in chosen_by_rec.get(r, []):
            gene.append((gb, ge, sc, r, s | (t << 1) | (F_OPEN3 if o3 else 0)))
            c = codons_of(b, begin, n, s)[j:]
            prot = "".join(tab[int(x)] for x in c)
            prots.append((prot if t == EDGE else "M" + prot[1:]).encode())
        off.append(len(gene))
    lens = np.array([len(q) for q in prots], np.uint64)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(prots) else np.zeros(0, np.uint64)
    return {"gene": np.array(gene, GENE_DTYPE) if gene else np.zeros(0, GENE_DTYPE), "aa": np.frombuffer(b"".join(prots), np.uint8), "aa_start": start, "aa_len": lens,
            "rec_gene_off": np.array(off, np.uint64), "info": info, "tables": tables, "proteins": prots, "cands": cands_by_rec}


# ---- files ---------------------------------------------------------------------------------------------------------------------------------------
def contig_genes(contigs, **params):
    """ASCII contigs of ONE genome -> per contig [(begin, end, strand, protein, score, flags)] in contig coordinates, (end, strand) ascending, and info"""
    segs = [(ci, off, RO.codes(seg)) for ci, ctg in enumerate(contigs) for off, seg in RO.split_contig(ctg)]
    res = call([s[2] for s in segs], [0, len(segs)], **params)
    out = [[] for _ in contigs]
    for gn, prot in zip(res["gene"], res["proteins"]):
        ci, off, _ = segs[int(gn["rec"])]
        out[ci].append((off + int(gn["begin"]), off + int(gn["end"]), int(gn["flags"]) & 1, prot, int(gn["score"]), int(gn["flags"])))
    return out, res["info"]


def faa_bytes(contig_ids, genes):
    return b"".join(b">" + RO.orf_name(cid, g[0], g[1], g[2]).encode() + b"\n" + g[3] + b"\n" for cid, lst in zip(contig_ids, genes) for g in lst)


def ffn_bytes(contig_ids, contigs, genes):
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    out = []
    for cid, ctg, lst in zip(contig_ids, contigs, genes):
        for g in lst:
            nt = bytes(ctg[g[0]:g[1]]).upper()
            if g[2]:
                nt = bytes(comp[x] for x in reversed(nt))
            out.append(b">" + RO.orf_name(cid, g[0], g[1], g[2]).encode() + b"\n" + nt + b"\n")
    return b"".join(out)


def gff_bytes(contig_ids, genes):
    out = [b"##gff-version 3\n"]
    for cid, lst in zip(contig_ids, genes):
        for b, e, s, _, sc, fl in lst:
            t = (fl >> 1) & 3
            out.append(("%s\tgsearch_amd\tCDS\t%d\t%d\t%.2f\t%s\t0\tID=%s;start_type=%s;partial=%d%d\n" % (
                cid, b + 1, e, sc / 1024.0, "-" if s else "+", RO.orf_name(cid, b, e, s), ("ATG", "GTG", "TTG", "edge")[t], int(t == EDGE), int(bool(fl & F_OPEN3)))).encode())
    return b"".join(out)
