"""Numpy / Python restatement of SPEC 14 (orfs: stop-to-stop six-frame translation), written from the SPEC text and sharing no code with gs_orf.hip.
Two independent definitions of the ORF set:
  orfs_scan   one forward pass over the codon positions with six carried "position after the last stop" values, one per (strand, class mod 3)
  orfs_naive  translate seq[f:] and revcomp(seq)[f:] for f = 0..2, split at `*`, map the coordinates back, sort by (end, strand)
Bases are codes A C G T = 0 1 2 3; a codon b0 b1 b2 has index 16 b0 + 4 b1 + b2."""
import numpy as np

TABLES = {11: "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF",
          4: "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSSWCWCLFLF"}
MIN_AA = 30
ORF_DTYPE = np.dtype([("begin", np.uint64), ("rec", np.uint32), ("strand", np.uint32)])
_CODE = np.full(256, 255, np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def codes(ascii_bytes):
    """ASCII ACGTacgt -> base codes (anything else is an error here: records hold no invalid base)"""
    c = _CODE[np.frombuffer(bytes(ascii_bytes), np.uint8)]
    assert (c < 4).all()
    return c


def ascii_of(code_arr):
    return bytes(b"ACGT"[int(x)] for x in code_arr)


def pack_at(records, starts):
    """records (code arrays) at the given base offsets -> the packed buffer: base w in byte w >> 2, bits 7 - 2 (w & 3) and the one below"""
    end = max([int(s) + len(r) for s, r in zip(starts, records)] + [0])
    buf = np.zeros((end + 3) // 4 + 1, np.uint8)
    for s, r in zip(starts, records):
        w = int(s) + np.arange(len(r))
        np.bitwise_or.at(buf, w >> 2, (np.asarray(r, np.uint8) << (6 - 2 * (w & 3))).astype(np.uint8))
    return buf


def _keep(n, min_aa, max_aa):
    return min_aa <= n and (max_aa == 0 or n <= max_aa)


def fwd_codon(b, p):
    return 16 * int(b[p]) + 4 * int(b[p + 1]) + int(b[p + 2])


def rev_codon(b, p):
    return 16 * (3 - int(b[p + 2])) + 4 * (3 - int(b[p + 1])) + (3 - int(b[p]))


def orfs_scan(b, min_aa=MIN_AA, max_aa=0, table=11):
    """-> ([(begin, n, strand)] of the kept ORFs in (end, strand) order, n_long)"""
    tab, L = TABLES[table], len(b)
    after = [[c for c in range(3)] for _ in range(2)]            # [strand][class]: the position after the last stop, or the class's first position
    out, n_long = [], 0

    def close(s, c, p):
        nonlocal n_long
        n = (p - after[s][c]) // 3
        if _keep(n, min_aa, max_aa):
            out.append((after[s][c], n, s))
        elif max_aa and n > max_aa:
            n_long += 1

    for p in range(0, L - 2):
        c = p % 3
        for s, idx in ((0, fwd_codon(b, p)), (1, rev_codon(b, p))):
            if tab[idx] == "*":
                close(s, c, p)
                after[s][c] = p + 3
    virt = []
    for c in range(3):
        p = c
        while p <= L - 3:
            p += 3
        virt += [(p, 0, c), (p, 1, c)]                             # the virtual end of the class: its first position past L - 3
    for p, s, c in sorted(virt):
        close(s, c, p)
    return out, n_long


def _translate(b, f, tab):
    return "".join(tab[fwd_codon(b, p)] for p in range(f, len(b) - 2, 3))


def orfs_naive(b, min_aa=MIN_AA, max_aa=0, table=11):
    """the same set from whole-frame translations; -> ([(begin, n, strand, protein)] sorted by (end, strand), n_long)"""
    tab, L = TABLES[table], len(b)
    rc = (3 - np.asarray(b, np.int64))[::-1]
    found, n_long = [], 0
    for s, seq in ((0, np.asarray(b, np.int64)), (1, rc)):
        for f in range(3):
            j = 0
            for run in _translate(seq, f, tab).split("*"):
                n = len(run)
                if _keep(n, min_aa, max_aa):
                    lo = f + 3 * j                                 # first base of the run on `seq`
                    begin = lo if s == 0 else L - (lo + 3 * n)
                    found.append((begin + 3 * n, s, begin, n, run))
                elif max_aa and n > max_aa:
                    n_long += 1
                j += n + 1
    return [(bg, n, s, run.encode()) for _, s, bg, n, run in sorted(found)], n_long


def protein(b, begin, n, strand, table=11):
    tab = TABLES[table]
    if strand == 0:
        return "".join(tab[fwd_codon(b, begin + 3 * t)] for t in range(n)).encode()
    end = begin + 3 * n
    return "".join(tab[rev_codon(b, end - 3 - 3 * t)] for t in range(n)).encode()


def translate_records(records, min_aa=MIN_AA, max_aa=0, table=11):
    """records: code arrays -> the arrays gs_orf_translate writes: dict of orf, aa, aa_start, aa_len, rec_orf_off, n_long (+ `proteins`, a list of bytes)"""
    orf, prots, off, n_long = [], [], [0], 0
    for r, b in enumerate(records):
        lst, nl = orfs_scan(b, min_aa, max_aa, table)
        n_long += nl
        for begin, n, s in lst:
            orf.append((begin, r, s))
            prots.append(protein(b, begin, n, s, table))
        off.append(len(orf))
    lens = np.array([len(p) for p in prots], np.uint64)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(prots) else np.zeros(0, np.uint64)
    return {"orf": np.array(orf, ORF_DTYPE) if orf else np.zeros(0, ORF_DTYPE), "aa": np.frombuffer(b"".join(prots), np.uint8), "aa_start": start, "aa_len": lens,
            "rec_orf_off": np.array(off, np.uint64), "n_long": n_long, "proteins": prots}


def split_contig(ascii_bytes):
    """[(offset, ascii segment)]: a contig cut at every byte outside ACGTacgt"""
    out, i, t = [], 0, bytes(ascii_bytes)
    while i < len(t):
        if _CODE[t[i]] > 3:
            i += 1
            continue
        j = i
        while j < len(t) and _CODE[t[j]] <= 3:
            j += 1
        out.append((i, t[i:j]))
        i = j
    return out


def contig_orfs(contigs, min_aa=MIN_AA, max_aa=0, table=11):
    """ASCII contigs -> per contig [(begin, end, strand, protein)] in contig coordinates, (end, strand) ascending"""
    out = []
    for ctg in contigs:
        lst = []
        for off, seg in split_contig(ctg):
            b = codes(seg)
            for begin, n, s in orfs_scan(b, min_aa, max_aa, table)[0]:
                lst.append((off + begin, off + begin + 3 * n, s, protein(b, begin, n, s, table)))
        out.append(lst)
    return out


def orf_name(contig_id, begin, end, strand):
    return "%s_%d_%d_%s" % (contig_id, begin + 1, end, "-" if strand else "+")


def faa_bytes(contig_ids, orfs):
    return b"".join(b">" + orf_name(cid, b, e, s).encode() + b"\n" + p + b"\n" for cid, lst in zip(contig_ids, orfs) for b, e, s, p in lst)


# ---- planted genes ------------------------------------------------------------------------------------------------------------------------
def back_translate(prot, table=11):
    """the first codon, in table order, of every residue -> code array"""
    tab = TABLES[table]
    out = []
    for ch in bytes(prot).decode():
        i = tab.index(ch)
        out += [i >> 4, (i >> 2) & 3, i & 3]
    return np.array(out, np.uint8)


def planted_genome(rng, prot, strand, f, left=300, right=250, table=11):
    """random bases, `prot` back-translated and planted on `strand` behind a left flank of left + f bases -> (code array, begin of the planted gene)"""
    gene = back_translate(prot, table)
    if strand:
        gene = (3 - gene)[::-1]
    lf = rng.integers(0, 4, left + f).astype(np.uint8)
    rf = rng.integers(0, 4, right).astype(np.uint8)
    return np.concatenate([lf, gene, rf]).astype(np.uint8), left + f


def planted_cases(models, seed=7):
    """the planted genomes of the tests: for each model, strand and f = 0..2 -> list of dicts (model index, strand, f, genome codes, gene begin, consensus)"""
    import pyref_hmm as R
    rng = np.random.default_rng(seed)
    out = []
    for mi, m in enumerate(models):
        cons = R.consensus(m["tables"])
        for strand in (0, 1):
            for f in range(3):
                g, at = planted_genome(rng, cons, strand, f)
                out.append({"model": mi, "strand": strand, "f": f, "genome": g, "at": at, "cons": cons})
    return out
