"""Independent numpy restatement of SPEC.md 11.2 (bigsig: tied top hits and the six-field identify report) on top of tests/pyref_bigsi.py (or, for a
minimizer index, tests/pyref_bigsi_mini.py): the ties and the most significant tied colour from the dense per-colour hits, the verdict table, and both text
files. Shares no code with the library."""
import numpy as np

import pyref_bigsi as R

NONE = 0xFFFFFFFF
TOO_SHORT, NO_HITS, NOT_SIGNIFICANT, UNIQUE, TIED = range(5)
STATUS = {TOO_SHORT: "too_short", NO_HITS: "no_hits", NOT_SIGNIFICANT: "no_significant_hits"}


def ties_of(hits, t, max_ties):
    """(best_hits, n_tied, tied[max_ties], sig_colour) of one read from the hits of every colour and the bits set t_c of every colour"""
    tied = np.full(max_ties, NONE, np.uint32)
    bh = int(hits.max()) if len(hits) else 0
    if bh == 0:
        return 0, 0, tied, NONE
    T = np.flatnonzero(hits == hits.max())                        # ascending
    tied[:min(len(T), max_ties)] = T[:max_ties]
    sig = min((int(t[c]), int(c)) for c in T)[1]                  # over all of T, not the listed ones
    return bh, len(T), tied, sig


def ties_from_dense(dense, t, max_ties):
    """(best_hits, n_tied, tied, sig_colour) of every read from the dense hits (n_reads, n_colours)"""
    assert 1 <= max_ties <= 1024
    n = len(dense)
    bh, nt, sc = (np.zeros(n, np.uint32) for _ in range(3))
    td = np.zeros((n, max_ties), np.uint32)
    for r in range(n):
        bh[r], nt[r], td[r], sc[r] = ties_of(dense[r], t, max_ties)
    return bh, nt, td, sc


def query_ties(ref, reads, quals=None, min_phred=15, down_sample=1, max_ties=16):
    """ref: an Index of pyref_bigsi or pyref_bigsi_mini -> (n_kmers, best_hits, n_tied, tied, sig_colour, dense)"""
    n = len(reads)
    nk = np.zeros(n, np.uint32)
    dense = np.zeros((n, len(ref.cols)), np.uint32)
    for r, read in enumerate(reads):
        nk[r], dense[r] = ref.counts(read, None if quals is None else quals[r], min_phred, down_sample)
    return (nk,) + ties_from_dense(dense, ref.t(), max_ties) + (dense,)


def verdict_code(n, best_hits, n_tied, tail, fp):
    """the first row of the table that holds"""
    if n == 0:
        return TOO_SHORT
    if best_hits == 0:
        return NO_HITS
    if not (tail < fp):
        return NOT_SIGNIFICANT
    return UNIQUE if n_tied == 1 else TIED


def verdict(ref, nk, bh, nt, sc, fp):
    """(tail f64 of sig_colour - 1.0 where best_hits is 0, code u8) of every read"""
    t = ref.t()
    tl = np.array([R.tail(int(t[c]), ref.B, ref.h, int(n), int(x)) if x > 0 else 1.0 for n, x, c in zip(nk, bh, sc)], np.float64)
    return tl, np.array([verdict_code(int(n), int(x), int(m), float(a), fp) for n, x, m, a in zip(nk, bh, nt, tl)], np.uint8)


def reads_txt(accessions, ids, nk, bh, nt, td, vd):
    out = []
    max_ties = np.asarray(td).shape[1]
    for i, rid in enumerate(ids):
        v = int(vd[i])
        if v in STATUS:
            status, hits, ties = STATUS[v], 0, 0
        elif v == UNIQUE:
            status, hits, ties = accessions[int(td[i][0])], int(bh[i]), 1
        else:
            names = [accessions[int(c)] for c in td[i][:min(int(nt[i]), max_ties)]]
            status, hits, ties = ",".join(names + (["..."] if int(nt[i]) > max_ties else [])), int(bh[i]), int(nt[i])
        out.append("%s\t%s\t%d\t%d\t%s\t%d\n" % (rid, status, hits, int(nk[i]), "reject" if v in (NOT_SIGNIFICANT, TIED) else "accept", ties))
    return "".join(out).encode()


def counts_txt(accessions, td, vd):
    per, vd = {}, [int(v) for v in vd]
    for i, v in enumerate(vd):
        if v == UNIQUE:
            a = accessions[int(td[i][0])]
            per[a] = per.get(a, 0) + 1
    lines = ["%s\t%d\n" % (a, n) for a, n in sorted(per.items(), key=lambda kv: (-kv[1], kv[0].encode()))]
    return ("".join(lines) + "reject\t%d\nno_hits\t%d\ntoo_short\t%d\n" %
            (vd.count(NOT_SIGNIFICANT) + vd.count(TIED), vd.count(NO_HITS), vd.count(TOO_SHORT))).encode()
