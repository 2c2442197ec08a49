"""Independent numpy restatement of SPEC.md section 11 (bigsig: a bit-sliced Bloom index of genomes and the genome each read comes from):
segments, k-mer values, row positions, the index as a sparse set of (row, colour) bits, per-colour hit counts, the best colour and the tail.

Shares no code with the library. k-mer values and positions are uint64 arrays (wrapping arithmetic, the 64 x 64 -> high 64 multiply from 32-bit
halves); the tail is Python floats, i.e. IEEE f64 with one rounding per operation, as the library is built (-ffp-contract=off)."""
import struct

import numpy as np

U64 = np.uint64
GAMMA = U64(0x9E3779B97F4A7C15)
FX = U64(0x517CC1B727220A95)
M32 = U64(0xFFFFFFFF)
CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
LN2_HI, LN2_LO, INV_LN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00


# ---- segments and k-mers ----------------------------------------------------------------------------------------------------------------------
def segments(text, qual=None, min_phred=15):
    """[(offset of the first base, [codes])]: maximal runs of A C G T (either case) whose quality, if given, is at least min_phred; line breaks
    are skipped and end nothing"""
    out, cur, begin = [], [], 0
    for i, ch in enumerate(text):
        if ch in (10, 13):
            continue
        ok = ch in CODE and (qual is None or qual[i] - 33 >= min_phred)
        if ok:
            if not cur:
                begin = i
            cur.append(CODE[ch])
        elif cur:
            out.append((begin, cur))
            cur = []
    if cur:
        out.append((begin, cur))
    return out


def kmers_of_codes(codes, k, fwd_only=False):
    """the k-mer values of one segment in order (SPEC 1.1): min(forward, reverse complement), or the forward window alone"""
    c = np.asarray(codes, np.uint64)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    fwd, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fwd |= c[j:j + n] << U64(2 * (k - 1 - j))
        rc |= (U64(3) - c[j:j + n]) << U64(2 * j)
    return fwd if fwd_only else np.minimum(fwd, rc)


def kmers(records, k, quals=None, min_phred=15, fwd_only=False):
    """the k-mer occurrences of a genome or a read (a list of records, bytes) in order"""
    out = [np.zeros(0, np.uint64)]
    for i, r in enumerate(records):
        for _, codes in segments(r, None if quals is None else quals[i], min_phred):
            out.append(kmers_of_codes(codes, k, fwd_only))
    return np.concatenate(out)


# ---- positions --------------------------------------------------------------------------------------------------------------------------------
def _mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def _mulhi(a, b):
    """high 64 bits of a x b for uint64 arrays a and a scalar b, from 32-bit halves"""
    b = U64(b)
    al, ah, bl, bh = a & M32, a >> U64(32), b & M32, b >> U64(32)
    with np.errstate(over="ignore"):
        ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
        mid = (ll >> U64(32)) + (lh & M32) + (hl & M32)
        return hh + (lh >> U64(32)) + (hl >> U64(32)) + (mid >> U64(32))


def positions(v, h, B):
    """(len(v), h) rows: pos_i = mulhi64(h1 + i (h2 | 1), B), h1 and h2 the first two SplitMix64 outputs from state fx64(v)"""
    v = np.atleast_1d(np.asarray(v, np.uint64))
    with np.errstate(over="ignore"):
        x = v * FX
        h1, st = _mix(x + GAMMA), _mix(x + U64(2) * GAMMA) | U64(1)
        return np.stack([_mulhi(h1 + U64(i) * st, B) for i in range(h)], axis=1)


# ---- index and query --------------------------------------------------------------------------------------------------------------------------
class Index:
    def __init__(self, k, h, B, fwd_only=False):
        self.k, self.h, self.B, self.fwd = k, h, B, fwd_only
        self.cols = []              # per colour: sorted unique rows
        self.nk = []

    def add(self, records, quals=None, min_phred=15):
        v = kmers(records, self.k, quals, min_phred, self.fwd)
        self.cols.append(np.unique(positions(v, self.h, self.B).ravel()) if len(v) else np.zeros(0, np.uint64))
        self.nk.append(len(v))

    def t(self):
        return np.array([len(c) for c in self.cols], np.uint64)

    def row_words(self, rows, n_words):
        """(len(rows), n_words) u64: colour c is bit c & 63 of word c >> 6"""
        rows = np.asarray(rows, np.uint64)
        out = np.zeros((len(rows), n_words), np.uint64)
        for c, col in enumerate(self.cols):
            out[np.isin(rows, col), c >> 6] |= U64(1) << U64(c & 63)
        return out

    def _pairs(self):
        """every set bit as (row, colour), sorted by row: the sparse matrix"""
        if getattr(self, "_built", None) != len(self.cols):
            rows = np.concatenate(self.cols) if self.cols else np.zeros(0, np.uint64)
            cols = np.concatenate([np.full(len(c), i, np.int64) for i, c in enumerate(self.cols)]) if self.cols else np.zeros(0, np.int64)
            o = np.argsort(rows, kind="stable")
            self._rows, self._colour, self._built = rows[o], cols[o], len(self.cols)
        return self._rows, self._colour

    def counts(self, read, quals=None, min_phred=15, down_sample=1):
        """(n, hits[n_colours]) of one read (a list of records; the mates of a pair are two records)"""
        v = kmers(read, self.k, quals, min_phred, self.fwd)[::down_sample]
        hits = np.zeros(len(self.cols), np.uint32)
        if len(v):
            rows, colour = self._pairs()
            pos = positions(v, self.h, self.B)
            lo, hi = np.searchsorted(rows, pos, "left"), np.searchsorted(rows, pos, "right")
            for j in range(len(v)):
                if (hi[j] == lo[j]).any():
                    continue
                common = set(colour[lo[j, 0]:hi[j, 0]].tolist())
                for i in range(1, self.h):
                    common &= set(colour[lo[j, i]:hi[j, i]].tolist())
                for c in common:
                    hits[c] += 1
        return len(v), hits

    def query(self, reads, quals=None, min_phred=15, down_sample=1):
        n_reads = len(reads)
        nk, bc, bh = np.zeros(n_reads, np.uint32), np.zeros(n_reads, np.uint32), np.zeros(n_reads, np.uint32)
        dense = np.zeros((n_reads, len(self.cols)), np.uint32)
        for r, read in enumerate(reads):
            nk[r], dense[r] = self.counts(read, None if quals is None else quals[r], min_phred, down_sample)
            bc[r], bh[r] = best(dense[r])
        return nk, bc, bh, dense

    def classify(self, nk, bc, bh, fp):
        t = self.t()
        tl = np.array([tail(int(t[c]), self.B, self.h, int(n), int(x)) for n, c, x in zip(nk, bc, bh)], np.float64)
        return tl, np.array([x > 0 and a < fp for x, a in zip(bh, tl)], bool)


def best(hits):
    """(colour, hits) maximising (hits, -colour)"""
    c = int(np.argmax(hits)) if len(hits) else 0        # argmax returns the first maximum
    return c, int(hits[c]) if len(hits) else 0


# ---- SPEC 2 LN / EXP and the tail, scalar f64 --------------------------------------------------------------------------------------------------
def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def LN(x):
    b = _bits(x)
    e = ((b >> 52) & 0x7FF) - 1023
    t = _from_bits((b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000)
    if t > 1.4142135623730951:
        t = t * 0.5
        e += 1
    s = (t - 1.0) / (t + 1.0)
    z = s * s
    p = 1.0 / 23.0
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    return float(e) * 0.6931471805599453 + 2.0 * s * p


def _pow2(k):
    return _from_bits((k + 1023) << 52)


def EXP(x):
    if x != x:
        return x
    if x < -745.2:
        return 0.0
    if x > 709.7:
        return float("inf")
    k = int(x * INV_LN2 + (-0.5 if x < 0.0 else 0.5))          # truncation towards zero
    r = (x - float(k) * LN2_HI) - float(k) * LN2_LO
    p = 1.0 / 6227020800.0
    for f in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / f
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    if k < -1022:
        return (p * _pow2(k + 1000)) * _pow2(-1000)
    return p * _pow2(k)


def tail(t_c, B, h, n, x0):
    """P(X >= x0), X ~ Binomial(n, (t_c / B)^h), SPEC 11 steps 1-6"""
    q = float(t_c) / float(B)
    p = q
    for _ in range(h - 1):
        p = p * q
    x0 = min(x0, n)
    if x0 == 0:
        return 1.0
    if p == 0.0:
        return 0.0
    if p >= 1.0:
        return 1.0
    l1 = LN(1.0 - p)
    lq = LN(p) - l1
    lp = float(n) * l1
    for x in range(x0):
        lp = lp + (LN(float(n - x) / float(x + 1)) + lq)
    tl = 0.0
    x = x0
    while True:
        term = EXP(lp)
        tl = tl + term
        if x >= n or (x > x0 and term < tl * 2.0 ** -60):
            break
        lp = lp + (LN(float(n - x) / float(x + 1)) + lq)
        x += 1
    return min(tl, 1.0)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def reads_txt(accessions, ids, bc, bh, nk, accept):
    out = []
    for i, rid in enumerate(ids):
        hit = bh[i] > 0
        out.append("%s\t%s\t%d\t%d\t%s\n" % (rid, accessions[bc[i]] if hit else "no_hits", bh[i], nk[i], "accept" if hit and accept[i] else "reject"))
    return "".join(out).encode()


def counts_txt(accessions, bc, bh, accept):
    per, rej, nohit = {}, 0, 0
    for c, x, a in zip(bc, bh, accept):
        if x == 0:
            nohit += 1
        elif a:
            per[accessions[c]] = per.get(accessions[c], 0) + 1
        else:
            rej += 1
    lines = ["%s\t%d\n" % (a, n) for a, n in sorted(per.items(), key=lambda kv: (-kv[1], kv[0].encode()))]
    return ("".join(lines) + "reject\t%d\nno_hits\t%d\n" % (rej, nohit)).encode()
