"""Independent numpy restatement of SPEC.md section 11, "Minimizer indexes and the coverage filter": the minimizer occurrences of a text, the values a
coverage filter keeps, and the index / query of tests/pyref_bigsi.py built on them. Written from SPEC.md, shares no code with the library.

Two definitions of the selection stand side by side. `minimizers` is the sequential one of SPEC (a_s per window, an occurrence wherever a_s changes),
vectorised; `minimizers_naive` sorts the (key, position) pairs of every window, takes the first and collects the SET of selected positions. The naive one
is the yardstick: `minimizers_checked` asserts that both agree."""
import numpy as np

import pyref_bigsi as R
from pyref_bigsi import segments, kmers_of_codes, positions, best, tail  # noqa: F401

U64 = np.uint64
GAMMA = U64(0x9E3779B97F4A7C15)
FX = U64(0x517CC1B727220A95)


def key_of(v):
    """h1 of SPEC 11 "Row positions": the first SplitMix64 output from state fx64(v)"""
    v = np.asarray(v, np.uint64)
    with np.errstate(over="ignore"):
        z = v * FX + GAMMA
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def _base_offsets(text, begin, n):
    """text offsets of the n bases of the segment that begins at `begin` (line breaks lie between them)"""
    out, i = [], begin
    while len(out) < n:
        if text[i] not in (10, 13):
            out.append(i)
        i += 1
    return np.array(out, np.uint64)


def _select(keys, k, m):
    """positions (m-mer indices of the segment) of the occurrences: a_0, then every a_s != a_{s-1}"""
    w = k - m + 1
    n_win = len(keys) - w + 1                       # = L - k + 1
    if n_win <= 0:
        return np.zeros(0, np.int64)
    win = np.lib.stride_tricks.sliding_window_view(keys, w)
    a = np.arange(n_win) + np.argmin(win, axis=1)   # argmin returns the first minimum: ties go to the leftmost
    keep = np.ones(n_win, bool)
    keep[1:] = a[1:] != a[:-1]
    return a[keep]


def _select_naive(keys, k, m):
    w = k - m + 1
    chosen = set()
    for s in range(len(keys) - w + 1):
        chosen.add(sorted((int(keys[p]), p) for p in range(s, s + w))[0][1])
    return np.array(sorted(chosen), np.int64)


def _minimizers(text, k, m, qual, min_phred, fwd_only, select):
    assert 1 <= m < k <= 32
    vals, pos = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)]
    for begin, codes in segments(text, qual, min_phred):
        if len(codes) < k:
            continue
        v = kmers_of_codes(codes, m, fwd_only)
        a = select(key_of(v), k, m)
        vals.append(v[a])
        pos.append(_base_offsets(text, begin, len(codes))[a])
    return np.concatenate(vals), np.concatenate(pos)


def minimizers(text, k, m, qual=None, min_phred=15, fwd_only=False):
    """(values, offsets of the m-mer's first base in text) of the minimizer occurrences of one text, in order"""
    return _minimizers(text, k, m, qual, min_phred, fwd_only, _select)


def minimizers_naive(text, k, m, qual=None, min_phred=15, fwd_only=False):
    return _minimizers(text, k, m, qual, min_phred, fwd_only, _select_naive)


def minimizers_checked(text, k, m, qual=None, min_phred=15, fwd_only=False):
    """the naive definition, after asserting that the sequential one gives the same"""
    v, p = minimizers(text, k, m, qual, min_phred, fwd_only)
    nv, np_ = minimizers_naive(text, k, m, qual, min_phred, fwd_only)
    assert np.array_equal(v, nv) and np.array_equal(p, np_)
    assert (np.diff(np_.astype(np.int64)) > 0).all()
    return nv, np_


def occurrences(records, k, m, quals=None, min_phred=15, fwd_only=False):
    """the occurrence values of a genome or a read (a list of records) in order: minimizer occurrences for m > 0, k-mer occurrences for m = 0"""
    if m == 0:
        return R.kmers(records, k, quals, min_phred, fwd_only)
    out = [np.zeros(0, np.uint64)]
    for i, r in enumerate(records):
        out.append(minimizers(r, k, m, None if quals is None else quals[i], min_phred, fwd_only)[0])
    return np.concatenate(out)


def filtered(values, min_count):
    """(values inserted, nk_c): with min_count >= 2 the distinct values that occur at least min_count times and the sum of their counts"""
    if min_count <= 1:
        return values, len(values)
    u, c = np.unique(values, return_counts=True)
    keep = c >= min_count
    return u[keep], int(c[keep].sum())


class Index(R.Index):
    """the index of pyref_bigsi over minimizer occurrences (m > 0) or k-mer occurrences (m = 0), with a coverage filter per added colour"""

    def __init__(self, k, m, h, B, fwd_only=False):
        super().__init__(k, h, B, fwd_only)
        self.m = m

    def add(self, records, quals=None, min_phred=15, min_count=1):
        v, nk = filtered(occurrences(records, self.k, self.m, quals, min_phred, self.fwd), min_count)
        self.cols.append(np.unique(positions(v, self.h, self.B).ravel()) if len(v) else np.zeros(0, np.uint64))
        self.nk.append(nk)

    def counts(self, read, quals=None, min_phred=15, down_sample=1):
        v = occurrences(read, self.k, self.m, quals, min_phred, self.fwd)[::down_sample]
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
