"""numpy references of the three device primitives of gs_radix.hip: the stable radix sort of 64-bit keys, the run lengths of a sorted array and the
exclusive prefix sum of 32-bit counts. Integers only; the GPU tests compare with ==. Shares no code with the library."""
import numpy as np

U64 = np.uint64


def passes(endbit):
    """8-bit digits the sort walks for `endbit`"""
    assert 1 <= endbit <= 64
    return (endbit + 7) // 8


def sort_mask(endbit):
    """the bits the order is on: [0, 8 * ceil(endbit / 8))"""
    return U64((1 << (8 * passes(endbit))) - 1)


def sort(keys, endbit):
    """keys in ascending order of their bits under sort_mask(endbit); equal ones keep their input order"""
    keys = np.asarray(keys, np.uint64)
    return keys[np.argsort(keys & sort_mask(endbit), kind="stable")]


def run_lengths(a):
    """(the key, the length) of every run of equal neighbours of a, in order"""
    a = np.asarray(a, np.uint64)
    assert len(a) >= 1
    heads = np.concatenate([np.zeros(1, np.int64), np.flatnonzero(a[1:] != a[:-1]) + 1])
    ends = np.concatenate([heads[1:], np.array([len(a)], np.int64)])
    return a[heads], (ends - heads).astype(np.uint32)


def scan(v):
    """(exclusive prefix sums, total) of 32-bit counts whose total stays below 2^32"""
    v = np.asarray(v, np.uint32)
    c = np.cumsum(v.astype(np.uint64), dtype=np.uint64)
    total = int(c[-1]) if len(v) else 0
    assert total < 1 << 32
    out = np.zeros(len(v), np.uint64)
    out[1:] = c[:-1]
    return out.astype(np.uint32), total
