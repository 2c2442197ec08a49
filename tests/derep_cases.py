"""Case table of the derep tests (SPEC 18): name -> (db uint32 rows of m = 96 slots, max_dist, priority or None). No library call, no GPU; the
references are computed once per case and shared (tests/test_derep_cpu.py, tests/test_gpu_derep.py)."""
import functools

import numpy as np

import pyref_derep as R

M = R.M


def cut(c):
    """the max_dist that names the count c exactly"""
    return R.f32_dist(c, M)


def _chain3():
    """A - B - C: c(A, B) = c(B, C) = 5, c(A, C) = 10; nodes A = 0, B = 1, C = 2"""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 20, M, dtype=np.uint32)
    b, c = a.copy(), a.copy()
    b[:5] = (1 << 21) + np.arange(5)
    c[:10] = (1 << 21) + np.arange(10)
    return np.stack([a, b, c])


def _boundary(c_max):
    rng = np.random.default_rng(8)
    base = rng.integers(0, 1 << 20, M, dtype=np.uint32)
    return np.concatenate([base[None, :], R.rows_at(base, [c_max - 1, c_max, c_max + 1], rng)])


def _duplicates():
    """every signature of 9 isolates and of one small family two to four times"""
    db = R.families(5, fams=1, size=6, isolates=9)[0]
    rng = np.random.default_rng(9)
    db = np.concatenate([np.repeat(db[i:i + 1], rng.integers(2, 5), axis=0) for i in range(len(db))])
    return np.ascontiguousarray(db[rng.permutation(len(db))])


def _straddle():
    """about 300 nodes: a 130-node path, families of 30 and isolates, under random priorities: in rank order the chains and the families are spread
    over all blocks of 64 or 96 rows. The path's slots and the families' are the same 96, with values of disjoint ranges."""
    path = R.path_graph(11, 130)[0]
    fam = R.families(12, fams=5, size=30, isolates=21, redraw=0.004)[0] + np.uint32(1 << 12)      # members differ in 0..3 slots: linked at c_max = 1 or not
    db = np.concatenate([path, fam])
    rng = np.random.default_rng(13)
    db = np.ascontiguousarray(db[rng.permutation(len(db))])
    return db, rng.integers(0, 50, len(db)).astype(np.uint64)                                     # (with ties)


INBLOCK = dict(n=150, r0=0, r1=80, x=85, c_max=10)


def _inblock():
    """R0 (rank 0) covers X (rank 85) at count 9; R1 (rank 80) is 12 from R0, so a representative, and 3 from X. With blocks of 50 or 75 rows R1 and
    X share a block that R0 is not in: X goes to R1. Everything else is an isolate."""
    rng = np.random.default_rng(14)
    n = INBLOCK["n"]
    rows = rng.integers(0, 1 << 20, (n, M), dtype=np.uint32)              # row r = the node of rank r
    x = rows[0].copy(); x[:9] = (1 << 21) + np.arange(9)
    r1 = x.copy(); r1[9:12] = (1 << 22) + np.arange(3)
    rows[INBLOCK["x"]], rows[INBLOCK["r1"]] = x, r1
    perm = rng.permutation(n)                                            # node v holds the row of rank perm[v]
    return np.ascontiguousarray(rows[perm]), (n - perm).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def case(name):
    fam0 = R.families(0)[0]
    n0 = len(fam0)
    table = {
        "families": lambda: (fam0, cut(30), None),
        "families_equal": lambda: (fam0, cut(30), np.full(n0, 7, np.uint64)),
        "families_reversed": lambda: (fam0, cut(30), np.arange(n0, dtype=np.uint64)),
        "families_ties": lambda: (fam0, cut(30), (np.arange(n0) % 3).astype(np.uint64)),
        "families_huge_priorities": lambda: (fam0, cut(30), (np.uint64(1 << 63) + (np.arange(n0) % 5).astype(np.uint64))),
        "n257": lambda: (R.families(1, fams=8, size=30, isolates=17)[0], cut(30), None),
        "n1": lambda: (fam0[:1].copy(), cut(30), None),
        "n2_linked": lambda: (_boundary(4)[[0, 1]].copy(), cut(5), None),
        "n2_apart": lambda: (_boundary(4)[[0, 3]].copy(), cut(4), None),
        "boundary": lambda: (_boundary(10), cut(10), None),
        "duplicates": lambda: (_duplicates(), 0.0, None),
        "chain3_b_first": lambda: (_chain3(), cut(5), np.array([1, 2, 1], np.uint64)),
        "chain3_a_first": lambda: (_chain3(), cut(5), np.array([3, 2, 1], np.uint64)),
        "chain3_c_first": lambda: (_chain3(), cut(5), np.array([1, 2, 3], np.uint64)),
        "path600": lambda: (R.path_graph(0, 600)[0], cut(1), None),
        "ring600": lambda: (R.path_graph(1, 600, ring=True)[0], cut(1), None),
        "all_linked": lambda: (R.families(2, fams=3, size=10, isolates=5)[0], 1.0, None),
        "beyond_one": lambda: (R.families(2, fams=3, size=10, isolates=5)[0], 1.5, None),
        "none_linked": lambda: (fam0, 0.0, None),
        "straddle": lambda: (_straddle()[0], cut(1), _straddle()[1]),
        "inblock": lambda: (_inblock()[0], cut(INBLOCK["c_max"]), _inblock()[1]),
    }
    return table[name]()


NAMES = ["families", "families_equal", "families_reversed", "families_ties", "families_huge_priorities", "n257", "n1", "n2_linked", "n2_apart", "boundary",
         "duplicates", "chain3_b_first", "chain3_a_first", "chain3_c_first", "path600", "ring600", "all_linked", "beyond_one", "none_linked", "straddle", "inblock"]


def as_dtype(db, dtype):
    """the generators' uint32 rows in another element type; the restatement counts the converted rows, which is what both sides see"""
    if np.dtype(dtype) == np.uint16:
        return np.ascontiguousarray((db & 0xFFFF).astype(np.uint16))
    return np.ascontiguousarray(db.astype(dtype))


@functools.lru_cache(maxsize=None)
def reference(name, dtype="uint32"):
    """-> (c_max, components, greedy by the sequential definition)"""
    db, max_dist, prio = case(name)
    db = as_dtype(db, np.dtype(dtype))
    c_max = R.c_max_of(max_dist, db.shape[1])
    return c_max, R.components(db, c_max), R.greedy_sequential(db, c_max, prio)
