"""numpy restatement of SPEC.md section 10 (coreset and k-medoid clustering of the database), written from the SPEC text: dense matrices,
whole-array argmins, no blocks and no symmetry tricks. The GPU tests require bit equality between this and gs_index_cluster."""
import math

import numpy as np

U64 = np.uint64
GAMMA, MIX1, MIX2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)


def h(seed, r, i):
    """SplitMix64 output (SPEC 2) from state x = seed ^ (r << 56) ^ i; i: uint64 array"""
    with np.errstate(over="ignore"):
        z = (U64(seed) ^ (U64(r) << U64(56)) ^ i.astype(U64)) + GAMMA
        z = (z ^ (z >> U64(30))) * MIX1
        z = (z ^ (z >> U64(27))) * MIX2
        return z ^ (z >> U64(31))


def counts(rows, db):
    """c(i, j): mismatch counts of every row against every row of db (the element type's !=), int64"""
    out = np.zeros((len(rows), len(db)), np.int64)
    for r0 in range(0, len(rows), 64):
        out[r0:r0 + 64] = (rows[r0:r0 + 64, None, :] != db[None, :, :]).sum(axis=2)
    return out


def nearest_of(db, cand):
    """for every node the position in cand that minimises (c, position), and that count"""
    cm = counts(db[np.asarray(cand, np.int64)], db)
    arg = cm.argmin(axis=0)                                   # (argmin returns the first minimum: the smallest position)
    return arg.astype(np.uint32), cm[arg, np.arange(len(db))].astype(np.uint16)


def coreset(db, k, fraction, seed):
    n = len(db)
    t = min(n, max(k, 1, math.ceil(fraction * n)))
    t0 = (t + 1) // 2
    t1 = t - t0
    i = np.arange(n, dtype=U64)
    h0 = h(seed, 0, i)
    in0 = np.zeros(n, bool)
    in0[np.lexsort((i, h0))[:max(k, 1)]] = True
    in0 |= (h0 >> U64(32)) * U64(n) < (U64(t0) << U64(32))
    s0 = np.nonzero(in0)[0]
    d0 = counts(db[s0], db).min(axis=0)
    D = int(d0.sum())
    assert n * db.shape[1] < 1 << 40
    h1 = h(seed, 1, i)
    in1 = ~in0 & ((h1 >> U64(40)) * U64(D) < (U64(t1) * d0.astype(U64)) << U64(24))
    return np.nonzero(in0 | in1)[0]


def cluster(db, n_cluster=0, fraction=0.1, max_iter=15, seed=0):
    """every output of gs_index_cluster as a dict (node numbers, not caller ids)"""
    n, k = len(db), int(n_cluster)
    C = coreset(db, k, fraction, seed)
    p = len(C)
    cm = counts(db[C], db)                                    # p x n
    near = cm.argmin(axis=0)
    near_cnt = cm[near, np.arange(n)]
    w = np.bincount(near, minlength=p).astype(np.int64)
    res = dict(core_nodes=C.astype(U64), core_weight=w.astype(U64), n_core=p)
    if k == 0:
        res.update(centre_node=C[near].astype(U64), centre_count=near_cnt.astype(np.uint16), medoids=np.zeros(0, U64), sizes=np.zeros(0, U64),
                   iterations=0, converged=1, cost_core=0, cost_all=int(near_cnt.sum()))
        return res
    P = cm[:, C]                                              # p x p
    med = [int((w[:, None] * P).sum(axis=0).argmin())]
    dmin = P[:, med[0]].copy()
    while len(med) < k:
        key = w * dmin
        key[med] = -1                                         # chosen ones never win; argmax returns the smallest j among equals
        j = int(key.argmax())
        med.append(j)
        dmin = np.minimum(dmin, P[:, j])
    med = np.array(med, np.int64)
    iterations, converged = 0, 0
    while iterations < max_iter:
        a = P[:, med].argmin(axis=1)                          # smallest t among equals
        a[med] = np.arange(k)
        cost_core = int((w * P[np.arange(p), med[a]]).sum())
        new = med.copy()
        for t in range(k):
            mem = np.nonzero(a == t)[0]
            tot = (w[mem, None] * P[np.ix_(mem, mem)]).sum(axis=0)
            new[t] = mem[tot.argmin()]
        iterations += 1
        if np.array_equal(new, med):
            converged = 1
            break
        med = new
    mnodes = np.sort(C[med])
    fm = counts(db[mnodes], db)
    cen = fm.argmin(axis=0)
    cen_cnt = fm[cen, np.arange(n)]
    res.update(centre_node=mnodes[cen].astype(U64), centre_count=cen_cnt.astype(np.uint16), medoids=mnodes.astype(U64),
               sizes=np.bincount(cen, minlength=k).astype(U64), iterations=iterations, converged=converged, cost_core=cost_core,
               cost_all=int(cen_cnt.sum()))
    return res


# ---- the inputs of the tests (shared by test_cluster_cpu.py and test_gpu_cluster.py) ----
def planted(seed, families=8, size=40, m=256, redraw=0.3):
    """`families` random roots, `size` members each with `redraw` of the slots re-randomised, rows shuffled -> (db uint32, family of each row)"""
    rng = np.random.default_rng(1000 + seed)
    roots = rng.integers(0, 1 << 30, (families, m), dtype=np.uint32)
    db = np.repeat(roots, size, axis=0)
    mask = rng.random(db.shape) < redraw
    db[mask] = rng.integers(0, 1 << 30, int(mask.sum()), dtype=np.uint32)
    fam = np.repeat(np.arange(families), size)
    perm = rng.permutation(len(db))
    return np.ascontiguousarray(db[perm]), fam[perm]


def chain(seed, n=400, m=256, redraw=0.04):
    """row i = row i-1 with `redraw` of the slots redrawn, rows shuffled"""
    rng = np.random.default_rng(2000 + seed)
    db = np.zeros((n, m), np.uint32)
    db[0] = rng.integers(0, 1 << 30, m, dtype=np.uint32)
    for i in range(1, n):
        db[i] = db[i - 1]
        pos = rng.random(m) < redraw
        db[i, pos] = rng.integers(0, 1 << 30, int(pos.sum()), dtype=np.uint32)
    return np.ascontiguousarray(db[rng.permutation(n)])
