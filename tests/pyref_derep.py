"""numpy restatement of SPEC.md section 18 (derep: clusters and representatives of the database at a distance cut), written from the SPEC text: the
whole count matrix at once, a naive union-find, the greedy representatives by two definitions, the two text files and the ANI cut. The GPU tests
require `==` between this and gs_index_components / gs_index_derep on every output word."""
import math

import numpy as np

from pyref_cluster import counts


def c_max_of(max_dist, m):
    """SPEC 6: the largest count c <= m with (f32)c / (f32)m <= (f32)max_dist"""
    md = np.float32(max_dist)
    ok = [c for c in range(m + 1) if np.float32(c) / np.float32(m) <= md]
    return ok[-1] if ok else 0


def links(db, c_max):
    """the link graph as a boolean matrix: u != v (by node number) and c(u, v) <= c_max"""
    cm = counts(db, db)
    L = cm <= c_max
    np.fill_diagonal(L, False)
    return cm, L


def ranks(n, priority=None):
    """order[r] = the node of rank r under (priority descending, node number ascending); rank_of[v]"""
    pr = [0] * n if priority is None else [int(p) for p in priority]
    order = sorted(range(n), key=lambda v: (-pr[v], v))
    rank_of = [0] * n
    for r, v in enumerate(order):
        rank_of[v] = r
    return order, rank_of


def info_of(cluster, c_max):
    size = np.bincount(np.asarray(cluster, np.int64))
    size = size[size > 0]
    return dict(n_clusters=int(len(size)), n_singletons=int((size == 1).sum()), largest=int(size.max()), c_max=int(c_max))


def components(db, c_max):
    """label[v] = the smallest node number of v's connected component: a union-find without ranks or compression, read off by walking up"""
    n = len(db)
    _, L = links(db, c_max)
    parent = list(range(n))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for u, v in zip(*np.nonzero(L)):
        a, b = root(int(u)), root(int(v))
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.array([root(v) for v in range(n)], np.uint64)
    return dict(label=label, **info_of(label, c_max))


def _assign(cm, L, order, rank_of, rep):
    """rep_node / rep_count from the representative flags: itself and 0, or the linked representative of earlier rank that minimises (c, rank)"""
    n = len(order)
    node, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint16)
    for v in range(n):
        if rep[v]:
            node[v], cnt[v] = v, 0
            continue
        cand = [(int(cm[u, v]), rank_of[u]) for u in range(n) if rep[u] and L[u, v] and rank_of[u] < rank_of[v]]
        c, r = min(cand)
        node[v], cnt[v] = order[r], c
    return node, cnt


def greedy_sequential(db, c_max, priority=None):
    """the loop over ranks: a node is a representative iff no representative before it is linked to it"""
    n = len(db)
    cm, L = links(db, c_max)
    order, rank_of = ranks(n, priority)
    rep = [False] * n
    for v in order:
        rep[v] = not any(rep[u] and L[u, v] for u in order[:rank_of[v]])
    node, cnt = _assign(cm, L, order, rank_of, rep)
    return dict(rep_node=node, rep_count=cnt, reps=np.array([v for v in order if rep[v]], np.uint64), **info_of(node, c_max))


def greedy_peeling(db, c_max, priority=None):
    """the lexicographically first maximal independent set by rounds: every undecided node all of whose undecided neighbours have a later rank is
    a representative; its undecided neighbours are none; repeat"""
    n = len(db)
    cm, L = links(db, c_max)
    order, rank_of = ranks(n, priority)
    rk = np.array(rank_of)
    state = np.zeros(n, np.int8)                              # 0 undecided, 1 representative, -1 covered
    while (state == 0).any():
        und = state == 0
        first = [v for v in np.nonzero(und)[0] if not (L[v] & und & (rk < rk[v])).any()]
        assert first
        for v in first:
            state[v] = 1
        for v in first:
            state[L[v] & (state == 0)] = -1
    rep = state == 1
    node, cnt = _assign(cm, L, order, rank_of, rep)
    return dict(rep_node=node, rep_count=cnt, reps=np.array([v for v in order if rep[v]], np.uint64), **info_of(node, c_max))


# ---- the ANI cut and the two files ---------------------------------------------------------------------------------------------------------------
def ani(distance, kmer, model):
    """reformat's transform of a DistHamming distance (SPEC 17): f = 2 (1 - d) / (2 - d); model 1: (1 + ln f / k) 100, model 2: f^(1 / k) 100"""
    f = (1.0 - distance) * 2.0 / (1.0 - distance + 1.0)
    if model == 1:
        return (1.0 + (math.log(f) if f > 0 else -math.inf) / kmer) * 100.0
    return math.pow(f, 1.0 / kmer) * 100.0


def f32_dist(c, m):
    return float(np.float32(c) / np.float32(m))


def ani_cut(ani_value, kmer, model, m):
    """the largest count whose forward transform is >= ani_value, by trying every count -> (c_max, max_dist)"""
    ok = [c for c in range(m + 1) if ani(f32_dist(c, m), kmer, model) >= ani_value]
    return ok[-1], f32_dist(ok[-1], m)


def _display_f64(x):
    """the shortest round-trip digits, positional, no `.0` (Rust's `{}`)"""
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = repr(float(x))
    if "e" in s or "E" in s:
        import decimal
        s = format(decimal.Decimal(s), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def _upper_exp5(x):
    mant, exp = ("%.5E" % x).split("E")
    return "%sE%d" % (mant, int(exp))


def clusters_text(paths, cluster_node, rep_count, m, kmer, model):
    """derep.clusters.tsv; rep_count None: single linkage, distance and ANI are `-`"""
    size = np.bincount(np.asarray(cluster_node, np.int64), minlength=len(paths))
    out = ["genome\trepresentative\tdistance\tani\tcluster_size\n"]
    for v in range(len(paths)):
        r = int(cluster_node[v])
        if rep_count is None:
            d_s = a_s = "-"
        else:
            d = f32_dist(int(rep_count[v]), m)
            d_s, a_s = _upper_exp5(d), _display_f64(ani(d, kmer, model))
        out.append("%s\t%s\t%s\t%s\t%d\n" % (paths[v], paths[r], d_s, a_s, size[r]))
    return "".join(out)


def representatives_text(paths, reps):
    return "".join(paths[int(r)] + "\n" for r in reps)


# ---- the inputs of the tests (shared by test_derep_cpu.py and test_gpu_derep.py) -------------------------------------------------------------------
M = 96


def rows_at(base, ks, rng):
    """rows that differ from `base` in exactly k slots, one per k in ks (values above every generator's range, all distinct)"""
    out = np.repeat(base[None, :], len(ks), axis=0).copy()
    for i, k in enumerate(ks):
        pos = rng.choice(len(base), k, replace=False)
        out[i, pos] = (1 << 30) + 1000 * (i + 1) + np.arange(k, dtype=np.uint32)
    return out


def families(seed, fams=6, size=12, isolates=9, redraw=0.06, m=M):
    """planted families (members = the root with `redraw` of the slots redrawn) plus isolates, shuffled -> (db uint32, family of each row; isolates -1)"""
    rng = np.random.default_rng(3000 + seed)
    roots = rng.integers(0, 1 << 30, (fams, m), dtype=np.uint32)
    db = np.repeat(roots, size, axis=0)
    mask = rng.random(db.shape) < redraw
    db[mask] = rng.integers(0, 1 << 30, int(mask.sum()), dtype=np.uint32)
    db = np.concatenate([db, rng.integers(0, 1 << 30, (isolates, m), dtype=np.uint32)])
    fam = np.concatenate([np.repeat(np.arange(fams), size), np.full(isolates, -1)])
    perm = rng.permutation(len(db))
    return np.ascontiguousarray(db[perm]), fam[perm]


def path_graph(seed, n, ring=False, m=M):
    """a path at c_max = 1: step p gives ONE slot a fresh value (slot p % m; the last n % m steps take the slots 0, 1, ... again) and row p is the
    state after step p, so rows p - 1 and p differ in one slot and rows further apart in min(distance, n % m) slots at least. ring: the state is
    cyclic (a slot no step <= p has touched holds the value of its last step of the cycle), so row n - 1 and row 0 differ in one slot too.
    Node numbers are a random permutation of the positions -> (db uint32, position of each node)"""
    full = n - n % m
    assert n % m != 1 and (n > 2 * m or not ring)
    slot = [p % m if p < full else p - full for p in range(n)]
    cur = -1 - np.arange(m, dtype=np.int64)                   # the base: one value per slot that no step gives
    if ring:
        for p in range(n):
            cur[slot[p]] = p
    pos_rows = np.zeros((n, m), np.int64)
    for p in range(n):
        cur[slot[p]] = p
        pos_rows[p] = cur
    perm = np.random.default_rng(4000 + seed).permutation(n)  # node v is position perm[v]
    return np.ascontiguousarray((pos_rows[perm] + m + 1).astype(np.uint32)), perm
