"""SPEC.md 8 on the host: the numpy restatement (tests/pyref_embed.py) against its own definitions (EXP, calibration, union, adjacency order),
the CSV format against a literal fixture, the library's default parameters against the reference's, and the embedding quality bar."""
import math
import os

import numpy as np
import pytest

import helpers as H
import pyref_embed as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embed")


def _ulps(a, b):
    ia, ib = np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def test_exp_within_two_ulp():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-745.0, 0.0, 200000), rng.uniform(-1.0, 0.0, 20000), -np.arange(0, 746, dtype=np.float64),
                        [-745.0, -744.44, -708.4, -708.39, -1e-300, -0.0, 0.0, -0.34657359027997264, -0.3465735902799727]])
    got = R.spec_exp(x)
    ref = np.array([math.exp(v) for v in x])
    assert _ulps(got, ref).max() <= 2
    assert R.spec_exp(-746.0) == 0.0 and R.spec_exp(0.0) == 1.0


def test_calibration_meets_target_where_solvable():
    rng = np.random.default_rng(4)
    n, k = 3000, 16
    cnt = rng.integers(2, k + 1, n)
    dist = np.full((n, k), np.inf, np.float32)
    for i in range(n):
        dist[i, :cnt[i]] = np.sort(rng.uniform(0.0, 1.0, cnt[i]).astype(np.float32))
    p = R.calibrate(dist, cnt)
    checked = floored = 0
    for i in range(n):
        c = int(cnt[i])
        d = dist[i, :c].astype(np.float64)
        pos = d[d > 0]
        rho = pos[0] if len(pos) else 0.0
        if (d - rho <= 0).sum() >= math.log2(c):
            continue                                  # no sigma reaches the target
        ps = float(np.sum(p[i, :c].astype(np.float64)))
        if abs(ps - math.log2(c)) < 1e-4:
            checked += 1
        else:
            assert ps < math.log2(c)                  # only the floor of sigma (1e-3 x the mean distance) may keep the sum below its target
            floored += 1
    assert checked > 0.9 * n and floored <= 0.01 * (checked + floored)
    assert (p[:, 0] == 1.0).all()                      # the nearest positive (or zero) distance has membership 1


def test_edge_rows():
    dist = np.array([[0.0, 0.0, 0.3], [0.5, 0.5, 0.5], [0.2, 0.0, 0.0], [0.7, 0.0, 0.0]], np.float32)
    cnt = np.array([3, 3, 0, 1])
    p = R.calibrate(dist, cnt)
    assert (p[1] == 1.0).all()                         # all-equal distances: every entry at rho
    assert (p[0] == 1.0).all()                         # duplicates at 0 lie left of rho = 0.3: membership 1, like rho itself
    assert (p[2] == 0).all() and p[3, 0] == 1.0 and (p[3, 1:] == 0).all()


def _graph():
    U = np.uint64(0xFFFFFFFFFFFFFFFF)
    ids = np.array([[1, 2], [0, 3], [1, U], [0, 2]], np.uint64)
    dist = np.array([[0.1, 0.2], [0.1, 0.4], [0.3, np.inf], [0.2, 0.25]], np.float32)
    return ids, dist, np.array([2, 2, 1, 2], np.uint32)


def test_adjacency_order_and_symmetric_weights():
    ids, dist, cnt = _graph()
    memb = R.calibrate(dist, cnt)
    off, adj, w, W = R.adjacency(ids, cnt, memb)
    lists = [adj[off[i]:off[i + 1]].tolist() for i in range(4)]
    assert lists == [[1, 2, 3], [0, 3, 2], [1, 0, 3], [0, 2, 1]]
    wd = {(i, int(adj[e])): w[e] for i in range(4) for e in range(off[i], off[i + 1])}
    assert all(wd[(j, i)] == v for (i, j), v in wd.items())
    assert wd[(0, 3)] == memb[3, 0]                   # one-sided: the weight is the other end's membership
    pij, pji = memb[0, 0], memb[1, 0]
    assert wd[(0, 1)] == (pij + pji) - pij * pji
    acc = np.float32(0)
    for x in w[off[2]:off[3]]:
        acc = np.float32(acc + x)
    assert W[2] == acc


def test_init_and_hash_ranges():
    y = R.init_positions(5000, 3, 17)
    assert y.dtype == np.float32 and y.min() >= -10 and y.max() < 10 and abs(float(y.mean())) < 0.3
    assert not np.array_equal(y, R.init_positions(5000, 3, 18))
    s = R.neg_samples(5, 3, 1000, 8)
    assert s.min() >= 0 and s.max() < 1000 and len(np.unique(s)) > 900


def test_library_defaults_are_the_reference_constants():
    import gsearch_amd as G
    p = G.EmbedParams()
    ref = R.defaults()
    for f in G.EmbedParams.FIELDS:
        assert np.float32(getattr(p, f)) == np.float32(ref[f]) if isinstance(ref[f], float) else getattr(p, f) == ref[f], f


def test_csv_writer_matches_fixture(tmp_path):
    import gsearch_amd as G
    xy = np.array([[1.0, -2.5], [0.1, 1e-7], [-0.0, 3.4028235e38], [123456.79, -7.0e-45], [np.float32(1) / np.float32(3), 10.0]], np.float32)
    out = tmp_path / "database_embedded.csv"
    assert G.write_embedding_csv(str(out), xy) == 5
    assert out.read_bytes() == open(os.path.join(GOLDEN, "small.csv"), "rb").read()
    back = np.array([[float(v) for v in line.split(",")] for line in out.read_text().splitlines()], np.float32)
    assert np.array_equal(back.view(np.uint32), xy.view(np.uint32))


def test_stats_reference_on_a_small_graph():
    ids, dist, cnt = _graph()
    st = R.stats(ids, dist, cnt)
    assert st["occ"].tolist() == [2, 2, 2, 1] and st["n_edges"] == 7 and st["max_occ"] == 2
    assert st["hubs"][:4] == [(0, 2), (1, 2), (2, 2), (3, 1)]
    assert st["hist"][1] == 1 and st["hist"][2] == 3
    assert st["q_first"][-1] == np.float32(0.2) and st["q_last"][0] == np.float32(0.2)       # sorted[floor(q (N - 1))]


def _families_graph(n_roots, per, m, seed, knbn=8):
    import oracle_lib as O
    db = H.synth_sig_db(n_roots, per, m, seed)
    n = len(db)
    ids, dist = O.bruteforce_topk(db, db, knbn + 1, 8)
    oi, od = np.zeros((n, knbn), np.uint64), np.zeros((n, knbn), np.float32)
    for i in range(n):
        keep = ids[i] != np.uint64(i)
        if keep.all():
            keep[-1] = False
        oi[i], od[i] = ids[i][keep], dist[i][keep]
    # families: connected components of the edges at distance < 0.99 (members of one root share >= 9 % of their slots, others none)
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for i in range(n):
        for t in range(knbn):
            if od[i, t] < 0.99:
                par[find(i)] = find(int(oi[i, t]))
    fam = np.array([find(i) for i in range(n)])
    return oi, od, np.full(n, knbn, np.uint32), fam


QUALITY_BAR = 0.95        # measured on the reference: 1.0 at the defaults (40 x 50 rows, m = 1000)


def test_quality_bar_on_reference():
    ids, dist, cnt, fam = _families_graph(40, 50, 1000, 5)
    assert len(np.unique(fam)) == 40
    y0 = R.init_positions(len(fam), R.DIM, R.SEED)
    assert R.family_purity(y0, fam) < 0.2
    y = R.embed(ids, dist, cnt)
    assert R.family_purity(y, fam) >= QUALITY_BAR
