"""Exact k-NN on the device: gs_index_exact_search (queries against every node) and gs_index_knn_graph (the database's own neighbour lists,
the output of upstream's hnsw2knn, exact instead of the HNSW layer-0 lists). Both are a block of the 16-bit count matrix followed by the top-k
select of gs_knn.hip; the answers must equal the CPU oracle's brute force (ascending (distance, node number)) bit for bit, with either count
producer (match-join or compare tile kernel)."""
import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
DTYPES = [np.float32, np.uint32, np.uint64, np.uint16]


def _index(G, db, M=8):
    """an index over db without an HNSW build: an empty layer-0 graph is imported (the exact paths never read the graph)"""
    n = len(db)
    hn = G.Hnsw.new(M, max(n, 1024), 16, 40, G.DistHamming(), dtype=db.dtype)
    hn.import_graph(db, dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32),
                             cnt0=np.zeros((n, 2 * M), np.uint32), upidx=np.full(n, -1, np.int32), n_upper=0))
    return hn


def _tie_db(dtype, m, seed):
    """dense families (jhi near 1), exact duplicate rows, n not a multiple of 8"""
    db = H.synth_sig_db(13, 23, m, seed, dtype=dtype, jlo=0.9, jhi=0.9999)            # 299 rows
    return np.ascontiguousarray(np.concatenate([db, db[[0, 5, 5, 100]]]))              # 303 rows


def _self_ref(db, rows, knbn, nthreads=8):
    """the oracle's answer for the self graph: brute force with one more neighbour, the row's own node removed by index"""
    ids, dist = O.bruteforce_topk(db, db[rows], knbn + 1, nthreads)
    oi, od = np.full((len(rows), knbn), U64MAX), np.full((len(rows), knbn), np.inf, np.float32)
    for i, r in enumerate(rows):
        keep = ids[i] != np.uint64(r)
        if keep.all():
            keep[-1] = False                     # the node itself lies beyond knbn + 1 (that many exact duplicates with smaller numbers)
        oi[i], od[i] = ids[i][keep], dist[i][keep]
    return oi, od


@pytest.mark.parametrize("impl", ["join", "tile"])
@pytest.mark.parametrize("m", [24, 1000, 18000])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_exact_search_equals_oracle(gpu_ctx, monkeypatch, dtype, m, impl):
    import gsearch_amd as G
    if impl == "tile":
        monkeypatch.setenv("GS_DENSE_IMPL", "tile")
    db = _tie_db(dtype, m, 11 + m)
    n = len(db)
    q = np.ascontiguousarray(np.concatenate([H.queries_from(db, 40, 3, frac=0.05), db[[0, 7, 302]]]))
    hn = _index(G, db)
    for knbn in (1, 7, 50, 1024):
        ids, dist, cnt = hn.exact_search_arrays(q, knbn)
        oi, od = O.bruteforce_topk(db, q, knbn, 8)
        assert np.array_equal(ids, oi) and np.array_equal(dist, od), knbn
        assert (cnt == min(knbn, n)).all()
        if knbn == 50:
            bi, bd = hn.bruteforce_search(q, knbn)
            assert np.array_equal(ids, bi) and np.array_equal(dist, bd)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_producers_give_identical_answers(gpu_ctx, monkeypatch, dtype):
    import gsearch_amd as G
    db = _tie_db(dtype, 1000, 5)
    q = H.queries_from(db, 64, 8, frac=0.02)
    hn = _index(G, db)
    a = hn.exact_search_arrays(q, 33)
    g = hn.knn_graph(33)
    monkeypatch.setenv("GS_DENSE_IMPL", "tile")
    b = hn.exact_search_arrays(q, 33)
    h = hn.knn_graph(33)
    for x, y in zip(a + g, b + h):
        assert np.array_equal(x, y)


def test_declined_join_gives_the_same_answers(gpu_ctx, monkeypatch, capfd):
    """a redundant batch against a redundant database: the join declines and the compare tile kernel fills the count rows"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_JOIN_VERBOSE", "1")
    db = H.synth_sig_db(2, 2600, 96, 7, jlo=0.85, jhi=0.99)          # two big families of near-identical signatures (5200 nodes)
    hn = _index(G, db)
    ids, dist, cnt = hn.knn_graph(20)
    assert ": tile" in capfd.readouterr().err
    oi, od = _self_ref(db, np.arange(len(db)), 20, 16)
    assert np.array_equal(ids, oi) and np.array_equal(dist, od) and (cnt == 20).all()
    q = np.repeat(db[:3], 400, axis=0)
    ids, dist, cnt = hn.exact_search_arrays(q, 10)
    oi, od = O.bruteforce_topk(db, q, 10, 16)
    assert np.array_equal(ids, oi) and np.array_equal(dist, od)


def test_cutoff_is_the_f32_distance(gpu_ctx):
    """max_dist keeps count c exactly when (float)c / (float)m <= max_dist; a neighbour one count above is dropped. The boundaries are taken
    where floor(max_dist * m) would keep one count less."""
    import gsearch_amd as G
    m = 18000
    cs = np.arange(3, m - 8, dtype=np.uint64)
    fd = cs.astype(np.float32) / np.float32(m)
    low = cs[np.floor(fd.astype(np.float64) * m).astype(np.uint64) < cs]           # the f32 distance rounds below c / m
    assert len(low) > 100
    rng = np.random.default_rng(4)
    q = rng.integers(0, 1 << 23, (1, m)).astype(np.float32) * np.float32(2.0 ** -23)
    for c in [int(low[0]), int(low[len(low) // 2]), 4500]:
        db = np.repeat(q, 12, axis=0)
        for i in range(12):                                  # two neighbours each at c - 2 .. c + 3 mismatches
            pos = rng.permutation(m)[:c - 2 + i // 2]
            db[i, pos] += np.float32(1.0)
        far = rng.integers(0, 1 << 23, (20, m)).astype(np.float32) * np.float32(2.0 ** -23) + np.float32(2.0)
        db = np.ascontiguousarray(np.concatenate([db, far]))
        hn = _index(G, db)
        max_dist = float(np.float32(c) / np.float32(m))
        ids, dist, cnt = hn.exact_search_arrays(q, 16, max_dist)
        oi, od = O.bruteforce_topk(db, q, 16)
        keep = od[0] <= np.float32(max_dist)
        assert int(cnt[0]) == int(keep.sum()) == 6, c                    # c - 2, c - 1 and c, two of each; c + 1 and beyond dropped
        assert np.array_equal(ids[0, :6], oi[0, keep]) and np.array_equal(dist[0, :6], od[0, keep])
        assert (ids[0, 6:] == U64MAX).all() and np.isinf(dist[0, 6:]).all()
        # the self graph under the same cut-off: the oracle's list filtered by numpy
        gi, gd, gc = hn.knn_graph(16, max_dist)
        oi, od = _self_ref(db, np.arange(len(db)), 16)
        for r in range(len(db)):
            keep = od[r] <= np.float32(max_dist)
            k = int(keep.sum())
            assert int(gc[r]) == k and np.array_equal(gi[r, :k], oi[r, keep]) and np.array_equal(gd[r, :k], od[r, keep])
            assert (gi[r, k:] == U64MAX).all() and np.isinf(gd[r, k:]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=lambda d: np.dtype(d).name)
def test_knn_graph_equals_oracle(gpu_ctx, dtype):
    import gsearch_amd as G
    db = _tie_db(dtype, 1000, 21)
    n = len(db)
    hn = _index(G, db)
    for knbn in (1, 32, 1024):
        ids, dist, cnt = hn.knn_graph(knbn)
        oi, od = _self_ref(db, np.arange(n), knbn)
        assert np.array_equal(ids, oi) and np.array_equal(dist, od), knbn
        assert (cnt == min(knbn, n - 1)).all()
    ids, dist, cnt = hn.knn_graph(8)
    assert 300 not in ids[300] and dist[300, 0] == 0.0                   # row 300 is a copy of row 5: only the node itself goes
    assert 5 in ids[300] or (dist[300] == 0.0).all()
    # a slice equals the same rows of the whole graph
    for first, nr in [(0, 1), (7, 50), (250, 53), (302, 1), (303, 0)]:
        s = hn.knn_graph(8, 1.0, first, nr)
        for x, y in zip(s, (ids, dist, cnt)):
            assert np.array_equal(x, y[first:first + nr])


def test_caller_ids_and_device_forms(gpu_ctx):
    import gsearch_amd as G
    m = 64
    db = H.synth_sig_db(6, 100, m, 9, jlo=0.5, jhi=0.999)
    n = len(db)
    cid = (10_000_000_000 + 7 * np.random.default_rng(2).permutation(n)).astype(np.uint64)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), seed=5, insert_batch=64)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db, ids=cid)
    ids, dist, cnt = hn.knn_graph(16)
    oi, od = _self_ref(db, np.arange(n), 16)
    assert np.array_equal(ids, cid[oi.astype(np.int64)]) and np.array_equal(dist, od)
    q = H.queries_from(db, 30, 4, frac=0.1)
    ei, ed, ec = hn.exact_search_arrays(q, 16)
    oi, od = O.bruteforce_topk(db, q, 16)
    assert np.array_equal(ei, cid[oi.astype(np.int64)]) and np.array_equal(ed, od)
    ctx = hn.ctx
    nq, k = len(q), 16
    dq, di, dd, dc = ctx.alloc(q.nbytes), ctx.alloc(8 * n * k), ctx.alloc(4 * n * k), ctx.alloc(4 * n)
    try:
        ctx.upload(dq, q)
        hn.exact_search_dev(dq, nq, k, di, dd, dc)
        got = ctx.download(di, (nq, k), np.uint64), ctx.download(dd, (nq, k), np.float32), ctx.download(dc, nq, np.uint32)
        for x, y in zip(got, (ei, ed, ec)):
            assert np.array_equal(x, y)
        hn.knn_graph_dev(k, 10, 200, di, dd, dc)
        got = ctx.download(di, (200, k), np.uint64), ctx.download(dd, (200, k), np.float32), ctx.download(dc, 200, np.uint32)
        for x, y in zip(got, (ids, dist, cnt)):
            assert np.array_equal(x, y[10:210])
    finally:
        for p in (dq, di, dd, dc):
            ctx.free(p)


def test_errors(gpu_ctx):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_STATE, GS_ERR_UNSUPPORTED
    db = H.synth_sig_db(3, 10, 32, 1)
    hn = _index(G, db)
    q = db[:2]

    def code(f, *a):
        with pytest.raises(G.GsError) as e:
            f(*a)
        return e.value.code
    for knbn in (0, 1025):
        assert code(hn.exact_search_arrays, q, knbn) == GS_ERR_INVALID
        assert code(hn.knn_graph, knbn, 1.0, 0, 5) == GS_ERR_INVALID
    for md in (float("nan"), -0.01):
        assert code(hn.exact_search_arrays, q, 5, md) == GS_ERR_INVALID
        assert code(hn.knn_graph, 5, md, 0, 5) == GS_ERR_INVALID
    for first, nr in [(0, 31), (30, 1), (31, 0)]:
        assert code(hn.knn_graph, 5, 1.0, first, nr) == GS_ERR_INVALID
    empty = G.Hnsw.new(8, 1000, 16, 40, G.DistHamming())
    empty._ensure(32)
    assert code(empty.knn_graph, 5, 1.0, 0, 0) == GS_ERR_STATE
    assert code(empty.exact_search_arrays, q, 5) == GS_ERR_STATE
    big = _index(G, np.zeros((4, 70000), np.float32))
    assert code(big.knn_graph, 2) == GS_ERR_UNSUPPORTED
    assert code(big.exact_search_arrays, np.zeros((1, 70000), np.float32), 2) == GS_ERR_UNSUPPORTED
    assert hn.knn_graph(5, 1.0, 30, 0)[0].shape == (0, 5)             # an empty range is no error


def test_knn_graph_at_size(gpu_ctx):
    """>= 100 k nodes: 256 sampled rows of the whole graph against the oracle"""
    import gsearch_amd as G
    m = 4096
    db = H.synth_sig_db(1000, 100, m, 31, dtype=np.uint32, jlo=0.2, jhi=0.999)         # 100 000 nodes
    hn = _index(G, db)
    ids, dist, cnt = hn.knn_graph(32)
    rows = np.sort(np.random.default_rng(6).choice(len(db), 256, replace=False))
    oi, od = _self_ref(db, rows, 32, 16)
    assert np.array_equal(ids[rows], oi) and np.array_equal(dist[rows], od)
    assert (cnt == 32).all()
