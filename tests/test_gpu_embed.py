"""ann on the device (SPEC.md 8): calibration, fuzzy union, adjacency, seeded positions, the light (one thread) and heavy (one wavefront) epoch
forms, and the k-NN graph statistics must equal the numpy restatement tests/pyref_embed.py bit for bit. Index forms are checked against the
reference fed with the oracle's exact self graph."""
import numpy as np
import pytest

import helpers as H
import oracle_lib as O
import pyref_embed as R

pytestmark = pytest.mark.gpu

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
DTYPES = [np.float32, np.uint32, np.uint64, np.uint16]


def _params(G, **kw):
    return G.EmbedParams(**kw), R.defaults(**kw)


def _rand_graph(n, knbn, seed, counts=None, dist_pool=None):
    """a valid graph in node numbers: distinct neighbours other than the node, ascending distances"""
    rng = np.random.default_rng(seed)
    ids = np.full((n, knbn), U64MAX)
    dist = np.full((n, knbn), np.inf, np.float32)
    cnt = rng.integers(0, knbn + 1, n).astype(np.uint32) if counts is None else np.asarray(counts, np.uint32)
    for i in range(n):
        c = int(cnt[i])
        nb = rng.choice(n - 1, c, replace=False)
        nb = nb + (nb >= i)
        ids[i, :c] = nb
        d = rng.choice(dist_pool, c) if dist_pool is not None else rng.integers(0, 1 << 12, c) * np.float32(2.0 ** -12)
        dist[i, :c] = np.sort(np.asarray(d, np.float32))
    return ids, dist, cnt


def _index(G, db, M=8):
    n = len(db)
    hn = G.Hnsw.new(M, max(n, 1024), 16, 40, G.DistHamming(), dtype=db.dtype)
    hn.import_graph(db, dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32),
                             cnt0=np.zeros((n, 2 * M), np.uint32), upidx=np.full(n, -1, np.int32), n_upper=0))
    return hn


def _self_graph(db, knbn, max_dist=1.0):
    """the oracle's exact self graph in node numbers, cut at max_dist"""
    n = len(db)
    ids, dist = O.bruteforce_topk(db, db, knbn + 1, 8)
    oi, od = np.full((n, knbn), U64MAX), np.full((n, knbn), np.inf, np.float32)
    for i in range(n):
        keep = ids[i] != np.uint64(i)
        if keep.all():
            keep[-1] = False
        oi[i], od[i] = ids[i][keep], dist[i][keep]
    cnt = (od <= np.float32(max_dist)).sum(axis=1).astype(np.uint32)
    for i in range(n):
        oi[i, cnt[i]:], od[i, cnt[i]:] = U64MAX, np.inf
    return oi, od, cnt


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("knbn", [1, 8, 32])
def test_memberships_equal_reference(gpu_ctx, knbn):
    import gsearch_amd as G
    n = 600
    counts = np.random.default_rng(knbn).integers(0, knbn + 1, n)
    counts[:3] = [0, 1, knbn]
    ids, dist, cnt = _rand_graph(n, knbn, 11 + knbn, counts)
    c = cnt.astype(np.int64)
    # row 3: all-equal distances; row 4: duplicates at 0; row 5: distance 1.0 (the farthest a DistHamming gives); row 6: all zero
    dist[3, :c[3]] = 0.25
    dist[4, :c[4]] = np.sort(np.where(np.arange(c[4]) < 3, 0.0, dist[4, :c[4]])).astype(np.float32)
    dist[5, :c[5]] = np.sort(np.where(np.arange(c[5]) >= c[5] - 2, 1.0, dist[5, :c[5]])).astype(np.float32)
    dist[6, :c[6]] = 0.0
    prm, _ = _params(G, epochs=0)
    _, memb = G.embed_knn_graph(ids, dist, cnt, prm, return_memb=True)
    ref = R.calibrate(dist, cnt)
    assert _same(memb, ref)
    assert (memb[0] == 0).all() and (knbn == 1 or memb[1, 0] == 1.0)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("given", [False, True], ids=["seeded", "given"])
def test_positions_random_graph(gpu_ctx, dim, given):
    import gsearch_amd as G
    n = 2000
    ids, dist, cnt = _rand_graph(n, 8, 3 + dim)
    init = np.random.default_rng(dim).normal(0, 3, (n, dim)).astype(np.float32) if given else None
    prm, p = _params(G, dim=dim, epochs=40, seed=99)
    got = G.embed_knn_graph(ids, dist, cnt, prm, init=init)
    assert _same(got, R.embed(ids, dist, cnt, p, init=init))


def test_positions_star_graph_wave_form(gpu_ctx):
    """a hub of in-degree ~1500 goes through the wavefront form"""
    import gsearch_amd as G
    n = 1600
    ids, dist, cnt = _rand_graph(n, 8, 5, np.full(1600, 8))
    for i in range(1, 1501):
        if 0 not in ids[i, :8]:
            ids[i, 0] = 0
    off, _, _, _ = R.adjacency(ids, cnt, R.calibrate(dist, cnt))
    assert off[1] - off[0] > 1400
    prm, p = _params(G, epochs=25, neg_samples=5)
    assert _same(G.embed_knn_graph(ids, dist, cnt, prm), R.embed(ids, dist, cnt, p))


def test_positions_at_the_light_limit(gpu_ctx):
    """one node with an adjacency of exactly L_H entries (one thread) and one with L_H + 1 (one wavefront)"""
    import gsearch_amd as G
    n, k, LH = 1000, 8, R.LIGHT
    ids, dist, cnt = _rand_graph(n, k, 8, np.full(n, k))
    for i in range(n):                           # clear the two hubs from every row, then add them to exactly LH - 8 (LH - 7) rows
        for t in range(k):
            if ids[i, t] in (0, 1):
                ids[i, t] = next(j for j in range(10, n) if j != i and j not in ids[i])
    rows0 = [i for i in range(10, n) if 0 not in ids[i] and i not in ids[0]][:LH - k]
    rows1 = [i for i in range(10, n) if 1 not in ids[i] and i not in ids[1] and i not in rows0][:LH - k + 1]
    for i in rows0:
        ids[i, 0] = 0
    for i in rows1:
        ids[i, 0] = 1
    assert not R.validate(ids, dist, cnt)
    off, _, _, _ = R.adjacency(ids, cnt, R.calibrate(dist, cnt))
    assert off[1] - off[0] == LH and off[2] - off[1] == LH + 1
    prm, p = _params(G, epochs=30)
    assert _same(G.embed_knn_graph(ids, dist, cnt, prm), R.embed(ids, dist, cnt, p))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_index_embed_equals_reference(gpu_ctx, dtype):
    import gsearch_amd as G
    db = H.synth_sig_db(10, 30, 256, 17, dtype=dtype, jlo=0.4, jhi=0.99)
    hn = _index(G, db)
    prm, p = _params(G, epochs=60)
    oi, od, oc = _self_graph(db, 8)
    assert _same(hn.embed(8, prm), R.embed(oi, od, oc, p))


def test_index_embed_caller_ids_and_cutoff(gpu_ctx):
    import gsearch_amd as G
    m = 128
    db = H.synth_sig_db(8, 40, m, 23, jlo=0.5, jhi=0.999)
    n = len(db)
    cid = (10_000_000_000 + 7 * np.random.default_rng(2).permutation(n)).astype(np.uint64)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), seed=5, insert_batch=64)
    hn.parallel_insert(db, ids=cid)
    prm, p = _params(G, epochs=50)
    oi, od, oc = _self_graph(db, 8)
    assert _same(hn.embed(8, prm), R.embed(oi, od, oc, p))          # rows in node order, whatever the caller's ids
    oi, od, oc = _self_graph(db, 8, 0.5)
    assert (oc < 8).any() and (oc > 0).any()
    assert _same(hn.embed(8, prm, max_dist=0.5), R.embed(oi, od, oc, p))
    st = hn.knn_graph_stats(8, 0.5)
    ref = R.stats(oi, od, oc)
    assert np.array_equal(st["occ"], ref["occ"]) and st["n_empty"] == ref["n_empty"]


def test_device_form_runs_and_seeds(gpu_ctx):
    import gsearch_amd as G
    n, k = 1500, 8
    ids, dist, cnt = _rand_graph(n, k, 41)
    prm, p = _params(G, epochs=30, dim=2)
    a, memb = G.embed_knn_graph(ids, dist, cnt, prm, return_memb=True)
    assert _same(G.embed_knn_graph(ids, dist, cnt, prm), a)                     # two runs are identical
    other = G.embed_knn_graph(ids, dist, cnt, G.EmbedParams(epochs=30, seed=7))
    assert not np.array_equal(other, a)
    ctx = gpu_ctx
    init = np.random.default_rng(1).normal(0, 2, (n, 2)).astype(np.float32)
    bufs = [ctx.alloc(x.nbytes) for x in (ids, dist, cnt, init)]
    dpos, dmemb = ctx.alloc(8 * n), ctx.alloc(4 * n * k)
    try:
        for b, x in zip(bufs, (ids, dist, cnt, init)):
            ctx.upload(b, x)
        G.embed_knn_graph_dev(ctx, n, k, bufs[0], bufs[1], bufs[2], dpos, prm, None, dmemb)
        assert _same(ctx.download(dpos, (n, 2), np.float32), a) and _same(ctx.download(dmemb, (n, k), np.float32), memb)
        G.embed_knn_graph_dev(ctx, n, k, bufs[0], bufs[1], bufs[2], dpos, prm, bufs[3], None)
        assert _same(ctx.download(dpos, (n, 2), np.float32), G.embed_knn_graph(ids, dist, cnt, prm, init=init))
    finally:
        for b in bufs + [dpos, dmemb]:
            ctx.free(b)


def _check_stats(st, ref):
    for key in ("n", "knbn", "n_edges", "n_empty", "max_occ", "hubs"):
        assert st[key] == ref[key], key
    for key in ("occ_mean", "occ_std", "occ_skew"):
        assert np.float64(st[key]).view(np.uint64) == np.float64(ref[key]).view(np.uint64), key        # the order is pinned: bit-exact
    assert np.array_equal(st["occ"], ref["occ"]) and np.array_equal(st["hist"], ref["hist"])
    assert _same(st["q_first"], ref["q_first"]) and _same(st["q_last"], ref["q_last"])


def test_stats_equal_numpy(gpu_ctx):
    import gsearch_amd as G
    ids, dist, cnt = _rand_graph(3000, 16, 77)
    for i in range(1, 200):                        # a hub
        if 0 not in ids[i, :cnt[i]] and cnt[i]:
            ids[i, 0] = 0
    _check_stats(G.knn_graph_stats(ids, dist, cnt), R.stats(ids, dist, cnt))
    db = H.synth_sig_db(12, 25, 200, 3, dtype=np.uint32)
    hn = _index(G, db)
    _check_stats(hn.knn_graph_stats(8), R.stats(*_self_graph(db, 8)))
    assert G.ann(hn, stats=True, embed=False)["stats"]["n"] == len(db)


def test_validation_errors(gpu_ctx):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_STATE, GS_ERR_UNSUPPORTED
    ids, dist, cnt = _rand_graph(50, 4, 1, np.full(50, 4))

    def code(f, *a, **kw):
        with pytest.raises(G.GsError) as e:
            f(*a, **kw)
        return e.value.code

    def broken(mod):
        i, d, c = ids.copy(), dist.copy(), cnt.copy()
        mod(i, d, c)
        return i, d, c
    cases = [lambda i, d, c: i.__setitem__((3, 1), 50),              # id >= n
             lambda i, d, c: i.__setitem__((3, 1), 3),               # own node
             lambda i, d, c: i.__setitem__((3, 1), i[3, 0]),         # repeat
             lambda i, d, c: d.__setitem__((3, 2), np.nan),
             lambda i, d, c: d.__setitem__((3, 0), -0.5),
             lambda i, d, c: d.__setitem__((3, 3), d[3, 2] / 2 if d[3, 2] > 0 else -1.0),   # descending
             lambda i, d, c: c.__setitem__(3, 5)]                    # count > knbn
    for mod in cases:
        g = broken(mod)
        assert code(G.embed_knn_graph, *g, G.EmbedParams(epochs=1)) == GS_ERR_INVALID
        assert code(G.knn_graph_stats, *g) == GS_ERR_INVALID
    for bad in (dict(dim=0), dict(dim=5), dict(neg_samples=0), dict(lr=float("nan"))):
        assert code(G.embed_knn_graph, ids, dist, cnt, G.EmbedParams(**bad)) == GS_ERR_INVALID
    empty = G.Hnsw.new(8, 1000, 16, 40, G.DistHamming())
    empty._ensure(32)
    assert code(empty.embed) == GS_ERR_STATE and code(empty.knn_graph_stats) == GS_ERR_STATE
    big = _index(G, np.zeros((4, 70000), np.float32))
    assert code(big.embed, 2) == GS_ERR_UNSUPPORTED and code(big.knn_graph_stats, 2) == GS_ERR_UNSUPPORTED


def test_index_embed_at_size(gpu_ctx):
    """100 k nodes, E = 50: the whole embedding bit-exact against the reference fed with the device's own exact graph
    (test_gpu_exact_knn checks that graph against the oracle)"""
    import gsearch_amd as G
    db = H.synth_sig_db(1000, 100, 256, 37, dtype=np.uint32, jlo=0.3, jhi=0.999)
    hn = _index(G, db)
    ids, dist, cnt = hn.knn_graph(8)
    prm, p = _params(G, epochs=50)
    got = hn.embed(8, prm)
    assert _same(got, R.embed(ids, dist, cnt, p))
    st = hn.knn_graph_stats(8)
    _check_stats(st, R.stats(ids, dist, cnt))
