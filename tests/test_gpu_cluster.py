"""hnswcore on the device (SPEC.md 10): gs_index_nearest_of against the argmin of the count matrix, gs_index_cluster against the numpy restatement
tests/pyref_cluster.py bit for bit (every output array, every info field), the multi-block paths against the single-block run, every error code that
a small index can reach, and hnswcore() end to end through an hnsw_rs dump."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import pyref_cluster as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.uint32, np.uint64, np.uint16]


def _index(G, db, M=8):
    """an index over db without an HNSW build: an empty layer-0 graph is imported (the clustering never reads the graph)"""
    n = len(db)
    hn = G.Hnsw.new(M, max(n, 1024), 16, 40, G.DistHamming(), dtype=db.dtype)
    hn.import_graph(db, dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32),
                             cnt0=np.zeros((n, 2 * M), np.uint32), upidx=np.full(n, -1, np.int32), n_upper=0))
    return hn


def _as(db, dtype):
    """the generators' uint32 rows in another element type (equal values stay equal, the mismatch counts of the converted rows are what both sides see)"""
    if np.dtype(dtype) == np.uint16:
        return np.ascontiguousarray((db & 0xFFFF).astype(np.uint16))
    return np.ascontiguousarray(db.astype(dtype))


# name -> (db, n_cluster, fraction, max_iter, seed)
@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "planted":
        return R.planted(0)[0], 8, 0.1, 15, 0
    if name == "chain":                                      # 5 iterations (test_cluster_cpu.py)
        return R.chain(0), 5, 0.25, 15, 0
    if name == "chain_max_iter_1":                           # stopped while medoids still move: converged = 0
        return R.chain(0), 5, 0.25, 1, 0
    if name == "chain_f32_k3":
        return _as(R.chain(3), np.float32), 3, 0.25, 15, 3
    if name == "triples":                                    # every signature three times: count-0 ties between coreset points, weights of 0
        db = R.planted(2, families=6, size=10)[0]
        db = np.concatenate([db, db, db])
        return np.ascontiguousarray(db[np.random.default_rng(5).permutation(len(db))]), 4, 0.3, 15, 7
    if name == "k1_u16":
        return _as(R.planted(1, families=3, size=30)[0], np.uint16), 1, 0.1, 15, 1
    if name == "k_equals_n":
        return R.chain(1, n=9), 9, 1.0, 15, 2
    if name == "coreset_only":
        return R.chain(2), 0, 0.25, 15, 4
    if name == "coreset_only_u64":
        return _as(R.planted(3)[0], np.uint64), 0, 0.1, 15, 5
    if name == "three_blocks":                               # a coreset of about 250 rows
        return R.chain(4, n=1000), 6, 0.25, 15, 11
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    db, k, f, it, seed = _case(name)
    return R.cluster(db, k, f, it, seed)


def _same(got, ref, ids=None):
    assert got.n_core == ref["n_core"]
    assert np.array_equal(got.core_nodes, ref["core_nodes"]) and np.array_equal(got.core_weight, ref["core_weight"])
    assert np.array_equal(got.centre_node, ref["centre_node"]) and np.array_equal(got.centre_count, ref["centre_count"])
    assert np.array_equal(got.medoids, ref["medoids"]) and np.array_equal(got.sizes, ref["sizes"])
    assert (got.iterations, got.converged, got.cost_core, got.cost_all) == (ref["iterations"], ref["converged"], ref["cost_core"], ref["cost_all"])
    if ids is None:
        ids = np.arange(len(got.centre_node), dtype=np.uint64)
    assert np.array_equal(got.centre_id, ids[ref["centre_node"].astype(np.int64)])
    assert np.array_equal(got.medoid_ids, ids[ref["medoids"].astype(np.int64)])


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_nearest_of_equals_the_count_matrix_argmin(gpu_ctx, dtype, n):
    """n = 257 is no multiple of the 8 columns a lane owns; duplicated candidate rows (other nodes with the same signature, and the same node
    listed twice) make position the tie-break"""
    import gsearch_amd as G
    db = H.synth_sig_db(25, 40, 96, 17 + n, dtype=dtype, jlo=0.5, jhi=0.999)[:n].copy()
    db[[3, 200, 201]] = db[[150, 150, 7]]                    # nodes 3, 150, 200 hold one signature; so do 7 and 201
    db = np.ascontiguousarray(db)
    hn = _index(G, db)
    rng = np.random.default_rng(n)
    for nc in (1, 7, 130):
        cand = rng.choice(n, nc, replace=False).astype(np.uint64)
        if nc >= 7:
            cand[:6] = [200, 3, 150, 201, 7, 200]
        cm = hn.count_matrix(db[cand.astype(np.int64)])
        want = cm.argmin(axis=0)                             # (the first minimum: the smallest position)
        arg, cnt = hn.nearest_of(cand)
        assert arg.dtype == np.uint32 and cnt.dtype == np.uint16
        assert np.array_equal(arg, want) and np.array_equal(cnt, cm[want, np.arange(n)]), nc
        if nc >= 7:
            assert arg[150] == 0 and arg[7] == 3 and cnt[150] == 0


@pytest.mark.parametrize("name", ["planted", "chain", "chain_max_iter_1", "chain_f32_k3", "triples", "k1_u16", "k_equals_n", "coreset_only",
                                  "coreset_only_u64"])
def test_cluster_equals_the_restatement(gpu_ctx, name):
    import gsearch_amd as G
    db, k, f, it, seed = _case(name)
    ref = _ref(name)
    print("%s: n %d p %d iterations %d converged %d cost_core %d cost_all %d" % (name, len(db), ref["n_core"], ref["iterations"], ref["converged"],
                                                                               ref["cost_core"], ref["cost_all"]))
    hn = _index(G, db)
    got = hn.cluster(k, f, it, seed, return_coreset=True)
    _same(got, ref)
    if name == "chain":
        assert ref["iterations"] >= 3
    if name == "chain_max_iter_1":
        assert got.converged == 0 and got.iterations == 1
    if name == "triples":
        assert (ref["core_weight"] == 0).any()
    if name == "k_equals_n":
        assert np.array_equal(got.medoids, np.arange(9, dtype=np.uint64)) and (got.sizes == 1).all() and got.cost_all == 0
    # without the coreset outputs the answer is the same
    plain = hn.cluster(k, f, it, seed)
    assert plain.core_nodes is None and np.array_equal(plain.centre_node, got.centre_node) and plain.n_core == got.n_core


def test_caller_ids(gpu_ctx):
    """centres come back as node numbers and as the caller's ids; the arithmetic sees node numbers only"""
    import gsearch_amd as G
    db, k, f, it, seed = _case("planted")
    hn = _index(G, db)
    ids = (7_000_000_000 + 3 * np.random.default_rng(1).permutation(len(db))).astype(np.uint64)
    hn.set_ids(ids)
    _same(hn.cluster(k, f, it, seed, return_coreset=True), _ref("planted"), ids)


def test_blocks_give_the_single_block_answers(gpu_ctx, monkeypatch):
    """GS_JOIN_MAXQ = 96: the coreset's rows go through the producer in three blocks (running column minima merged across blocks, P gathered
    block by block), 130 candidates of nearest_of in two"""
    import gsearch_amd as G
    db, k, f, it, seed = _case("three_blocks")
    ref = _ref("three_blocks")
    assert 2 * 96 < ref["n_core"] <= 3 * 96
    hn = _index(G, db)
    cand = np.random.default_rng(3).choice(len(db), 130, replace=False).astype(np.uint64)
    one = hn.cluster(k, f, it, seed, return_coreset=True)
    near = hn.nearest_of(cand)
    monkeypatch.setenv("GS_JOIN_MAXQ", "96")                 # (read at every call)
    three = hn.cluster(k, f, it, seed, return_coreset=True)
    near2 = hn.nearest_of(cand)
    _same(one, ref)
    _same(three, ref)
    assert np.array_equal(near[0], near2[0]) and np.array_equal(near[1], near2[1])
    want = R.nearest_of(db, cand)
    assert np.array_equal(near[0], want[0]) and np.array_equal(near[1], want[1])


def test_errors(gpu_ctx):
    import gsearch_amd as G
    from gsearch_amd import _lib
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_STATE, GS_ERR_UNSUPPORTED
    db = R.planted(0, families=3, size=10)[0]
    n = len(db)
    hn = _index(G, db)

    def code(f, *a, **kw):
        with pytest.raises(G.GsError) as e:
            f(*a, **kw)
        return e.value.code
    assert code(hn.cluster, n + 1) == GS_ERR_INVALID
    for f in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        assert code(hn.cluster, 2, f) == GS_ERR_INVALID
    assert code(hn.cluster, 2, 0.5, 0) == GS_ERR_INVALID
    assert hn.cluster(n, 1.0).n_core == n                                # k = n is served
    assert code(hn.nearest_of, np.zeros(0, np.uint64)) == GS_ERR_INVALID
    assert code(hn.nearest_of, np.array([0, n], np.uint64)) == GS_ERR_INVALID
    empty = G.Hnsw.new(8, 1000, 16, 40, G.DistHamming())
    empty._ensure(32)
    assert code(empty.cluster, 2) == GS_ERR_STATE
    assert code(empty.nearest_of, np.zeros(1, np.uint64)) == GS_ERR_STATE
    big = _index(G, np.zeros((4, 70000), np.float32))
    assert code(big.cluster, 2) == GS_ERR_UNSUPPORTED
    assert code(big.nearest_of, np.zeros(1, np.uint64)) == GS_ERR_UNSUPPORTED
    # a coreset buffer that is too small: GS_ERR_INVALID, and n_core says how much room it takes
    prm = G.load().gs_cluster_params_default()
    prm.n_cluster, prm.fraction, prm.seed = 2, 0.5, 1
    want = R.cluster(db, 2, 0.5, 15, 1)
    assert want["n_core"] > 1
    cen, cnt, med, sizes = np.zeros(n, np.uint64), np.zeros(n, np.uint16), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    core, wgt, info = np.zeros(n, np.uint64), np.zeros(n, np.uint64), _lib.ClusterInfoC()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                         # noqa: E731
    rc = hn.ctx.L.gs_index_cluster(hn.h, C.byref(prm), p(cen), p(cnt), p(med), p(sizes), p(core), p(wgt), 1, C.byref(info))
    assert rc == GS_ERR_INVALID and info.n_core == want["n_core"]
    rc = hn.ctx.L.gs_index_cluster(hn.h, C.byref(prm), p(cen), p(cnt), p(med), p(sizes), p(core), p(wgt), int(info.n_core), C.byref(info))
    assert rc == 0 and np.array_equal(core[:info.n_core], want["core_nodes"]) and np.array_equal(cen, want["centre_node"])
    assert hn.ctx.L.gs_index_cluster(hn.h, C.byref(prm), None, p(cnt), p(med), p(sizes), None, None, 0, C.byref(info)) == GS_ERR_INVALID


@pytest.mark.parametrize("cluster", [4, 0])
def test_hnswcore_end_to_end(gpu_ctx, tmp_path, cluster):
    """dump an index in hnsw_rs' format, run hnswcore() on the files: the CSV is write_cluster_csv of Hnsw.cluster on the original"""
    import gsearch_amd as G
    db = H.synth_sig_db(6, 50, 96, 11, dtype=np.uint32, jlo=0.2, jhi=0.95)
    ids = (5_000_000_000 + 3 * np.random.default_rng(2).permutation(len(db))).astype(np.uint64)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), dtype=np.uint32, seed=3, insert_batch=64)
    hn.modify_level_scale(0.25); hn.set_extend_candidates(True)
    hn.parallel_insert(db, ids=ids)
    hn.file_dump_hnswrs(tmp_path / "hnswdump")
    out = tmp_path / "out"
    out.mkdir()
    path, res = G.hnswcore(tmp_path, "hnswdump", "u32", cluster=cluster, fraction=0.2, out_dir=out, seed=6)
    assert path == str(out / ("clustercoreset.csv" if cluster else "coreset.csv"))
    want = hn.cluster(cluster, 0.2, 15, 6)
    G.write_cluster_csv(tmp_path / "want.csv", hn.get_ids(), want.centre_id)
    text = open(path).read()
    assert text == (tmp_path / "want.csv").read_text() and text.count("\n") == len(db)
    assert np.array_equal(res.centre_node, want.centre_node)
    ref = R.cluster(db, cluster, 0.2, 15, 6)
    assert np.array_equal(want.centre_id, ids[ref["centre_node"].astype(np.int64)])
    with pytest.raises(G.GsError):                           # the dump holds u32
        G.hnswcore(tmp_path, "hnswdump", "f32", cluster=cluster, out_dir=out)
