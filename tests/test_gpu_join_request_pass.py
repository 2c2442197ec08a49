"""A request of several match-join batches in one call (gs_join.hip): the prologue of all batches is queued together, the host waits
once, the batches that end in the plain main pass share one k_match_join launch (the batch as the slowest grid dimension) and a batch that clusters
follows on its own. Whatever way a batch went, every count must equal anndists' DistHamming (the oracle) for every (query, node) pair, and
GS_JOIN_MERGE=0 (batch by batch, the path the fused sketch-and-search keeps) must give the same matrix.

Shapes: m = 800 / 802 (slot blocks end ragged; phase 0 and the main pass both run: m > 48), 8400 nodes (two node chunks of 8192, the second nearly
empty), batches forced with GS_JOIN_MAXQ."""
import os

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

N_ROOTS, PER = 12, 700          # 8400 nodes


def _rnd(rng, shape, dtype, universe):
    v = rng.integers(0, universe, shape)
    return v.astype(np.float32) if np.dtype(dtype) == np.float32 else v.astype(dtype)


def _family_db(rng, m, dtype, universe):
    roots = _rnd(rng, (N_ROOTS, m), dtype, universe)
    db = np.repeat(roots, PER, axis=0)
    mk = rng.random(db.shape) > rng.uniform(0.25, 0.95, (len(db), 1))
    db[mk] = _rnd(rng, db.shape, dtype, universe)[mk]
    return np.ascontiguousarray(db[rng.permutation(len(db))]), roots


def _isolates(rng, roots, fam, dtype, universe):
    q = roots[fam].copy()
    mk = rng.random(q.shape) > rng.uniform(0.2, 0.98, (len(q), 1))
    q[mk] = _rnd(rng, q.shape, dtype, universe)[mk]
    return q


def _isolated_graph(n, M):
    return dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32), cnt0=np.zeros((n, 2 * M), np.uint32),
                upidx=np.full(n, -1, np.int32), n_upper=0)


def _oracle_counts(q, db, m):
    d = O.hamming_qxc(q, db, nthreads=os.cpu_count())
    return np.rint(d.astype(np.float64) * m).astype(np.uint16)


_CASES = {}


def _case(dtype, m, universe):
    """database, 641 queries (isolates of five families, twins of nodes, unrelated rows, in random order) and the oracle's matrix: built once per shape"""
    key = (np.dtype(dtype).name, m, universe)
    if key not in _CASES:
        rng = np.random.default_rng(m * 7 + universe % 89)
        db, roots = _family_db(rng, m, dtype, universe)
        q = np.concatenate([_isolates(rng, roots, rng.integers(0, 5, 520), dtype, universe), db[[5, 5, 77, 77]], _rnd(rng, (90, m), dtype, universe),
                            db[rng.integers(0, len(db), 27)]])
        assert len(q) == 641
        if np.dtype(dtype) == np.float32:
            q[3, :40] = np.nan; q[4, 40:60] = -0.0; db[9, 40:60] = 0.0; db[10, :8] = np.nan
        q = np.ascontiguousarray(q[rng.permutation(len(q))])
        want = _oracle_counts(q, db, m)
        want.setflags(write=False)
        _CASES[key] = (db, q, want)
    return _CASES[key]


def _index(db, dtype):
    import gsearch_amd as G
    hn = G.Hnsw.new(8, len(db), 16, 16, G.DistHamming(), dtype=dtype, seed=1)
    hn.import_graph(db, _isolated_graph(len(db), 8))
    return hn


def _mismatch(got, want):
    bad = np.argwhere(got != want)
    return None if len(bad) == 0 else (len(bad), bad[:5].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def _batch_lines(err):
    return [l for l in err.splitlines() if l.startswith("[GS_JOIN] nq=") and " clusters," in l]


SHAPES = [(np.float32, 800, 1600), (np.uint32, 802, 1 << 30), (np.uint64, 800, 1500)]
# (queries, environment, batch sizes the verbose lines must show)
SPLITS = [(640, {"GS_JOIN_MAXQ": "400"}, [320, 320]),                                   # equal batches, the default cluster rule (>= 256 queries, >= 8192 nodes)
          (640, {"GS_JOIN_MAXQ": "256", "GS_JOIN_CLUSTER": "2"}, [214, 214, 212]),      # a shorter last batch
          (640, {}, [640]),                                                             # one batch
          (641, {"GS_JOIN_MAXQ": "400"}, [321, 320])]


@pytest.mark.parametrize("dtype,m,universe", SHAPES)
@pytest.mark.parametrize("nq,env,sizes", SPLITS)
def test_count_matrix_of_a_request_in_batches(gpu_ctx, monkeypatch, capfd, dtype, m, universe, nq, env, sizes):
    db, q, want = _case(dtype, m, universe)
    hn = _index(db, dtype)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GS_JOIN_VERBOSE", "1")
    capfd.readouterr()
    got = hn.count_matrix(q[:nq])
    lines = _batch_lines(capfd.readouterr().err)
    assert [int(l.split("nq=")[1].split()[0]) for l in lines] == sizes, lines       # one line per batch, in order
    assert _mismatch(got, want[:nq]) is None, _mismatch(got, want[:nq])
    monkeypatch.setenv("GS_JOIN_MERGE", "0")                                           # batch by batch: the same matrix
    got0 = hn.count_matrix(q[:nq])
    assert _mismatch(got0, want[:nq]) is None, _mismatch(got0, want[:nq])
    hn.close()


@pytest.mark.parametrize("dtype,m,universe", [(np.float32, 800, 1 << 22), (np.uint32, 802, 1 << 30)])
def test_one_batch_clusters_and_one_takes_the_plain_pass(gpu_ctx, monkeypatch, capfd, dtype, m, universe):
    """batch 0: isolates of three families; batch 1: unrelated rows (not permuted across the boundary). One call: batch 1 is joined by the merged launch, batch 0
    by the cluster-aware kernel and the block compare after it."""
    rng = np.random.default_rng(m + 5)
    db, roots = _family_db(rng, m, dtype, universe)
    q0 = _isolates(rng, roots, rng.integers(0, 3, 320), dtype, universe)
    q1 = _rnd(rng, (320, m), dtype, universe)
    q = np.ascontiguousarray(np.concatenate([q0[rng.permutation(320)], q1]))
    want = _oracle_counts(q, db, m)
    hn = _index(db, dtype)
    monkeypatch.setenv("GS_JOIN_MAXQ", "400")
    monkeypatch.setenv("GS_JOIN_VERBOSE", "1")
    capfd.readouterr()
    got = hn.count_matrix(q)
    lines = _batch_lines(capfd.readouterr().err)
    assert len(lines) == 2, lines
    assert " 0 clusters" not in lines[0] and "not worth" not in lines[0], lines
    assert " 0 clusters" in lines[1], lines
    assert _mismatch(got, want) is None, _mismatch(got, want)
    for env in ({"GS_JOIN_MERGE": "0"}, {"GS_JOIN_CLUSTER": "0"}, {"GS_DENSE_IMPL": "tile"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g2 = hn.count_matrix(q)
        assert _mismatch(g2, want) is None, (env, _mismatch(g2, want))
        for k in env:
            monkeypatch.delenv(k)
    hn.close()


def test_regions_sized_by_batches_are_reused(gpu_ctx, monkeypatch):
    """two calls in a row on one index: 640 queries in three batches, then 300 in two - the lists, labels and staging sized x batches serve both"""
    db, q, want = _case(np.float32, 800, 1600)
    hn = _index(db, np.float32)
    monkeypatch.setenv("GS_JOIN_MAXQ", "256")
    monkeypatch.setenv("GS_JOIN_CLUSTER", "2")
    for nq in (640, 300, 640):
        got = hn.count_matrix(q[:nq])
        assert _mismatch(got, want[:nq]) is None, (nq, _mismatch(got, want[:nq]))
    hn.close()


@pytest.mark.parametrize("merge", ["1", "0"])
def test_pair_list_overflow_repeats_the_scan_of_that_batch(gpu_ctx, monkeypatch, capfd, merge):
    """GS_JOIN_PAIR_CAP=64: every batch's list of heavy pairs overflows, is sized to the exact count and its scan and labels repeated - the families are still found"""
    db, q, want = _case(np.float32, 800, 1600)
    hn = _index(db, np.float32)
    monkeypatch.setenv("GS_JOIN_MAXQ", "400")
    monkeypatch.setenv("GS_JOIN_PAIR_CAP", "64")
    monkeypatch.setenv("GS_JOIN_MERGE", merge)
    monkeypatch.setenv("GS_JOIN_VERBOSE", "1")
    capfd.readouterr()
    got = hn.count_matrix(q[:640])
    lines = _batch_lines(capfd.readouterr().err)
    assert len(lines) == 2 and all(" 0 clusters" not in l for l in lines), lines
    assert all(int(l.split("heavy pairs ")[1].split()[0]) > 64 for l in lines), lines
    assert _mismatch(got, want[:640]) is None, _mismatch(got, want[:640])
    hn.close()


@pytest.mark.parametrize("cluster", ["2", "0"])
def test_search_of_a_request_in_small_batches_matches_oracle(gpu_ctx, monkeypatch, cluster):
    """the whole dense search on a built graph with the count matrix produced in batches of 64 queries (300 queries: five batches in one call): ids, distances,
    counts and evaluation counts == oracle.parallel_search"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_JOIN_CLUSTER", cluster)
    m = 256
    db = H.synth_sig_db(4, 500, m, 23, jlo=0.3, jhi=0.97)               # 2000 nodes, four families
    oix = O.Index(np.float32, m, 8, 40, seed=12)
    oix.parallel_insert(db, batch=200)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), seed=12, insert_batch=200)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    monkeypatch.setenv("GS_JOIN_MAXQ", "64")                            # (after the build: an insert batch of 200 rows is one join call)
    rng = np.random.default_rng(4)
    base = db[rng.integers(0, 40, 300)].copy()                          # 300 queries drawn from 40 nodes: twins and siblings
    mk = rng.random(base.shape) < 0.15
    base[mk] = rng.random(base.shape, dtype=np.float32)[mk]
    got, want = hn.search_arrays(base, 10, 80), oix.parallel_search(base, 10, 80, nthreads=os.cpu_count())
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    hn.close()
