"""Dense traversal with the bookkeeping of a phase-1 pop taken off the waves that do not need it: the waves of the hint half publish no counts and the
sums read the four words of the half that expanded, the wave's number and its half are scalars, the row test is made from the lane number. What changed is
what the waves hand one another through LDS, so the cases are those where a stale or mis-buffered hand-over shows: many queries per persistent workgroup on two
grids, every steering branch with the queries given in two calls of odd sizes, the ONEG / WLOG / SPLIT instantiations, and poisoned scratch. Everything
against the CPU oracle: ids, distances, neighbour counts and evaluation counts with ==."""
import os

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

VIS = ["lds", "global", "split"]
COUNTERS = ("pops", "accepting_pops", "pops_phase1", "pops_phase2")


def _pair(db, M, efc, seed, batch, m):
    """the same database in the oracle and on the device (both build the graph themselves)"""
    import gsearch_amd as G
    oix = O.Index(np.float32, m, M, efc, seed=seed)
    oix.parallel_insert(db, batch=batch)
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=seed, insert_batch=batch)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    return oix, hn


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])       # ids, distances
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])       # neighbour counts, evaluation counts


def _dense_env():
    old = os.environ.get("GS_DIST_MODE")
    os.environ["GS_DIST_MODE"] = "dense"
    return old


def _env_back(old):
    if old is None:
        os.environ.pop("GS_DIST_MODE", None)
    else:
        os.environ["GS_DIST_MODE"] = old


@pytest.fixture(scope="module")
def noise(gpu_ctx):
    """3 000 noise rows over five values, m = 96, M = 10, efc = 40 (the database of test_gpu_trav_diet.py, rebuilt). `many`: 1 600 queries, random rows
    (long searches) alternating with rows of the database itself (short ones); `few`: 40 random rows and four of the database's. The oracle's answers
    are computed once per (query set, knbn, ef) and shared by the cases."""
    old = _dense_env()
    try:
        m = 96
        db = np.random.default_rng(502).integers(0, 5, (3000, m)).astype(np.float32)
        oix, hn = _pair(db, 10, 40, 31, 128, m)
    finally:
        _env_back(old)
    many = np.empty((1600, m), dtype=np.float32)
    many[0::2] = np.random.default_rng(611).integers(0, 5, (800, m)).astype(np.float32)
    many[1::2] = db[np.random.default_rng(612).permutation(3000)[:800]]
    few = np.concatenate([np.random.default_rng(503).integers(0, 5, (40, m)).astype(np.float32), db[7:11]])
    return {"oix": oix, "hn": hn, "many": many, "few": few, "want": {}}


def _want(noise, which, knbn, ef):
    key = (which, knbn, ef)
    if key not in noise["want"]:
        noise["want"][key] = noise["oix"].parallel_search(noise[which], knbn, ef)
    return noise["want"][key]


def _many_on_two_grids(noise, monkeypatch, vis, ef, poke=None):
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    hn, q = noise["hn"], noise["many"]
    want = _want(noise, "many", 10, ef)
    stats = []
    for per_cu in (None, "1"):
        if per_cu is None:
            monkeypatch.delenv("GS_DENSE_PER_CU", raising=False)
        else:
            monkeypatch.setenv("GS_DENSE_PER_CU", per_cu)
        hn.search_stats(reset=True)
        if poke:
            poke(hn)
        got = hn.search_arrays(q, 10, ef)
        st = hn.search_stats(reset=True)
        print("vis %s ef %d per_cu %s: %s" % (vis, ef, per_cu, {k: st[k] for k in COUNTERS + ("wg_in_flight",)}))
        _same(got, want)
        assert 0 < st["wg_in_flight"] < len(q), st                   # a workgroup takes several queries, one after the other
        assert st["pops_phase1"] + st["pops_phase2"] == st["pops"], st
        assert st["pops_phase1"] > 0 and st["accepting_pops"] > 0, st
        stats.append(st)
    # the counters are properties of the algorithm, not of the launch
    for k in COUNTERS:
        assert stats[0][k] == stats[1][k], (k, stats)


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("ef", [64, 300])
def test_many_queries_per_workgroup(noise, monkeypatch, vis, ef):
    """1 600 queries, more than a launch has workgroups, long and short searches alternating, on the default grid and on one workgroup per CU: what a
    workgroup leaves behind in LDS after one query (the wave words of the half that did not expand, the front's published keys, T) is what its next query
    finds. Answers are the oracle's on both grids, and the work counters of the two launches are equal."""
    _many_on_two_grids(noise, monkeypatch, vis, ef)


@pytest.fixture
def fill_guard():
    """no other test ever runs in fill mode"""
    import gsearch_amd as G
    try:
        yield
    finally:
        G.debug_mem_fill(None)


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("ef", [64, 300])
def test_many_queries_poisoned_scratch(noise, monkeypatch, fill_guard, vis, ef):
    """the same once more with every buffer the library hands out, and the per-call scratch of the index, filled with 0xFF first: nothing of what the
    waves hand one another may be read before it is written"""
    import gsearch_amd as G
    G.debug_mem_fill(0xFF)
    _many_on_two_grids(noise, monkeypatch, vis, ef, poke=lambda hn: hn.debug_fill_scratch(0xFF))


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("ef", [40, 64, 65, 300, 1500, 3001])
def test_steering_branches_in_two_calls(noise, monkeypatch, vis, ef):
    """ef in {40, 64, 65, 300, 1500, 3001} x knbn in {1, 10, 40}: R filling in the middle of an expansion, B > tieT (rank path), the fast trim followed
    by the histogram walk, T merges, n < ef. The 44 queries are given in two calls, 7 then 37: the pop counter starts at 0
    for every query, so what the split changes is which workgroup takes which query and what its LDS holds from the query before"""
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    hn, q = noise["hn"], noise["few"]
    for knbn in (1, 10, 40):
        want = _want(noise, "few", knbn, ef)
        a, b = hn.search_arrays(q[:7], knbn, ef), hn.search_arrays(q[7:], knbn, ef)
        _same([np.concatenate([x, y]) for x, y in zip(a, b)], want)
        assert want[3].mean() > min(2500, 15 * ef)                    # the searches really walk the graph


@pytest.fixture(scope="module")
def ties(gpu_ctx):
    """150 unrelated families of 8, m = 200: nearly everything ties at distance 1 (the second database of test_gpu_trav_diet.py, rebuilt)"""
    old = _dense_env()
    try:
        m = 200
        db = H.synth_sig_db(150, 8, m, 77, jlo=0.0, jhi=0.6)
        oix, hn = _pair(db, 8, 64, 9, 64, m)
    finally:
        _env_back(old)
    q = np.concatenate([H.queries_from(db, 300, 5, frac=0.25), db[:40]])
    return {"oix": oix, "hn": hn, "q": q, "want": {ef: oix.parallel_search(q, 10, ef) for ef in (400, 40)}}


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("ef", [400, 40])
def test_ties_in_two_calls(ties, monkeypatch, vis, ef):
    """the tie-heavy data (T's last key ties with most accepted keys, so the T test sits on its edge), in two calls of 7 and 333 queries,
    with the phase counters adding up"""
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    hn, q, want = ties["hn"], ties["q"], ties["want"][ef]
    hn.search_stats(reset=True)
    a, b = hn.search_arrays(q[:7], 10, ef), hn.search_arrays(q[7:], 10, ef)
    st = hn.search_stats(reset=True)
    _same([np.concatenate([x, y]) for x, y in zip(a, b)], want)
    assert st["pops_phase1"] + st["pops_phase2"] == st["pops"] and st["pops_phase1"] > 0, st


@pytest.mark.parametrize("vis", VIS)
def test_one_group_form_wide_rows(gpu_ctx, monkeypatch, vis):
    """ONEG (max_nb_conn = 200 on 1 500 nodes: rows of up to 400 ids, one 512-lane group): it keeps the eight wave words, and takes the scalar wave
    number and the row test made from the lane number like the other forms. Graph and answers are the oracle's; the
    queries go in two calls"""
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    m, M = 64, 200
    db = H.synth_sig_db(125, 12, m, 177, jlo=0.0, jhi=0.6)
    oix, hn = _pair(db, M, 2 * M + 90, 19, 64, m)                     # (extend_candidates needs efc > 2M on the device)
    assert np.array_equal(hn.export_graph()["deg0"], oix.export()["deg0"])
    q = np.concatenate([H.queries_from(db, 100, 5, frac=0.25), db[:20]])
    for knbn, ef in ((10, 600), (7, 7), (1, 40)):
        a, b = hn.search_arrays(q[:7], knbn, ef), hn.search_arrays(q[7:], knbn, ef)
        _same([np.concatenate([x, y]) for x, y in zip(a, b)], oix.parallel_search(q, knbn, ef))


@pytest.mark.parametrize("vis", ["lds", "split"])
def test_prepass_build_in_two_calls(gpu_ctx, monkeypatch, vis):
    """WLOG (and WLOG + SPLIT): 5 200 nodes built in two calls, the second from 4 300, where an insert batch takes its layer-0 searches through the
    traversal kernel's accepted-key log (the pre-pass wants 4 096 nodes). The exported graph is the oracle's, and so are the answers of a search on it"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    n, cut, m, M, efc, B = 5200, 4300, 64, 8, 40, 256
    db = H.synth_sig_db(n // 40, 40, m, 321, jlo=0.05, jhi=0.9)
    oix = O.Index(np.float32, m, M, efc, scale_modify=0.5, seed=4)
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=4, insert_batch=B)
    hn.modify_level_scale(0.5); hn.set_extend_candidates(True)
    for part in (db[:cut], db[cut:]):
        oix.parallel_insert(part, batch=B); hn.parallel_insert(part)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"]) and np.array_equal(g["levels"], og["levels"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]), i
    q = np.concatenate([H.queries_from(db, 60, 5, frac=0.25), db[:20]])
    for knbn, ef in ((10, 64), (1, 300)):
        _same(hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef))
