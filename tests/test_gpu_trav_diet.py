"""Dense traversal after its instruction diet: the paths a phase-1 pop can take, each against the CPU oracle - ids, distances, neighbour counts AND
evaluation counts, bit for bit. Small databases, built once per module and shared by the cases."""
import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

VIS = ["lds", "global", "split"]


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


@pytest.fixture(scope="module")
def noise(gpu_ctx):
    """3 000 noise rows over five values, m = 96 (every pair agrees in 19 +- 4 slots: dense count levels), M = 10, efc = 40; the oracle's answers are
    computed once per (knbn, ef) and shared by the three placements of the visited bitmap"""
    import os
    old = os.environ.get("GS_DIST_MODE")
    os.environ["GS_DIST_MODE"] = "dense"
    try:
        m = 96
        db = np.random.default_rng(502).integers(0, 5, (3000, m)).astype(np.float32)
        oix, hn = _pair(db, 10, 40, 31, 128, m)
    finally:
        if old is None:
            os.environ.pop("GS_DIST_MODE", None)
        else:
            os.environ["GS_DIST_MODE"] = old
    q = np.concatenate([np.random.default_rng(503).integers(0, 5, (40, m)).astype(np.float32), db[7:11]])
    return {"oix": oix, "hn": hn, "q": q, "want": {}}


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("ef", [40, 64, 65, 300, 1500, 3001])
def test_dense_tie_levels_sweep(noise, monkeypatch, vis, ef):
    """ef in {40, 64, 65, 300, 1500, 3001} x knbn in {1, 10, 40} under the three placements of the visited bitmap: R fills in the middle of an expansion
    (nR + ne > efs), more candidates below dmax than keys tied at it (B > tieT: the rank path), the fast trim and the histogram walk, T merges, and
    n < ef (3001 > 3000 nodes: R never fills, tau is never reached)"""
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    for knbn in (1, 10, 40):
        assert ef >= knbn
        if (knbn, ef) not in noise["want"]:
            noise["want"][(knbn, ef)] = noise["oix"].parallel_search(noise["q"], knbn, ef)
        want = noise["want"][(knbn, ef)]
        _same(noise["hn"].search_arrays(noise["q"], knbn, ef), want)
        assert want[3].mean() > min(2500, 15 * ef)                    # the searches really walk the graph


@pytest.fixture(scope="module")
def ties(gpu_ctx):
    """150 unrelated families of 8, m = 200: nearly everything ties at distance 1"""
    import os
    old = os.environ.get("GS_DIST_MODE")
    os.environ["GS_DIST_MODE"] = "dense"
    try:
        m = 200
        db = H.synth_sig_db(150, 8, m, 77, jlo=0.0, jhi=0.6)
        oix, hn = _pair(db, 8, 64, 9, 64, m)
    finally:
        if old is None:
            os.environ.pop("GS_DIST_MODE", None)
        else:
            os.environ["GS_DIST_MODE"] = old
    q = np.concatenate([H.queries_from(db, 300, 5, frac=0.25), db[:40]])
    return {"oix": oix, "hn": hn, "q": q, "want": {ef: oix.parallel_search(q, 10, ef) for ef in (400, 40)}}


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("ef", [400, 40])
def test_both_phases_ran(ties, monkeypatch, vis, ef):
    """the tie-heavy data at ef = 400 and ef = 40, with the work counters of the call: pops before dmax reached tau (phase 1, sequential) and after
    (phase 2, order-free) add up to all pops, so neither can have been skipped unseen. On this data the graph is a few hubs (mean layer-0 degree 1.2)
    and a search evaluates 122 to 133 of the 1 200 nodes whatever ef is (the oracle's evaluation counts), so at ef = 400 the result set cannot fill
    and NO implementation reaches phase 2 there: the counters must say so (phase 2 = 0). At ef = 40 every query evaluates at least 77 nodes, R fills,
    dmax = tau = m at once (eight nodes of 1 200 lie below m) with candidates still waiting: both phases must have made pops."""
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    hn, q, want = ties["hn"], ties["q"], ties["want"][ef]
    hn.search_stats(reset=True)
    got = hn.search_arrays(q, 10, ef)
    st = hn.search_stats(reset=True)
    print("ef %d: evaluations per query %d..%d, pops phase 1 %d, phase 2 %d, all %d" % (ef, want[3].min(), want[3].max(), st["pops_phase1"], st["pops_phase2"], st["pops"]))
    _same(got, want)
    assert st["pops_phase1"] + st["pops_phase2"] == st["pops"], st
    assert st["pops_phase1"] > 0, st
    if want[3].max() < ef:                                            # fewer nodes evaluated than R holds: it never fills, tau is never reached
        assert ef == 400 and st["pops_phase2"] == 0, st
    else:
        assert want[3].min() >= ef and st["pops_phase2"] > 0, st
    assert (want[1] == 1.0).mean() > 0.3                              # the data really is tie-heavy


@pytest.mark.parametrize("vis", VIS)
def test_one_group_form_wide_rows(gpu_ctx, monkeypatch, vis):
    """max_nb_conn = 200 on 1 500 nodes: rows of up to 400 ids, expanded by one 512-lane group (ONEG), which keeps the word-by-word wave sums"""
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")
    m, M = 64, 200
    db = H.synth_sig_db(125, 12, m, 177, jlo=0.0, jhi=0.6)
    oix, hn = _pair(db, M, 2 * M + 90, 19, 64, m)                     # (extend_candidates needs efc > 2M on the device)
    assert np.array_equal(hn.export_graph()["deg0"], oix.export()["deg0"])
    q = np.concatenate([H.queries_from(db, 100, 5, frac=0.25), db[:20]])
    for knbn, ef in ((10, 600), (7, 7)):
        _same(hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef))


def _same_graph(hn, oix, n):
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"]) and np.array_equal(g["levels"], og["levels"])
    for i in range(n):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]), i


@pytest.mark.parametrize("n,cut", [(2000, 1200), (5200, 4300)])
def test_insert_in_two_calls_builds_the_oracle_graph(gpu_ctx, monkeypatch, n, cut):
    """a build in two parallel_insert calls, dense mode: the exported graph is the oracle's. 2 000 nodes; and 5 200 with the second call starting past
    4 096 nodes, where an insert batch takes its layer-0 searches through the traversal kernel's accepted-key log (WLOG) - below that size the
    pre-pass is not taken, so the small build alone would not run that form"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    m, M, efc, B = 64, 8, 40, 256
    db = H.synth_sig_db(n // 40, 40, m, 321, jlo=0.05, jhi=0.9)
    oix = O.Index(np.float32, m, M, efc, scale_modify=0.5, seed=4)
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=4, insert_batch=B)
    hn.modify_level_scale(0.5); hn.set_extend_candidates(True)
    for part in (db[:cut], db[cut:]):
        oix.parallel_insert(part, batch=B); hn.parallel_insert(part)
    _same_graph(hn, oix, len(db))
