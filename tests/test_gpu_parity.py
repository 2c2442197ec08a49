"""GPU parity tests: the HIP path (through the C ABI) must equal the CPU oracle bit for bit."""
import os

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _oracle_sketch(k, m, algo, genomes, data="dna"):
    recs = [r for g in genomes for r in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    if data != "aa":
        seq, rs, rl = O.pack_dna(recs)
    else:
        seq, rs, rl = O.filter_aa(recs)
    return O.sketch_batch(O.params(k, m, algo, data), seq, rs, rl, goff)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("k,m,algo", [(21, 2000, "optdens"), (16, 1024, "optdens"), (14, 512, "optdens"), (32, 777, "optdens"),
                                      (21, 2000, "revoptdens"), (7, 300, "optdens"), (1, 64, "optdens")])
def test_sketch_dna_matches_oracle(gpu_ctx, k, m, algo):
    import gsearch_amd as G
    rng = np.random.default_rng(k * 1000 + m)
    fam = H.family(rng, 50000, [0.001, 0.01, 0.05])
    genomes = [[H.dna_ascii(g)] for g in fam]
    # multi-record genome with N's / lower case / short records (< k) / empty record
    g0 = H.dna_ascii(fam[0])
    genomes.append([g0[:7000] + b"NNNNnnnn" + g0[7000:9000].lower(), b"ACGT", b"", g0[9000:9031], g0[20000:45003]])
    genomes.append([b"ACGTN"])                       # too short for most k: no k-mer at all
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, algo))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, algo, genomes)
    assert got.dtype == ref.dtype
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("k,m,algo", [(12, 512, "optdens"), (14, 2000, "optdens"), (12, 700, "revoptdens"), (14, 1024, "revoptdens"), (21, 1000, "optdens"),
                                      (12, 300, "super2"), (14, 600, "super"), (12, 400, "prob"), (14, 512, "hll")])
def test_sketch_forward_only_kmers_match_oracle(gpu_ctx, k, m, algo):
    """a15: bindash-rs hashes the window as read for k <= 14 (bindash.rs:346-354) - GS_DATA_DNA_FWD. Both closures on the same genomes: each equals
    its oracle, the two differ, and the forward-only sketch of the reverse strand differs from the forward strand's (the canonical one does not).
    Genomes long enough for the filtered emitter (optdens) and with record boundaries / N runs / short records for the bounds-tested words."""
    import gsearch_amd as G
    rng = np.random.default_rng(k * 100 + m)
    big = H.dna_ascii(H.rand_dna(rng, 260_000))
    fam = H.family(rng, 40000, [0.001, 0.02])
    genomes = [[H.dna_ascii(g)] for g in fam] + [[big], [H.revcomp_ascii(big)]]
    g0 = H.dna_ascii(fam[0])
    genomes.append([g0[:7000] + b"NNNNnnnn" + g0[7000:9000].lower(), b"ACGT", b"", g0[9000:9031], g0[20000:35003]])
    genomes.append([b"ACGTN"])
    out = {}
    for data in ("dna_fwd", "dna"):
        sk = G.sketcher_for(G.SeqSketcherParams(k, m, algo, data))
        got = sk.sketch_genomes(genomes)
        ref = _oracle_sketch(k, m, algo, genomes, data)
        assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref)), data
        out[data] = got
    nb = len(fam)
    assert not np.array_equal(_bits(out["dna_fwd"][nb]), _bits(out["dna_fwd"][nb + 1]))      # strand specific
    assert np.array_equal(_bits(out["dna"][nb]), _bits(out["dna"][nb + 1]))                  # strand invariant
    assert not np.array_equal(_bits(out["dna_fwd"][nb]), _bits(out["dna"][nb]))


def test_bindash_closure_by_kmer_size(gpu_ctx):
    """bindash_sketch_params picks the closure bindash.rs:340-400 picks: k <= 14 forward only, k = 16 / 17..32 canonical; dens 0 / 1 = OptDens / RevOptDens"""
    import gsearch_amd as G
    assert G.bindash_sketch_params(12, 1000).c.data_t == 2 and G.bindash_sketch_params(14, 1000, 1).c.data_t == 2
    assert G.bindash_sketch_params(16, 1000).c.data_t == 0 and G.bindash_sketch_params(21, 1000).c.data_t == 0
    assert G.bindash_sketch_params(12, 1000, 1).c.algo == 5 and G.bindash_sketch_params(12, 1000, 0).c.algo == 4
    with pytest.raises(ValueError):
        G.bindash_sketch_params(12, 1000, 2)
    rng = np.random.default_rng(1)
    a = H.rand_dna(rng, 30000)
    genomes = [[H.dna_ascii(a)], [H.dna_ascii(H.mutate(rng, a, 0.02))]]
    p = G.bindash_sketch_params(12, 2000)
    sig = G.sketcher_for(p).sketch_genomes(genomes)
    assert np.array_equal(_bits(sig), _bits(_oracle_sketch(12, 2000, "optdens", genomes, "dna_fwd")))
    d = G.DistHamming().eval_qxc(sig[:1], sig)
    assert d[0, 0] == 0.0 and 0.0 < G.bindash_distance(d[0, 1], 12) < 1.0


@pytest.mark.parametrize("algo,m", [("optdens", 2000), ("revoptdens", 1500), ("super", 2000), ("super2", 1200)])
def test_sketch_early_rejection_is_exact(gpu_ctx, monkeypatch, algo, m):
    """genomes long enough to warm the slot table up (200+ k-mers per slot): the filtered emitter (keys that cannot lower any slot are
    dropped after two of the three SplitMix64 mixes, survivors go through the per-wave queues) must give the oracle's bits, and the
    same bits as the unfiltered kernel (GS_SKETCH_FILTER=0)"""
    import gsearch_amd as G
    rng = np.random.default_rng(77 + m)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (420_000, 300_011, 515_000)]
    genomes.append([H.dna_ascii(H.rand_dna(rng, 200_000)), b"ACGTNNACGT", H.dna_ascii(H.rand_dna(rng, 250_007))])     # record boundaries inside
    sk = G.sketcher_for(G.SeqSketcherParams(21, m, algo))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(21, m, algo, genomes)
    assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref))
    monkeypatch.setenv("GS_SKETCH_FILTER", "0")
    plain = sk.sketch_genomes(genomes)
    assert np.array_equal(_bits(got), _bits(plain))
    monkeypatch.delenv("GS_SKETCH_FILTER")
    # round 5, the speculative bound of the filtered emitter ((m / N)(ln m + c), checked after the walk): c = 7 above; a guess that is far too tight
    # (c = -3: most genomes fail the check and are walked again under the running bound) and no cap at all must give the same bits
    for c in ("-3", "0.5", "0"):
        monkeypatch.setenv("GS_SKETCH_CAP", c)
        assert np.array_equal(_bits(sk.sketch_genomes(genomes)), _bits(ref)), c


@pytest.mark.parametrize("algo", ["optdens", "revoptdens"])
def test_sketch_densification_matches_oracle(gpu_ctx, algo):
    """few k-mers, many bins: exercises the empty-bin densification (cold path at BASELINE sizes)."""
    import gsearch_amd as G
    rng = np.random.default_rng(5)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (40, 300, 1500, 5000)]
    sk = G.sketcher_for(G.SeqSketcherParams(21, 4096, algo))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(21, 4096, algo, genomes)
    assert np.array_equal(_bits(got), _bits(ref))


def test_sketch_aa_optdens_matches_oracle(gpu_ctx):
    import gsearch_amd as G
    rng = np.random.default_rng(8)
    fam = H.family(rng, 30000, [0.01, 0.1], alphabet=20)
    genomes = [[H.aa_ascii(g)] for g in fam]
    genomes.append([H.aa_ascii(fam[0])[:5000] + b"*XBZ" + H.aa_ascii(fam[0])[5000:9000].lower(), b"MK", H.aa_ascii(fam[1])[100:7000]])
    for k, m in ((7, 1000), (5, 512), (12, 256)):
        sk = G.sketcher_for(G.SeqSketcherParams(k, m, "optdens", "aa"))
        got = sk.sketch_genomes(genomes)
        ref = _oracle_sketch(k, m, "optdens", genomes, "aa")
        assert np.array_equal(_bits(got), _bits(ref))


def test_sketch_split_over_workgroups(gpu_ctx):
    """one long genome alone in the batch is split over several workgroups (global atomicMin merge)."""
    import gsearch_amd as G
    rng = np.random.default_rng(9)
    genomes = [[H.dna_ascii(H.rand_dna(rng, 1200000))]]
    sk = G.sketcher_for(G.SeqSketcherParams(21, 12000, "optdens"))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(21, 12000, "optdens", genomes)
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("dtype,m", [(np.float32, 18000), (np.uint64, 2400), (np.uint32, 1001), (np.float32, 37)])
def test_hamming_matches_oracle(gpu_ctx, dtype, m):
    import gsearch_amd as G
    db = H.synth_sig_db(5, 20, m, 1, dtype=dtype)
    q = H.queries_from(db, 70, 2)
    dh = G.DistHamming()
    got = dh.eval_qxc(q, db)
    ref = O.hamming_qxc(q, db)
    assert np.array_equal(got, ref)
    rng = np.random.default_rng(3)
    ia, ib = rng.integers(0, len(q), 200), rng.integers(0, len(db), 200)
    assert np.array_equal(dh.eval_pairs(q, db, ia, ib), O.hamming_pairs(q, db, ia, ib))
    assert dh.eval(q[0], q[0]) == 0.0


def test_hamming_float_semantics(gpu_ctx):
    import gsearch_amd as G
    a = np.array([[0.0, np.nan, 1.0, -0.0]], dtype=np.float32)
    b = np.array([[-0.0, np.nan, 1.0, 0.0]], dtype=np.float32)
    assert G.DistHamming().eval_qxc(a, b)[0, 0] == O.hamming_qxc(a, b)[0, 0] == np.float32(0.25)


@pytest.mark.parametrize("dtype,m,M,efc,ef,knbn,scale", [(np.float32, 256, 8, 32, 48, 10, 1.0), (np.uint64, 120, 16, 64, 200, 50, 1.0),
                                                         (np.float32, 1000, 24, 100, 300, 20, 0.25), (np.uint32, 64, 4, 16, 5, 8, 1.0)])
def test_search_matches_oracle(gpu_ctx, dtype, m, M, efc, ef, knbn, scale):
    """same graph (built by the oracle, imported) -> identical ids, distances, counts and number of DistHamming evaluations"""
    import gsearch_amd as G
    db = H.synth_sig_db(30, 40, m, 4, dtype=dtype, jlo=0.05, jhi=0.95)
    oix = O.Index(dtype, m, M, efc, scale_modify=scale, seed=123)
    oix.parallel_insert(db, batch=1)
    hn = G.Hnsw.new(M, 10000, 16, efc, G.DistHamming(), dtype=dtype)
    hn.import_graph(db, oix.export())
    q = H.queries_from(db, 64, 6, frac=0.3)
    ids, dist, cnt, ev = hn.search_arrays(q, knbn, ef)
    oids, odist, ocnt, oev = oix.parallel_search(q, knbn, ef)
    assert np.array_equal(cnt, ocnt)
    assert np.array_equal(ids, oids)
    assert np.array_equal(dist.view(np.uint32), odist.view(np.uint32))
    assert np.array_equal(ev, oev)
    # graph round trip
    g = hn.export_graph()
    og = oix.export()
    for key in ("levels", "deg0", "nbr0", "cnt0", "upidx", "degU", "nbrU", "cntU"):
        assert np.array_equal(g[key], og[key]), key
    assert np.array_equal(hn.get_data().view(np.uint8), db.view(np.uint8))


def test_bruteforce_matches_oracle(gpu_ctx):
    import gsearch_amd as G
    db = H.synth_sig_db(10, 30, 500, 14)
    oix = O.Index(np.float32, 500, 8, 32, seed=1)
    oix.parallel_insert(db, batch=1)
    hn = G.Hnsw.new(8, 10000, 16, 32, G.DistHamming())
    hn.import_graph(db, oix.export())
    q = H.queries_from(db, 33, 15)
    ids, dist = hn.bruteforce_search(q, 12)
    oids, odist = O.bruteforce_topk(db, q, 12)
    assert np.array_equal(ids, oids) and np.array_equal(dist, odist)


@pytest.mark.parametrize("dtype,m,M,efc,B,scale,n_roots,per", [
    (np.float32, 256, 8, 32, 1, 1.0, 10, 12),
    (np.float32, 256, 8, 32, 16, 1.0, 20, 25),
    (np.uint64, 120, 16, 64, 64, 1.0, 30, 30),
    (np.float32, 1000, 12, 100, 256, 0.25, 25, 40),
    (np.uint32, 64, 4, 16, 7, 1.0, 15, 20),
])
def test_parallel_insert_matches_oracle(gpu_ctx, dtype, m, M, efc, B, scale, n_roots, per):
    """device-built graph == oracle-built graph (same batch size), then identical search answers"""
    import gsearch_amd as G
    db = H.synth_sig_db(n_roots, per, m, 21, dtype=dtype, jlo=0.05, jhi=0.95)
    oix = O.Index(dtype, m, M, efc, scale_modify=scale, seed=77)
    hn = G.Hnsw.new(M, 10000, 16, efc, G.DistHamming(), dtype=dtype, seed=77, insert_batch=B)
    hn.modify_level_scale(scale)
    hn.set_extend_candidates(True)
    hn.set_keeping_pruned(False)
    # two calls: the second one continues an existing graph (the `add` path of the reference)
    half = len(db) // 2 + 3
    for part in (db[:half], db[half:]):
        oix.parallel_insert(part, batch=B)
        hn.parallel_insert(part)
    assert hn.get_nb_point() == oix.nb_point() == len(db)
    g, og = hn.export_graph(), oix.export()
    assert g["entry"] == og["entry"] and g["n_upper"] == og["n_upper"]
    for key in ("levels", "upidx", "deg0", "degU"):
        assert np.array_equal(g[key], og[key]), key
    # adjacency beyond deg is unspecified: compare the valid prefix
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]), ("nbr0", i)
        assert np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), ("cnt0", i)
    for u in range(og["n_upper"]):
        for L in range(og["degU"].shape[1]):
            d = int(og["degU"][u, L])
            assert np.array_equal(g["nbrU"][u, L, :d], og["nbrU"][u, L, :d]), ("nbrU", u, L)
    q = H.queries_from(db, 40, 6, frac=0.3)
    ids, dist, cnt, ev = hn.search_arrays(q, 10, 50)
    oids, odist, ocnt, oev = oix.parallel_search(q, 10, 50)
    assert np.array_equal(ids, oids) and np.array_equal(dist, odist) and np.array_equal(ev, oev)


@pytest.mark.parametrize("mode", ["gather", "dense"])
@pytest.mark.parametrize("dtype,m,M,efc,B,scale,n_roots,per,jlo", [
    (np.float32, 256, 8, 8, 16, 1.0, 20, 25, 0.05),        # efc < 2M: every layer-0 selection extends
    (np.float32, 256, 8, 16, 1, 1.0, 12, 12, 0.05),        # efc == 2M, sequential insertion
    (np.uint64, 120, 16, 20, 64, 0.5, 30, 30, 0.05),
    (np.float32, 512, 255, 400, 256, 0.25, 40, 60, 0.3),   # gsearch -n 255 with the default --ef 400 (gsearch.rs:219-225,268)
    (np.uint32, 200, 200, 400, 128, 0.25, 25, 50, 0.0),    # -n 200, many ties at distance 1.0 (jlo = 0: unrelated members)
    (np.float32, 128, 16, 24, 256, 0.25, 50, 100, 0.05),   # 5000 points: in dense mode W comes from the insert pre-pass (n >= 4096)
])
def test_extend_candidates_with_small_ef_construction(gpu_ctx, monkeypatch, mode, dtype, m, M, efc, B, scale, n_roots, per, jlo):
    """extend_candidates = true (always, dnasketch.rs:159) with ef_construction <= 2 * max_nb_conn: hnsw_rs' select_neighbours adds the
    neighbours of the candidates (SPEC 5); device graph == oracle graph, searches identical"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", mode)
    db = H.synth_sig_db(n_roots, per, m, 5, dtype=dtype, jlo=jlo, jhi=0.95)
    oix = O.Index(dtype, m, M, efc, scale_modify=scale, seed=3)
    hn = G.Hnsw.new(M, 10000, 16, efc, G.DistHamming(), dtype=dtype, seed=3, insert_batch=B)
    hn.modify_level_scale(scale)
    hn.set_extend_candidates(True)
    hn.set_keeping_pruned(False)
    half = len(db) // 2 + 1
    for part in (db[:half], db[half:]):
        oix.parallel_insert(part, batch=B)
        hn.parallel_insert(part)
    g, og = hn.export_graph(), oix.export()
    assert g["entry"] == og["entry"] and g["n_upper"] == og["n_upper"]
    for key in ("levels", "upidx", "deg0", "degU"):
        assert np.array_equal(g[key], og[key]), key
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]), ("nbr0", i)
        assert np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), ("cnt0", i)
    for u in range(og["n_upper"]):
        for L in range(og["degU"].shape[1]):
            d = int(og["degU"][u, L])
            assert np.array_equal(g["nbrU"][u, L, :d], og["nbrU"][u, L, :d]), ("nbrU", u, L)
    q = H.queries_from(db, 24, 6, frac=0.3)
    ids, dist, cnt, ev = hn.search_arrays(q, 10, 50)
    oids, odist, ocnt, oev = oix.parallel_search(q, 10, 50)
    assert np.array_equal(ids, oids) and np.array_equal(dist, odist) and np.array_equal(ev, oev)


@pytest.mark.parametrize("k,m,algo,data", [(21, 2000, "super", "dna"), (21, 2000, "super2", "dna"), (16, 1024, "super2", "dna"), (14, 300, "super2", "dna"),
                                           (7, 1000, "super2", "aa"), (5, 640, "super2", "aa"), (7, 24000, "super2", "aa"), (12, 512, "super", "aa")])
def test_sketch_super_matches_oracle(gpu_ctx, k, m, algo, data):
    """SuperMinHash / SuperMinHash2: level-0 parallel pass (every slot filled) — config 5 is (7, 24000, super2, aa)"""
    import gsearch_amd as G
    rng = np.random.default_rng(k * 7 + m)
    if data == "dna":
        fam = H.family(rng, 150000 if m <= 2000 else 60000, [0.01, 0.05])
        genomes = [[H.dna_ascii(g)] for g in fam]
        genomes.append([H.dna_ascii(fam[0])[:70000], b"ACGTNN", H.dna_ascii(fam[1])[1000:90000]])
    else:
        n = 600000 if m > 10000 else 120000
        fam = H.family(rng, n, [0.02], alphabet=20)
        genomes = [[H.aa_ascii(g)] for g in fam]
        genomes.append([H.aa_ascii(fam[0])[:n // 2] + b"*X", H.aa_ascii(fam[1])[10:n - 7]])
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, algo, data))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, algo, genomes, data)
    assert got.dtype == ref.dtype
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("algo,data,k", [("super", "dna", 21), ("super2", "dna", 21), ("super2", "dna", 12), ("super2", "aa", 7)])
@pytest.mark.parametrize("serial", [False, True])
def test_sketch_super_cold_path_matches_oracle(gpu_ctx, algo, data, k, serial, monkeypatch):
    """few k-mers, many slots: slots stay empty after level 0 -> exact walk on the device: one workgroup per genome with atomicMin on
    packed (level, r) keys, or (large sketches; forced here) the sequential one-lane-per-genome kernel"""
    import gsearch_amd as G
    if serial:
        monkeypatch.setenv("GS_SMH_COLD_SERIAL", "1")
    rng = np.random.default_rng(17)
    if data == "dna":
        genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (30, 500, 3000)] + [[b"ACGT"]]
    else:
        genomes = [[H.aa_ascii(rng.integers(0, 20, n))] for n in (20, 400, 2500)] + [[b"MK"]]
    genomes.append([H.dna_ascii(H.rand_dna(rng, 40000))] if data == "dna" else [H.aa_ascii(rng.integers(0, 20, 40000))])
    # several records, one of them shorter than k, and a genome whose k-mers all repeat
    if data == "dna":
        genomes.append([H.dna_ascii(H.rand_dna(rng, 700)), b"ACG", H.dna_ascii(H.rand_dna(rng, 90))])
        genomes.append([b"ACGT" * 40])
    else:
        genomes.append([H.aa_ascii(rng.integers(0, 20, 300)), b"MK", H.aa_ascii(rng.integers(0, 20, 60))])
        genomes.append([b"MKV" * 30])
    sk = G.sketcher_for(G.SeqSketcherParams(k, 1024, algo, data))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, 1024, algo, genomes, data)
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("mode", ["dense", "gather"])
def test_dense_and_gather_modes_are_identical(gpu_ctx, mode, monkeypatch):
    """the dense (tile kernel + lookup) and gather (row streaming) evaluation strategies give the same graph and answers"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", mode)
    db = H.synth_sig_db(20, 30, 300, 31, jlo=0.05, jhi=0.95)
    oix = O.Index(np.float32, 300, 8, 40, seed=5)
    hn = G.Hnsw.new(8, 10000, 16, 40, G.DistHamming(), seed=5, insert_batch=32)
    hn.set_extend_candidates(True)
    oix.parallel_insert(db, batch=32)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d])
    q = H.queries_from(db, 200, 8, frac=0.3)
    ids, dist, cnt, ev = hn.search_arrays(q, 10, 100)
    oids, odist, ocnt, oev = oix.parallel_search(q, 10, 100)
    assert np.array_equal(ids, oids) and np.array_equal(dist, odist) and np.array_equal(ev, oev)


@pytest.mark.parametrize("k,m,data", [(21, 2000, "dna"), (16, 1024, "dna"), (12, 300, "dna"), (32, 500, "dna"), (7, 800, "aa"), (5, 256, "aa")])
def test_sketch_prob_matches_oracle(gpu_ctx, k, m, data):
    """ProbMinHash3a: weighted multiset sketch — repeats matter"""
    import gsearch_amd as G
    rng = np.random.default_rng(k + m)
    if data == "dna":
        fam = H.family(rng, 60000, [0.01, 0.05])
        rep = H.dna_ascii(fam[0])[:300] * 60                     # a heavy repeat: multiplicities up to 60
        genomes = [[H.dna_ascii(g)] for g in fam]
        genomes.append([H.dna_ascii(fam[0])[:30000] + rep, b"ACGTNN", H.dna_ascii(fam[1])[1000:40000], rep])
        genomes.append([b"A" * 500])                             # a single distinct k-mer with weight 480
        genomes.append([H.dna_ascii(H.rand_dna(rng, 60))])       # a handful of k-mers: many passes
        genomes.append([b"ACG"])                                 # nothing
    else:
        fam = H.family(rng, 40000, [0.02], alphabet=20)
        rep = H.aa_ascii(fam[0])[:100] * 30
        genomes = [[H.aa_ascii(g)] for g in fam] + [[H.aa_ascii(fam[0])[:9000] + rep + b"*", rep], [b"MKV"], [H.aa_ascii(rng.integers(0, 20, 40))]]
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, "prob", data))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, "prob", genomes, data)
    assert got.dtype == ref.dtype
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("k,m,data,length", [(21, 1000, "dna", 200000), (16, 512, "dna", 90000), (32, 700, "dna", 120000), (7, 600, "aa", 100000), (21, 18000, "dna", 1600000)])
@pytest.mark.parametrize("impl", ["tiers", "buckets", "buckets_one_level", "sort"])
def test_sketch_prob_bucketed_form_matches_oracle(gpu_ctx, monkeypatch, k, m, data, length, impl):
    """ProbMinHash3a on genomes with >= 64 k-mers per slot, which take the bucketed form (partition by hash bits -> LDS hash -> (value,
    multiplicity) -> first points under a running rejection threshold; the partition in two levels - coarse scatter + LDS-sorted refinement that
    leaves 4-byte ids, 8-byte values for k = 32 - or in one): repeats of multiplicity 2..40 (pass 2 and later over the active
    list), a genome in two parts workgroups split, multi-record genomes, and small genomes in the same batch (sorted form) - bit-exact
    against the oracle, and the sorted form (GS_PROB_IMPL=sort) gives the same signatures"""
    import gsearch_amd as G
    # "tiers": the default since round 6 (the tiered form where it suits - here the k = 16, k = 21 / 1.6 Mbp and amino-acid cases - with the bucketed form as its fallback);
    # "buckets" / "buckets_one_level": GS_PROB_IMPL=buckets keeps the round-4 / round-3 forms under test for every genome they suit (they are the exact fallback)
    if impl == "sort":
        monkeypatch.setenv("GS_PROB_IMPL", "sort")
    if impl in ("buckets", "buckets_one_level"):
        monkeypatch.setenv("GS_PROB_IMPL", "buckets")
    if impl == "buckets_one_level":                               # the round-3 partition (one scatter over all buckets, 8-byte values): kept for A/B
        monkeypatch.setenv("GS_PROB_ONELEVEL", "1")
    rng = np.random.default_rng(k * 131 + m)
    if data == "dna":
        fam = H.family(rng, length, [0.01, 0.05])
        asc = [H.dna_ascii(g) for g in fam]
        rep = asc[0][:400] * 40                                   # multiplicities up to 40: alive in pass 2 and beyond
        genomes = [[a] for a in asc]
        genomes.append([asc[0][: length // 2] + rep, b"ACGTNN", asc[1][1000: length // 2], rep, asc[2][: length // 3]])
        genomes.append([asc[1][:5000]])                           # a small genome between big ones: sorted form
        genomes.append([asc[2] + asc[2][: length // 4]])          # a quarter of the k-mers twice
        genomes.append([b"ACG"])
    else:
        fam = H.family(rng, length, [0.02], alphabet=20)
        asc = [H.aa_ascii(g) for g in fam]
        rep = asc[0][:150] * 30
        genomes = [[a] for a in asc] + [[asc[0][: length // 2] + rep + b"*", rep, asc[1][: length // 2]], [b"MKV"], [asc[1] + asc[1][: length // 5]]]
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, "prob", data))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, "prob", genomes, data)
    assert got.dtype == ref.dtype
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert len(bad) == 0, ("genomes differing", bad.tolist(), [int((got[i] != ref[i]).sum()) for i in bad])


def test_sketch_prob_bucketed_form_hands_flagged_genomes_to_the_sorted_form(gpu_ctx):
    """a k-mer repeated more than 65 536 times wraps the bucket kernel's 16-bit duplicate count: the genome is flagged on the device and redone by
    the sorted form, its neighbours in the batch are not disturbed - bit-exact against the oracle either way"""
    import gsearch_amd as G
    rng = np.random.default_rng(77)
    k, m = 21, 1000
    a = H.dna_ascii(H.rand_dna(rng, 150000)); b = H.dna_ascii(H.rand_dna(rng, 120000))
    genomes = [[a], [b[:60000] + b"A" * 90000 + b[60000:]], [b], [b"ACGT" * 40000 + a[:30000]]]       # 2nd: poly-A run; 4th: 4 k-mers 40 000 times each
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, "prob", "dna"))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, "prob", genomes, "dna")
    assert np.array_equal(got, ref), np.nonzero((got != ref).any(axis=1))[0].tolist()


@pytest.mark.parametrize("mode", ["default", "cap_fails", "two_walk"])
def test_sketch_prob_tiered_form_and_its_exact_fallback(gpu_ctx, monkeypatch, capfd, mode):
    """ProbMinHash3a, tiered form (round 6: value-level first-draw filter under a speculative cap, count-min bounds of the multiplicity, one-pass
    partition into per-part slices). Genomes large enough for it at k = 21 (2048 buckets of >= 256 k-mers), with what stresses each mechanism:
    a 5 kb repeat in 50 copies (real multiplicities far above what the count-min cells of singletons hold: the repeats must enter the exact table
    with w = 50, and survive into pass 2), a quarter of a genome twice (w = 2 everywhere in it), a poly-A run and four k-mers 40 000 times each
    (one slice / one count-min cell / the table overflow: the genome is flagged on the device and redone by the bucketed, then the sorted form),
    multi-record genomes and a small genome between them. `cap_fails`: GS_PROB_CAP_C = -6 makes the speculative cap ~400x too tight, the check
    max_b q[b] <= cap fails for EVERY genome and all of them take the fallback (the stderr trace says so). `two_walk`: the amino-acid form of the
    partition kernel on DNA. Bit-exact against the oracle in every mode."""
    import gsearch_amd as G
    if mode == "cap_fails":
        monkeypatch.setenv("GS_PROB_CAP_C", "-6")
    if mode == "two_walk":
        monkeypatch.setenv("GS_PROB_TWOWALK", "1")
    monkeypatch.setenv("GS_PROB_VERBOSE", "1")
    rng = np.random.default_rng(606)
    k, m = 21, 1000
    base = [H.dna_ascii(H.rand_dna(rng, n)) for n in (760_000, 640_000, 700_000)]
    rep = base[0][1000:6000]
    genomes = [
        [base[0]],
        [base[1][:300_000] + rep * 50 + base[1][300_000:]],                       # the 50-copy 5 kb repeat
        [base[2] + base[2][: len(base[2]) // 4]],                                 # a quarter of the k-mers twice
        [base[0][:200_000], b"ACGTNN", base[1][1000:420_000], b"", base[2][5000:150_000].lower()],      # records, N, lower case
        [base[1][:30_000]],                                                       # small: sorted form
        [base[2][:350_000] + b"A" * 90_000 + base[2][350_000:]],                  # poly-A: one k-mer 89 980 times
        [b"ACGT" * 40_000 + base[0][:600_000]],                                   # four k-mers 40 000 times each
        [base[1]],
        [base[2][i:i + 997] for i in range(0, 700_000, 997)],                     # a draft assembly: 703 contigs of 997 bases (every unit of the walk touches a record boundary)
    ]
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, "prob", "dna"))
    got = sk.sketch_genomes(genomes)
    err = capfd.readouterr().err
    ref = _oracle_sketch(k, m, "prob", genomes, "dna")
    assert got.dtype == ref.dtype
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (mode, bad.tolist())
    flagged = "tiered form flagged genomes" in err
    assert flagged, err[-500:]                                  # (default / two_walk: the poly-A and the 4-k-mer genome; cap_fails: every genome)
    if mode == "cap_fails":
        assert "[0," in err
    else:                                                       # the tiered form itself must have run: a plain random genome is never flagged, and its scratch fits
        assert "no room for the scratch" not in err and "flagged genomes [0," not in err, err[-800:]


def test_prob_differential_run_over_random_shapes():
    """tools/prob_fuzz.py (round 6): the ProbMinHash3a sketcher against the oracle over random k / sketch sizes / genome sizes around the thresholds of its forms / records /
    repeats / poly-A runs. Its third case (seed 1) is the one that hung the round-6 code for good: a genome flagged by the tiered form (slice overflow) was left with an
    EMPTY slot - largest slot minimum +inf - while another genome's repeats sat on the active list, and the loop over passes >= 2 waited for the flagged genome to fall
    out of "w^-1 (pass - 1) <= max q". Twelve cases, bounded time, zero mismatches."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-u", os.path.join(root, "tools", "prob_fuzz.py"), "12", "1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    assert "12 cases, 0 mismatches" in out.stdout, out.stdout[-1500:]


def test_sketchers_and_hnsw_differential_runs():
    """the same differential idea over every sketcher (`prob_fuzz.py .. any`: optdens / revoptdens / super / super2 / hll / prob on random k, sizes, records, repeats) and over the
    HNSW build + search (`hnsw_fuzz.py`: random element type, sketch size, M, ef_construction, level scale, family structure with duplicates, insert batch and calls, knbn / ef,
    every distance strategy - device-built graph == oracle graph, answers and evaluation counts == oracle search). Bounded: 12 + 10 cases."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a = subprocess.run([sys.executable, "-u", os.path.join(root, "tools", "prob_fuzz.py"), "12", "23", "any"], capture_output=True, text=True, timeout=900)
    assert a.returncode == 0 and "12 cases, 0 mismatches" in a.stdout, (a.stdout[-1500:], a.stderr[-800:])
    b = subprocess.run([sys.executable, "-u", os.path.join(root, "tools", "hnsw_fuzz.py"), "10", "4"], capture_output=True, text=True, timeout=1200)
    assert b.returncode == 0 and "10 cases, 0 mismatches" in b.stdout, (b.stdout[-1500:], b.stderr[-800:])


def test_index_dump_and_reload(gpu_ctx, tmp_path):
    """file_dump / load round trip (own format): identical graph, data and answers; `add` continues on the reloaded index"""
    import gsearch_amd as G
    db = H.synth_sig_db(12, 25, 200, 41, dtype=np.uint64, jlo=0.05, jhi=0.95)
    hn = G.Hnsw.new(8, 10000, 16, 40, G.DistHamming(), dtype=np.uint64, seed=3, insert_batch=16)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db[:200])
    path = tmp_path / "hnswdump.gsamd"
    hn.file_dump(path)
    h2 = G.Hnsw.load(path)
    assert h2.get_nb_point() == 200
    g1, g2 = hn.export_graph(), h2.export_graph()
    for key in ("levels", "deg0", "upidx"):
        assert np.array_equal(g1[key], g2[key])
    assert np.array_equal(hn.get_data(), h2.get_data())
    q = H.queries_from(db, 20, 3)
    a, b = hn.search_arrays(q, 5, 40), h2.search_arrays(q, 5, 40)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    hn.parallel_insert(db[200:])
    h2.parallel_insert(db[200:])
    a, b = hn.search_arrays(q, 5, 40), h2.search_arrays(q, 5, 40)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a truncated or corrupt dump is refused with an error code (never an exception across the C ABI)
    raw = path.read_bytes()
    for bad in (raw[:len(raw) // 2], raw[:40], raw[:8] + b"\xff" * 80 + raw[88:], b"GSAMDIX1"):
        (tmp_path / "bad.gsamd").write_bytes(bad)
        with pytest.raises(G.GsError) as e:
            G.Hnsw.load(tmp_path / "bad.gsamd")
        assert e.value.code == -5


def test_cpp_host_mirror(gpu_ctx, tmp_path):
    """the C++ mirror of the reference's call sequence (include/gsearch_amd.hpp, tohnsw + request) gives the Python path's answers"""
    import subprocess
    import gsearch_amd as G
    rng = np.random.default_rng(77)
    roots = [H.rand_dna(rng, 30000) for _ in range(4)]
    db = [H.dna_ascii(H.mutate(rng, roots[i % 4], 0.01 * (1 + i // 4))) for i in range(24)]
    qs = [H.dna_ascii(H.mutate(rng, roots[i], 0.02)) for i in range(4)]
    for name, seqs in (("db.fa", db), ("q.fa", qs)):
        with open(tmp_path / name, "w") as f:
            for i, s in enumerate(seqs):
                f.write(">g%d\n" % i)
                for o in range(0, len(s), 80):
                    f.write(s[o:o + 80].decode() + "\n")
    exe = os.path.join(os.path.dirname(G.SO_PATH), "tohnsw_request_demo")
    k, s, M, efc, ef, knbn = 21, 2000, 8, 32, 64, 5
    out = subprocess.run([exe, str(tmp_path / "db.fa"), str(tmp_path / "q.fa")] + [str(x) for x in (k, s, M, efc, ef, knbn)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    # python path
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(k, s, "optdens"))
    hn = G.Hnsw.new(M, 1500000, 16, efc, G.DistHamming(), seed=1)
    hn.modify_level_scale(0.25); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
    hn.parallel_insert(sk.sketch_genomes([[g] for g in db]))
    res = hn.parallel_search(sk.sketch_genomes([[q] for q in qs]), knbn, ef)
    # the reference's text output (ReqAnswer::dump, answer.rs:35-76) produced by the Python mirror must equal the C++ mirror's
    import io
    seqdict = [(str(tmp_path / "db.fa"), "g%d" % i, len(db[i])) for i in range(len(db))]
    buf = io.StringIO()
    for i, r in enumerate(res):
        G.ReqAnswer(i, (str(tmp_path / "q.fa"), "g%d" % i, len(qs[i])), r).dump(seqdict, 0.99, buf)
    assert out.stdout == buf.getvalue() + "\n"
    assert out.stdout.count("query_id:") >= 5


def test_three_evaluation_strategies_agree_with_oracle(gpu_ctx, monkeypatch):
    """gather / dense (LDS-resident C) / dense (3 workgroups per CU, C in global memory): same ids, distances AND the same
    number of DistHamming evaluations as the oracle, on a graph with real merges (ef well below the reachable set)."""
    import gsearch_amd as G
    db = H.synth_sig_db(60, 50, 256, 77, jlo=0.02, jhi=0.9)
    oix = O.Index(np.float32, 256, 16, 64, seed=9)
    oix.parallel_insert(db, batch=64)
    hn = G.Hnsw.new(16, 100000, 16, 64, G.DistHamming(), seed=9, insert_batch=64)
    hn.set_extend_candidates(True)
    hn.import_graph(db, oix.export())
    q = H.queries_from(db, 300, 5, frac=0.25)
    want = oix.parallel_search(q, 20, 400)
    for mode, legacy in (("gather", None), ("dense", "1"), ("dense", None)):
        monkeypatch.setenv("GS_DIST_MODE", mode)
        if legacy:
            monkeypatch.setenv("GS_DENSE_LEGACY", legacy)
        else:
            monkeypatch.delenv("GS_DENSE_LEGACY", raising=False)
        got = hn.search_arrays(q, 20, 400)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), mode
        assert np.array_equal(got[3], want[3]), (mode, legacy, "evaluation counts")


def test_fasta_ingest_pack_and_sketch(gpu_ctx):
    """f2: FASTA text -> record scan (host) -> filter/case-fold/2-bit pack (device) -> sketch, against the oracle's encode + sketch"""
    import gsearch_amd as G
    rng = np.random.default_rng(91)

    def fasta(records, width):
        out = []
        for name, s in records:
            out.append(b">" + name + b" some description\n")
            out += [s[o:o + width] + b"\n" for o in range(0, len(s), width)]
        return b"".join(out)

    g1 = H.dna_ascii(H.rand_dna(rng, 50000))
    g2 = H.dna_ascii(H.rand_dna(rng, 33333))
    files = [
        fasta([(b"chr1", g1[:20000] + b"NNNNNRYKM" + g1[20000:30000].lower()), (b"phage_capsid_gene", g1[30000:31000]), (b"chr2", g1[31000:]), (b"tiny", b"ACG")], 60),
        fasta([(b"contig%d" % i, g2[i * 3000:(i + 1) * 3000 + 17]) for i in range(11)], 80),
        b">only_header\n",
        fasta([(b"single", g2)], 70).replace(b"\n", b"\r\n"),
    ]
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(21, 1500, "optdens"))
    sig, (rs, rl, packed) = G.sketch_fasta_files(sk, files)
    # oracle: same records (capsid record skipped like dnafiles.rs:67), encode_and_add semantics
    genomes = []
    for f in files:
        genomes.append([f[b:e] for _, b, e in G.fasta_scan(f)])
    assert [len(g) for g in genomes] == [3, 11, 1, 1]          # ">only_header" is one empty record
    recs = [r for g in genomes for r in g]
    oseq, ors, orl = O.pack_dna(recs)
    assert np.array_equal(rl, orl)
    for i in range(len(recs)):           # packed bytes of every record are identical (records start on different boundaries)
        nb = (int(rl[i]) + 3) // 4
        got = packed[int(rs[i]) // 4: int(rs[i]) // 4 + nb]
        want = oseq[int(ors[i]) // 4: int(ors[i]) // 4 + nb]
        assert np.array_equal(got, want), i
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    ref = O.sketch_batch(O.params(21, 1500, "optdens"), oseq, ors, orl, goff)
    assert np.array_equal(sig.view(np.uint32), ref.view(np.uint32))


def test_edge_cases_and_error_behaviour(gpu_ctx):
    """empty / ragged inputs, extreme k, and the loud failures of the boundary (no silent fallbacks)"""
    import gsearch_amd as G
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(21, 128, "optdens"))
    # empty batch, empty genome, genome of only N's, genome shorter than k
    assert sk.sketch_genomes([]).shape == (0, 128)
    got = sk.sketch_genomes([[], [b""], [b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"], [b"ACGTACGTACGTACGTACGT"]])
    assert got.shape == (4, 128) and (got == 1.0).all()                       # no k-mer at all -> all slots 1.0 (SPEC 3.1)
    # exactly one k-mer; k = 32 (64-bit values fully used) ; k = 1
    one = b"ACGTTGCAACGTTGCAACGTA"
    ref = _oracle_sketch(21, 128, "optdens", [[one]])
    assert np.array_equal(sk.sketch_genomes([[one]]).view(np.uint32), ref.view(np.uint32))
    rng = np.random.default_rng(2)
    g = H.dna_ascii(H.rand_dna(rng, 5000))
    for k, algo in ((32, "optdens"), (32, "prob"), (1, "super2"), (2, "prob"), (31, "super")):
        s2 = G.sketcher_for(G.SeqSketcherParams(k, 96, algo))
        assert np.array_equal(_bits(s2.sketch_genomes([[g], [g[:77]]])), _bits(_oracle_sketch(k, 96, algo, [[g], [g[:77]]]))), (k, algo)
    # ragged: 300 records of wildly different lengths in one genome, many shorter than k
    recs = [g[i * 13:i * 13 + (i % 40)] for i in range(300)]
    assert np.array_equal(sk.sketch_genomes([recs]).view(np.uint32), _oracle_sketch(21, 128, "optdens", [recs]).view(np.uint32))
    # DistHamming: zero rows / single element
    dh = G.DistHamming()
    assert dh.eval_qxc(np.zeros((0, 5), np.float32), np.zeros((3, 5), np.float32)).shape == (0, 3)
    assert dh.eval(np.array([1.5], np.float32), np.array([1.5], np.float32)) == 0.0
    with pytest.raises(G.GsError):
        dh.eval_qxc(np.zeros((2, 5), np.float32), np.zeros((2, 6), np.float32))
    # index: search on empty index, wrong signature length, knbn > nb_point, ef beyond the LDS budget, ragged id list
    hn = G.Hnsw.new(8, 1000, 16, 32, dh)
    with pytest.raises(G.GsError):
        hn.search_arrays(np.zeros((1, 16), np.float32), 3, 10)
    db = H.synth_sig_db(3, 4, 64, 1)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    with pytest.raises(G.GsError):
        hn.modify_level_scale(0.5)                                              # parameters are frozen once the index holds points
    with pytest.raises(G.GsError):
        hn.parallel_insert(np.zeros((2, 65), np.float32))
    with pytest.raises(G.GsError):
        hn.parallel_insert(db[:2], ids=[99])                                    # one id per vector (any ids are fine: tests/test_gpu_ids.py)
    ids, dist, cnt, _ = hn.search_arrays(db[:2], 50, 10)                        # knbn > nb_point: short lists, padded
    oix = O.Index(np.float32, 64, 8, 32, seed=0)
    oix.parallel_insert(db, batch=64)
    oids, odist, ocnt, _ = oix.parallel_search(db[:2], 50, 10)
    assert np.array_equal(cnt, ocnt) and (cnt <= 12).all() and np.array_equal(ids, oids) and np.array_equal(dist, odist)
    for i in range(2):
        assert (ids[i, cnt[i]:] == np.iinfo(np.uint64).max).all() and np.isinf(dist[i, cnt[i]:]).all()
    with pytest.raises(G.GsError) as e:
        hn.search_arrays(db[:1], 5, 200000)
    assert e.value.code == -3
    with pytest.raises(G.GsError):
        G.Hnsw.new(300, 1000, 16, 32, dh).parallel_insert(db)                   # max_nb_conn > 255 (gsearch.rs:268)


def test_full_size_properties(gpu_ctx):
    """BASELINE sizes (k=21, s=18000, Mbp genomes, M=128, efc=1600, ef=5000, n=50) checked through size-independent properties:
    strand / record-order invariance, slot-wise-min mergeability, d(x,x)=0, sortedness, self-retrieval, and distances that agree
    with an independent DistHamming evaluation of the returned ids."""
    import gsearch_amd as G
    rng = np.random.default_rng(123)
    k, m = 21, 18000
    roots = [H.rand_dna(rng, 1_000_000) for _ in range(3)]
    genomes = [[H.dna_ascii(H.mutate(rng, roots[i % 3], 0.002 * (1 + i // 3)))] for i in range(60)]
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(k, m, "optdens"))
    sig = sk.sketch_genomes(genomes)
    assert ((sig >= 0) & (sig < 1)).all()
    g0 = genomes[0][0]
    extra = sk.sketch_genomes([[H.revcomp_ascii(g0)], [g0[:400000], g0[400000 - 20:]], [g0[400000 - 20:], g0[:400000]], [g0[:500000]], [g0[500000 - 20:]]])
    assert np.array_equal(extra[0], sig[0])                              # reverse complement
    assert np.array_equal(extra[1], sig[0]) and np.array_equal(extra[2], sig[0])     # record split / order
    assert np.array_equal(np.minimum(extra[3], extra[4]), sig[0])        # mergeability of the slot-wise minimum
    dh = G.DistHamming()
    D = dh.eval_qxc(sig[:8], sig)
    assert (np.diag(D[:, :8]) == 0).all() and np.array_equal(D[:8, :8], D[:8, :8].T)
    hn = G.Hnsw.new(128, 1_500_000, 16, 1600, dh, seed=5)
    hn.modify_level_scale(0.25); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
    hn.parallel_insert(sig)
    ids, dist, cnt, ev = hn.search_arrays(sig[:16], 50, 5000)
    assert (np.diff(dist[:, :cnt.min()], axis=1) >= 0).all()            # ascending
    assert np.array_equal(ids[:, 0], np.arange(16, dtype=np.uint64)) and (dist[:, 0] == 0).all()   # every point retrieves itself first
    for i in range(4):                                                   # reported distances == independent evaluation of the reported ids
        n = int(cnt[i])
        pairs = dh.eval_pairs(sig[:16], sig, np.full(n, i), ids[i, :n])
        assert np.array_equal(pairs, dist[i, :n])
    d01 = float(dist[0, 1])
    assert abs(G.ani(d01, k) - (1 + np.log(2 * (1 - d01) / (2 - d01)) / k) * 100) < 1e-6      # ANI within 1e-6 (reformat.rs:80-86)


@pytest.mark.parametrize("dtype,m,impl", [(np.uint64, 97, "join"), (np.uint32, 130, "join"), (np.uint64, 97, "tile"), (np.float32, 75, "tile")])
def test_dense_strategies_for_every_signature_kind(gpu_ctx, monkeypatch, dtype, m, impl):
    """match-join and compare-tile producers of the dense count matrix, for u64 / u32 / f32 signatures and odd sizes (n=1201)"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_IMPL", impl)
    db = H.synth_sig_db(30, 40, m, 55, dtype=dtype, jlo=0.02, jhi=0.9)[:1201]
    if dtype == np.float32:                                   # float `==` corner cases inside the index: -0.0 == +0.0, NaN != NaN
        db[5, :10] = -0.0; db[6, :10] = 0.0; db[7, 3] = np.nan; db[8, 3] = np.nan
    oix = O.Index(dtype, m, 12, 48, seed=4)
    oix.parallel_insert(db, batch=100)
    hn = G.Hnsw.new(12, 100000, 16, 48, G.DistHamming(), dtype=dtype, seed=4, insert_batch=100)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]) and np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d])
    q = np.concatenate([H.queries_from(db, 150, 3, frac=0.2), db[5:9]])
    got, want = hn.search_arrays(q, 15, 300), oix.parallel_search(q, 15, 300)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("vis", ["lds", "global", "split"])
@pytest.mark.parametrize("regime", ["spread", "ties", "tiny_ef"])
def test_dense_traversal_placements_and_regimes(gpu_ctx, monkeypatch, vis, regime):
    """dense traversal (histogram result set): visited bitmap in LDS / in global memory / split (round 5: ids below GS_SPLIT_W in LDS, the rest in global
    memory with the Bloom filter in front of it in the order-free phase and the evaluation count of what it dropped taken by a walk after the drain), on
    data with spread-out distances (the rank path), with almost everything tied at distance 1 (the flood regime of the request workload) and with ef = knbn = small"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")                    # 1200 nodes: ids 1024.. live in the global part (two walks' worth would need > 2048)
    m = 200
    if regime == "ties":
        db = H.synth_sig_db(150, 8, m, 77, jlo=0.0, jhi=0.6)      # many small unrelated families: most pairs share no slot
        knbn, ef = 10, 400
    elif regime == "spread":
        db = H.synth_sig_db(3, 400, m, 78, jlo=0.02, jhi=0.98)
        knbn, ef = 25, 300
    else:
        db = H.synth_sig_db(12, 100, m, 79, jlo=0.1, jhi=0.9)
        knbn, ef = 7, 7
    oix = O.Index(np.float32, m, 8, 64, seed=9)
    oix.parallel_insert(db, batch=64)
    hn = G.Hnsw.new(8, 100000, 16, 64, G.DistHamming(), seed=9, insert_batch=64)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    q = np.concatenate([H.queries_from(db, 300, 5, frac=0.25), db[:40]])
    got, want = hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    if regime == "ties":
        assert (want[1] == 1.0).mean() > 0.3                      # the data really is tie-heavy


@pytest.mark.parametrize("knbn,ef", [(1, 1), (1, 2), (3, 3), (5, 63), (50, 64), (50, 65), (64, 64), (100, 100), (130, 700)])
def test_dense_traversal_small_and_odd_ef(gpu_ctx, monkeypatch, knbn, ef):
    """ef and knbn around the sizes the candidate front is built on (64 keys, one per lane of a wavefront): ef = 1 (the entry point's own rule), ef below,
    at and just above 64, knbn above 64 (T spans more than the front), on noise rows (every pair agrees in 19 +- 4 of 96 slots: dense count levels) - dense strategy == oracle, evaluation counts included"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    m = 96
    db = np.random.default_rng(502).integers(0, 5, (3000, m)).astype(np.float32)
    oix = O.Index(np.float32, m, 10, 40, seed=31)
    oix.parallel_insert(db, batch=128)
    hn = G.Hnsw.new(10, 100000, 16, 40, G.DistHamming(), seed=31, insert_batch=128)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    q = np.concatenate([np.random.default_rng(503).integers(0, 5, (100, m)).astype(np.float32), db[7:11]])
    got, want = hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert want[3].mean() > min(2500, 15 * ef)                           # the searches really walk the graph


@pytest.mark.parametrize("vis", ["lds", "split"])
def test_dense_traversal_front_refill_on_dense_tie_levels(gpu_ctx, monkeypatch, capfd, vis):
    """late round 5: the waiting candidates of k_hnsw_search_dense are a 64-key sorted front in the registers of wavefront 0 over an unsorted overflow,
    refilled with the smallest keys of the overflow's best count level by histogram selection (pq_rebuild). Here the levels are DENSE: 40 000 noise rows
    over six values (every pair agrees in 5 +- 2 of 32 slots: a dozen count levels of thousands of nodes each) and ef = 6000 (the API's limit at this
    max_nb_conn), so a level of the overflow holds a few dozen keys per id bin (256 bins of 256 ids, 157 of them populated): a refill that stops below
    48 keys with the next bin not fitting goes into the selection's second round (binning inside the bin that straddles the quota) - the counters of
    workgroup 0 (GS_TRAV_PHASES) say that it happened. ids, distances, counts and evaluation counts == oracle."""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "16384")
    monkeypatch.setenv("GS_TRAV_PHASES", "1")
    m = 32
    db = np.random.default_rng(11).integers(0, 6, (40000, m)).astype(np.float32)
    oix = O.Index(np.float32, m, 12, 48, seed=29)
    oix.parallel_insert(db, batch=256)
    hn = G.Hnsw.new(12, 100000, 16, 48, G.DistHamming(), seed=29, insert_batch=256)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    q = np.concatenate([np.random.default_rng(12).integers(0, 6, (48, m)).astype(np.float32), db[100:108]])
    for knbn, ef in ((10, 6000), (30, 900), (10, 12000)):           # (12 000: beyond what the sorted-array traversal can hold - the call must go dense by itself)
        if ef == 12000:
            monkeypatch.delenv("GS_DIST_MODE")
        hn.search_stats(reset=True)
        got, want = hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        assert want[3].mean() > (20000 if ef >= 6000 else 5000)
        hn.search_stats()                                               # GS_TRAV_PHASES: prints the refill counters of the call
        line = [l for l in capfd.readouterr().err.splitlines() if "phase 1 front" in l][-1].replace(",", " ").split()
        refills, rounds = int(line[line.index("refills") + 1]), int(line[-1])
        assert refills >= 3 * len(q) and (ef == 900 or rounds >= 1), line


@pytest.mark.parametrize("vis", ["lds", "global", "split"])
@pytest.mark.parametrize("M,regime", [(160, "spread"), (140, "ties"), (200, "tiny_ef")])
def test_dense_traversal_wide_adjacency(gpu_ctx, monkeypatch, vis, M, regime):
    """max_nb_conn above 128 (gsearch allows -n up to 255, gsearch.rs:268): layer-0 rows of up to 510 ids are expanded by one 512-lane group
    (k_hnsw_search_dense<..., ONEG>) instead of two 256-lane halves; same answers and evaluation counts as the oracle, and the lists
    really are longer than 256"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", vis)
    monkeypatch.setenv("GS_SPLIT_W", "1024")                    # "ties": 6000 nodes = the LDS part + five walks over the global part
    m = 160
    if regime == "ties":
        m = 64
        db = H.synth_sig_db(500, 12, m, 177, jlo=0.0, jhi=0.6)   # 6000 mostly unrelated rows: everything ties at distance 1, hubs collect reverse links
        knbn, ef = 10, 600
    elif regime == "spread":
        db = H.synth_sig_db(3, 420, m, 178, jlo=0.02, jhi=0.98)
        knbn, ef = 25, 700
    else:
        db = H.synth_sig_db(10, 110, m, 179, jlo=0.1, jhi=0.9)
        knbn, ef = 7, 7
    efc = 2 * M + 90                                            # extend_candidates needs efc > 2M on the device
    oix = O.Index(np.float32, m, M, efc, seed=19)
    oix.parallel_insert(db, batch=64)
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=19, insert_batch=64)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g = hn.export_graph()
    assert np.array_equal(g["deg0"], oix.export()["deg0"])
    if regime == "ties":
        assert int(g["deg0"].max()) > 256                        # lanes 256..511 of the group really carry neighbours
    q = np.concatenate([H.queries_from(db, 200, 5, frac=0.25), db[:30]])
    got, want = hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("dtype,M,efc,scale", [(np.float32, 12, 60, 1.0), (np.uint32, 8, 40, 0.5)])
def test_insert_prepass_builds_the_oracle_graph(gpu_ctx, monkeypatch, dtype, M, efc, scale):
    """past 4096 nodes a dense-mode insert batch takes its layer-0 searches through the dense traversal kernel (accepted-key log ->
    sorted result set W, plan_prepass) and k_hnsw_plan runs in two phases around it; the graph must still be the oracle's, level > 0
    points included (scale 1.0 gives plenty), and the same as with GS_PLAN_PREPASS=0"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    m = 64
    db = H.synth_sig_db(130, 50, m, 321, jlo=0.05, jhi=0.9).astype(dtype)
    oix = O.Index(dtype, m, M, efc, scale_modify=scale, seed=4)
    oix.parallel_insert(db, batch=256)
    og = oix.export()
    graphs = []
    # (GS_INSERT_GROUP: batches joined together - one match-join of the points of several batches against the nodes present at the group's start,
    # the nodes the earlier batches of the group add come from the compare tile kernel; 1 = every batch its own join, default 8)
    for pre, grp in (("1", None), ("0", None), ("1", "1"), ("1", "3")):
        monkeypatch.setenv("GS_PLAN_PREPASS", pre)
        if grp is None:
            monkeypatch.delenv("GS_INSERT_GROUP", raising=False)
        else:
            monkeypatch.setenv("GS_INSERT_GROUP", grp)
        hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=4, insert_batch=256)
        hn.modify_level_scale(scale); hn.set_extend_candidates(True)
        hn.parallel_insert(db)
        graphs.append(hn.export_graph())
    for g in graphs:
        assert np.array_equal(g["levels"], og["levels"]) and np.array_equal(g["deg0"], og["deg0"])
        for i in range(len(db)):
            d = int(og["deg0"][i])
            assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d])
    assert (og["levels"][4096:] > 0).sum() >= 3


@pytest.mark.parametrize("L,grp,data", [("4096", None, "families"), ("192", None, "families"), ("192", "1", "families"), ("64", "3", "families"),
                                        ("4096", None, "noise"), ("512", None, "noise"), ("512", "0", "noise"),
                                        ("4096", "grow", "families"), ("512", "full", "noise")])
def test_insert_with_sparse_pair_rows_builds_the_oracle_graph(gpu_ctx, monkeypatch, capfd, L, grp, data):
    """round 5: with the dense pair cache switched off (GS_PAIR_CACHE_GB=0 - what a build beyond ~400 k genomes runs into) the selection heuristic
    takes c(e,s) from the SPARSE pair rows: every node keeps the counts of its <= L closest older nodes and a cut; a pair that is not listed lies above
    the cut, which decides every candidate whose own count is <= the cut, and the rest is checked by streaming rows. 21 000 nodes in 210 families, so a
    list of 4096 holds a family and the best of the chance level, lists of 192 / 64 are cut inside the family (candidates above the cut: the level bitmap
    one level below the cut, then the streaming path, must agree too). "noise": 21 000 unrelated rows over a narrow value band - every pair agrees in
    ~16 +- 4 of 96 slots, so the lists are cut in the middle of the bulk and the selection walks are long. grp "0": without the level bitmaps
    (GS_SPARSE_BITMAP_GB=0). "grow": the arena the lists live in is mapped 4 MB at a time (it grows in place under the lists already written); "full": an arena
    of 24 MB that fills up half-way - the later nodes get no list and their pairs are checked by streaming rows. Graph (levels, degrees, neighbour ids AND their counts) == oracle; batches joined in groups without a slab (group buffer)."""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_PAIR_CACHE_GB", "0")
    monkeypatch.setenv("GS_SPARSE_L", L)
    monkeypatch.setenv("GS_SPARSE_VERBOSE", "1")
    if grp == "0":
        monkeypatch.setenv("GS_SPARSE_BITMAP_GB", "0")
    elif grp == "grow":
        monkeypatch.setenv("GS_SPARSE_ARENA_GB", "1"); monkeypatch.setenv("GS_SPARSE_ARENA_CHUNK_MB", "4")
    elif grp == "full":
        monkeypatch.setenv("GS_SPARSE_ARENA_GB", "0.024"); monkeypatch.setenv("GS_SPARSE_ARENA_CHUNK_MB", "2")
    elif grp is not None:
        monkeypatch.setenv("GS_INSERT_GROUP", grp)
    m, M, efc = 96, 10, 48
    if data == "families":
        db = H.synth_sig_db(210, 100, m, 77, jlo=0.05, jhi=0.9)
    else:
        db = np.random.default_rng(5).integers(0, 6, (21000, m)).astype(np.float32)
    oix = O.Index(np.float32, m, M, efc, scale_modify=0.5, seed=6)
    oix.parallel_insert(db, batch=256)
    og = oix.export()
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=6, insert_batch=256)
    hn.modify_level_scale(0.5); hn.set_extend_candidates(True)
    for lo in range(0, len(db), 6144):                                   # several insert calls (whole batches each: the graph depends on the batch boundaries): the lists of earlier calls serve the later ones
        hn.parallel_insert(db[lo:lo + 6144])
    err = capfd.readouterr().err
    last = [l for l in err.splitlines() if l.startswith("[GS_SPARSE]")][-1]
    f = last.replace(",", " ").replace(":", " ").replace("(", " ").replace(")", " ").replace(";", " ").split()
    with_list = int(f[f.index("list") + 1]); chunks = int(f[f.index("lists") + 1]); dense_bytes = int(f[f.index("bytes") + 1])
    away = int(f[f.index("away") + 1]); mapped = float(f[f.index("mapped") - 1])
    if grp == "full":
        assert dense_bytes == 0 and 0 < with_list < len(db) and with_list + away == len(db) and mapped <= 0.0262, last             # (24 MB rounded up to whole 2 MiB steps)
    else:
        assert dense_bytes == 0 and with_list == len(db) and away == 0 and chunks > (len(db) if data == "noise" else 1000), last
    if grp == "grow":
        assert 0.008 < mapped < 0.5, last                                # several 4 MB steps, far from the 1 GB it may take
    g = hn.export_graph()
    assert np.array_equal(g["levels"], og["levels"]) and np.array_equal(g["deg0"], og["deg0"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]) and np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), i


def test_insert_prepass_with_split_bitmap(gpu_ctx, monkeypatch):
    """the insert pre-pass (k_hnsw_search_dense<.., WLOG>) with the split visited bitmap - what a build beyond ~1.08 M nodes runs (before round 5 the
    pre-pass was given up there and every point searched by the sorted-array kernel): same graph as the oracle, levels > 0 included"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_DENSE_VIS", "split")
    monkeypatch.setenv("GS_SPLIT_W", "2048")
    m, M, efc = 64, 12, 60
    db = H.synth_sig_db(130, 50, m, 321, jlo=0.05, jhi=0.9)
    oix = O.Index(np.float32, m, M, efc, scale_modify=1.0, seed=4)
    oix.parallel_insert(db, batch=256)
    og = oix.export()
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=4, insert_batch=256)
    hn.modify_level_scale(1.0); hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g = hn.export_graph()
    assert np.array_equal(g["levels"], og["levels"]) and np.array_equal(g["deg0"], og["deg0"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d])
    q = np.concatenate([H.queries_from(db, 200, 5, frac=0.25), db[:30]])
    got, want = hn.search_arrays(q, 10, 200), oix.parallel_search(q, 10, 200)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_dense_insert_in_two_calls_builds_the_oracle_graph(gpu_ctx, monkeypatch):
    """dense mode, the points inserted in two calls (count rows of the insert batches produced group by group): the oracle's graph, counts included"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    for dtype, m, M, efc, B in ((np.uint64, 120, 16, 20, 64), (np.float32, 200, 8, 40, 32)):
        db = H.synth_sig_db(30, 30, m, 8, dtype=dtype, jlo=0.05, jhi=0.95)
        oix = O.Index(dtype, m, M, efc, scale_modify=0.5, seed=3)
        hn = G.Hnsw.new(M, 10000, 16, efc, G.DistHamming(), dtype=dtype, seed=3, insert_batch=B)
        hn.modify_level_scale(0.5); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
        for part in (db[:500], db[500:]):
            oix.parallel_insert(part, batch=B); hn.parallel_insert(part)
        g, og = hn.export_graph(), oix.export()
        assert np.array_equal(g["deg0"], og["deg0"]) and np.array_equal(g["levels"], og["levels"])
        for i in range(len(db)):
            d = int(og["deg0"][i])
            assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]) and np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), i


def test_insert_with_global_visited_bitmap(gpu_ctx, monkeypatch):
    """k_hnsw_plan keeps its visited bitmap in LDS when it fits; the global-memory fallback (large n) must build the same graph"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_PLAN_VIS_GLOBAL", "1")
    db = H.synth_sig_db(10, 60, 128, 91, jlo=0.05, jhi=0.9)
    oix = O.Index(np.float32, 128, 8, 48, seed=2)
    oix.parallel_insert(db, batch=50)
    hn = G.Hnsw.new(8, 10000, 16, 48, G.DistHamming(), seed=2, insert_batch=50)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"]) and np.array_equal(g["levels"], og["levels"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d])


@pytest.mark.parametrize("dtype,nq,knbn,ef", [(np.float32, 4000, 5, 40), (np.uint64, 2000, 600, 700), (np.uint32, 3500, 1024, 1024)])
def test_dense_search_large_batches_and_wide_answers(gpu_ctx, monkeypatch, dtype, nq, knbn, ef):
    """join batches beyond one hash table (3276 queries), the 8-byte-key table (104 kB of LDS) and answers wider than one key per lane"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    m = 48
    db = H.synth_sig_db(25, 80, m, 123, dtype=dtype, jlo=0.05, jhi=0.9)
    oix = O.Index(dtype, m, 8, 40, seed=6)
    oix.parallel_insert(db, batch=128)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), dtype=dtype, seed=6, insert_batch=128)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    q = H.queries_from(db, nq, 11, frac=0.3)
    got, want = hn.search_arrays(q, knbn, ef), oix.parallel_search(q, knbn, ef)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["dense", "gather"])
def test_wide_graph_falls_back_to_sorted_array_traversal(gpu_ctx, monkeypatch, mode):
    """max_nb_conn > 128 (2M > 256 lanes per half): the dense traversal kernel does not apply, the sorted-array kernel answers"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", mode)
    m, M = 64, 160
    db = H.synth_sig_db(6, 150, m, 321, jlo=0.05, jhi=0.9)
    oix = O.Index(np.float32, m, M, 400, seed=8)
    oix.parallel_insert(db, batch=200)
    hn = G.Hnsw.new(M, 100000, 16, 400, G.DistHamming(), seed=8, insert_batch=200)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"])
    q = H.queries_from(db, 200, 4, frac=0.2)
    got, want = hn.search_arrays(q, 20, 350), oix.parallel_search(q, 20, 350)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("force", ["0", "1", None])
def test_join_declines_to_tile_kernel_on_redundant_batches(gpu_ctx, monkeypatch, force, capfd):
    """the join samples the match density of the batch; a redundant query set against a redundant database (everything matches
    everything) is handed to the fixed-cost compare kernel. Either producer gives the same counts (forced both ways + natural)."""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", "dense")
    monkeypatch.setenv("GS_JOIN_VERBOSE", "1")
    if force is not None:
        monkeypatch.setenv("GS_JOIN_DECLINE", force)
    m = 96
    db = H.synth_sig_db(2, 2600, m, 7, jlo=0.85, jhi=0.99)          # two big families of near-identical signatures (5200 nodes)
    oix = O.Index(np.float32, m, 8, 40, seed=12)
    oix.parallel_insert(db, batch=200)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), seed=12, insert_batch=200)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"])
    q = np.repeat(db[:3], 400, axis=0)                              # 1200 queries, three distinct signatures
    got, want = hn.search_arrays(q, 10, 60), oix.parallel_search(q, 10, 60)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    err = capfd.readouterr().err
    if force is None:
        assert "-> est." in err and ": tile" in err                 # the natural decision on this data is the tile kernel


@pytest.mark.parametrize("mode", ["dense", "auto"])
def test_tiny_query_batches(gpu_ctx, monkeypatch, mode):
    """one, two, three queries at a time (the join builds a 64-entry table, one traversal workgroup); auto mode learns the evaluated
    fraction from its first gather call and may switch strategy for the following ones - answers never change"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", mode)
    m = 64
    db = H.synth_sig_db(40, 120, m, 77, jlo=0.0, jhi=0.7)           # 4800 nodes
    oix = O.Index(np.float32, m, 8, 40, seed=3)
    oix.parallel_insert(db, batch=256)
    hn = G.Hnsw.new(8, 100000, 16, 40, G.DistHamming(), seed=3, insert_batch=256)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    q = H.queries_from(db, 12, 9, frac=0.2)
    want = oix.parallel_search(q, 5, 300)
    for lo, hi in [(0, 1), (1, 3), (3, 6), (6, 7), (7, 12)]:
        got = hn.search_arrays(q[lo:hi], 5, 300)
        for a, b in zip(got, want):
            assert np.array_equal(a, b[lo:hi])


def test_config5_distance_leg_u64_m24000(gpu_ctx, monkeypatch):
    """BASELINE configs[4] beyond the sketch: DistHamming and the HNSW build/search on u64 signatures of m = 24000 (192 kB rows;
    the EW=2 tile path, the 8-byte-key join table at full width, row-gather traversal) against the oracle, bit for bit."""
    import gsearch_amd as G
    m, dtype = 24000, np.uint64
    db = H.synth_sig_db(20, 110, m, 505, dtype=dtype, jlo=0.05, jhi=0.95)       # 2200 rows, 422 MB
    q = H.queries_from(db, 96, 12, frac=0.3)
    dh = G.DistHamming()
    assert np.array_equal(dh.eval_qxc(q[:70], db[:600]), O.hamming_qxc(q[:70], db[:600], nthreads=os.cpu_count()))
    rng = np.random.default_rng(4)
    ia, ib = rng.integers(0, len(q), 300), rng.integers(0, len(db), 300)
    assert np.array_equal(dh.eval_pairs(q, db, ia, ib), O.hamming_pairs(q, db, ia, ib))
    M, efc, B = 16, 64, 128
    oix = O.Index(dtype, m, M, efc, scale_modify=0.25, seed=31)
    oix.parallel_insert(db, batch=B)
    og = oix.export()
    want = oix.parallel_search(q, 50, 200, nthreads=os.cpu_count())
    for mode, impl in (("gather", None), ("dense", "join"), ("dense", "tile")):
        monkeypatch.setenv("GS_DIST_MODE", mode)
        if impl:
            monkeypatch.setenv("GS_DENSE_IMPL", impl)
        hn = G.Hnsw.new(M, 10000, 16, efc, dh, dtype=dtype, seed=31, insert_batch=B)
        hn.modify_level_scale(0.25); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
        hn.parallel_insert(db)
        g = hn.export_graph()
        assert g["entry"] == og["entry"] and np.array_equal(g["levels"], og["levels"]) and np.array_equal(g["deg0"], og["deg0"]), (mode, impl)
        for i in range(len(db)):
            d = int(og["deg0"][i])
            assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]) and np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), (mode, impl, i)
        got = hn.search_arrays(q, 50, 200)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (mode, impl)
        hn.close()


def test_baseline_parameter_build_and_search(gpu_ctx):
    """one build at BASELINE parameters - s = 18000 f32, M = 128, efc = 1600, level scale 0.25, insert_batch = 256, n = 4096
    sketch-level rows (SURVEY 8d generator) - device graph == oracle graph, then the request search ef = 5000, n = 50 == oracle"""
    import gsearch_amd as G
    m, M, efc, B, n = 18000, 128, 1600, 256, 4096
    db = H.synth_sig_db(41, 100, m, 2024, jlo=0.3, jhi=0.99)[:n]
    oix = O.Index(np.float32, m, M, efc, scale_modify=0.25, seed=18000)
    oix.parallel_insert(db, batch=B)
    hn = G.Hnsw.new(M, 1_500_000, 16, efc, G.DistHamming(), seed=18000, insert_batch=B)
    hn.modify_level_scale(0.25); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert g["entry"] == og["entry"] and g["n_upper"] == og["n_upper"]
    for key in ("levels", "upidx", "deg0", "degU"):
        assert np.array_equal(g[key], og[key]), key
    assert og["deg0"].max() > 64 and og["deg0"].min() >= 1            # a real graph: the heuristic keeps tens of neighbours per node
    for i in range(n):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]), ("nbr0", i)
        assert np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), ("cnt0", i)
    for u in range(og["n_upper"]):
        for L in range(og["degU"].shape[1]):
            d = int(og["degU"][u, L])
            assert np.array_equal(g["nbrU"][u, L, :d], og["nbrU"][u, L, :d]), ("nbrU", u, L)
    q = H.queries_from(db, 64, 6, frac=0.2)
    got = hn.search_arrays(q, 50, 5000)
    want = oix.parallel_search(q, 50, 5000, nthreads=os.cpu_count())
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("k,m,data,length", [(21, 2000, "dna", 150000), (16, 512, "dna", 60000), (21, 18000, "dna", 1000000), (7, 1024, "aa", 80000)])
def test_sketch_hll_matches_oracle(gpu_ctx, k, m, data, length):
    """--algo hll: SetSketch registers (u16), warm regime (hundreds of k-mers per register: two passes in one workgroup, walks of a
    few steps kept in registers) - including BASELINE's s = 18000 - bit for bit against the oracle"""
    import gsearch_amd as G
    rng = np.random.default_rng(k * 31 + m)
    if data == "dna":
        fam = H.family(rng, length, [0.01, 0.05])
        genomes = [[H.dna_ascii(g)] for g in fam]
        g0 = H.dna_ascii(fam[0])
        genomes.append([g0[:length // 3] + b"NNNNnn" + g0[length // 3:length // 2].lower(), b"ACGT", g0[length // 2:]])
    else:
        fam = H.family(rng, length, [0.02], alphabet=20)
        genomes = [[H.aa_ascii(g)] for g in fam]
        genomes.append([H.aa_ascii(fam[0])[:length // 2] + b"*X", H.aa_ascii(fam[1])[10:length - 7]])
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, "hll", data))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, "hll", genomes, data)
    assert got.dtype == ref.dtype == np.uint16
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("spec", ["7", "-4", "2", "0"])
def test_sketch_hll_speculative_single_pass(gpu_ctx, monkeypatch, spec):
    """round 5: SetSketch in ONE pass under a guessed lower bound of the smallest register (K_g from (ln m + c) / (a N)), checked afterwards; a guess that
    does not hold (c = -4: far too high for every genome; c = 2: for some; a genome that is one 20 kb segment repeated - its N distinct k-mers are a fraction
    of what its length says) falls back to the two exact passes over the same table. Same registers as the oracle in every case, c = 0 = the round-4 form."""
    import gsearch_amd as G
    monkeypatch.setenv("GS_HLL_SPEC", spec)
    rng = np.random.default_rng(91)
    k, m = 21, 2000
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (900_000, 600_011, 1_300_000)]
    rep = H.dna_ascii(H.rand_dna(rng, 20_000))
    genomes.append([rep * 40])                                              # 800 kb of 20 000 distinct k-mers
    genomes.append([H.dna_ascii(H.rand_dna(rng, 400_000)), b"ACGTNNACGT", H.dna_ascii(H.rand_dna(rng, 350_007))])
    sk = G.sketcher_for(G.SeqSketcherParams(k, m, "hll"))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(k, m, "hll", genomes)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("cap", ["0", "4096", None])
def test_sketch_hll_survivor_lists(gpu_ctx, monkeypatch, cap):
    """SetSketch pass B runs over the hashes pass A recorded instead of hashing the genome again (gs_sketch.hip HllEmit::record_wave): without lists
    (0), with lists that overflow for every genome (4096 entries: the second walk is taken) and with the default lists - the same registers"""
    import gsearch_amd as G
    if cap is not None:
        monkeypatch.setenv("GS_HLL_SURVIVORS", cap)
    monkeypatch.setenv("GS_HLL_SURVIVORS_MINCHUNKS", "4")               # (default 64 chunks = 8.4 Mbp: the lists only pay for long genomes)
    rng = np.random.default_rng(41)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (1_200_000, 400_011, 2_300_000)]          # 9 / 3 / 17 chunks of 131 072 k-mers
    genomes.append([H.dna_ascii(H.rand_dna(rng, 700_000)), b"ACGTNNACGT", H.dna_ascii(H.rand_dna(rng, 650_007))])
    sk = G.sketcher_for(G.SeqSketcherParams(21, 4000, "hll"))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(21, 4000, "hll", genomes)
    assert got.dtype == ref.dtype and np.array_equal(got, ref)


def test_sketch_hll_cold_path_matches_oracle(gpu_ctx):
    """few k-mers per register: the lower bound stays near 0 and elements walk hundreds of steps - the genome is flagged by the warm
    kernel and redone with the permutation in per-lane global scratch; empty and tiny inputs included"""
    import gsearch_amd as G
    rng = np.random.default_rng(23)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (30, 400, 3000, 20000)] + [[b"ACGT"], [b""], [b"ACGT" * 50]]
    genomes.append([H.dna_ascii(H.rand_dna(rng, 900)), b"ACG", H.dna_ascii(H.rand_dna(rng, 100))])
    genomes.append([H.dna_ascii(H.rand_dna(rng, 300000))])                      # a warm genome in the same batch
    for m in (256, 1024):
        sk = G.HyperLogLogSketch.new(G.SeqSketcherParams(21, m, "hll"))
        got = sk.sketch_genomes(genomes)
        ref = _oracle_sketch(21, m, "hll", genomes)
        assert np.array_equal(got, ref), m
    assert (got[4] == 0).all() and (got[5] == 0).all()                          # no k-mer at all -> all registers 0


@pytest.mark.parametrize("m,length", [(50000, 1600000), (90000, 2600000)])
def test_sketch_hll_register_file_beyond_lds(gpu_ctx, m, length):
    """sketch_size is taken as is by the reference (dnasketch.rs:541-574): beyond ~40 000 registers the table moves to global memory behind a
    2-byte LDS filter (50 000), beyond ~80 000 without one (90 000); warm genomes, a cold one (walks of hundreds of steps) and an empty one"""
    import gsearch_amd as G
    rng = np.random.default_rng(m)
    fam = H.family(rng, length, [0.03])
    genomes = [[H.dna_ascii(g)] for g in fam] + [[H.dna_ascii(H.rand_dna(rng, 5000))], [b"ACGT"]]
    sk = G.HyperLogLogSketch.new(G.SeqSketcherParams(21, m, "hll"))
    got = sk.sketch_genomes(genomes)
    ref = _oracle_sketch(21, m, "hll", genomes)
    assert got.dtype == ref.dtype == np.uint16 and got.shape == (4, m)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("mode,impl", [("gather", None), ("dense", "join"), ("dense", "tile")])
def test_u16_signatures_distance_and_index(gpu_ctx, monkeypatch, mode, impl):
    """DistHamming and the HNSW build / search on u16 signatures (hll): rows are zero-extended to u32 on the device, so every count -
    tile kernel, pair kernel, row gather, match-join - equals the oracle's u16 comparison"""
    import gsearch_amd as G
    monkeypatch.setenv("GS_DIST_MODE", mode)
    if impl:
        monkeypatch.setenv("GS_DENSE_IMPL", impl)
    m = 333
    db = H.synth_sig_db(25, 40, m, 61, dtype=np.uint16, jlo=0.05, jhi=0.9)
    q = H.queries_from(db, 130, 7, frac=0.25)
    dh = G.DistHamming()
    assert np.array_equal(dh.eval_qxc(q, db), O.hamming_qxc(q, db))
    rng = np.random.default_rng(8)
    ia, ib = rng.integers(0, len(q), 150), rng.integers(0, len(db), 150)
    assert np.array_equal(dh.eval_pairs(q, db, ia, ib), O.hamming_pairs(q, db, ia, ib))
    oix = O.Index(np.uint16, m, 10, 48, seed=13)
    oix.parallel_insert(db, batch=96)
    hn = G.Hnsw.new(10, 100000, 16, 48, dh, dtype=np.uint16, seed=13, insert_batch=96)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    g, og = hn.export_graph(), oix.export()
    assert np.array_equal(g["deg0"], og["deg0"]) and np.array_equal(g["levels"], og["levels"])
    for i in range(len(db)):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]) and np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d])
    assert np.array_equal(hn.get_data(), db)
    got, want = hn.search_arrays(q, 12, 200), oix.parallel_search(q, 12, 200)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    bi, bd = hn.bruteforce_search(q[:9], 7)
    oi, od = O.bruteforce_topk(db, q[:9], 7)
    assert np.array_equal(bi, oi) and np.array_equal(bd, od)


def test_context_is_safe_for_concurrent_calls(gpu_ctx):
    """the reference clones its sketcher into --nbthreads workers and calls DistHamming / parallel_search through &self from many threads
    (dnasketch.rs:252,305,322): eight host threads hammer ONE context with sketch, distance and search calls; every result must equal the
    single-threaded one"""
    import threading
    import gsearch_amd as G
    rng = np.random.default_rng(42)
    genomes = [[H.dna_ascii(H.rand_dna(rng, 40000 + 1000 * i))] for i in range(12)]
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(21, 1024, "optdens"))
    sk2 = G.SuperHash2Sketch.new(G.SeqSketcherParams(21, 512, "super2"))
    db = H.synth_sig_db(20, 40, 128, 5, jlo=0.05, jhi=0.9)
    q = H.queries_from(db, 64, 6, frac=0.2)
    hn = G.Hnsw.new(8, 10000, 16, 40, G.DistHamming(), seed=3, insert_batch=64)
    hn.set_extend_candidates(True)
    hn.parallel_insert(db)
    dh = G.DistHamming()
    want = (sk.sketch_genomes(genomes), sk2.sketch_genomes(genomes), dh.eval_qxc(q, db), hn.search_arrays(q, 10, 100))
    errors = []

    def worker(t):
        try:
            for it in range(6):
                job = (t + it) % 4
                if job == 0:
                    assert np.array_equal(sk.sketch_genomes(genomes).view(np.uint32), want[0].view(np.uint32))
                elif job == 1:
                    assert np.array_equal(sk2.sketch_genomes(genomes), want[1])
                elif job == 2:
                    assert np.array_equal(dh.eval_qxc(q, db), want[2])
                else:
                    got = hn.search_arrays(q, 10, 100)
                    assert all(np.array_equal(a, b) for a, b in zip(got, want[3]))
        except Exception as e:            # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_worker_table_of_one_under_many_threads(gpu_ctx):
    """with the worker table full (GS_THREAD_CONTEXTS_MAX=1) every further thread evicts the least recently used worker - which used to be
    possible while that worker's thread was between worker_ctx() and its body's lock, or in worker_done(). Workers are pinned now; six threads on a
    table of one worker must finish with every sketch equal to the single-threaded one (own process: the cap is read once per process)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GS_THREAD_CONTEXTS_MAX="1")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "thread_ctx_probe.py"), "6", "10", "2", "200000"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "genomes/s" in out.stdout and "MISMATCH" not in out.stdout, out.stdout


def test_release_build_scratch_then_search_and_insert_more(gpu_ctx):
    """gs_index_release_build_scratch (round 6: what a replica of a multi-GPU request, or a server that only answers, calls after its last insert) gives
    the insert-time pair cache back. Searches are unchanged, and inserting MORE points afterwards still builds the graph an index that never
    released anything builds (pairs among the older nodes are then evaluated from their rows instead of looked up) - both equal the oracle's."""
    import gsearch_amd as G
    db = H.synth_sig_db(40, 60, 256, 77, jlo=0.05, jhi=0.95)                 # 2400 rows
    q = H.queries_from(db, 48, 78, frac=0.2)
    cut = 2048                                                               # a multiple of the insert batch: the graph depends on the batch boundaries
    hs = []
    for release in (False, True):
        hn = G.Hnsw.new(12, 10000, 16, 60, G.DistHamming(), seed=9, insert_batch=64)
        hn.set_extend_candidates(True)
        hn.parallel_insert(db[:cut])
        before = hn.search_arrays(q, 10, 120)
        if release:
            G._lib.check(hn.ctx.L.gs_index_release_build_scratch(hn.h))
            after = hn.search_arrays(q, 10, 120)
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
        hn.parallel_insert(db[cut:], ids=np.arange(cut, len(db), dtype=np.uint64))
        hs.append(hn)
    g0, g1 = hs[0].export_graph(), hs[1].export_graph()
    for key in ("levels", "deg0", "nbr0", "cnt0", "upidx"):
        assert np.array_equal(g0[key], g1[key]), key
    oix = O.Index(np.float32, db.shape[1], 12, 60, seed=9)
    oix.parallel_insert(db[:cut], batch=64); oix.parallel_insert(db[cut:], batch=64)
    og = oix.export()
    assert np.array_equal(og["deg0"], g1["deg0"]) and np.array_equal(og["nbr0"], g1["nbr0"])
    a, b = hs[0].search_arrays(q, 10, 120), hs[1].search_arrays(q, 10, 120)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_comm_allgather_single_rank(gpu_ctx):
    """C-level multi-GPU helper (gs_comm_*, RCCL): a one-rank communicator gathers the rank's own top-k block; the N > 1 exchange is the
    same call (covered for layout by the gloo world-size-2 test of the packed Python exchange)"""
    import gsearch_amd as G
    ctx = gpu_ctx
    nq, knbn = 37, 5
    ids = (np.arange(nq * knbn, dtype=np.uint64) * np.uint64(7919)).reshape(nq, knbn)
    dist = (np.arange(nq * knbn, dtype=np.float32) / np.float32(64)).reshape(nq, knbn)
    comm = G.Comm(ctx, 1, 0, G.Comm.unique_id())
    d_i, d_d, d_ai, d_ad = ctx.alloc(ids.nbytes), ctx.alloc(dist.nbytes), ctx.alloc(ids.nbytes), ctx.alloc(dist.nbytes)
    try:
        ctx.upload(d_i, ids); ctx.upload(d_d, dist)
        comm.allgather_topk_dev(d_i, d_d, nq, knbn, d_ai, d_ad)
        assert np.array_equal(ctx.download(d_ai, ids.shape, np.uint64), ids)
        assert np.array_equal(ctx.download(d_ad, dist.shape, np.float32), dist)
        assert comm.n_ranks == 1 and comm.rank == 0 and comm.size() == 1
        # the unequal-shard form: 37 rows in a block sized for 50, and an empty rank
        d_bi, d_bd = ctx.alloc(50 * knbn * 8), ctx.alloc(50 * knbn * 4)
        try:
            counts = comm.allgatherv_topk_dev(d_i, d_d, nq, 50, knbn, d_bi, d_bd)
            assert list(counts) == [nq]
            assert np.array_equal(ctx.download(d_bi, ids.shape, np.uint64), ids) and np.array_equal(ctx.download(d_bd, dist.shape, np.float32), dist)
            assert list(comm.allgatherv_topk_dev(None, None, 0, 50, knbn, d_bi, d_bd)) == [0]
            # the same exchange without the host round trip (round 6): queued on the stream, counts on the device, gs_comm_wait is the synchronising half
            d_cn = ctx.alloc(16)
            try:
                ctx.upload(d_bi, np.zeros(50 * knbn, np.uint64))
                comm.allgatherv_topk_async_dev(d_i, d_d, nq, 50, knbn, d_bi, d_bd, d_cn)
                assert list(comm.wait()) == [nq]
                assert list(ctx.download(d_cn, (2,), np.uint64)) == [nq, 0]
                assert np.array_equal(ctx.download(d_bi, ids.shape, np.uint64), ids) and np.array_equal(ctx.download(d_bd, dist.shape, np.float32), dist)
            finally:
                ctx.free(d_cn)
        finally:
            ctx.free(d_bi); ctx.free(d_bd)
    finally:
        for p_ in (d_i, d_d, d_ai, d_ad):
            ctx.free(p_)
        comm.close()


@pytest.mark.parametrize("S,nq,kin,kout", [(8, 300, 50, 50), (3, 41, 7, 10), (2, 5, 128, 20), (1, 9, 6, 6)])
def test_topk_merge_of_db_shards_on_the_device(gpu_ctx, S, nq, kin, kout):
    """the DB-sharded alternative (scripts/multiple_search.sh:71-107): every shard answers all queries, gs_topk_merge_dev keeps the best under
    (distance, id) - against the numpy k-way merge of gsearch_amd.sharding, with ties across shards, unused slots (UINT64_MAX / +inf) and local ->
    global id offsets"""
    import gsearch_amd as G
    from gsearch_amd import sharding as Sh
    ctx = gpu_ctx
    rng = np.random.default_rng(S * 1000 + nq)
    per = 100000
    ids = np.stack([np.sort(rng.choice(per, (nq, kin)), axis=1) for _ in range(S)]).astype(np.uint64)          # local ids
    dist = np.sort((rng.integers(0, 40, (S, nq, kin)) / np.float32(64)).astype(np.float32), axis=2)               # plenty of ties
    short = rng.random((S, nq)) < 0.2                                                                              # some lists hold fewer than kin answers
    for s_ in range(S):
        for q_ in np.nonzero(short[s_])[0]:
            cut = int(rng.integers(0, kin))
            ids[s_, q_, cut:] = np.uint64(0xFFFFFFFFFFFFFFFF); dist[s_, q_, cut:] = np.inf
    off = (np.arange(S, dtype=np.uint64) * np.uint64(per))
    glob = np.where(ids == np.uint64(0xFFFFFFFFFFFFFFFF), ids, ids + off[:, None, None])
    want_i, want_d = Sh.merge_topk_shards([glob[s_] for s_ in range(S)], [dist[s_] for s_ in range(S)], kout)
    d_i, d_d, d_oi, d_od = ctx.alloc(ids.nbytes), ctx.alloc(dist.nbytes), ctx.alloc(nq * kout * 8), ctx.alloc(nq * kout * 4)
    try:
        ctx.upload(d_i, ids); ctx.upload(d_d, dist)
        G.topk_merge_dev(ctx, d_i, d_d, S, nq, kin, kout, d_oi, d_od, id_offset=off)
        got_i, got_d = ctx.download(d_oi, (nq, kout), np.uint64), ctx.download(d_od, (nq, kout), np.float32)
    finally:
        for p_ in (d_i, d_d, d_oi, d_od):
            ctx.free(p_)
    if S * kin < kout:
        want_i = np.concatenate([want_i, np.full((nq, kout - S * kin), 0xFFFFFFFFFFFFFFFF, np.uint64)], axis=1)
        want_d = np.concatenate([want_d, np.full((nq, kout - S * kin), np.inf, np.float32)], axis=1)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)) and np.array_equal(got_i, want_i)


@pytest.mark.parametrize("block", [False, True])
def test_sketch_files_pipeline_matches_oracle(gpu_ctx, tmp_path, block):
    """f2 end to end: FASTA files on disk (plain, gz, bz2, xz; multi-record, CRLF, lower case, N runs, a `capsid` record, an empty
    file) -> host threads read / decode / scan -> pinned double-buffered H2D -> device filter + 2-bit pack -> sketch, in groups of 3
    files, against the oracle fed with the same records; --block concatenates the records of a file (k-mers span the joins)"""
    import bz2, gzip, lzma
    import gsearch_amd as G
    rng = np.random.default_rng(2025)

    def fasta(records, width, nl=b"\n"):
        out = []
        for name, s in records:
            out.append(b">" + name + nl)
            out += [s[o:o + width] + nl for o in range(0, len(s), width)]
        return b"".join(out)

    gs_ = [H.dna_ascii(H.rand_dna(rng, n)) for n in (60000, 45000, 30011, 52000, 70000, 41000, 38000)]
    files = [
        ("a.fna", fasta([(b"chr1 first", gs_[0][:25000] + b"NNNNNRYK" + gs_[0][25000:40000].lower()), (b"p1 phage capsid protein", gs_[0][40000:41000]), (b"chr2", gs_[0][41000:])], 60)),
        ("b.fna.gz", gzip.compress(fasta([(b"c%d" % i, gs_[1][i * 4000:(i + 1) * 4000 + 9]) for i in range(11)], 80))),
        ("c.fa.bz2", bz2.compress(fasta([(b"single", gs_[2])], 70, b"\r\n"))),
        ("d.fasta.xz", lzma.compress(fasta([(b"x", gs_[3][:26000]), (b"tiny", b"ACG"), (b"y", gs_[3][26000:])], 100))),
        ("e.fna", b""),
        ("f.fna", fasta([(b"only", gs_[4])], 61)),
        ("g.fa.gz", gzip.compress(fasta([(b"g1", gs_[5])], 60)[:20000]) + gzip.compress(fasta([(b"g1", gs_[5])], 60)[20000:])),
        ("h.fasta", fasta([(b"h", gs_[6])], 75)),
    ]
    paths = []
    for name, data in files:
        (tmp_path / name).write_bytes(data)
        paths.append(tmp_path / name)
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(21, 1500, "optdens"))
    sig, nrec, nsym, st = sk.sketch_files(paths, block=block, pio=3, threads=4)
    # oracle on the same records
    genomes = []
    for p_ in paths:
        text = G.read_fasta_file(p_)
        recs = [text[b:e] for _, b, e in G.fasta_scan(text)]
        genomes.append([b"".join(recs)] if block else recs)
    assert list(nrec) == [2, 11, 1, 3, 0, 1, 1, 1]
    ref = _oracle_sketch(21, 1500, "optdens", genomes)
    assert np.array_equal(sig.view(np.uint32), ref.view(np.uint32))
    orecs = [r for g in genomes for r in g]
    _, _, orl = O.pack_dna(orecs)
    goff = np.cumsum([0] + [len(g) for g in genomes])
    assert [int(orl[goff[i]:goff[i + 1]].sum()) for i in range(len(genomes))] == [int(x) for x in nsym]
    assert (sig[4] == 1.0).all() and st["wall_s"] > 0


def test_sketch_files_amino_acids(gpu_ctx, tmp_path):
    """.faa files: the AA alphabet filter (filter_out_non_aa, aafiles.rs:11-28) runs on the device"""
    import gzip
    import gsearch_amd as G
    rng = np.random.default_rng(77)
    prot = [H.aa_ascii(rng.integers(0, 20, n)) for n in (40000, 35000, 28000)]
    texts = [b">p1 some protein\n" + prot[0][:15000] + b"*XBZ\n" + prot[0][15000:].lower() + b"\n>p2 capsid\nMKV\n>p3\n" + prot[1][:5000] + b"\n",
             b"".join(b">q%d\n%s*\n" % (i, prot[1][i * 700:(i + 1) * 700]) for i in range(40)),
             b">r\n" + b"\n".join(prot[2][o:o + 60] for o in range(0, len(prot[2]), 60)) + b"\n"]
    paths = [tmp_path / "a.faa", tmp_path / "b.faa.gz", tmp_path / "c.faa"]
    paths[0].write_bytes(texts[0]); paths[1].write_bytes(gzip.compress(texts[1])); paths[2].write_bytes(texts[2])
    for algo in ("super2", "optdens"):
        sk = G.sketcher_for(G.SeqSketcherParams(7, 800, algo, "aa"))
        sig, nrec, nsym, _ = sk.sketch_files(paths, pio=2)
        genomes = [[t[b:e] for _, b, e in G.fasta_scan(t)] for t in texts]
        ref = _oracle_sketch(7, 800, algo, genomes, "aa")
        assert np.array_equal(_bits(sig), _bits(ref)), algo
    assert list(nrec) == [2, 40, 1]


@pytest.mark.parametrize("dtype", [np.float32, np.uint64, np.uint16])
def test_hnswrs_dump_round_trip(gpu_ctx, tmp_path, dtype):
    """f3: the database files gsearch keeps - hnswdump.hnsw.graph / hnswdump.hnsw.data in hnsw_rs' format 3 (layout recalled from the
    crate, gs_hnswio.hip) - written and read back: same graph, same vectors, same answers, and insertions continue (the `add` path)"""
    import gsearch_amd as G
    m = 150
    db = H.synth_sig_db(15, 30, m, 71, dtype=dtype, jlo=0.05, jhi=0.9)
    hn = G.Hnsw.new(12, 1_500_000, 16, 48, G.DistHamming(), dtype=dtype, seed=5, insert_batch=32)
    hn.modify_level_scale(1.0); hn.set_extend_candidates(True)
    hn.parallel_insert(db[:400])
    base = tmp_path / "hnswdump"
    hn.file_dump_hnswrs(base)
    assert (tmp_path / "hnswdump.hnsw.graph").exists() and (tmp_path / "hnswdump.hnsw.data").exists()
    # the description is readable the way reloadhnsw.rs:13-38 reads it: magic, dump mode, M, 16 layers, ef, nb_point, dimension, names
    import struct
    raw = (tmp_path / "hnswdump.hnsw.graph").read_bytes()
    magic, mode, M8, nbl, ef, npnt, dim, ln = struct.unpack_from("<IBBBQQQQ", raw, 0)
    assert (magic, mode, M8, nbl, ef, npnt, dim) == (0x002A6771, 1, 12, 16, 48, 400, m)
    o = struct.calcsize("<IBBBQQQQ")
    assert raw[o:o + ln].endswith(b"DistHamming")
    ln2, = struct.unpack_from("<Q", raw, o + ln)
    assert raw[o + ln + 8:o + ln + 8 + ln2].decode() == {np.float32: "f32", np.uint64: "u64", np.uint16: "u16"}[dtype]
    h2 = G.Hnsw.load_hnswrs(base, hint=hn)
    assert h2.get_nb_point() == 400 and h2.dtype == np.dtype(dtype)
    g1, g2 = hn.export_graph(), h2.export_graph()
    assert g1["entry"] == g2["entry"] and g1["n_upper"] == g2["n_upper"] and g1["n_upper"] > 0
    for key in ("levels", "deg0"):
        assert np.array_equal(g1[key], g2[key]), key
    for i in range(400):
        d = int(g1["deg0"][i])
        assert np.array_equal(g1["nbr0"][i, :d], g2["nbr0"][i, :d]) and np.array_equal(g1["cnt0"][i, :d], g2["cnt0"][i, :d])
    assert np.array_equal(hn.get_data(), h2.get_data())
    q = H.queries_from(db, 30, 3, frac=0.2)
    a, b = hn.search_arrays(q, 8, 60), h2.search_arrays(q, 8, 60)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    hn.parallel_insert(db[400:]); h2.parallel_insert(db[400:])
    a, b = hn.search_arrays(q, 8, 60), h2.search_arrays(q, 8, 60)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(G.GsError):
        G.Hnsw.load_hnswrs(tmp_path / "missing")


def test_hnswrs_dump_assembled_by_hand(gpu_ctx, tmp_path):
    """a three-point dump written byte by byte from the documented layout (not by this library's writer) loads and searches"""
    import struct
    import gsearch_amd as G
    m = 4
    vec = np.array([[1, 2, 3, 4], [1, 2, 3, 9], [7, 7, 7, 7]], np.float32)
    cnt = lambda a, b: int((vec[a] != vec[b]).sum())           # noqa: E731
    MAGD, MAGP, MAGL, MAGV = 0x002A6771, 0x000A678F, 0x000A676F, 0xA67F0000
    name = b"anndists::dist::distances::DistHamming"
    g = struct.pack("<IBBBQQQ", MAGD, 1, 4, 16, 10, 3, m) + struct.pack("<Q", len(name)) + name + struct.pack("<Q", 3) + b"f32" + struct.pack("<B", 16)
    # layer 0 holds points 0 and 2 (ranks 0, 1), layer 1 holds point 1 (rank 0) - the entry point
    pid = {0: (0, 0), 2: (0, 1), 1: (1, 0)}

    def point(i, lists):
        out = struct.pack("<IQBi", MAGP, i, pid[i][0], pid[i][1])
        for l in range(16):
            nb = lists.get(l, [])
            out += struct.pack("<B", len(nb))
            for j in nb:
                out += struct.pack("<QBif", j, pid[j][0], pid[j][1], cnt(i, j) / m)
        return out
    g += struct.pack("<IQ", MAGL, 2) + point(0, {0: [1, 2]}) + point(2, {0: [0, 1]})
    g += struct.pack("<IQ", MAGL, 1) + point(1, {0: [0, 2], 1: []})
    for _ in range(14):
        g += struct.pack("<IQ", MAGL, 0)
    g += struct.pack("<QBi", 1, 1, 0)
    d = struct.pack("<IQ", MAGV, m)
    for i in (0, 2, 1):
        d += struct.pack("<IQQ", MAGV, i, 4 * m) + vec[i].tobytes()
    (tmp_path / "hnswdump.hnsw.graph").write_bytes(g)
    (tmp_path / "hnswdump.hnsw.data").write_bytes(d)
    hn = G.Hnsw.load_hnswrs(tmp_path / "hnswdump")
    assert hn.get_nb_point() == 3 and np.array_equal(hn.get_data(), vec)
    ids, dist, cnt_, _ = hn.search_arrays(np.array([[1, 2, 3, 4]], np.float32), 3, 10)
    assert ids[0].tolist() == [0, 1, 2] and dist[0].tolist() == [0.0, 0.25, 1.0] and cnt_[0] == 3


def test_hnswrs_dump_of_full_m128_lists(gpu_ctx, tmp_path):
    """gsearch's own parameters (-n 128: layer 0 holds 2M = 256 ids) against the format's ONE-byte neighbour count: a graph with full
    lists is refused by the plain dump (nothing silently wrapped), dumped with GS_DUMP_TRUNCATE_255 it reloads with every such list cut
    to its 255 closest entries and everything else identical; the library's own dump stays lossless"""
    import gsearch_amd as G
    m, M = 96, 128
    db = H.synth_sig_db(6, 80, m, 9, dtype=np.uint32, jlo=0.5, jhi=0.99)               # 480 points
    built = G.Hnsw.new(M, 1_500_000, 16, 400, G.DistHamming(), dtype=np.uint32, seed=2, insert_batch=64)
    built.modify_level_scale(0.25); built.set_extend_candidates(True)
    built.parallel_insert(db)
    g0 = built.export_graph()
    # hubs with full lists (what reverse links do to popular nodes of a 300 k-genome database): nodes 0..4 get their 256 / 255 / 256 ...
    # closest other nodes as layer-0 neighbours, in the library's (count, id) order with the true counts
    for hub, deg in ((0, 256), (1, 255), (2, 256), (7, 256), (11, 254)):
        cnt = (db != db[hub]).sum(axis=1).astype(np.uint64)
        keys = np.sort(np.delete((cnt << np.uint64(32)) | np.arange(len(db), dtype=np.uint64), hub))[:deg]
        g0["deg0"][hub] = deg
        g0["nbr0"][hub, :deg] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        g0["cnt0"][hub, :deg] = (keys >> np.uint64(32)).astype(np.uint32)
    hn = G.Hnsw.new(M, 1_500_000, 16, 400, G.DistHamming(), dtype=np.uint32, seed=2, insert_batch=64)
    hn.modify_level_scale(0.25); hn.set_extend_candidates(True)
    hn.import_graph(db, g0)
    g1 = hn.export_graph()
    assert int(g1["deg0"].max()) == 2 * M
    with pytest.raises(G.GsError) as e:
        hn.file_dump_hnswrs(tmp_path / "plain")
    assert e.value.code == -3 and "one byte" in str(e.value)
    hn.file_dump_hnswrs(tmp_path / "hnswdump", truncate_255=True)
    h2 = G.Hnsw.load_hnswrs(tmp_path / "hnswdump", hint=hn)
    g2 = h2.export_graph()
    assert np.array_equal(g2["deg0"], np.minimum(g1["deg0"], 255)) and np.array_equal(g1["levels"], g2["levels"]) and g1["entry"] == g2["entry"]
    for i in range(len(db)):
        d = int(g2["deg0"][i])
        assert np.array_equal(g1["nbr0"][i, :d], g2["nbr0"][i, :d]) and np.array_equal(g1["cnt0"][i, :d], g2["cnt0"][i, :d])
    assert np.array_equal(hn.get_data(), h2.get_data())
    hn.file_dump(tmp_path / "own.gsix")
    h3 = G.Hnsw.load(tmp_path / "own.gsix")
    g3 = h3.export_graph()
    assert np.array_equal(g1["deg0"], g3["deg0"]) and np.array_equal(g1["nbr0"], g3["nbr0"])


def test_hnswrs_dump_sizes_against_the_readme_sample(gpu_ctx, tmp_path):
    """The only reference-held datum that touches the dump layout: README.md:164-168 lists the sample database (README.md:69: -k 16
    -s 18000 -n 128 optdens, i.e. 18000 f32 per vector; its parameters.json is the 180-byte KAT of test_state_json) at 9.7G for
    hnswdump.hnsw.data and 58M for hnswdump.hnsw.graph (`ls -lh`: powers of 1024, rounded UP to one decimal). The per-vector and
    per-neighbour byte costs are taken from files THIS writer produces (two dumps, linear fit - not from the layout comment); the sample's
    sizes must then be explained by an integer number of genomes and a mean degree a -n 128 graph can have."""
    import gsearch_amd as G
    m = 40

    def dump(n, M, tag):
        db = H.synth_sig_db(8, (n + 7) // 8, m, 13, jlo=0.1, jhi=0.9)[:n]
        hn = G.Hnsw.new(M, 1_500_000, 16, 64, G.DistHamming(), seed=11, insert_batch=32)
        hn.modify_level_scale(0.5); hn.set_extend_candidates(True)
        hn.parallel_insert(db)
        hn.file_dump_hnswrs(tmp_path / tag)
        g = hn.export_graph()
        links = int(g["deg0"].sum()) + int(g["degU"].sum())
        return n, links, os.path.getsize(tmp_path / (tag + ".hnsw.data")), os.path.getsize(tmp_path / (tag + ".hnsw.graph"))
    (n1, l1, d1, gr1), (n2, l2, d2, gr2), (n3, l3, d3, gr3) = dump(200, 8, "a"), dump(330, 8, "b"), dump(330, 16, "c")
    # data file = fixed + n * (header + 4 * m)
    per_vec = (d2 - d1) // (n2 - n1)
    assert (d2 - d1) % (n2 - n1) == 0 and per_vec > 4 * m
    fixed_d, hdr = d1 - n1 * per_vec, per_vec - 4 * m
    assert fixed_d == d3 - n3 * per_vec and 0 < fixed_d < 64 and 0 < hdr < 64
    # graph file = fixed + n * per_point + links * per_link: three dumps, three unknowns
    A = np.array([[1, n1, l1], [1, n2, l2], [1, n3, l3]], float)
    fixed_g, per_point, per_link = np.linalg.solve(A, np.array([gr1, gr2, gr3], float))
    assert abs(per_point - round(per_point)) < 1e-6 and abs(per_link - round(per_link)) < 1e-6 and 8 < per_link < 40 and 16 < per_point < 80
    per_point, per_link = round(per_point), round(per_link)
    GiB, MiB = 1 << 30, 1 << 20
    row = hdr + 4 * 18000
    n_lo, n_hi = int(9.6 * GiB - fixed_d) // row + 1, int(9.7 * GiB - fixed_d) // row            # 9.6G < size <= 9.7G
    assert n_lo <= n_hi and 100_000 <= n_lo and n_hi < 1_000_000, (n_lo, n_hi)     # a 6-digit genome count: the sample's processing_state.json is 55 bytes, {"nb_seq":NNNNNN,"nb_file":NNNNNN,"elapsed_t":...}
    deg_lo = ((57 * MiB - fixed_g) / n_hi - per_point) / per_link                      # 57M < size <= 58M
    deg_hi = ((58 * MiB - fixed_g) / n_lo - per_point) / per_link
    assert 1.0 < deg_lo < deg_hi < 2 * 128, (deg_lo, deg_hi)
    print("README sample explained by %d..%d genomes with %.1f..%.1f links per node (vector record %d + 72000 B, point %d B, link %d B)" %
          (n_lo, n_hi, deg_lo, deg_hi, hdr, per_point, per_link))


def test_config0_tohnsw_then_request_end_to_end(gpu_ctx):
    """BASELINE configs[0], the reference's own CPU-runnable case, on the HIP path end to end: `tohnsw` on 1000 synthetic 1 Mbp DNA genomes
    (10 roots x 100 mutants), k=21 s=12000 --algo optdens, -n 128 --ef 1600 --scale_modify_f 0.25, then `request` with 100 queries, n=50,
    ef_search=5000 (gsearch.rs:893). Sketch bits, graph, neighbour ids / distances / evaluation counts == oracle; recall@50 == CPU == 1
    against exhaustive search; the answers formatted like ReqAnswer::dump (answer.rs:45-71) agree between both sides."""
    import gsearch_amd as G
    N, NQ, L, k, m, M, efc, ef, knbn, B = 1000, 100, 1_000_000, 21, 12000, 128, 1600, 5000, 50, 64
    rng = np.random.default_rng(1)
    roots = [H.rand_dna(rng, L) for _ in range(10)]
    mus = [0.001, 0.005, 0.01, 0.02, 0.05, 0.10]
    genomes = [[H.dna_ascii(H.mutate(rng, roots[i % 10], mus[(i // 10) % 6]))] for i in range(N)]
    queries = [[H.dna_ascii(H.mutate(rng, roots[i % 10], 0.01))] for i in range(NQ)]
    cores = os.cpu_count()
    # CPU side (oracle)
    seq, rs, rl = O.pack_dna([g[0] for g in genomes])
    osig = O.sketch_batch(O.params(k, m, "optdens"), seq, rs, rl, np.arange(N + 1, dtype=np.uint64), nthreads=cores)
    oix = O.Index(np.float32, m, M, efc, scale_modify=0.25, seed=7)
    oix.parallel_insert(osig, batch=B)
    qseq, qrs, qrl = O.pack_dna([q[0] for q in queries])
    oq = O.sketch_batch(O.params(k, m, "optdens"), qseq, qrs, qrl, np.arange(NQ + 1, dtype=np.uint64), nthreads=cores)
    oids, odist, ocnt, oev = oix.parallel_search(oq, knbn, ef, nthreads=cores)
    # HIP side
    sk = G.OptDensHashSketch.new(G.SeqSketcherParams(k, m, "optdens"))
    gsig = sk.sketch_genomes(genomes)
    assert gsig.dtype == np.float32 and np.array_equal(gsig.view(np.uint32), osig.view(np.uint32))
    hn = G.Hnsw.new(M, 1_500_000, 16, efc, G.DistHamming(), seed=7, insert_batch=B)
    hn.modify_level_scale(0.25); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
    hn.parallel_insert(gsig)
    g, og = hn.export_graph(), oix.export()
    assert g["entry"] == og["entry"] and np.array_equal(g["levels"], og["levels"]) and np.array_equal(g["deg0"], og["deg0"])
    for i in range(N):
        d = int(og["deg0"][i])
        assert np.array_equal(g["nbr0"][i, :d], og["nbr0"][i, :d]) and np.array_equal(g["cnt0"][i, :d], og["cnt0"][i, :d]), i
    gq = sk.sketch_genomes(queries)
    assert np.array_equal(gq.view(np.uint32), oq.view(np.uint32))
    ids, dist, cnt, ev = hn.search_arrays(gq, knbn, ef)
    assert np.array_equal(ids, oids) and np.array_equal(dist.view(np.uint32), odist.view(np.uint32)) and np.array_equal(cnt, ocnt) and np.array_equal(ev, oev)
    bi, bd = O.bruteforce_topk(osig, oq, knbn, nthreads=cores)
    rec = float(np.mean([(dist[i] <= bd[i, -1]).mean() for i in range(NQ)]))
    assert rec == 1.0
    # every query's best hits are its own root's family (ids i % 10 == root), nearest first
    assert all(int(ids[i, 0]) % 10 == i % 10 for i in range(NQ)) and (np.diff(dist, axis=1) >= 0).all()
    assert abs(G.ani(float(dist[0][0]), k, 1) - O.ani(float(dist[0][0]), k, 1)) < 1e-6
