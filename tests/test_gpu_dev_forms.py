"""Device-resident entry points that are a few lines over a core their host twins share: one comparison each with the host twin (or, for
the synthetic-input generators, with the formula include/gsearch_amd.h states), on inputs uploaded with Context.alloc / upload."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _index(G, M=8, efc=40, scale=1.0, seed=21):
    hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(), seed=seed, insert_batch=64)
    hn.modify_level_scale(scale); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
    return hn


def test_search_pid_dev_equals_host(gpu_ctx):
    """gs_index_parallel_search_pid_dev: ids, distances, counts, evaluations and both PointId parts of search_arrays_pid"""
    import gsearch_amd as G
    ctx, m, knbn, ef = gpu_ctx, 128, 10, 60
    db = H.synth_sig_db(8, 60, m, 5, jlo=0.2, jhi=0.95)
    n = len(db)
    ids = (10_000_000_000 + 7 * np.random.default_rng(1).permutation(n)).astype(np.uint64)
    hn = _index(G)
    hn.parallel_insert(db, ids=ids)
    q = H.queries_from(db, 41, 9, frac=0.2)
    want = hn.search_arrays_pid(q, knbn, ef)
    assert (want[4] > 0).any() and (want[2] > 0).all()                       # upper layers exist: PointIds are not all (0, i)
    nq = len(q)
    shapes = [((nq, knbn), np.uint64), ((nq, knbn), np.float32), ((nq,), np.uint32), ((nq,), np.uint64), ((nq, knbn), np.uint8), ((nq, knbn), np.int32)]
    d_q = ctx.alloc(q.nbytes)
    outs = [ctx.alloc(int(np.prod(s)) * np.dtype(t).itemsize) for s, t in shapes]
    try:
        ctx.upload(d_q, q)
        for p, (s, t) in zip(outs, shapes):
            ctx.memset(p, 0xC5, int(np.prod(s)) * np.dtype(t).itemsize)
        G._lib.check(ctx.L.gs_index_parallel_search_pid_dev(hn.h, d_q, nq, knbn, ef, *outs))
        ctx.sync()
        got = [ctx.download(p, s, t) for p, (s, t) in zip(outs, shapes)]
    finally:
        for p in [d_q] + outs:
            ctx.free(p)
    for name, a, b in zip(("ids", "dist", "count", "evals", "pid_layer", "pid_rank"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def test_insert_ids_dev_equals_host(gpu_ctx):
    """gs_index_parallel_insert_ids_dev: an index built from device-resident signatures with the caller's ids (two calls, the second after
    implicit ids) has the graph, the ids and the answers of one built from the host with parallel_insert"""
    import gsearch_amd as G
    ctx, m = gpu_ctx, 128
    db = H.synth_sig_db(8, 60, m, 5, jlo=0.2, jhi=0.95)
    n, split = len(db), 100
    ids = np.arange(n, dtype=np.uint64)
    ids[split:] = (10_000_000_000 + 7 * np.random.default_rng(1).permutation(n - split)).astype(np.uint64)      # beyond 2^32, not monotone
    host = _index(G)
    host.parallel_insert(db[:split])
    host.parallel_insert([(db[i], int(ids[i])) for i in range(split, n)])
    dev = _index(G)
    dev._ensure(m)
    d_db = ctx.alloc(db.nbytes)
    try:
        ctx.upload(d_db, db)
        G._lib.check(ctx.L.gs_index_parallel_insert_dev(dev.h, d_db, split))
        tail = np.ascontiguousarray(ids[split:])
        G._lib.check(ctx.L.gs_index_parallel_insert_ids_dev(dev.h, d_db + split * m * 4, _p(tail), n - split))
        ctx.sync()
    finally:
        ctx.free(d_db)
    assert dev.get_nb_point() == n and np.array_equal(dev.get_ids(), ids) and np.array_equal(host.get_ids(), ids)
    gh, gd = host.export_graph(), dev.export_graph()
    assert (gh["levels"] > 0).any() and set(gh) == set(gd)
    for key in gh:
        assert np.array_equal(gh[key], gd[key]), key
    assert np.array_equal(dev.get_data(), db)
    assert dev.insert_evals() == host.insert_evals() > 0                    # (gs_index_insert_evals: the same work was spent)
    q = H.queries_from(db, 40, 9, frac=0.2)
    for a, b in zip(dev.search_arrays_pid(q, 10, 60), host.search_arrays_pid(q, 10, 60)):
        assert np.array_equal(a, b)
    assert set(np.unique(dev.search_arrays(q, 10, 60)[0])) <= set(ids.tolist())


def test_filter_aa_dev_equals_host(gpu_ctx):
    """gs_filter_aa_dev: residues and record coordinates of filter_aa_records on text with lower case, '*', 'X', digits, CRLF, an empty
    record and a record longer than one device chunk"""
    import gsearch_amd as G
    ctx = gpu_ctx
    rng = np.random.default_rng(3)
    long = bytearray(H.aa_ascii(rng.integers(0, 20, 150_000)))
    odd = b"*Xx\n\r-1bjouzBJOUZ "
    for pos in rng.integers(0, len(long), 3000):
        long[pos] = odd[int(rng.integers(0, len(odd)))]
    recs = [b"MKV*LLxz\r\nacdef\r\n", b"", b"mkvXX*ab12 34\nWY\n", b"\n\r\n", bytes(long), b"*X9", b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwy",
            bytes(range(256))]
    want_seq, want_start, want_len = G.filter_aa_records(recs)
    total = int(want_len.sum())
    assert total > 140_000 and want_len[1] == 0 and want_len[3] == 0 and want_len[5] == 0
    # the records inside one text, with bytes between them that belong to no record
    text, beg, end = b"", [], []
    for r in recs:
        text += b">h\n"
        beg.append(len(text)); text += r; end.append(len(text))
    beg, end = np.array(beg, np.uint64), np.array(end, np.uint64)
    start, ln = np.full(len(recs), M64, np.uint64), np.full(len(recs), M64, np.uint64)
    d_text, d_out = ctx.alloc(len(text) + 64), ctx.alloc(len(text) + 64)
    try:
        ctx.upload(d_text, np.frombuffer(text, np.uint8))
        ctx.memset(d_out, 0xC5, len(text) + 64)
        G._lib.check(ctx.L.gs_filter_aa_dev(ctx.h, d_text, len(text), _p(beg), _p(end), len(recs), d_out, _p(start), _p(ln)))
        ctx.sync()
        out = ctx.download(d_out, (len(text) + 64,), np.uint8)
    finally:
        ctx.free(d_text); ctx.free(d_out)
    assert np.array_equal(ln, want_len) and np.array_equal(start, want_start)
    assert bytes(out[:total]) == bytes(want_seq[:total]) and (out[total:] == 0xC5).all()


@pytest.mark.parametrize("dtype", [np.float32, np.uint32, np.uint64, np.uint16])
def test_hamming_qxc_dev_equals_host(gpu_ctx, dtype):
    """gs_hamming_qxc_dev on uploaded signatures: the matrix of DistHamming.eval_qxc, which is count(a != b) / m"""
    import gsearch_amd as G
    ctx, m = gpu_ctx, 333
    db = H.synth_sig_db(5, 29, m, 17, dtype=dtype)
    q = H.queries_from(db, 37, 3, frac=0.3)
    want = G.DistHamming().eval_qxc(q, db)
    assert np.array_equal(want, ((q[:, None, :] != db[None, :, :]).sum(axis=2).astype(np.float32) / np.float32(m)))
    d_q, d_c, d_o = ctx.alloc(q.nbytes), ctx.alloc(db.nbytes), ctx.alloc(4 * len(q) * len(db))
    try:
        ctx.upload(d_q, q); ctx.upload(d_c, db)
        ctx.memset(d_o, 0xC5, 4 * len(q) * len(db))
        G._lib.check(ctx.L.gs_hamming_qxc_dev(ctx.h, G.api.DTYPE_KIND[np.dtype(dtype)], m, d_q, len(q), d_c, len(db), d_o))
        ctx.sync()
        got = ctx.download(d_o, (len(q), len(db)), np.float32)
    finally:
        for p in (d_q, d_c, d_o):
            ctx.free(p)
    assert np.array_equal(got, want)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _synth_words(seed, genomes, n_words):
    """include/gsearch_amd.h: word w of genome g = splitmix64 finaliser of (seed * 0x9e3779b97f4a7c15 + g * 0xbf58476d1ce4e5b9 + w)"""
    with np.errstate(over="ignore"):
        base = np.uint64((seed * 0x9E3779B97F4A7C15) & M64) + np.asarray(genomes, np.uint64) * np.uint64(0xBF58476D1CE4E5B9)
        return _mix(base[:, None] + np.arange(n_words, dtype=np.uint64)[None, :])


def test_synth_aa_dev_matches_its_formula(gpu_ctx):
    """gs_synth_aa_dev: residue j of word w of proteome g = "ACDEFGHIKLMNPQRSTVWY"[byte j of the synth word of (seed ^ 0xAA5EED, g, w) mod 20],
    ceil(L / 8) words per proteome"""
    import gsearch_amd as G
    ctx, seed, g0, ng, L = gpu_ctx, 20240607, 3_000_000_007, 37, 1003
    wp = (L + 7) // 8
    d = ctx.alloc(ng * wp * 8 + 64)
    try:
        ctx.memset(d, 0xC5, ng * wp * 8 + 64)
        G._lib.check(ctx.L.gs_synth_aa_dev(ctx.h, seed, g0, ng, L, d))
        ctx.sync()
        got = ctx.download(d, (ng * wp * 8 + 64,), np.uint8)
    finally:
        ctx.free(d)
    words = _synth_words(seed ^ 0xAA5EED, g0 + np.arange(ng), wp)
    want = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)[words.astype("<u8").view(np.uint8).reshape(-1) % 20]
    assert np.array_equal(got[:ng * wp * 8], want) and (got[ng * wp * 8:] == 0xC5).all()
    assert len(np.unique(got[:ng * wp * 8])) == 20


def _bases(words):
    """packed words (8 bytes little endian as stored, base j of a byte at bits 6 - 2j) -> (rows, 32 * words) base codes"""
    b = np.ascontiguousarray(words).astype("<u8").view(np.uint8).reshape(words.shape[0], -1)
    return np.stack([(b >> s) & 3 for s in (6, 4, 2, 0)], axis=2).reshape(words.shape[0], -1)


def test_synth_dna_family_skew_dev(gpu_ctx):
    """gs_synth_dna_family_skew_dev: without substitutions every genome IS its root genome (gs_synth_dna_dev of seed ^ 0x5DEECE66D, tested in
    test_gpu_hmh.py against its formula), the root being floor(n_roots u^alpha) of the header's hash u; with alpha = 0 the call is
    gs_synth_dna_family_dev; with substitutions at rate mu a genome differs from its root in a fraction mu of its bases"""
    import gsearch_amd as G
    ctx, seed, g0, ng, L, n_roots, alpha = gpu_ctx, 991, 5_000_000_000, 3000, 1000, 50, 3.5
    wp = (L + 31) // 32
    d_fam, d_root = ctx.alloc(ng * wp * 8), ctx.alloc(n_roots * wp * 8)

    def family(mu_lo, mu_hi, a, skew=True):
        ctx.memset(d_fam, 0xC5, ng * wp * 8)
        if skew:
            G._lib.check(ctx.L.gs_synth_dna_family_skew_dev(ctx.h, seed, g0, ng, L, n_roots, mu_lo, mu_hi, a, d_fam))
        else:
            G._lib.check(ctx.L.gs_synth_dna_family_dev(ctx.h, seed, g0, ng, L, n_roots, mu_lo, mu_hi, d_fam))
        ctx.sync()
        return ctx.download(d_fam, (ng, wp), np.uint64)

    try:
        G._lib.check(ctx.L.gs_synth_dna_dev(ctx.h, seed ^ 0x5DEECE66D, 0, n_roots, L, d_root))
        ctx.sync()
        roots = ctx.download(d_root, (n_roots, wp), np.uint64)
        exact = family(0.0, 0.0, alpha)
        mutated = family(0.05, 0.05, alpha)
        uniform = family(0.001, 0.08, 0.0)
        uniform_twin = family(0.001, 0.08, 0.0, skew=False)
    finally:
        ctx.free(d_fam); ctx.free(d_root)
    assert len(np.unique(roots, axis=0)) == n_roots
    with np.errstate(over="ignore"):
        g = g0 + np.arange(ng, dtype=np.uint64)
        h = _mix(np.uint64(seed * 31) + g * np.uint64(0xA24BAED4963EE407) + np.uint64(3))
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    root_of = np.minimum(np.floor(n_roots * u ** alpha).astype(np.int64), n_roots - 1)
    assert np.array_equal(exact, roots[root_of])
    sizes = np.bincount(root_of, minlength=n_roots)
    assert sizes[0] == sizes.max() and abs(sizes[0] / ng - n_roots ** (-1 / alpha)) < 0.05          # root 0 holds n_roots^(-1/alpha) of everything
    diff = (_bases(mutated) != _bases(exact))[:, :L].mean(axis=1)
    assert abs(diff.mean() - 0.05) < 0.002 and diff.min() > 0.01 and diff.max() < 0.1
    assert not (_bases(mutated)[:, L:] != 0).any()                                                  # bits past the end stay zero
    assert np.array_equal(uniform, uniform_twin)
    assert np.array_equal(np.unique(np.argmin((_bases(uniform)[:, None, :64] != _bases(roots)[None, :, :64]).sum(axis=2), axis=1)), np.arange(n_roots))
