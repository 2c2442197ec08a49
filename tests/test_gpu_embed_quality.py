"""The quality of an embedding on the device (gs_embq.hip, SPEC.md 8.1): every word of rank, e2, rad2, the histogram and the summary must equal the numpy
restatement tests/pyref_embed_quality.py over the case table of tests/embed_quality_cases.py, on clean and on poisoned memory; host form, device form
and index form are held to each other; every refusal returns its code; and end to end the measure prefers an embedding to the positions it started from."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import embed_quality_cases as K
import helpers as H
import pyref_embed_quality as R

pytestmark = pytest.mark.gpu

FILLS = [None, 0x00, 0xFF]
BY_NAME = {c[0]: c for c in K.CASES}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


INTS = ("n", "knbn", "kq_eff", "n_rows", "n_edges", "n_conserved", "n_nomatch")
FLOATS = ("mean_conserved", "frac_conserved")
ARRAYS = ("hist_conserved", "q_edge", "q_radius", "q_ratio")


def _check(got, ref, arrays=True):
    for key in INTS:
        assert got[key] == ref[key], key
    for key in FLOATS:
        assert np.float64(got[key]).view(np.uint64) == np.float64(ref[key]).view(np.uint64), (key, got[key], ref[key])
    for key in ARRAYS + (("rank", "e2", "rad2") if arrays else ()):
        assert _same(got[key], ref[key]), key


@functools.lru_cache(maxsize=None)
def _case(name):
    ids, dist, cnt, pos, kq = K.make(BY_NAME[name])
    return ids, dist, cnt, pos, kq, R.quality(ids, dist, cnt, pos, kq)


@pytest.fixture
def fill():
    import gsearch_amd as G

    def set_fill(byte):
        G.debug_mem_fill(byte)
    yield set_fill
    G.debug_mem_fill(None)


def test_tile_sizes_are_the_tables(gpu_ctx):
    import gsearch_amd as G
    assert (G.EMBQ_TILE_Q, G.EMBQ_TILE_P) == (K.TILE_Q, K.TILE_P) and R.DIM_MAX == 4


@pytest.mark.parametrize("name", [c[0] for c in K.CASES])
def test_host_form_equals_the_restatement(gpu_ctx, fill, name):
    import gsearch_amd as G
    ids, dist, cnt, pos, kq, ref = _case(name)
    for byte in FILLS:
        fill(byte)
        _check(G.embed_quality(ids, dist, cnt, pos, kq, return_arrays=True), ref)


@pytest.mark.parametrize("name", [c[0] for c in K.KNOB_CASES])
def test_blocks_of_rows_and_of_points(gpu_ctx, fill, monkeypatch, name):
    """257 nodes in launches of at most 100 rows against at most 100 points: three blocks of each, the counts of the point blocks added up"""
    import gsearch_amd as G
    ids, dist, cnt, pos, kq, ref = _case(name)
    monkeypatch.setenv("GS_EMBQ_MAXQ", "100")
    monkeypatch.setenv("GS_EMBQ_MAXP", "100")
    for byte in FILLS:
        fill(byte)
        _check(G.embed_quality(ids, dist, cnt, pos, kq, return_arrays=True), ref)
    monkeypatch.setenv("GS_EMBQ_MAXQ", "64")                   # blocks that are no multiple of anything: 5 of rows, 37 of points
    monkeypatch.setenv("GS_EMBQ_MAXP", "7")
    fill(0xFF)
    _check(G.embed_quality(ids, dist, cnt, pos, kq, return_arrays=True), ref)


@pytest.mark.parametrize("name", ["gauss-n1025-d1-kq200-k8", "lattice-n257-d3-kq8-k8", "clumps-n257-d4-kq256-k1", "negzero-n257-d2-kq2-k17"])
def test_device_form_and_optional_outputs(gpu_ctx, fill, name):
    import gsearch_amd as G
    ctx = gpu_ctx
    ids, dist, cnt, pos, kq, ref = _case(name)
    n, k = ids.shape
    dim = pos.shape[1]
    bufs = [ctx.alloc(x.nbytes) for x in (ids, dist, cnt, pos)]
    drank, de2, drad = ctx.alloc(4 * n * k), ctx.alloc(4 * n * k), ctx.alloc(4 * n)
    shapes = ((drank, (n, k), np.uint32, "rank"), (de2, (n, k), np.float32, "e2"), (drad, (n,), np.float32, "rad2"))
    try:
        for b, x in zip(bufs, (ids, dist, cnt, pos)):
            ctx.upload(b, x)
        for byte in FILLS:
            fill(byte)
            for p, shape, dt, _ in shapes:
                ctx.memset(p, 0xA5, int(np.prod(shape)) * 4)
            G.embed_quality_dev(ctx, n, k, *bufs, dim, kq, drank, de2, drad)
            for p, shape, dt, key in shapes:
                assert _same(ctx.download(p, shape, dt), ref[key]), key
            # one output at a time: the pre-filled others stay as they are
            for want in range(3):
                for p, shape, dt, _ in shapes:
                    ctx.memset(p, 0x5A, int(np.prod(shape)) * 4)
                G.embed_quality_dev(ctx, n, k, *bufs, dim, kq, *[s[0] if j == want else None for j, s in enumerate(shapes)])
                for j, (p, shape, dt, key) in enumerate(shapes):
                    got = ctx.download(p, shape, dt)
                    assert _same(got, ref[key]) if j == want else (got.view(np.uint8) == 0x5A).all(), (want, key)
    finally:
        for b in bufs + [drank, de2, drad]:
            ctx.free(b)
    # the host form without its optional outputs: the summary alone
    s = G._lib.EmbedQualityC()
    G._lib.check(ctx.L.gs_embed_quality(ctx.h, n, k, ids.ctypes.data, dist.ctypes.data, cnt.ctypes.data, pos.ctypes.data, dim, kq, C.byref(s), None, None, None, None))
    assert (s.n_rows, s.n_edges, s.n_conserved, s.n_nomatch, s.kq_eff) == tuple(ref[x] for x in ("n_rows", "n_edges", "n_conserved", "n_nomatch", "kq_eff"))
    assert _same(np.array(s.q_ratio[:]), ref["q_ratio"])
    _check(G.embed_quality(ids, dist, cnt, pos, kq), ref, arrays=False)


def test_stage_times_of_the_last_call(gpu_ctx):
    import gsearch_amd as G
    ids, dist, cnt, pos, kq, ref = _case("gauss-n1025-d1-kq200-k8")
    G.embed_quality(ids, dist, cnt, pos, kq)
    ms = G.embed_quality_last_ms(gpu_ctx)
    assert len(ms["radius"]) == 16 and all(0 < t < 1000 for t in [ms["edge"], ms["rank"], ms["finish"]] + ms["radius"]) and 0 <= ms["summary"] < 1000
    assert gpu_ctx.L.gs_embed_quality_last_ms(gpu_ctx.h, None) == G._lib.GS_ERR_INVALID


def _index(G, db, M=8):
    n = len(db)
    hn = G.Hnsw.new(M, max(n, 1024), 16, 40, G.DistHamming(), dtype=db.dtype)
    hn.import_graph(db, dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32),
                             cnt0=np.zeros((n, 2 * M), np.uint32), upidx=np.full(n, -1, np.int32), n_upper=0))
    return hn


@pytest.mark.parametrize("dim,knbn,kq,max_dist", [(2, 8, 200, 1.0), (3, 17, 5, 1.0), (1, 8, 29, 0.6)])
def test_index_form_equals_host_form_and_restatement(gpu_ctx, fill, dim, knbn, kq, max_dist):
    """planted families at m = 256: the index builds its own exact graph; the same graph through the host form and through numpy"""
    import gsearch_amd as G
    db = H.synth_sig_db(10, 30, 256, 17, jlo=0.4, jhi=0.99)
    hn = _index(G, db)
    n = len(db)
    ids, dist, cnt = hn.knn_graph(knbn, max_dist)
    if max_dist < 1.0:
        assert (cnt < knbn).any() and (cnt > 0).any()
    pos = np.random.default_rng(dim).normal(0, 1, (n, dim)).astype(np.float32)
    ref = R.quality(ids, dist, cnt, pos, kq)
    for byte in FILLS:
        fill(byte)
        got = hn.embed_quality(pos, knbn, kq, max_dist, return_arrays=True)
        _check(got, ref)
        _check(G.embed_quality(ids, dist, cnt, pos, kq, return_arrays=True), ref)


def test_refusals(gpu_ctx):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_STATE, GS_ERR_UNSUPPORTED
    ctx = gpu_ctx
    n, k = 50, 4
    ids, dist, cnt = np.zeros((n, k), np.uint64), np.zeros((n, k), np.float32), np.full(n, k, np.uint32)
    for i in range(n):
        nb = np.random.default_rng(i).choice(n - 1, k, replace=False)
        ids[i] = nb + (nb >= i)
        dist[i] = np.sort(np.random.default_rng(i).integers(0, 4096, k) * np.float32(2.0 ** -12))
    pos = K.positions("gauss", n, 2, 5)
    assert not R.refusals(ids, dist, cnt, pos, 3)

    def code(f, *a, **kw):
        with pytest.raises(G.GsError) as e:
            f(*a, **kw)
        return e.value.code

    def dev(i, d, c, p, kq):
        bufs = [ctx.alloc(max(x.nbytes, 16)) for x in (i, d, c, p)]
        out = ctx.alloc(4 * max(len(i), 1))
        try:
            for b, x in zip(bufs, (i, d, c, p)):
                if x.nbytes:
                    ctx.upload(b, x)
            G.embed_quality_dev(ctx, len(i), i.shape[1], *bufs, p.shape[1], kq, None, None, out)
        finally:
            for b in bufs + [out]:
                ctx.free(b)

    def both(i, d, c, p, kq):
        assert R.refusals(i, d, c, p, kq)
        a, b = code(G.embed_quality, i, d, c, p, kq), code(dev, i, d, c, p, kq)
        assert a == b
        return a
    assert both(ids[:1], dist[:1], cnt[:1] * 0, pos[:1], 3) == GS_ERR_INVALID                  # n = 1
    assert both(ids, dist, cnt, pos, 0) == GS_ERR_INVALID                                      # kq = 0
    for v in (np.nan, np.inf, -np.inf):
        p = pos.copy()
        p[n - 1, 1] = v
        assert both(ids, dist, cnt, p, 3) == GS_ERR_INVALID
    assert both(ids, dist, cnt, np.zeros((n, 0), np.float32), 3) == GS_ERR_INVALID             # dim = 0
    assert both(ids, dist, cnt, np.zeros((n, R.DIM_MAX + 1), np.float32), 3) == GS_ERR_INVALID
    graph_cases = [lambda i, d, c: i.__setitem__((3, 1), n),               # id >= n
                   lambda i, d, c: i.__setitem__((3, 1), 3),               # own node
                   lambda i, d, c: i.__setitem__((3, 1), i[3, 0]),         # repeat
                   lambda i, d, c: d.__setitem__((3, 2), np.nan),
                   lambda i, d, c: d.__setitem__((3, 0), -0.5),
                   lambda i, d, c: d.__setitem__((3, 3), d[3, 2] / 2 if d[3, 2] > 0 else -1.0),   # descending
                   lambda i, d, c: c.__setitem__(3, k + 1)]                # count > knbn
    for mod in graph_cases:
        i, d, c = ids.copy(), dist.copy(), cnt.copy()
        mod(i, d, c)
        assert both(i, d, c, pos, 3) == GS_ERR_INVALID
    assert G.embed_quality(ids, dist, cnt, pos, 3)["n_edges"] == n * k                         # and the unbroken call goes through
    # the index form: the same codes, an empty index, signatures too long for the count matrix
    db = H.synth_sig_db(5, 10, 256, 3)
    hn = _index(G, db)
    assert code(hn.embed_quality, pos, 4, 0) == GS_ERR_INVALID
    p = pos.copy()
    p[0, 0] = np.nan
    assert code(hn.embed_quality, p, 4, 3) == GS_ERR_INVALID
    assert code(hn.embed_quality, np.zeros((n, 5), np.float32), 4, 3) == GS_ERR_INVALID
    assert code(hn.embed_quality, pos[:-1], 4, 3) == GS_ERR_INVALID                            # not one position per node
    empty = G.Hnsw.new(8, 1000, 16, 40, G.DistHamming())
    assert code(empty.embed_quality, pos) == GS_ERR_STATE
    empty._ensure(32)
    assert code(empty.embed_quality, np.zeros((0, 2), np.float32)) == GS_ERR_STATE
    big = _index(G, np.zeros((4, 70000), np.float32))
    assert code(big.embed_quality, np.zeros((4, 2), np.float32), 2) == GS_ERR_UNSUPPORTED


def test_end_to_end_the_embedding_beats_its_start(gpu_ctx, tmp_path):
    """20 families x 20 at m = 256, kq = 19"""
    import gsearch_amd as G
    db = H.synth_sig_db(20, 20, 256, 29, jlo=0.4, jhi=0.99)
    hn = _index(G, db)
    n, kq = len(db), 19
    prm = G.EmbedParams()
    start = hn.embed(params=G.EmbedParams(epochs=0))
    xy = hn.embed(params=prm)
    q0, q1 = hn.embed_quality(start, kq=kq), hn.embed_quality(xy, kq=kq)
    print("seeded positions: frac_conserved %.4f (chance %.4f); after %d epochs: %.4f, %d rows without a match"
          % (q0["frac_conserved"], kq / (n - 1), prm.epochs, q1["frac_conserved"], q1["n_nomatch"]))
    assert q1["frac_conserved"] > q0["frac_conserved"]
    assert q0["frac_conserved"] <= 1.5 * kq / (n - 1)
    ids, dist, cnt = hn.knn_graph(8)
    _check(q1, R.quality(ids, dist, cnt, xy, kq), arrays=False)
    # ann: the report is embed_quality_text of the same summary, byte for byte
    out, csv = io.StringIO(), str(tmp_path / "with.csv")
    res = G.ann(hn, stats=False, embed=True, params=prm, csv_path=csv, out=out, quality=kq)
    assert sorted(res) == ["embedding", "quality", "stats"] and _same(res["embedding"], xy)
    _check(res["quality"], q1, arrays=False)
    assert out.getvalue() == G.embed_quality_text(q1) == R.text(q1) and out.getvalue().count("\n") == 7
    # without `quality`: the dictionary, the text and the file of before
    out2, csv2, csv3 = io.StringIO(), str(tmp_path / "without.csv"), str(tmp_path / "direct.csv")
    res2 = G.ann(hn, stats=True, embed=True, params=prm, csv_path=csv2, out=out2)
    assert sorted(res2) == ["embedding", "stats"] and _same(res2["embedding"], xy)
    G.write_embedding_csv(csv3, xy)
    assert open(csv2, "rb").read() == open(csv3, "rb").read() == open(csv, "rb").read()
    assert out2.getvalue().count("\n") == 5 and "quality" not in out2.getvalue()
    out3 = io.StringIO()
    G.ann(hn, stats=True, embed=False, out=out3, quality=kq)                                  # quality without embed: nothing to measure
    assert out3.getvalue() == out2.getvalue()
