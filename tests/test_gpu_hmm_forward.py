"""Forward scores on the device (gs_hmm.hip, SPEC 13.1) against the numpy restatement (tests/pyref_hmm_forward.py). Every score comparison is `==`
on int32 (the table of hmmsearch(): on bytes); device outputs sit between canaries. lse is not associative, so a wrong order of the scan, of the
fold or of the tree shows - but only in a few scores in a hundred, hence the thousands of scores below. The expected matrices are computed once
per module.

The profiles, the records and the reasons for their shapes are those of test_gpu_hmm.py (both sides of the class edges Q = 1 | 2 and 2 | 3, the
largest table with T behind it in LDS; lengths on both sides of the 64-residue block; the 200-node deletion at Q = 20 is the scan's guard `a lane
below 2^s keeps its b` across many lanes)."""

import numpy as np
import pytest

import pyref_hmm as R
import pyref_hmm_forward as F
from test_gpu_hmm import CANARY, FIXTURES, GUARD, _Dev, _write_faa, case, fixture_path  # noqa: F401  (case: the module fixture of the Viterbi tests)

pytestmark = pytest.mark.gpu
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def fcase(case):
    """the Forward matrix of every pair of the main case, once"""
    _, fwd = F.search_forward(case["models"], case["records"], vit=case["want"])
    stats = [s for t in case["texts"] for s in F.stats_lines(t)]
    return dict(case, fwd=fwd, stats=stats)


@pytest.fixture(scope="module")
def db(fcase, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(fcase["texts"], gpu_ctx, texts=True)
    yield d
    d.close()


@pytest.fixture(scope="module")
def many(case):
    """3 000 records of 1..40 residues against the nine small profiles: 27 000 scores of each kind"""
    rng = np.random.default_rng(19)
    keep = [i for i, m in enumerate(case["models"]) if m["M"] != 1238]
    models, texts = [case["models"][i] for i in keep], [case["texts"][i] for i in keep]
    lens = rng.integers(1, 41, size=3000)
    records = [R.background(rng, int(L)) for L in lens]
    for j in range(0, 3000, 97):
        records[j] = (case["cons"][57] * 2)[j % 50:][:int(lens[j])]
    vit, fwd = F.search_forward(models, records)
    return {"models": models, "texts": texts, "records": records, "vit": vit, "fwd": fwd}


def forward_dev(ctx, db, records=None, packed=None, floor=None, want_vit=True):
    """gs_hmm_search_forward_dev on guarded outputs -> (vit or None, fwd)"""
    d = _Dev(ctx, records, packed)
    try:
        n = d.n_rec * len(db)
        pf, pv = d.out(n), (d.out(n) if want_vit else None)
        pfl = None
        if floor is not None:
            fl = np.ascontiguousarray(floor, np.int32)
            pfl = ctx.alloc(max(fl.nbytes, 16))
            d.outs.append(pfl)
            ctx.upload(pfl, fl)
        db.search_forward_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, pfl, pv + 4 * GUARD if want_vit else None, pf + 4 * GUARD)
        return (d.read(pv, (d.n_rec, len(db))) if want_vit else None), d.read(pf, (d.n_rec, len(db)))
    finally:
        d.free()


def mismatches(got, want):
    return [(int(r), int(p), int(got[r, p]), int(want[r, p])) for r, p in np.argwhere(got != want)[:8]]


def test_all_pairs_host_and_device_form(fcase, db, gpu_ctx):
    want_vit, want = fcase["want"], fcase["fwd"]
    assert want.shape == (19, 10) and [len(r) for r in fcase["records"][:7]] == [0, 1, 2, 63, 64, 65, 300]
    vit, fwd = db.search_forward(fcase["records"], filter_p=None)
    assert fwd.dtype == np.int32 and fwd.shape == want.shape
    assert not mismatches(fwd, want)
    assert np.array_equal(vit, want_vit) and np.array_equal(vit, db.search(fcase["records"]))
    dvit, dfwd = forward_dev(gpu_ctx, db, fcase["records"])
    assert np.array_equal(dfwd, want) and np.array_equal(dvit, want_vit)
    assert np.array_equal(forward_dev(gpu_ctx, db, fcase["records"], want_vit=False)[1], want)       # the Viterbi matrix nobody asked for: scratch
    both = (want != R.NO_SCORE) & (want_vit != R.NO_SCORE)
    assert np.array_equal(both, want_vit != R.NO_SCORE) and (fwd[both] >= vit[both]).all() and both.sum() == 170
    assert (want[[0, 18]] == R.NO_SCORE).all()                                                      # the empty records
    # the deletions take the D path: scores far above noise, and Forward gains on Viterbi
    assert want[11, 8] > 100 * 1024 and want[12, 9] > 100 * 1024 and (want[both] - want_vit[both]).max() > 4 * 1024
    assert np.array_equal(db.tau[:2], [-3.8068, -4.3433]) and np.array_equal(db.lam_fwd[:2], [0.71333, 0.719])
    assert np.array_equal(db.viterbi_floor(1e-3), F.floors(fcase["models"])) and np.array_equal(db.viterbi_floor(0.02), F.floors(fcase["models"], 0.02))


def test_many_short_records_and_one_by_one(many, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(many["texts"], gpu_ctx, texts=True)
    try:
        vit, fwd = d.search_forward(many["records"], filter_p=None)
        assert not mismatches(fwd, many["fwd"]) and np.array_equal(vit, many["vit"])
        dvit, dfwd = forward_dev(gpu_ctx, d, many["records"])
        assert np.array_equal(dfwd, many["fwd"]) and np.array_equal(dvit, many["vit"])
        assert (fwd >= vit).all() and (fwd != R.NO_SCORE).all()
    finally:
        d.close()
    one = G.HmmDb(many["texts"][:1], gpu_ctx, texts=True)
    try:
        vit, fwd = one.search_forward(many["records"][:1], filter_p=None)
        assert np.array_equal(fwd, many["fwd"][:1, :1]) and np.array_equal(vit, many["vit"][:1, :1])
        assert np.array_equal(forward_dev(gpu_ctx, one, many["records"][:1])[1], many["fwd"][:1, :1])
        vit0, fwd0 = one.search_forward([])
        assert vit0.shape == fwd0.shape == (0, 1)
        p = gpu_ctx.alloc(64)
        try:
            one.search_forward_dev(p, p, p, 0, None, None, p)
        finally:
            gpu_ctx.free(p)
    finally:
        one.close()


def test_filtered_by_a_viterbi_floor(many, gpu_ctx):
    import gsearch_amd as G
    vit, all_fwd, models = many["vit"].astype(np.int64), many["fwd"], many["models"]
    floor = F.floors(models).astype(np.int64)
    floor[0] = vit[:, 0].max() + 1                                              # nothing
    top = np.sort(vit[:, 1])
    assert top[-1] > top[-2]
    floor[1] = top[-1]                                                          # exactly one record
    floor[2] = F.FLOOR_ALL                                                      # everything
    floor[3] = np.sort(vit[:, 3])[3000 - 1700]                                  # more than 512: a wavefront of the first workgroups takes several
    floor = floor.astype(np.int32)
    sel = vit >= floor[None, :]
    n_sel = sel.sum(axis=0)
    assert n_sel[0] == 0 and n_sel[1] == 1 and n_sel[2] == 3000 and 512 < n_sel[3] < 3000
    want = np.where(sel, all_fwd, R.NO_SCORE).astype(np.int32)
    assert np.array_equal(F.search_forward(models[:2], many["records"], floor=floor[:2], vit=many["vit"][:, :2])[1], want[:, :2])
    d = G.HmmDb(many["texts"], gpu_ctx, texts=True)
    try:
        got_vit, got = d.search_forward(many["records"], floor=floor)
        assert not mismatches(got, want) and np.array_equal(got_vit, many["vit"])
        dvit, dgot = forward_dev(gpu_ctx, d, many["records"], floor=floor)
        assert np.array_equal(dgot, want) and np.array_equal(dvit, many["vit"])
        # the default floors: the selection of the restatement
        dflt = F.floors(models)
        assert np.array_equal(d.viterbi_floor(), dflt)
        want_d = np.where(vit >= dflt[None, :].astype(np.int64), all_fwd, R.NO_SCORE).astype(np.int32)
        share = (want_d != R.NO_SCORE).mean()
        assert 0 < share < 0.5, share
        _, got_d = d.search_forward(many["records"])
        assert not mismatches(got_d, want_d)
        assert np.array_equal(forward_dev(gpu_ctx, d, many["records"], floor=dflt)[1], want_d)
    finally:
        d.close()


def test_one_long_record_against_the_longest_profile(case, gpu_ctx):
    """5 000 residues against 1 238 nodes: 79 blocks of 64 residues, the largest table with T behind it (155 168 bytes of LDS), a raw score above 2^21"""
    import gsearch_amd as G
    rng = np.random.default_rng(17)
    c = case["cons"][1238]
    long_rec = R.background(rng, 1500) + c + R.background(rng, 1000) + c[:900] + R.background(rng, 5000 - 2500 - 1238 - 900)
    assert len(long_rec) == 5000
    model = [m for m in case["models"] if m["M"] == 1238]
    text = [t for t, m in zip(case["texts"][2:], case["models"][2:]) if m["M"] == 1238]
    vit, want = F.search_forward(model, [long_rec])
    assert want[0, 0] > (1 << 21) and want[0, 0] >= vit[0, 0]
    d = G.HmmDb(text, gpu_ctx, texts=True)
    try:
        got_vit, got = d.search_forward([long_rec], filter_p=None)
        assert np.array_equal(got, want) and np.array_equal(got_vit, vit)
        assert np.array_equal(forward_dev(gpu_ctx, d, [long_rec])[1], want)
    finally:
        d.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_on_poisoned_scratch(fcase, gpu_ctx, byte):
    """all pairs and a filtered search, host and device form, twice on scratch and allocations filled with a chosen byte: nothing reads what nothing wrote"""
    import gsearch_amd as G
    floor = F.floors(fcase["models"])
    want_f = np.where(fcase["want"].astype(np.int64) >= floor[None, :], fcase["fwd"], R.NO_SCORE).astype(np.int32)
    assert 0 < (want_f != R.NO_SCORE).sum() < (fcase["fwd"] != R.NO_SCORE).sum()
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        d = G.HmmDb(fcase["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                vit, fwd = d.search_forward(fcase["records"], filter_p=None)
                assert np.array_equal(fwd, fcase["fwd"]) and np.array_equal(vit, fcase["want"])
                assert np.array_equal(d.search_forward(fcase["records"])[1], want_f)
                dvit, dfwd = forward_dev(gpu_ctx, d, fcase["records"], floor=floor)
                assert np.array_equal(dfwd, want_f) and np.array_equal(dvit, fcase["want"])
                assert np.array_equal(forward_dev(gpu_ctx, d, fcase["records"], want_vit=False)[1], fcase["fwd"])
        finally:
            d.close()
    finally:
        G.debug_mem_fill(None)


def test_refusals_write_nothing(fcase, db, gpu_ctx):
    import gsearch_amd as G
    assert F.FWD_MAX_L == 65536 < R.MAX_L
    aa = np.frombuffer(b"ACDEFGHIKL" * 4, np.uint8)
    rs, rl = np.array([0, 0, 10], np.uint64), np.array([10, F.FWD_MAX_L + 1, 10], np.uint64)
    d = _Dev(gpu_ctx, packed=(aa, rs, rl))
    try:
        pv, pf = d.out(3 * len(db)), d.out(3 * len(db))
        rc = gpu_ctx.L.gs_hmm_search_forward_dev(gpu_ctx.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 3, None, pv + 4 * GUARD, pf + 4 * GUARD)
        assert rc == GS_ERR_UNSUPPORTED
        assert (d.read(pv, (3, len(db))) == CANARY).all() and (d.read(pf, (3, len(db))) == CANARY).all()
        # a set of another context
        other = G.Context(0)
        try:
            rc = other.L.gs_hmm_search_forward_dev(other.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 1, None, pv + 4 * GUARD, pf + 4 * GUARD)
            assert rc == GS_ERR_INVALID
            v1, f1 = np.full((1, len(db)), 77, np.int32), np.full((1, len(db)), 78, np.int32)
            rc = other.L.gs_hmm_search_forward(other.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, None, v1.ctypes.data, f1.ctypes.data)
            assert rc == GS_ERR_INVALID and (v1 == 77).all() and (f1 == 78).all()
        finally:
            other.close()
        assert (d.read(pv, (3, len(db))) == CANARY).all() and (d.read(pf, (3, len(db))) == CANARY).all()
    finally:
        d.free()
    vit, fwd = np.full((3, len(db)), 77, np.int32), np.full((3, len(db)), 78, np.int32)
    rc = gpu_ctx.L.gs_hmm_search_forward(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, None, vit.ctypes.data, fwd.ctypes.data)
    assert rc == GS_ERR_UNSUPPORTED and (vit == 77).all() and (fwd == 78).all()
    with pytest.raises(G.GsError) as e:
        db.search_forward_packed(aa, rs, rl)
    assert e.value.code == GS_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        db.search_forward([b"ACD"], floor=np.zeros(3, np.int32))


def _straddling_fragment(model):
    """a piece of the consensus whose Viterbi score is below GA and whose Forward score is at or above it: found by trying starts and lengths"""
    c, ga = R.consensus(model["tables"]), model["ga_units"]
    pieces = [c[s:s + n] for s in range(0, 60, 5) for n in range(10, 31)]
    vit, fwd = R.viterbi_batch(model["tables"], pieces), F.forward_batch(model["tables"], pieces)
    hit = np.flatnonzero((vit < ga) & (fwd >= ga))
    assert len(hit) > 0
    return pieces[int(hit[0])], int(vit[hit[0]]), int(fwd[hit[0]])


def test_hmmsearch_and_universal_genes_by_the_forward_score(fcase, gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(29)
    paths = [fixture_path(n) for n in FIXTURES]
    models, stats = fcase["models"][:2], fcase["stats"][:2]
    c0, c1 = fcase["cons"][121], fcase["cons"][57]
    frag, frag_vit, frag_fwd = _straddling_fragment(models[0])
    assert frag_vit < models[0]["ga_units"] == 22630 <= frag_fwd
    seqs = [R.background(rng, 150), c0, c1 + R.background(rng, 30), c0[:80], R.background(rng, 90) + c1[10:], frag, R.background(rng, 40), c0[:12]]
    ids = ["prot%d" % i for i in range(len(seqs))]
    want_vit, want_fwd = F.search_forward(models, seqs, floor=F.floors(models))
    want = F.table_bytes(models, stats, ids, want_fwd)
    want_v = R.table_bytes(models, ids, want_vit)
    row = lambda t: [ln.split(b"\t") for ln in t.split(b"\n") if ln.startswith(b"prot5\tRibosomal_S9")]          # noqa: E731
    assert row(want)[0][5] == b"1" and row(want_v)[0][5] == b"0" and want != want_v and want.count(b"\n") >= 7
    for gz in (False, True):
        faa = str(tmp_path / ("p.faa.gz" if gz else "p.faa"))
        out = str(tmp_path / ("out%d.tsv" % gz))
        _write_faa(faa, ids, seqs, gz)
        got_ids, scores, table = G.hmmsearch(faa, paths, out, ctx=gpu_ctx, score="forward")
        assert got_ids == ids and np.array_equal(scores, want_fwd)
        assert table == want and open(out, "rb").read() == want
        got_ids, scores, table = G.hmmsearch(faa, paths, ctx=gpu_ctx)                            # the default: what it was
        assert got_ids == ids and np.array_equal(scores, want_vit) and table == want_v
    # every pair: more rows of noise, the same rows above the floor
    _, all_fwd = F.search_forward(models, seqs)
    _, scores, table = G.hmmsearch(str(tmp_path / "p.faa"), paths, ctx=gpu_ctx, score="forward", filter_p=None)
    assert np.array_equal(scores, all_fwd) and table == F.table_bytes(models, stats, ids, all_fwd)
    with pytest.raises(ValueError):
        G.hmmsearch(str(tmp_path / "p.faa"), paths, ctx=gpu_ctx, score="msv")

    genomes = [[R.background(rng, 100), c1, frag],                               # S9 only as the fragment: a hit by Forward, none by Viterbi
               [R.background(rng, 60), R.background(rng, 200)],
               [c1, c0[:100], c0]]
    files = []
    for g, gs in enumerate(genomes):
        files.append(str(tmp_path / ("g%d.faa" % g)))
        _write_faa(files[-1], ["g%d_%d" % (g, i) for i in range(len(gs))], gs)
    flat = [s for g in genomes for s in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    ga = [m["ga_units"] for m in models]
    gvit, gfwd = F.search_forward(models, flat, floor=F.floors(models))
    wrec_f, _ = R.best_hits(gfwd, goff, ga)
    wrec_v, _ = R.best_hits(gvit, goff, ga)
    got_f, local_f = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward")
    got_v, local_v = G.universal_genes(files, paths, ctx=gpu_ctx)
    assert got_f == [[flat[r] for r in wrec_f[g] if r != R.NO_HIT] for g in range(3)] == [[frag, c1], [], [c0, c1]]
    assert got_v == [[flat[r] for r in wrec_v[g] if r != R.NO_HIT] for g in range(3)] == [[c1], [], [c0, c1]]
    assert local_f.tolist() == [[2, 1], [R.NO_HIT, R.NO_HIT], [2, 0]] and local_v.tolist() == [[R.NO_HIT, 1], [R.NO_HIT, R.NO_HIT], [2, 0]]
    with pytest.raises(ValueError):
        G.universal_genes(files, paths, ctx=gpu_ctx, score="msv")
