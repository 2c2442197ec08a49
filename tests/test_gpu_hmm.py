"""hmmsearch on the device (gs_hmm.hip) against the numpy restatement of SPEC 13 (tests/pyref_hmm.py). Every comparison is `==` on int32 (the
table of hmmsearch(): on bytes). The expected scores are computed once per module.

What these cases cover: the interface, the real profiles, best hits and the tables that are written. A lane holds Q = 1, 2, 3, 4, 6, 8, 12, 16 or 20
consecutive nodes (the smallest Q with 64 Q >= M; one launch per Q that occurs); the profiles here run in Q = 1, 2, 3 and 20 only, and their
deletions are too dear to travel through the lane scan. Every class, both sides of every class edge, GS_HMM_MAX_M, the six steps of the scan, bytes
that are no residue and the length limits are the subject of tests/test_gpu_hmm_classes.py. What is chosen here: a workgroup has 8 wavefronts and a
profile gets at most 64 workgroups, so beyond 512 records a wavefront takes several records in turn (3 000 records: five or six each); a wavefront
reads 64 residues at a time, so lengths 63 / 64 / 65 sit on both sides of that edge. There is no other chunk of records or of profiles per launch."""
import gzip
import os

import numpy as np
import pytest

import pyref_hmm as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
SYN_M = (1, 2, 63, 64, 65, 128, 129, 1238)
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3
GUARD = 1024                              # int32 words of 0xC5 in front of and behind every device output
CANARY = np.int32(np.uint32(0xC5C5C5C5).astype(np.int64) - (1 << 32))


def fixture_path(name):
    return os.path.join(HERE, "golden", "hmm", name)


@pytest.fixture(scope="module")
def case():
    """the profiles, the main records and their expected scores, once"""
    rng = np.random.default_rng(13)
    texts = [open(fixture_path(n), "rb").read() for n in FIXTURES]
    texts += [R.write_hmm(R.synth_model(rng, M), "b" if i % 2 else "f", compo=bool(i % 3)) for i, M in enumerate(SYN_M)]
    models = [m for t in texts for m in R.parse_hmm(t)]
    by_m = {m["M"]: m for m in models}
    cons = {M: R.consensus(by_m[M]["tables"]) for M in (121, 57, 65, 129, 1238)}
    bgr = lambda n: R.background(rng, n)                                                       # noqa: E731
    records = [bgr(L) for L in (0, 1, 2, 63, 64, 65, 300)]
    records += [cons[121], cons[57], cons[65], cons[129]]
    records += [cons[129][:30] + cons[129][100:],                                              # 70 nodes deleted: a D run over more than 23 lanes at Q = 3
                cons[1238][:500] + cons[1238][700:],                                           # 200 nodes deleted: ten lanes at Q = 20
                cons[121][:60] + bgr(50) + cons[121][60:],                                     # a 50-residue insertion
                cons[121] + bgr(50) + cons[121],                                               # two copies: the J state
                cons[57] + bgr(3) + cons[57] + bgr(70) + cons[57],
                b"W" * 100, b"K" * 64, b""]
    want = R.search(models, records)
    return {"texts": texts, "models": models, "records": records, "want": want, "cons": cons}


@pytest.fixture(scope="module")
def db(case, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(case["texts"], gpu_ctx, texts=True)
    yield d
    d.close()


class _Dev:
    """records on the device as gs_hmm_search_dev takes them, and guarded outputs"""

    def __init__(self, ctx, records=None, packed=None):
        import gsearch_amd as G
        self.ctx = ctx
        aa, rs, rl = packed if packed is not None else G.filter_aa_records([bytes(r) for r in records])
        self.n_rec = len(rs)
        self.ptrs = [ctx.alloc(max(a.nbytes, 16)) for a in (aa, rs, rl)]
        for p, a in zip(self.ptrs, (aa, rs, rl)):
            if a.nbytes:
                ctx.upload(p, a)
        self.outs = []

    def out(self, n_words):
        p = self.ctx.alloc(4 * (n_words + 2 * GUARD))
        self.ctx.memset(p, 0xC5, 4 * (n_words + 2 * GUARD))
        self.outs.append(p)
        return p

    def read(self, p, shape, dtype=np.int32):
        """the payload; the guards must still hold the canary"""
        n = int(np.prod(shape))
        raw = self.ctx.download(p, (n + 2 * GUARD,), np.int32)
        assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + n:] == CANARY).all(), "written outside the output"
        return raw[GUARD:GUARD + n].view(dtype).reshape(shape)

    def free(self):
        for p in self.ptrs + self.outs:
            self.ctx.free(p)


def search_dev(ctx, db, records=None, packed=None):
    d = _Dev(ctx, records, packed)
    try:
        p = d.out(d.n_rec * len(db))
        db.search_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, p + 4 * GUARD)
        return d.read(p, (d.n_rec, len(db)))
    finally:
        d.free()


def test_profiles_on_the_device_are_the_parsed_ones(case, db):
    assert len(db) == len(case["models"]) == 10
    assert db.names == [m["name"] for m in case["models"]] and db.acc == [m["acc"] for m in case["models"]]
    assert [int(x) for x in db.M] == [m["M"] for m in case["models"]]
    assert db.ga[0] == 22.1 and db.ga[1] == 27.55 and db.mu[0] == -10.5953 and db.lam[1] == 0.719
    for p, m in enumerate(case["models"]):
        assert np.array_equal(db.tables(p), m["tables"]), p


def test_scores_host_and_device_form(case, db, gpu_ctx):
    want = case["want"]
    got_host = db.search(case["records"])
    got_dev = search_dev(gpu_ctx, db, case["records"])
    assert got_host.dtype == np.int32 and got_host.shape == want.shape
    bad = np.argwhere(got_host != want)
    assert len(bad) == 0, [(int(r), int(p), int(got_host[r, p]), int(want[r, p])) for r, p in bad[:8]]
    assert np.array_equal(got_dev, got_host)
    empty = [i for i, r in enumerate(case["records"]) if len(r) == 0]
    assert len(empty) == 2 and (want[empty] == R.NO_SCORE).all()
    # the planted copies are found: one consensus far above the profile's GA, two copies above one
    assert want[7, 0] > 150 * 1024 and want[14, 0] > want[7, 0] and want[12, 9] > 100 * 1024


def test_long_record_against_the_longest_profile(case, gpu_ctx):
    """20 000 residues against 1 238 nodes: scores in the millions of units, the largest table (143 360 bytes of LDS), 313 blocks of 64 residues"""
    import gsearch_amd as G
    rng = np.random.default_rng(17)
    c = case["cons"][1238]
    long_rec = R.background(rng, 6000) + c + R.background(rng, 5000) + c[:900] + R.background(rng, 20000 - 11000 - 1238 - 900)
    assert len(long_rec) == 20000
    model = [m for m in case["models"] if m["M"] == 1238]
    text = [t for t, m in zip(case["texts"][2:], case["models"][2:]) if m["M"] == 1238]
    want = R.search(model, [long_rec, b"", c])
    assert want[0, 0] > (1 << 21)
    d = G.HmmDb(text, gpu_ctx, texts=True)
    try:
        assert np.array_equal(d.search([long_rec, b"", c]), want)
        assert np.array_equal(search_dev(gpu_ctx, d, [long_rec, b"", c]), want)
    finally:
        d.close()


def test_many_short_records_and_one_by_one(case, gpu_ctx):
    import gsearch_amd as G
    rng = np.random.default_rng(19)
    keep = [i for i, m in enumerate(case["models"]) if m["M"] != 1238]
    assert len(keep) == 9
    models, texts = [case["models"][i] for i in keep], [case["texts"][i] for i in keep]
    lens = rng.integers(1, 41, size=3000)
    records = [R.background(rng, int(L)) for L in lens]
    for j in range(0, 3000, 97):                                                # some carry a piece of a consensus, so that not all scores are noise
        records[j] = (case["cons"][57] * 2)[j % 50:][:int(lens[j])]
    want = R.search(models, records)
    d = G.HmmDb(texts, gpu_ctx, texts=True)
    try:
        assert np.array_equal(d.search(records), want)
        assert np.array_equal(search_dev(gpu_ctx, d, records), want)
    finally:
        d.close()
    one = G.HmmDb(texts[:1], gpu_ctx, texts=True)
    try:
        assert np.array_equal(one.search(records[:1]), want[:1, :1])
        assert np.array_equal(search_dev(gpu_ctx, one, records[:1]), want[:1, :1])
        assert one.search([]).shape == (0, 1)
    finally:
        one.close()


# the main records as genomes: 0 = background only, 1 = no records, 2 = the four consensus records, 3 = the rest, 4 = genome 2's proteins twice
GENOME_OFF = np.array([0, 7, 7, 11, 19, 27], np.uint64)


def _best_cases(case):
    want = case["want"]
    return np.concatenate([want, want[7:11], want[7:11]]), GENOME_OFF


def test_best_hits(case, db):
    scores, goff = _best_cases(case)
    ga = np.array([m["ga_units"] for m in case["models"]], np.int32)
    rec, sc = db.best_hits(scores, goff, "ga")
    wrec, wsc = R.best_hits(scores, goff, ga)
    assert rec.dtype == np.uint32 and sc.dtype == np.int32 and np.array_equal(rec, wrec) and np.array_equal(sc, wsc)
    assert (rec[1] == R.NO_HIT).all() and (sc[1] == R.NO_SCORE).all()                        # a genome with no records
    assert (rec[0] == R.NO_HIT).all() and (sc[0] == R.NO_SCORE).all()                        # only background: no protein reaches a GA
    assert rec[2, 0] == 7 and rec[2, 1] == 8 and sc[2, 0] == scores[7, 0]                    # the consensus of each fixture
    assert rec[4, 0] == 19 and rec[4, 1] == 20                                               # a duplicated protein: the lower record, not 23 / 24
    # a caller's bits: the score itself as the threshold passes, one unit more does not
    s70 = int(scores[7, 0])
    for bits, hit in ((s70 / 1024.0, True), ((s70 + 1) / 1024.0, False)):
        thr = np.full(len(db), R.threshold_units(bits), np.int32)
        assert thr[0] == s70 + (0 if hit else 1)
        rec_b, sc_b = db.best_hits(scores[:11], goff[:4], bits)
        wrec_b, wsc_b = R.best_hits(scores[:11], goff[:4], thr)
        assert np.array_equal(rec_b, wrec_b) and np.array_equal(sc_b, wsc_b)
        assert rec_b[2, 0] == (7 if hit else R.NO_HIT)
    assert not np.array_equal(wrec_b, wrec[:3])                                              # GA and the caller's bits choose differently
    low, slow = db.best_hits(scores, goff, -1000.0)                                          # everything passes: the plain argmax
    wlow, wslow = R.best_hits(scores, goff, np.full(len(db), R.threshold_units(-1000.0), np.int32))
    assert np.array_equal(low, wlow) and np.array_equal(slow, wslow) and (low[[0, 2, 3, 4]] != R.NO_HIT).all() and (low[1] == R.NO_HIT).all()
    assert db.best_hits(scores, np.array([0], np.uint64))[0].shape == (0, len(db))


def test_best_hits_writes_only_its_matrices(case, db, gpu_ctx):
    scores, goff = _best_cases(case)
    ga = np.array([m["ga_units"] for m in case["models"]], np.int32)
    ng, npf = len(goff) - 1, len(db)
    d = _Dev(gpu_ctx, [b"A"])
    try:
        ps, pg = gpu_ctx.alloc(scores.nbytes), gpu_ctx.alloc(goff.nbytes)
        d.outs += [ps, pg]
        gpu_ctx.upload(ps, scores); gpu_ctx.upload(pg, goff)
        pr, pc = d.out(ng * npf), d.out(ng * npf)
        db.best_hits_dev(ps, len(scores), pg, ng, None, pr + 4 * GUARD, pc + 4 * GUARD)      # no thresholds: the set's GA cutoffs
        wrec, wsc = R.best_hits(scores, goff, ga)
        assert np.array_equal(d.read(pr, (ng, npf), np.uint32), wrec) and np.array_equal(d.read(pc, (ng, npf)), wsc)
    finally:
        d.free()


def test_a_set_without_ga_needs_thresholds(case, gpu_ctx):
    import gsearch_amd as G
    s = R.synth_model(np.random.default_rng(23), 40)
    d = G.HmmDb([R.write_hmm(dict(s, ga=None))], gpu_ctx, texts=True)
    try:
        sc = d.search([R.consensus(R.parse_hmm(R.write_hmm(s))[0]["tables"])])
        with pytest.raises(G.GsError) as e:
            d.best_hits(sc, [0, 1], "ga")
        assert e.value.code == GS_ERR_INVALID
        p = gpu_ctx.alloc(64)
        try:
            assert gpu_ctx.L.gs_hmm_best_hits_dev(gpu_ctx.h, d.h, p, 1, p, 1, None, p, p) == GS_ERR_INVALID
        finally:
            gpu_ctx.free(p)
        rec, _ = d.best_hits(sc, [0, 1], 10.0)
        assert rec[0, 0] == 0
    finally:
        d.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_on_poisoned_scratch(case, gpu_ctx, byte):
    """the whole search and best_hits twice on scratch and allocations filled with a chosen byte: nothing reads what nothing wrote"""
    import gsearch_amd as G
    goff = GENOME_OFF[:5]
    ga = np.array([m["ga_units"] for m in case["models"]], np.int32)
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        d = G.HmmDb(case["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                scores = d.search(case["records"])
                assert np.array_equal(scores, case["want"])
                assert np.array_equal(search_dev(gpu_ctx, d, case["records"]), case["want"])
                rec, sc = d.best_hits(scores, goff)
                wrec, wsc = R.best_hits(case["want"], goff, ga)
                assert np.array_equal(rec, wrec) and np.array_equal(sc, wsc)
        finally:
            d.close()
    finally:
        G.debug_mem_fill(None)


def _write_faa(path, ids, seqs, gz=False):
    text = b"".join(b">%s some description\n" % i.encode() + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n" for i, s in zip(ids, seqs))
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(text)


def test_hmmsearch_writes_the_restatements_table(case, gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(29)
    paths = [fixture_path(n) for n in FIXTURES]
    models = case["models"][:2]
    c0, c1 = case["cons"][121], case["cons"][57]
    seqs = [R.background(rng, 150), c0, c1 + R.background(rng, 30), c0[:80], R.background(rng, 90) + c1[10:], c0, R.background(rng, 40),
            c0[:12]]                                                             # 15 bits: reported, below GA (22.1)
    ids = ["prot%d" % i for i in range(len(seqs))]
    want_scores = R.search(models, seqs)
    want = R.table_bytes(models, ids, want_scores)
    assert want.count(b"\n") >= 7 and b"\t1\n" in want and b"prot7\tRibosomal_S9\tPF00380.20\t14.97\t" in want and want.count(b"\t0\n") == 1
    outs = []
    for gz in (False, True):
        faa = str(tmp_path / ("p.faa.gz" if gz else "p.faa"))
        out = str(tmp_path / ("out%d.tsv" % gz))
        _write_faa(faa, ids, seqs, gz)
        got_ids, scores, table = G.hmmsearch(faa, paths, out, ctx=gpu_ctx)
        assert got_ids == ids and np.array_equal(scores, want_scores)
        assert table == want and open(out, "rb").read() == want
        outs.append(table)
    # a directory of profile files is the same set in name order
    ids2, scores2, table2 = G.hmmsearch(str(tmp_path / "p.faa"), os.path.join(HERE, "golden", "hmm"), ctx=gpu_ctx)
    assert table2 == want
    first = want.split(b"\n")[1].split(b"\t")
    assert first[0] in (b"prot1", b"prot5") and first[1] == b"Ribosomal_S9" and first[2] == b"PF00380.20" and first[5] == b"1"
    assert float(first[3]) == round(G.hmm_bits(int(want_scores[1, 0])), 2)


def test_universal_genes_are_the_best_hits(case, gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(31)
    paths = [fixture_path(n) for n in FIXTURES]
    models = case["models"][:2]
    c0, c1 = case["cons"][121], case["cons"][57]
    genomes = [[R.background(rng, 100), c1, c0[:100], c0],                     # both markers; the whole S9 beats its fragment
               [R.background(rng, 60), R.background(rng, 200)],                 # none
               [c1, R.background(rng, 50), c1]]                                 # a duplicated protein: the first; no S9
    files = []
    for g, seqs in enumerate(genomes):
        files.append(str(tmp_path / ("g%d.faa" % g)))
        _write_faa(files[-1], ["g%d_%d" % (g, i) for i in range(len(seqs))], seqs)
    got, local = G.universal_genes(files, paths, ctx=gpu_ctx)
    flat = [s for g in genomes for s in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    wrec, _ = R.best_hits(R.search(models, flat), goff, [m["ga_units"] for m in models])
    want = [[flat[r] for r in wrec[g] if r != R.NO_HIT] for g in range(len(genomes))]
    assert got == want == [[c0, c1], [], [c1]]
    assert local.tolist() == [[3, 1], [R.NO_HIT, R.NO_HIT], [R.NO_HIT, 0]]


def test_oversize_is_refused_and_writes_nothing(case, db, gpu_ctx):
    import gsearch_amd as G
    s = R.synth_model(np.random.default_rng(37), 3)
    too_long = R.write_hmm(s).replace(b"LENG  3", b"LENG  %d" % (R.MAX_M + 1))
    with pytest.raises(G.GsError) as e:
        G.HmmDb([case["texts"][0], too_long], gpu_ctx, texts=True)
    assert e.value.code == GS_ERR_UNSUPPORTED
    # a record of GS_HMM_MAX_L + 1 residues: refused from the lengths alone, before anything is queued
    aa = np.frombuffer(b"ACDEFGHIKL" * 4, np.uint8)
    rs, rl = np.array([0, 0, 10], np.uint64), np.array([10, R.MAX_L + 1, 10], np.uint64)
    d = _Dev(gpu_ctx, packed=(aa, rs, rl))
    try:
        p = d.out(3 * len(db))
        rc = gpu_ctx.L.gs_hmm_search_dev(gpu_ctx.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 3, p + 4 * GUARD)
        assert rc == GS_ERR_UNSUPPORTED
        assert (d.read(p, (3, len(db))) == CANARY).all()
    finally:
        d.free()
    out = np.full((3, len(db)), 77, np.int32)
    rc = gpu_ctx.L.gs_hmm_search(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, out.ctypes.data)
    assert rc == GS_ERR_UNSUPPORTED and (out == 77).all()
    rl[1] = R.MAX_L                                                             # the limit itself is a length the length model takes
    assert G.hmm_specials(R.MAX_L, 1238) == R.specials(R.MAX_L, 1238)
