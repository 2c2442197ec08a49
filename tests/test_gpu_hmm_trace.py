"""The trace-back of SPEC 13.2 on the device (k_hmm_trace<Q> and k_hmm_walk of gs_hmm.hip, gs_hmm_trace / gs_hmm_trace_dev) against the numpy
restatement tests/pyref_hmm_trace.py. Every comparison is `==` on int32 or on bytes, through the host form and the device form; every device output sits
between canaries. The expected domains are computed once per module; those of the length limit against the largest profile come from
tests/golden/hmm_trace_limits.json.

What is chosen here: the pairs of a call are cut into blocks by max_block_cells and a block's pairs are grouped by profile, so the pair lists below are
shuffled and hold repeats; a lane's nibbles fill one word up to Q = 8, two at 12 and 16, three at 20, and the class set runs every one of them; the D
pointer of a lane's first node comes from the lane below, which the deletion-friendly profiles exercise, the I pointer is exercised by the
insertion-friendly ones."""
import json
import os

import numpy as np
import pytest

import hmm_classes_case as K
import hmm_trace_case as TC
import pyref_hmm as R
import pyref_hmm_trace as T
from test_gpu_hmm import CANARY, FIXTURES, GENOME_OFF, GUARD, _Dev, _write_faa, case, db, fixture_path, search_dev  # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GS_OK, GS_ERR_INVALID, GS_ERR_UNSUPPORTED = 0, -1, -3


def trace_dev(ctx, d_b, pair_rec, pair_prof, records=None, packed=None, max_dom=8, max_block_cells=0, rc_want=GS_OK):
    """gs_hmm_trace_dev on guarded outputs -> (raw, n_dom, dom); with rc_want another code: that code is returned and the outputs hold the canary"""
    d = _Dev(ctx, records, packed)
    try:
        pr, pp = np.ascontiguousarray(pair_rec, np.uint32), np.ascontiguousarray(pair_prof, np.uint32)
        n = len(pr)
        for a in (pr, pp):
            d.outs.append(ctx.alloc(max(a.nbytes, 16)))
            if a.nbytes:
                ctx.upload(d.outs[-1], a)
        p_pr, p_pp = d.outs[-2], d.outs[-1]
        p_raw, p_nd, p_dom = d.out(n), d.out(n), d.out(n * max_dom * T.DOM_WORDS)
        rc = ctx.L.gs_hmm_trace_dev(ctx.h, d_b.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, p_pr, p_pp, n, max_dom, max_block_cells, p_raw + 4 * GUARD,
                                    p_nd + 4 * GUARD, (p_dom + 4 * GUARD) if max_dom else None)
        assert rc == rc_want, rc
        got = d.read(p_raw, (n,)), d.read(p_nd, (n,), np.uint32), d.read(p_dom, (n, max_dom, T.DOM_WORDS))
        if rc != GS_OK:
            assert (got[0] == CANARY).all() and (got[1].view(np.int32) == CANARY).all() and (got[2] == CANARY).all()
        return got
    finally:
        d.free()


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def both_forms(ctx, d_b, records, pair_rec, pair_prof, want, max_dom=8, max_block_cells=0):
    """the host form and the device form against the restatement's (raw, n_dom, dom)"""
    host = d_b.trace(records, np.stack([pair_rec, pair_prof], axis=1), max_dom=max_dom, max_block_cells=max_block_cells)
    bad = np.flatnonzero((host[0] != want[0]) | (host[1] != want[1]) | (host[2] != want[2]).any(axis=(1, 2)))
    assert len(bad) == 0, [(int(pair_rec[j]), int(pair_prof[j]), int(host[0][j]), int(want[0][j]), host[2][j].tolist(), want[2][j].tolist()) for j in bad[:3]]
    assert same(host, want)
    assert same(trace_dev(ctx, d_b, pair_rec, pair_prof, records=records, max_dom=max_dom, max_block_cells=max_block_cells), want)
    return host


@pytest.fixture(scope="module")
def main(case):
    """all 190 pairs of the main set in a shuffled order, 30 of them a second time, and what the restatement says"""
    rng = np.random.default_rng(1321)
    n_rec, n_prof = len(case["records"]), len(case["models"])
    assert (n_rec, n_prof) == (19, 10)
    idx = rng.permutation(n_rec * n_prof)
    idx = np.concatenate([idx, idx[:30]])
    pr, pp = (idx // n_prof).astype(np.uint32), (idx % n_prof).astype(np.uint32)
    want = T.trace_pairs(case["models"], case["records"], pr, pp, 8)
    assert (want[0] == case["want"][pr, pp]).all() and (want[1][want[0] == R.NO_SCORE] == 0).all()
    return {"pr": pr, "pp": pp, "want": want}


def test_all_pairs_of_the_main_set(case, main, db, gpu_ctx):
    host = both_forms(gpu_ctx, db, case["records"], main["pr"], main["pp"], main["want"])
    assert np.array_equal(host[0], db.search(case["records"])[main["pr"], main["pp"]])
    # the planted copies: two and three domains through J; in this profile a 50-residue insertion is dearer than leaving and entering again
    by = {(int(r), int(p)): j for j, (r, p) in enumerate(zip(main["pr"], main["pp"]))}
    nd, dom = host[1], host[2]
    assert nd[by[14, 0]] == 2 and nd[by[15, 1]] == 3 and nd[by[13, 0]] == 2 and dom[by[13, 0], :2, :4].tolist() == [[1, 60, 1, 60], [111, 171, 61, 121]]
    assert nd.max() == 8 == dom.shape[1]                                       # W * 100 against 63 nodes: no slot to spare


@pytest.fixture(scope="module")
def cset():
    """every kernel class: the 19 profiles of hmm_classes_case.SET_ORDER with the deletion records of each deletion-friendly one, and the
    insertion-friendly profiles with a 30-residue insertion"""
    rng = np.random.default_rng(1323)
    sets = [K.model_text(M) for M in K.SET_ORDER] + [R.write_hmm(TC.insertion_model(M)) for M in TC.INSERTION_M]
    models = [m for t in sets for m in R.parse_hmm(t)]
    records, pr, pp = [], [], []
    for p, m in enumerate(models):
        c = R.consensus(m["tables"])
        if m["name"].startswith("DEL"):
            recs = K.deletion_records(c, m["M"])
        elif m["name"].startswith("INS"):
            recs = [TC.insertion_record(c), c]
        else:
            recs = [c[:40] + R.background(rng, 20) + c[100:160]]
        pr += list(range(len(records), len(records) + len(recs)))
        pp += [p] * len(recs)
        records += recs
    order = rng.permutation(len(pr))
    pr, pp = np.array(pr, np.uint32)[order], np.array(pp, np.uint32)[order]
    want = T.trace_pairs(models, records, pr, pp, 4)
    return {"texts": sets, "models": models, "records": records, "pr": pr, "pp": pp, "want": want}


def test_every_class(cset, gpu_ctx):
    import gsearch_amd as G
    models, pr, pp, (raw, nd, dom) = cset["models"], cset["pr"], cset["pp"], cset["want"]
    assert (raw != R.NO_SCORE).all() and (nd >= 1).all() and nd.max() <= 4
    for j in range(len(pr)):                                                     # the long runs are on the expected paths
        m = models[pp[j]]
        if m["name"].startswith("INS") and len(cset["records"][pr[j]]) == m["M"] + 30:
            assert nd[j] == 1 and dom[j, 0].tolist()[5:] == [m["M"], 30, 0], m["M"]
    n_del = {m["M"]: int(max(dom[j, :, 7].max() for j in range(len(pr)) if pp[j] == p)) for p, m in enumerate(models) if m["name"].startswith("DEL")}
    assert n_del[129] == 105 and n_del[1280] > 1000 and all(v > 32 for v in n_del.values()), n_del
    d = G.HmmDb(cset["texts"], gpu_ctx, texts=True)
    try:
        both_forms(gpu_ctx, d, cset["records"], pr, pp, cset["want"], max_dom=4)
    finally:
        d.close()


def test_ties(gpu_ctx):
    """all_zero_model: nearly every cell ties, so the order of the alternatives is the path; M on both sides of the first class edges, records on both
    sides of the 64-residue block"""
    import gsearch_amd as G
    texts = [R.write_hmm(K.all_zero_model(M)) for M in TC.TIE_M]
    models = [m for t in texts for m in R.parse_hmm(t)]
    pr = np.repeat(np.arange(len(TC.TIE_RECORDS), dtype=np.uint32), len(models))
    pp = np.tile(np.arange(len(models), dtype=np.uint32), len(TC.TIE_RECORDS))
    want = T.trace_pairs(models, TC.TIE_RECORDS, pr, pp, 8)
    assert want[1].max() > 8 and want[1].min() == 1                              # W * 65 against one node: 65 domains, eight of them written
    d = G.HmmDb(texts, gpu_ctx, texts=True)
    try:
        both_forms(gpu_ctx, d, TC.TIE_RECORDS, pr, pp, want)
    finally:
        d.close()


def test_long_record_against_the_longest_profile(case, gpu_ctx):
    """the 20 000-residue record of tests/test_gpu_hmm.py against M = 1238: 313 residue blocks, two domains, 75 MB of pointers"""
    import gsearch_amd as G
    rng = np.random.default_rng(17)
    c = case["cons"][1238]
    long_rec = R.background(rng, 6000) + c + R.background(rng, 5000) + c[:900] + R.background(rng, 20000 - 11000 - 1238 - 900)
    model = [m for m in case["models"] if m["M"] == 1238]
    text = [t for t, m in zip(case["texts"][2:], case["models"][2:]) if m["M"] == 1238]
    pr, pp = np.array([0, 2, 1], np.uint32), np.zeros(3, np.uint32)
    want = T.trace_pairs(model, [long_rec, b"", c], pr, pp, 4)
    assert want[1].tolist() == [2, 1, 0] and want[2][0, 0, :4].tolist() == [6001, 7238, 1, 1238] and want[2][0, 1, :4].tolist() == [12239, 13138, 1, 900]
    d = G.HmmDb(text, gpu_ctx, texts=True)
    try:
        both_forms(gpu_ctx, d, [long_rec, b"", c], pr, pp, want, max_dom=4)
    finally:
        d.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_block_loop_on_poisoned_scratch(case, main, gpu_ctx, byte):
    """max_block_cells that cuts the main set's pairs into many blocks, and one below a single pair's cells (a block then holds one pair), twice on
    scratch and allocations filled with a chosen byte: a block reads no pointer and no row that an earlier block or nobody wrote"""
    import gsearch_amd as G
    cells = sum(len(case["records"][r]) * 64 * K.F.group_size(case["models"][p]["M"]) for r, p in zip(main["pr"], main["pp"]))
    assert cells > 7 * 1_000_000 and 1038 * 64 * 20 > 1_000_000                  # seven blocks or more, one of them a single pair above the bound
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        d = G.HmmDb(case["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                for cap in (1_000_000, 1):
                    both_forms(gpu_ctx, d, case["records"], main["pr"], main["pp"], main["want"], max_block_cells=cap)
        finally:
            d.close()
    finally:
        G.debug_mem_fill(None)


def test_max_dom(case, db, gpu_ctx):
    rng = np.random.default_rng(1327)
    c = case["cons"][121]
    rec = R.background(rng, 8).join([c] * 5)
    pr, pp = np.array([0, 0], np.uint32), np.array([0, 1], np.uint32)
    full = T.trace_pairs(case["models"], [rec], pr, pp, 8)
    assert full[1][0] == 5 and [w[0] for w in full[2][0, :5]] == [1 + 129 * j for j in range(5)]
    for max_dom in (4, 0, 5):
        want = T.trace_pairs(case["models"], [rec], pr, pp, max_dom)
        assert want[1][0] == 5 and np.array_equal(want[2][0], full[2][0, :max_dom])
        both_forms(gpu_ctx, db, [rec], pr, pp, want, max_dom=max_dom)


def test_empty_pairs(case, db, gpu_ctx):
    """GS_HMM_NO_HIT pairs, empty records and records with a byte that is no residue (the packed forms: the Python layer filters such bytes away)"""
    c = case["cons"][121]
    recs = [c, b"", c[:40] + b"X" + c[41:], c[:64] + b"*", c.lower()]
    rl = np.array([len(r) for r in recs], np.uint64)
    rs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64)
    aa = np.frombuffer(b"".join(recs) + bytes(8), np.uint8)
    pr = np.array([0, R.NO_HIT, 1, 2, 3, 4, R.NO_HIT, 0], np.uint32)
    pp = np.array([0, 3, 0, 0, 9, 0, 0, 1], np.uint32)
    want = T.trace_pairs(case["models"], [c, b"", b"X", b"*", c], pr, pp, 3)
    assert (want[0][[1, 2, 3, 4, 6]] == R.NO_SCORE).all() and want[1].tolist() == [1, 0, 0, 0, 0, 1, 0, want[1][7]] and np.array_equal(want[2][0], want[2][5])
    assert same(db.trace_packed(aa, rs, rl, pr, pp, max_dom=3), want)
    assert same(trace_dev(gpu_ctx, db, pr, pp, packed=(aa, rs, rl), max_dom=3), want)
    # a pair list of empty pairs only, and no pair at all
    only = T.trace_pairs(case["models"], [c, b""], pr[1:3], pp[1:3], 2)
    assert same(db.trace_packed(aa, rs, rl, pr[1:3], pp[1:3], max_dom=2), only) and same(trace_dev(gpu_ctx, db, pr[1:3], pp[1:3], packed=(aa, rs, rl), max_dom=2), only)
    assert db.trace([c], np.zeros((0, 2), np.int64))[2].shape == (0, 8, 8)


def test_refusals_write_nothing(case, db, gpu_ctx):
    L = gpu_ctx.L
    aa = np.frombuffer(b"ACDEFGHIKL" * 4, np.uint8)
    rs, rl = np.array([0, 0, 10], np.uint64), np.array([10, T.TRACE_MAX_L + 1, 10], np.uint64)        # faked lengths: nothing reads record 1
    n_prof = len(db)

    def host(pr, pp):
        pr, pp = np.array(pr, np.uint32), np.array(pp, np.uint32)
        raw, nd, dom = np.full(len(pr), 77, np.int32), np.full(len(pr), 77, np.uint32), np.full((len(pr), 2, 8), 77, np.int32)
        rc = L.gs_hmm_trace(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, pr.ctypes.data, pp.ctypes.data, len(pr), 2, 0, raw.ctypes.data,
                            nd.ctypes.data, dom.ctypes.data)
        return rc, (raw == 77).all() and (nd == 77).all() and (dom == 77).all()

    for pr, pp, code in (([0, 3], [0, 0], GS_ERR_INVALID), ([0, 2], [0, n_prof], GS_ERR_INVALID), ([R.NO_HIT], [n_prof], GS_ERR_INVALID),
                         ([0, 1, 2], [0, 0, 0], GS_ERR_UNSUPPORTED)):
        assert host(pr, pp) == (code, True), (pr, pp)
        trace_dev(gpu_ctx, db, pr, pp, packed=(aa, rs, rl), max_dom=2, rc_want=code)                    # asserts the code and the canaries
    # an over-long record that no pair names is accepted
    pr, pp = np.array([2, 0, R.NO_HIT], np.uint32), np.array([1, 0, 0], np.uint32)
    want = T.trace_pairs(case["models"], [b"ACDEFGHIKL", b"", b"ACDEFGHIKL"], pr, pp, 2)
    assert same(db.trace_packed(aa, rs, rl, pr, pp, max_dom=2), want) and same(trace_dev(gpu_ctx, db, pr, pp, packed=(aa, rs, rl), max_dom=2), want)
    rl[1] = T.TRACE_MAX_L                                                        # the limit itself is not refused by the lengths (not run: the bytes do not exist)
    assert T.TRACE_MAX_L == 65536 == R.MAX_L // 4


def test_device_chain_from_best_hits(case, db, gpu_ctx):
    """search_dev -> best_hits_dev -> trace_dev: the [n_genomes][n_prof] matrix of best records is the pair list as it lies"""
    goff = GENOME_OFF[:5]
    ng, n_prof = len(goff) - 1, len(db)
    ga = np.array([m["ga_units"] for m in case["models"]], np.int32)
    wrec, _ = R.best_hits(case["want"], goff, ga)
    pp = np.tile(np.arange(n_prof, dtype=np.uint32), ng)
    want = T.trace_pairs(case["models"], case["records"], wrec.reshape(-1), pp, 4)
    assert (wrec == R.NO_HIT).sum() > 10 and (want[1] > 0).sum() == (wrec != R.NO_HIT).sum() >= 8
    d = _Dev(gpu_ctx, case["records"])
    try:
        p_score, p_rec, p_sc = d.out(d.n_rec * n_prof), d.out(ng * n_prof), d.out(ng * n_prof)
        p_goff, p_pp = gpu_ctx.alloc(goff.nbytes), gpu_ctx.alloc(pp.nbytes)
        d.outs += [p_goff, p_pp]
        gpu_ctx.upload(p_goff, goff); gpu_ctx.upload(p_pp, pp)
        db.search_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, p_score + 4 * GUARD)
        db.best_hits_dev(p_score + 4 * GUARD, d.n_rec, p_goff, ng, None, p_rec + 4 * GUARD, p_sc + 4 * GUARD)
        p_raw, p_nd, p_dom = d.out(ng * n_prof), d.out(ng * n_prof), d.out(ng * n_prof * 4 * 8)
        db.trace_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, p_rec + 4 * GUARD, p_pp, ng * n_prof, 4, p_raw + 4 * GUARD, p_nd + 4 * GUARD, p_dom + 4 * GUARD)
        assert np.array_equal(d.read(p_rec, (ng, n_prof), np.uint32), wrec)
        got = d.read(p_raw, (ng * n_prof,)), d.read(p_nd, (ng * n_prof,), np.uint32), d.read(p_dom, (ng * n_prof, 4, 8))
        assert same(got, want)
        assert np.array_equal(got[0], d.read(p_sc, (ng * n_prof,)))                # the raw of a traced best hit is its best score
    finally:
        d.free()


def test_the_length_limit(gpu_ctx):
    """b"W" * GS_HMM_TRACE_MAX_L against all_zero_model: M = 64 computed here, M = 1280 (84 million cells, one default block) from the golden file"""
    import gsearch_amd as G
    with open(os.path.join(HERE, "golden", "hmm_trace_limits.json")) as f:
        (gold,) = json.load(f)["cases"]
    assert (gold["kind"], gold["M"], gold["L"]) == ("zero", 1280, T.TRACE_MAX_L)
    texts = [K.limit_text("zero", 64), K.limit_text("zero", 1280)]
    assert K.sha256(texts[1]) == gold["sha256"], "the profile text is not the one the golden file was computed from"
    rec = b"W" * T.TRACE_MAX_L
    raw64, dom64 = T.trace(R.parse_hmm(texts[0])[0]["tables"], rec)
    n64, n1280 = len(dom64), len(gold["domains"])
    assert n64 > 1000 and 50 < n1280 < 64
    d = G.HmmDb(texts, gpu_ctx, texts=True)
    try:
        pr, pp = np.zeros(2, np.uint32), np.array([1, 0], np.uint32)
        host = d.trace([rec], np.stack([pr, pp], axis=1), max_dom=64)
        assert host[0].tolist() == [gold["raw"], raw64] and host[1].tolist() == [n1280, n64]
        assert host[2][0, :n1280].tolist() == gold["domains"] and (host[2][0, n1280:] == 0).all()
        assert host[2][1].tolist() == [list(w) for w in dom64[:64]]
        assert same(trace_dev(gpu_ctx, d, pr, pp, records=[rec], max_dom=64), host)
        assert np.array_equal(d.search([rec])[0, [1, 0]], host[0])
    finally:
        d.close()


def test_tables_of_hmmsearch_and_aligned_universal_genes(case, gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(1329)
    paths = [fixture_path(n) for n in FIXTURES]
    models = case["models"][:2]
    c0, c1 = case["cons"][121], case["cons"][57]
    seqs = [R.background(rng, 150), R.background(rng, 40) + c0 + R.background(rng, 25), c1 + R.background(rng, 30) + c1, c0[:80], R.background(rng, 90) + c1[10:],
            c0[:30] + c0[70:], R.background(rng, 40)]
    ids = ["prot%d" % i for i in range(len(seqs))]
    scores = R.search(models, seqs)
    listed = [(r, p) for p in range(2) for r in range(len(seqs)) if scores[r, p] != R.NO_SCORE and scores[r, p] >= 0]
    pr, pp = np.array([r for r, _ in listed], np.uint32), np.array([p for _, p in listed], np.uint32)
    raw, nd, dom = T.trace_pairs(models, seqs, pr, pp, 8)
    want = T.domain_table_bytes(models, ids, scores, raw, nd, dom, pr, pp)
    assert want.count(b"\n") >= 8 and b"prot1\tRibosomal_S9\tPF00380.20\t1\t1\t41\t161\t1\t121\t121\t" in want and b"\t2\t2\t" in want
    for gz in (False, True):
        faa, out, dout = str(tmp_path / ("p.faa.gz" if gz else "p.faa")), str(tmp_path / ("out%d.tsv" % gz)), str(tmp_path / ("dom%d.tsv" % gz))
        _write_faa(faa, ids, seqs, gz)
        got_ids, got_scores, table, dom_table = G.hmmsearch(faa, paths, out, ctx=gpu_ctx, domains=dout)
        assert got_ids == ids and np.array_equal(got_scores, scores) and table == R.table_bytes(models, ids, scores)
        assert dom_table == want and open(dout, "rb").read() == want
        assert len(G.hmmsearch(faa, paths, ctx=gpu_ctx)) == 3                      # without domains= the return value is what it was
    # the Forward table's pairs, the Viterbi path
    fres = G.hmmsearch(str(tmp_path / "p.faa"), paths, ctx=gpu_ctx, score="forward", domains=str(tmp_path / "fdom.tsv"))
    flisted = [(r, p) for p in range(2) for r in range(len(seqs)) if fres[1][r, p] != R.NO_SCORE and fres[1][r, p] >= 0]
    fpr, fpp = np.array([r for r, _ in flisted], np.uint32), np.array([p for _, p in flisted], np.uint32)
    assert fres[3] == T.domain_table_bytes(models, ids, fres[1], *T.trace_pairs(models, seqs, fpr, fpp, 8), fpr, fpp)
    # universal genes: the aligned region of every best hit, and the default still the whole protein
    genomes = [[R.background(rng, 100), seqs[2], c0[:100], seqs[1]], [R.background(rng, 60)], [seqs[5]]]
    files = []
    for g, gs in enumerate(genomes):
        files.append(str(tmp_path / ("g%d.faa" % g)))
        _write_faa(files[-1], ["g%d_%d" % (g, i) for i in range(len(gs))], gs)
    whole, local = G.universal_genes(files, paths, ctx=gpu_ctx)
    aligned, local2 = G.universal_genes(files, paths, ctx=gpu_ctx, region="aligned")
    assert whole == [[seqs[1], seqs[2]], [], [seqs[5]]] and np.array_equal(local, local2)
    assert aligned == [[c0, c1 + seqs[2][57:87] + c1], [], [seqs[5]]]
