"""The packed int16 Viterbi filter on the device (gs_hmm.hip, SPEC 13.7) against the numpy restatement (tests/pyref_hmm_vit16.py). Every score
comparison is `==` on int32 (the tables of hmmsearch(): on bytes); device outputs sit between canaries. The expected matrices are computed once per module.

The profile set (tests/hmm_vit16_case.py) has every kernel class, both sides of every class edge, M = 1, 2, 3 and 1 280, in an order that is a real
permutation of the classes. The records: lengths on both sides of the 64-residue block, a byte that is no residue, a record that overflows, and for every
profile two records that score through one deletion over most of the lanes in use without passing 64 bits - the lane scan of D carries their scores.
The properties of vf itself (vf >= vit, the measured excess, no hit lost on the reference's profiles) are asserted on the restatement alone in
tests/test_hmm_vit16_cpu.py; the device inherits them through `==`. The three lossless claims are held here byte for byte against the library's own
unfiltered and MSV-filtered searches."""
import numpy as np
import pytest

import hmm_classes_case as HC
import hmm_msv_case as MC
import hmm_vit16_case as VC
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_msv as V
import pyref_hmm_vit16 as W
from test_gpu_hmm import CANARY, GUARD, _Dev, _write_faa

pytestmark = pytest.mark.gpu
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3
INT32_MAX = (1 << 31) - 1
NO = R.NO_SCORE


@pytest.fixture(scope="module")
def case():
    """the set, its records, and what the restatement says of them: vf of every pair, the staged matrices without and with MSV in front"""
    ps = VC.profile_set()
    records = list(VC.set_records())
    models = ps["models"]
    mfl, vfl = V.floors(ps["stats"]), F.floors(models)
    plain = W.search_staged(models, records, vfl, forward=True, vit_floor=vfl)
    msv_first = W.search_staged(models, records, vfl, use_msv=True, msv_floor=mfl, forward=True, vit_floor=vfl)
    return dict(ps, records=records, packed=MC.pack(records), mfl=mfl, vfl=vfl, vf=plain[1], plain=plain, msv_first=msv_first)


@pytest.fixture(scope="module")
def db(case, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(case["texts"], gpu_ctx, texts=True)
    yield d
    d.close()


def _floor_dev(ctx, d, floor):
    if floor is None:
        return None
    fl = np.ascontiguousarray(floor, np.int32)
    p = ctx.alloc(max(fl.nbytes, 16))
    d.outs.append(p)
    ctx.upload(p, fl)
    return p


def vit16_dev(ctx, db, packed):
    """gs_hmm_search_vit16_dev on a guarded output"""
    d = _Dev(ctx, packed=packed)
    try:
        p = d.out(d.n_rec * len(db))
        db.search_vit16_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, p + 4 * GUARD)
        return d.read(p, (d.n_rec, len(db)))
    finally:
        d.free()


def staged_dev(ctx, db, packed, vf_floor, use_msv=False, msv_floor=None, vit_floor=None, forward=True, want_msv=True, want_vf=True):
    """gs_hmm_search_staged_dev on guarded outputs -> (msv or None, vf or None, vit, fwd or None)"""
    d = _Dev(ctx, packed=packed)
    try:
        n, shape = d.n_rec * len(db), (d.n_rec, len(db))
        want_msv = want_msv and use_msv
        pm, pw, pv, pf = (d.out(n) if want_msv else None), (d.out(n) if want_vf else None), d.out(n), (d.out(n) if forward else None)
        at = lambda p: None if p is None else p + 4 * GUARD        # noqa: E731
        db.search_staged_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, use_msv, _floor_dev(ctx, d, msv_floor), _floor_dev(ctx, d, vf_floor), _floor_dev(ctx, d, vit_floor),
                             at(pm), at(pw), at(pv), at(pf))
        rd = lambda p: None if p is None else d.read(p, shape)     # noqa: E731
        return rd(pm), rd(pw), rd(pv), rd(pf)
    finally:
        d.free()


def mismatches(got, want):
    return [(int(r), int(p), int(got[r, p]), int(want[r, p])) for r, p in np.argwhere(got != want)[:8]]


def same(got, want):
    """every matrix of a staged result that both sides have"""
    for g, w in zip(got, want):
        if g is not None and w is not None:
            assert g.dtype == np.int32 and not mismatches(g, w)


def check_vf(ctx, db, case):
    got = db.search_vit16_packed(*case["packed"])
    assert got.dtype == np.int32 and got.shape == case["vf"].shape and not mismatches(got, case["vf"])
    assert not mismatches(vit16_dev(ctx, db, case["packed"]), case["vf"])


def check_staged(ctx, db, case):
    """both kernel forms: k_hmm_vit16 over all records (no MSV) and k_hmm_vit16_sel over the MSV survivors, host and device entry points"""
    got = db.search_staged_packed(*case["packed"], case["vfl"], forward=True, floor=case["vfl"])
    same((None,) + got, case["plain"])
    same(staged_dev(ctx, db, case["packed"], case["vfl"], vit_floor=case["vfl"]), case["plain"])
    got = db.search_staged_packed(*case["packed"], case["vfl"], msv=True, msv_floor=case["mfl"], forward=True, floor=case["vfl"])
    same(got, case["msv_first"])
    same(staged_dev(ctx, db, case["packed"], case["vfl"], True, case["mfl"], case["vfl"]), case["msv_first"])
    # without Forward and without the matrices nobody asked for: the same Viterbi words
    same(staged_dev(ctx, db, case["packed"], case["vfl"], True, case["mfl"], None, forward=False, want_msv=False, want_vf=False), case["msv_first"])
    same(staged_dev(ctx, db, case["packed"], case["vfl"], forward=False, want_vf=False), case["plain"])


def test_vf_equals_the_restatement_in_every_class(case, db, gpu_ctx):
    want, recs = case["vf"], case["records"]
    assert want.shape == (len(recs), 22) and [len(r) for r in recs[:6]] == [0, 1, 63, 64, 65, 130]
    assert sorted(set(F.group_size(m["M"]) for m in case["models"])) == list(F.CLASS_G) and {1, 2, 3, 1280} <= set(VC.SET_M)
    check_vf(gpu_ctx, db, case)
    assert (want[[0, VC.BAD_RECORD]] == NO).all() and (np.delete(want, [0, VC.BAD_RECORD], axis=0) != NO).all()
    col = {M: p for p, M in enumerate(VC.SET_M)}
    assert want[VC.OVER_RECORD, col[300]] == W.VF_OVER and (want[VC.AFTER_OVER] != W.VF_OVER).all() and 1 <= (want == W.VF_OVER).sum() < 40
    # the deletion pairs score on their own profile, through the lane scan, without an overflow
    at = 10
    for M in VC.CASE_M:
        for r in VC.deletion_pair(case["cons"][M], M):
            assert recs[at] == r and 4 * 1024 < want[at, col[M]] < W.VF_OVER
            at += 1
    assert at == len(recs)


def test_staged_matrices_equal_the_restatement(case, db, gpu_ctx):
    _, vf, vit, fwd = case["plain"]
    msv, vf2, vit2, fwd2 = case["msv_first"]
    sel = W.passes(vf, case["vfl"])
    assert 0 < sel.sum() < sel.size and ((vit != NO) == sel).all() and 0 < (fwd != NO).sum() <= sel.sum()
    ran = V.passes(msv, case["mfl"])
    assert 0 < ran.sum() < ran.size and ((vf2 != NO) == ran).all() and np.array_equal(vf2[ran], vf[ran]) and (vit2 != NO).sum() <= (vit != NO).sum()
    check_staged(gpu_ctx, db, case)
    # the Viterbi words behind the filter are the words of the unfiltered search, and every pair at or above the floor is among them
    full = db.search_packed(*case["packed"])
    assert np.array_equal(vit[sel], full[sel]) and ((full != NO) & (full.astype(np.int64) >= case["vfl"][None, :].astype(np.int64)) <= sel).all()


def test_nothing_and_everything_selected(case, db, gpu_ctx):
    """an MSV floor of INT32_MAX: no list has an entry, every workgroup of k_hmm_vit16_sel and k_hmm_viterbi_sel returns before it stages anything.
    No floors at all: every pair that has a score runs through all stages - the words of the unfiltered searches"""
    top = np.full(len(db), INT32_MAX, np.int32)
    msv, vf, vit, fwd = db.search_staged_packed(*case["packed"], case["vfl"], msv=True, msv_floor=top, forward=True, filter_p=None)
    assert not mismatches(msv, case["msv_first"][0]) and (vf == NO).all() and (vit == NO).all() and (fwd == NO).all()
    dm, dvf, dvit, dfwd = staged_dev(gpu_ctx, db, case["packed"], case["vfl"], True, top, None)
    assert (dvf == NO).all() and (dvit == NO).all() and (dfwd == NO).all()
    # a vf floor of INT32_MAX takes the pairs that overflow and no other: GS_HMM_VF_OVER passes every floor
    vf, vit = db.search_staged_packed(*case["packed"], top)
    assert not mismatches(vf, case["vf"]) and ((vit != NO) == (case["vf"] == W.VF_OVER)).all()
    plain = db.search_packed(*case["packed"])
    _, plain_fwd = db.search_forward_packed(*case["packed"], filter_p=None)
    for use_msv in (False, True):
        got = db.search_staged_packed(*case["packed"], None, msv=use_msv, msv_p=None, forward=True, filter_p=None)
        assert not mismatches(got[-3], case["vf"]) and not mismatches(got[-2], plain) and not mismatches(got[-1], plain_fwd)
        got = staged_dev(gpu_ctx, db, case["packed"], None, use_msv)
        assert not mismatches(got[1], case["vf"]) and not mismatches(got[2], plain) and not mismatches(got[3], plain_fwd)


def test_tables16_byte_for_byte(case, db):
    for p, m in enumerate(case["models"]):
        got = db.tables16(p)
        assert got.dtype == np.int16 and got.shape == m["tables"].shape and got.tobytes() == W.tables16(m["tables"]).tobytes(), m["M"]
        assert np.array_equal(db.tables(p), m["tables"])
    buf = np.zeros(4, np.int16)
    assert db.ctx.L.gs_hmm_db_tables16(db.h, 0, buf.ctypes.data, buf.size) == GS_ERR_INVALID
    assert db.ctx.L.gs_hmm_db_tables16(db.h, len(db), buf.ctypes.data, buf.size) == GS_ERR_INVALID and (buf == 0).all()


def test_an_ordinary_record_behind_an_overflow_in_the_same_wavefront(gpu_ctx):
    """528 records: the eight wavefronts of the first workgroup take the eight overflowing records first and entries 512 .. 519 of the list by length
    after them. The early exit must leave no state behind, in k_hmm_vit16 and in k_hmm_vit16_sel (every pair selected)"""
    import gsearch_amd as G
    ps = VC.profile_set()
    keep = [VC.SET_M.index(M) for M in VC.REUSE_M]
    models = [ps["models"][p] for p in keep]
    recs = list(VC.wave_reuse_records())
    want = W.search(models, recs)
    assert (want[:8, 0] == W.VF_OVER).all() and (want[8:] != W.VF_OVER).all() and (want != NO).all()
    d = G.HmmDb([ps["texts"][p] for p in keep], gpu_ctx, texts=True)
    try:
        packed = MC.pack(recs)
        assert not mismatches(d.search_vit16_packed(*packed), want)
        assert not mismatches(vit16_dev(gpu_ctx, d, packed), want)
        msv, vf, vit = d.search_staged_packed(*packed, None, msv=True, msv_p=None)
        assert not mismatches(vf, want) and np.array_equal(vit, d.search_packed(*packed))
    finally:
        d.close()


def test_the_overflow_edge(gpu_ctx):
    """the profile that emits W alone, at no cost: the restatement puts the edge at n = 12 residues of W; n - 2 .. n + 1 on the device, with the
    int32 score behind each (everything selected: vf_floor = NULL)"""
    import gsearch_amd as G
    text = HC.limit_text("w_only", 64)
    tab = R.parse_hmm(text)[0]["tables"]
    recs = [b"W" * n for n in (10, 11, 12, 13)]
    want = [W.vit16(tab, r) for r in recs]
    assert want[2:] == [W.VF_OVER, W.VF_OVER] and W.VF_OVER not in want[:2] and want[1] == 60916
    d = G.HmmDb([text], gpu_ctx, texts=True)
    try:
        assert d.search_vit16(recs).reshape(-1).tolist() == want
        vf, vit = d.search_staged(recs, None)
        assert vf.reshape(-1).tolist() == want and vit.reshape(-1).tolist() == [R.viterbi(tab, r) for r in recs]
    finally:
        d.close()


def test_a_record_of_65537_residues(gpu_ctx):
    """past 2^16 rows, against one profile of class 2 (the restatement walks the rows once)"""
    import gsearch_amd as G
    ps = VC.profile_set()
    p = VC.SET_M.index(65)
    rec = R.background(np.random.default_rng(59), 65537)
    want = W.vit16(ps["models"][p]["tables"], rec)
    assert want not in (NO, W.VF_OVER)
    d = G.HmmDb([ps["texts"][p]], gpu_ctx, texts=True)
    try:
        assert d.search_vit16([rec]).tolist() == [[want]]
        assert 0 <= want - int(d.search([rec])[0, 0]) <= 65537
    finally:
        d.close()


def test_small_calls(case, db, gpu_ctx):
    """one record, no record"""
    one = MC.pack(case["records"][5:6])
    assert np.array_equal(db.search_vit16_packed(*one), case["vf"][5:6]) and np.array_equal(vit16_dev(gpu_ctx, db, one), case["vf"][5:6])
    assert np.array_equal(db.search_staged_packed(*one, case["vfl"])[1], case["plain"][2][5:6])
    assert db.search_vit16([]).shape == (0, len(db)) and [a.shape for a in db.search_staged([], None, msv=True, forward=True)] == [(0, len(db))] * 4
    p = gpu_ctx.alloc(64)
    try:
        db.search_vit16_dev(p, p, p, 0, p)
        db.search_staged_dev(p, p, p, 0, True, None, None, None, None, None, p, None)
    finally:
        gpu_ctx.free(p)


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_on_poisoned_scratch(case, gpu_ctx, byte):
    """every form above twice on scratch and allocations filled with a chosen byte: nothing reads what nothing wrote"""
    import gsearch_amd as G
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        d = G.HmmDb(case["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                check_vf(gpu_ctx, d, case)
                check_staged(gpu_ctx, d, case)
        finally:
            d.close()
    finally:
        G.debug_mem_fill(None)


def test_refusals_write_nothing(case, db, gpu_ctx):
    import gsearch_amd as G
    L = gpu_ctx.L
    aa = np.frombuffer(b"ACDEFGHIKL" * 4, np.uint8)
    n = 3 * len(db)
    for too_long, with_fwd in ((R.MAX_L + 1, False), (R.MAX_L + 1, True), (F.FWD_MAX_L + 1, True)):
        rs, rl = np.array([0, 0, 10], np.uint64), np.array([10, too_long, 10], np.uint64)
        d = _Dev(gpu_ctx, packed=(aa, rs, rl))
        try:
            pm, pw, pv, pf = d.out(n), d.out(n), d.out(n), d.out(n)
            for use_msv in (0, 1):
                rc = L.gs_hmm_search_staged_dev(gpu_ctx.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 3, use_msv, None, None, None, pm + 4 * GUARD, pw + 4 * GUARD, pv + 4 * GUARD,
                                                pf + 4 * GUARD if with_fwd else None)
                assert rc == GS_ERR_UNSUPPORTED
            if too_long > R.MAX_L:
                assert L.gs_hmm_search_vit16_dev(gpu_ctx.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 3, pw + 4 * GUARD) == GS_ERR_UNSUPPORTED
            for p in (pm, pw, pv, pf):
                assert (d.read(p, (3, len(db))) == CANARY).all()
        finally:
            d.free()
        m, w, v, f = (np.full((3, len(db)), k, np.int32) for k in (76, 77, 78, 79))
        rc = L.gs_hmm_search_staged(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, 1, None, None, None, m.ctypes.data, w.ctypes.data, v.ctypes.data,
                                    f.ctypes.data if with_fwd else None)
        assert rc == GS_ERR_UNSUPPORTED and (m == 76).all() and (w == 77).all() and (v == 78).all() and (f == 79).all()
        if too_long > R.MAX_L:
            assert L.gs_hmm_search_vit16(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, w.ctypes.data) == GS_ERR_UNSUPPORTED and (w == 77).all()
            with pytest.raises(G.GsError) as e:
                db.search_vit16_packed(aa, rs, rl)
            assert e.value.code == GS_ERR_UNSUPPORTED
    # a set of another context, a missing Viterbi output, and floors of the wrong length
    rs, rl = np.array([0], np.uint64), np.array([10], np.uint64)
    w, v = np.full((1, len(db)), 77, np.int32), np.full((1, len(db)), 78, np.int32)
    other = G.Context(0)
    try:
        assert other.L.gs_hmm_search_vit16(other.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, w.ctypes.data) == GS_ERR_INVALID
        assert other.L.gs_hmm_search_staged(other.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, 0, None, None, None, None, w.ctypes.data, v.ctypes.data, None) == GS_ERR_INVALID
    finally:
        other.close()
    assert L.gs_hmm_search_staged(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, 0, None, None, None, None, w.ctypes.data, None, None) == GS_ERR_INVALID
    assert (w == 77).all() and (v == 78).all()
    with pytest.raises(ValueError):
        db.search_staged([b"ACD"], np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        db.search_staged([b"ACD"], None, msv=True, msv_floor=np.zeros(3, np.int32))


def _rows(table):
    return table.split(b"\n")[1:-1]


def test_hmmsearch_behind_vit16_is_hmmsearch(gpu_ctx, tmp_path):
    """the lossless claim on a .faa with planted hits in background: with prefilter="vit16" the tables of hmmsearch() byte for byte, with
    "msv+vit16" those of prefilter="msv", for both scores - and the filter does leave pairs out"""
    import gsearch_amd as G
    paths = [MC.fixture_path(n) for n in MC.FIXTURES]
    models = MC.fixtures()["models"]
    ids, seqs = MC.faa_case()
    seqs = list(seqs)
    faa = str(tmp_path / "p.faa")
    _write_faa(faa, ids, seqs)
    vf = W.search(models, seqs)
    for score in ("viterbi", "forward"):
        floor = F.floors(models) if score == "forward" else np.zeros(len(models), np.int32)
        _, plain, table = G.hmmsearch(faa, paths, ctx=gpu_ctx, score=score)
        out = str(tmp_path / ("out_%s.tsv" % score))
        got_ids, got, got_table = G.hmmsearch(faa, paths, out, ctx=gpu_ctx, score=score, prefilter="vit16")
        assert got_ids == ids and got_table == table and open(out, "rb").read() == table and len(_rows(table)) >= 2
        ran = W.passes(vf, floor)
        if score == "viterbi":
            assert np.array_equal(got, np.where(ran, plain, NO)) and 0 < ran.sum() < ran.size
        else:
            assert np.array_equal(got, plain)          # Forward runs behind the same Viterbi floor either way
        _, msv_scores, msv_table = G.hmmsearch(faa, paths, ctx=gpu_ctx, score=score, prefilter="msv")
        _, both, both_table = G.hmmsearch(faa, paths, ctx=gpu_ctx, score=score, prefilter="msv+vit16")
        assert both_table == msv_table and (both != NO).sum() <= (msv_scores != NO).sum() and np.array_equal(both[both != NO], msv_scores[both != NO])
    for bad in ("ssv", "vit16+msv", "viterbi", ""):
        with pytest.raises(ValueError):
            G.hmmsearch(faa, paths, ctx=gpu_ctx, prefilter=bad)
        with pytest.raises(ValueError):
            G.universal_genes([faa], paths, ctx=gpu_ctx, prefilter=bad)
    for pre in ("vit16", "msv+vit16"):                 # nothing to cut by
        with pytest.raises(ValueError):
            G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward", filter_p=None, prefilter=pre)
        with pytest.raises(ValueError):
            G.universal_genes([faa], paths, ctx=gpu_ctx, score="forward", filter_p=None, prefilter=pre)


def test_universal_genes_and_translated_targets_behind_vit16(gpu_ctx, tmp_path):
    """one genome with two planted genes, as proteins and as contigs for the gene caller and the six-frame ORFs"""
    import gsearch_amd as G
    from test_gpu_gene import _write_fa
    paths = [MC.fixture_path(n) for n in MC.FIXTURES]
    cons = MC.fixtures()["cons"]
    contigs, proteins = MC.genome_case()
    faa, fna = str(tmp_path / "g.faa"), str(tmp_path / "g.fna")
    _write_faa(faa, ["gene%d" % i for i in range(len(proteins))], proteins)
    _write_fa(fna, ["c%d" % i for i in range(len(contigs))], contigs)
    for score in ("viterbi", "forward"):
        ref, ref_local = G.universal_genes([faa], paths, ctx=gpu_ctx, score=score)
        got, local = G.universal_genes([faa], paths, ctx=gpu_ctx, score=score, prefilter="vit16")
        assert got == ref == [[b"M" + cons[0], b"M" + cons[1]]] and np.array_equal(local, ref_local)
        ref_m = G.universal_genes([faa], paths, ctx=gpu_ctx, score=score, prefilter="msv")
        got_m = G.universal_genes([faa], paths, ctx=gpu_ctx, score=score, prefilter="msv+vit16")
        assert got_m[0] == ref_m[0] and np.array_equal(got_m[1], ref_m[1])
    # translated targets, once: the genes of the self-trained caller, both entry points
    ref = G.universal_genes([fna], paths, ctx=gpu_ctx, translate="genes")
    got = G.universal_genes([fna], paths, ctx=gpu_ctx, translate="genes", prefilter="vit16")
    assert got[0] == ref[0] and len(got[0][0]) == 2 and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    ids_u, sc_u, tab_u = G.hmmsearch(fna, paths, ctx=gpu_ctx, translate="genes")
    ids_f, sc_f, tab_f = G.hmmsearch(fna, paths, ctx=gpu_ctx, translate="genes", prefilter="vit16")
    assert ids_f == ids_u and tab_f == tab_u and len(_rows(tab_u)) >= 2
    ran = sc_f != NO
    assert np.array_equal(sc_f[ran], sc_u[ran]) and 0 < ran.sum() < (sc_u != NO).sum()
    ids_m, sc_m, tab_m = G.hmmsearch(fna, paths, ctx=gpu_ctx, score="forward", translate=True, prefilter="msv")
    ids_b, sc_b, tab_b = G.hmmsearch(fna, paths, ctx=gpu_ctx, score="forward", translate=True, prefilter="msv+vit16")
    assert ids_b == ids_m and tab_b == tab_m and np.array_equal(sc_b, sc_m)
