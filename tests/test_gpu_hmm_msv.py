"""The MSV prefilter on the device (gs_hmm.hip, SPEC 13.3) against the numpy restatement (tests/pyref_hmm_msv.py). Every score comparison is `==` on
int32 (the tables of hmmsearch(): on bytes); device outputs sit between canaries. The expected matrices are computed once per module.

The profile set is that of the class tests plus M = 1 and 2 (tests/hmm_msv_case.py): every kernel class, both sides of every class edge, lanes that
hold padding only - the staged copy of k_hmm_msv holds its own padding word there, and the fold into E has no select - and a set order that is a real
permutation. The records: lengths on both sides of the 64-residue block, a byte that is no residue, two consensus copies apart (the J state carries
the score), a consensus piece across a lane edge of every class, an entry at node 1 and an exit at node M, and two records that score through long
deletions (parity only: the filter may lose them, which is its stated cost).

The end-to-end tests lean on a condition that tests/test_hmm_msv_cpu.py asserts on the restatement alone: no pair of their planted inputs at or above
the gathering cutoff falls below the MSV floor of P = 0.02."""
import numpy as np
import pytest

import hmm_msv_case as MC
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_msv as V
from test_gpu_hmm import CANARY, GUARD, _Dev, _write_faa

pytestmark = pytest.mark.gpu
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3
INT32_MAX = (1 << 31) - 1
NO = R.NO_SCORE


@pytest.fixture(scope="module")
def case():
    """the set, its records, and what the restatement says of them: MSV of every pair; Viterbi and Forward behind the floors of P = 0.02 and 1e-3"""
    ps = MC.profile_set()
    records = list(MC.set_records())
    models = ps["models"]
    msv = V.search(models, records)
    mfl, vfl = V.floors(ps["stats"]), F.floors(models)
    _, vit, fwd = V.search_filtered(models, records, floor=mfl, forward=True, vit_floor=vfl, msv=msv)
    return dict(ps, records=records, packed=MC.pack(records), msv=msv, mfl=mfl, vfl=vfl, vit=vit, fwd=fwd)


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


def msv_dev(ctx, db, packed):
    """gs_hmm_search_msv_dev on a guarded output"""
    d = _Dev(ctx, packed=packed)
    try:
        p = d.out(d.n_rec * len(db))
        db.search_msv_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, p + 4 * GUARD)
        return d.read(p, (d.n_rec, len(db)))
    finally:
        d.free()


def filtered_dev(ctx, db, packed, msv_floor=None, vit_floor=None, forward=True, want_msv=True):
    """gs_hmm_search_filtered_dev on guarded outputs -> (msv or None, vit, fwd or None)"""
    d = _Dev(ctx, packed=packed)
    try:
        n, shape = d.n_rec * len(db), (d.n_rec, len(db))
        pm, pv, pf = (d.out(n) if want_msv else None), d.out(n), (d.out(n) if forward else None)
        db.search_filtered_dev(d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, _floor_dev(ctx, d, msv_floor), _floor_dev(ctx, d, vit_floor),
                               pm + 4 * GUARD if want_msv else None, pv + 4 * GUARD, pf + 4 * GUARD if forward else None)
        return (d.read(pm, shape) if want_msv else None), d.read(pv, shape), (d.read(pf, shape) if forward else None)
    finally:
        d.free()


def mismatches(got, want):
    return [(int(r), int(p), int(got[r, p]), int(want[r, p])) for r, p in np.argwhere(got != want)[:8]]


def check_msv(ctx, db, case):
    got = db.search_msv_packed(*case["packed"])
    assert got.dtype == np.int32 and got.shape == case["msv"].shape and not mismatches(got, case["msv"])
    assert not mismatches(msv_dev(ctx, db, case["packed"]), case["msv"])


def check_filtered(ctx, db, case):
    want = (case["msv"], case["vit"], case["fwd"])
    got = db.search_filtered_packed(*case["packed"], msv_floor=case["mfl"], forward=True, floor=case["vfl"])
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and not mismatches(g, w)
    for g, w in zip(filtered_dev(ctx, db, case["packed"], case["mfl"], case["vfl"]), want):
        assert not mismatches(g, w)
    # without Forward and without the MSV matrix: the same Viterbi words
    m2, v2 = db.search_filtered_packed(*case["packed"], msv_floor=case["mfl"])
    assert not mismatches(m2, case["msv"]) and not mismatches(v2, case["vit"])
    assert not mismatches(filtered_dev(ctx, db, case["packed"], case["mfl"], None, forward=False, want_msv=False)[1], case["vit"])


def check_unfiltered(ctx, db, case):
    """msv_floor = NULL: every pair that has an MSV score - the words of gs_hmm_search and gs_hmm_search_forward for the same input"""
    plain = db.search_packed(*case["packed"])
    _, plain_fwd = db.search_forward_packed(*case["packed"], filter_p=None)
    msv, vit, fwd = db.search_filtered_packed(*case["packed"], msv_p=None, forward=True, filter_p=None)
    assert not mismatches(msv, case["msv"]) and not mismatches(vit, plain) and not mismatches(fwd, plain_fwd)
    dmsv, dvit, dfwd = filtered_dev(ctx, db, case["packed"])
    assert not mismatches(dmsv, case["msv"]) and not mismatches(dvit, plain) and not mismatches(dfwd, plain_fwd)
    return plain


def test_msv_matrix_equals_the_restatement(case, db, gpu_ctx):
    want, recs = case["msv"], case["records"]
    assert want.shape == (len(recs), 21) and 22 <= len(recs) <= 28 and [len(r) for r in recs[:7]] == [0, 1, 63, 64, 65, 129, 200]
    assert sorted(set(F.group_size(m["M"]) for m in case["models"])) == list(MC.CLASS_Q)            # every class has a profile
    check_msv(gpu_ctx, db, case)
    assert (want[[0, MC.BAD_RECORD, len(recs) - 1]] == NO).all() and (np.delete(want, [0, MC.BAD_RECORD, len(recs) - 1], axis=0) != NO).all()
    col = {M: p for p, M in enumerate(MC.SET_M)}
    # the J state carries the second copy: two copies score far above one
    one = V.msv(case["models"][col[300]]["tables"], recs[8][:80])
    assert want[8, col[300]] > one + 20 * 1024
    # the pieces across a lane edge, at node 1 and at node M score on their own profile, far above its floor
    for j, q in enumerate(MC.CLASS_Q[1:]):
        assert want[9 + j, col[MC.Q_PROFILE[q]]] > case["mfl"][col[MC.Q_PROFILE[q]]] + 10 * 1024, q
    assert want[17, col[513]] > 20 * 1024 and want[18, col[513]] > 20 * 1024


def test_filtered_search_equals_the_restatement(case, db, gpu_ctx):
    sel = V.passes(case["msv"], case["mfl"])
    assert 0 < sel.sum() < sel.size and sel.any(axis=0).sum() >= 15 and (~sel).any(axis=0).all()      # profiles with and without selected records
    assert ((case["vit"] != NO) == sel).all() and 0 < (case["fwd"] != NO).sum() <= sel.sum()
    assert np.array_equal(db.msv_floor(0.02), case["mfl"]) and np.array_equal(db.msv_floor(1e-3), V.floors(case["stats"], 1e-3))
    check_filtered(gpu_ctx, db, case)
    # the default floors of the keywords are these
    got = db.search_filtered_packed(*case["packed"], forward=True)
    assert not mismatches(got[1], case["vit"]) and not mismatches(got[2], case["fwd"])


def test_selected_viterbi_equals_plain_viterbi(case, db, gpu_ctx):
    plain = check_unfiltered(gpu_ctx, db, case)
    sel = V.passes(case["msv"], case["mfl"])
    _, vit = db.search_filtered_packed(*case["packed"], msv_floor=case["mfl"])
    assert np.array_equal(vit[sel], plain[sel]) and (vit[~sel] == NO).all() and (plain[sel] != NO).all()


def test_nothing_selected_in_any_class(case, db, gpu_ctx):
    """a floor of INT32_MAX: every workgroup of every class returns before it stages anything, and the fills alone write the outputs"""
    top = np.full(len(db), INT32_MAX, np.int32)
    msv, vit, fwd = db.search_filtered_packed(*case["packed"], msv_floor=top, forward=True, filter_p=None)
    assert not mismatches(msv, case["msv"]) and (vit == NO).all() and (fwd == NO).all()
    dmsv, dvit, dfwd = filtered_dev(gpu_ctx, db, case["packed"], top, None)
    assert not mismatches(dmsv, case["msv"]) and (dvit == NO).all() and (dfwd == NO).all()


def test_small_calls(case, db, gpu_ctx):
    """one record, no record, and a set of one profile"""
    import gsearch_amd as G
    one = MC.pack(case["records"][6:7])
    assert np.array_equal(db.search_msv_packed(*one), case["msv"][6:7]) and np.array_equal(msv_dev(gpu_ctx, db, one), case["msv"][6:7])
    assert np.array_equal(db.search_filtered_packed(*one, msv_floor=case["mfl"])[1], case["vit"][6:7])
    assert db.search_msv([]).shape == (0, len(db)) and [a.shape for a in db.search_filtered([], forward=True)] == [(0, len(db))] * 3
    p = gpu_ctx.alloc(64)
    try:
        db.search_msv_dev(p, p, p, 0, p)
        db.search_filtered_dev(p, p, p, 0, None, None, None, p, None)
    finally:
        gpu_ctx.free(p)
    solo = G.HmmDb(case["texts"][2:3], gpu_ctx, texts=True)                     # M = 1280 alone
    try:
        recs = [r for i, r in enumerate(case["records"]) if i != MC.BAD_RECORD]
        keep = [i for i in range(len(case["records"])) if i != MC.BAD_RECORD]
        assert np.array_equal(solo.search_msv(recs), case["msv"][keep, 2:3])
        m, v = solo.search_filtered(recs, msv_floor=case["mfl"][2:3])
        assert np.array_equal(m, case["msv"][keep, 2:3]) and np.array_equal(v, case["vit"][keep, 2:3])
    finally:
        solo.close()


def test_cells_at_the_top_of_the_range(gpu_ctx):
    """GS_HMM_MAX_L residues of W against the profile whose file holds 0.00000 everywhere, M = 65: every row adds 6 608 units, the cells end near
    1.7 * 10^9, and lanes 33 .. 63 of class 2 hold padding only - the padding word of the staged copy must stay below every E up to here, with no
    clamp and no select in the row loop (gs_hmm.hip). One pair; the restatement walks the 2^18 rows once."""
    import gsearch_amd as G
    import hmm_classes_case as HC
    text = R.write_hmm(HC.all_zero_model(65))
    rec = b"W" * R.MAX_L
    want = V.msv(R.parse_hmm(text)[0]["tables"], rec)
    assert want > 1_600_000_000
    d = G.HmmDb([text], gpu_ctx, texts=True)
    try:
        assert d.search_msv([rec]).tolist() == [[want]]
        msv, vit = d.search_filtered([rec], msv_p=None)
        assert msv.tolist() == [[want]] and np.array_equal(vit, d.search([rec]))
    finally:
        d.close()


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
                check_msv(gpu_ctx, d, case)
                check_filtered(gpu_ctx, d, case)
                check_unfiltered(gpu_ctx, d, case)
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
            pm, pv, pf = d.out(n), d.out(n), d.out(n)
            rc = L.gs_hmm_search_filtered_dev(gpu_ctx.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 3, None, None, pm + 4 * GUARD, pv + 4 * GUARD, pf + 4 * GUARD if with_fwd else None)
            assert rc == GS_ERR_UNSUPPORTED
            if too_long > R.MAX_L:
                assert L.gs_hmm_search_msv_dev(gpu_ctx.h, db.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], 3, pm + 4 * GUARD) == GS_ERR_UNSUPPORTED
            for p in (pm, pv, pf):
                assert (d.read(p, (3, len(db))) == CANARY).all()
        finally:
            d.free()
        m, v, f = (np.full((3, len(db)), k, np.int32) for k in (76, 77, 78))
        rc = L.gs_hmm_search_filtered(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, None, None, m.ctypes.data, v.ctypes.data, f.ctypes.data if with_fwd else None)
        assert rc == GS_ERR_UNSUPPORTED and (m == 76).all() and (v == 77).all() and (f == 78).all()
        if too_long > R.MAX_L:
            assert L.gs_hmm_search_msv(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, m.ctypes.data) == GS_ERR_UNSUPPORTED and (m == 76).all()
            with pytest.raises(G.GsError) as e:
                db.search_msv_packed(aa, rs, rl)
            assert e.value.code == GS_ERR_UNSUPPORTED
    # a set of another context, and floors of the wrong length
    rs, rl = np.array([0], np.uint64), np.array([10], np.uint64)
    other = G.Context(0)
    try:
        m, v = np.full((1, len(db)), 76, np.int32), np.full((1, len(db)), 77, np.int32)
        assert other.L.gs_hmm_search_msv(other.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, m.ctypes.data) == GS_ERR_INVALID
        assert other.L.gs_hmm_search_filtered(other.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, None, None, m.ctypes.data, v.ctypes.data, None) == GS_ERR_INVALID
        assert (m == 76).all() and (v == 77).all()
    finally:
        other.close()
    with pytest.raises(ValueError):
        db.search_filtered([b"ACD"], msv_floor=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        db.search_filtered([b"ACD"], forward=True, floor=np.zeros(3, np.int32))


def _rows(table):
    return table.split(b"\n")[1:-1]


def _is_ordered_subset(sub, full):
    it = iter(full)
    return all(any(x == y for y in it) for x in sub)


def test_hmmsearch_behind_the_prefilter(gpu_ctx, tmp_path):
    import gsearch_amd as G
    fx = MC.fixtures()
    paths = [MC.fixture_path(n) for n in MC.FIXTURES]
    models, stats = fx["models"], fx["stats"]
    ids, seqs = MC.faa_case()
    seqs = list(seqs)
    faa = str(tmp_path / "p.faa")
    _write_faa(faa, ids, seqs)
    mfl = V.floors(stats)
    msv, vit, fwd = V.search_filtered(models, seqs, floor=mfl, forward=True, vit_floor=F.floors(models))
    sel = V.passes(msv, mfl)
    full_v = R.search(models, seqs)
    full_f = F.search_forward(models, seqs, floor=F.floors(models), vit=full_v)[1]
    for score, want_scores, want, full in (("viterbi", vit, R.table_bytes(models, ids, vit), R.table_bytes(models, ids, full_v)),
                                           ("forward", fwd, F.table_bytes(models, stats, ids, fwd), F.table_bytes(models, stats, ids, full_f))):
        out = str(tmp_path / ("out_%s.tsv" % score))
        got_ids, scores, table = G.hmmsearch(faa, paths, out, ctx=gpu_ctx, score=score, prefilter="msv")
        assert got_ids == ids and np.array_equal(scores, want_scores) and table == want and open(out, "rb").read() == want
        # byte for byte the rows of the unfiltered table whose pairs pass the floor (Z is still the number of records), every pass_ga = 1 row among them
        assert G.hmmsearch(faa, paths, ctx=gpu_ctx, score=score)[2] == full
        keep = [ln for ln in _rows(full) if sel[ids.index(ln.split(b"\t")[0].decode()), [m["name"] for m in models].index(ln.split(b"\t")[1].decode())]]
        assert _rows(table) == keep and 0 < len(keep) <= len(_rows(full)) and (want_scores == NO).sum() > (full_v == NO).sum()
        assert [ln for ln in _rows(full) if ln.endswith(b"\t1")] == [ln for ln in keep if ln.endswith(b"\t1")] and any(ln.endswith(b"\t1") for ln in keep)
    # msv_p = None: every pair - the unfiltered table
    assert G.hmmsearch(faa, paths, ctx=gpu_ctx, prefilter="msv", msv_p=None)[2] == R.table_bytes(models, ids, full_v)
    with pytest.raises(ValueError):
        G.hmmsearch(faa, paths, ctx=gpu_ctx, prefilter="ssv")
    with pytest.raises(ValueError):
        G.universal_genes([faa], paths, ctx=gpu_ctx, prefilter="viterbi")


def test_universal_genes_and_translated_targets_behind_the_prefilter(gpu_ctx, tmp_path):
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
        got, local = G.universal_genes([faa], paths, ctx=gpu_ctx, score=score, prefilter="msv")
        ref, ref_local = G.universal_genes([faa], paths, ctx=gpu_ctx, score=score)
        assert got == ref == [[b"M" + cons[0], b"M" + cons[1]]] and np.array_equal(local, ref_local) and local.tolist() == [[16 + 7, 32 + 7]]
        got = G.universal_genes([fna], paths, ctx=gpu_ctx, score=score, translate="genes", prefilter="msv")
        ref = G.universal_genes([fna], paths, ctx=gpu_ctx, score=score, translate="genes")
        assert got[0] == ref[0] and len(got[0][0]) == 2 and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and (got[1] != R.NO_HIT).all()
    # hmmsearch on the translated forms: the rows of the unfiltered table that the filter keeps, every pass_ga = 1 row among them, the same scores
    for translate in ("genes", True):
        for score in ("viterbi", "forward"):
            ids_f, sc_f, tab_f = G.hmmsearch(fna, paths, ctx=gpu_ctx, score=score, translate=translate, prefilter="msv")
            ids_u, sc_u, tab_u = G.hmmsearch(fna, paths, ctx=gpu_ctx, score=score, translate=translate)
            assert ids_f == ids_u and sc_f.shape == sc_u.shape and len(ids_f) > 40
            ran = sc_f != NO
            assert np.array_equal(sc_f[ran], sc_u[ran]) and 0 < ran.sum() <= (sc_u != NO).sum()
            assert score == "forward" or ran.sum() < (sc_u != NO).sum()            # (Forward's own Viterbi floor may leave no pair for MSV to take out)
            assert _is_ordered_subset(_rows(tab_f), _rows(tab_u))
            ga1 = [ln for ln in _rows(tab_u) if ln.endswith(b"\t1")]
            assert len(ga1) == 2 and [ln for ln in _rows(tab_f) if ln.endswith(b"\t1")] == ga1
