"""The null2 bias correction of SPEC 13.5 on the device (k_hmm_n2_forward<Q>, k_hmm_n2_backward<Q>, k_hmm_n2_flag, k_hmm_n2_fill and k_hmm_n2_seq of
gs_hmm.hip, gs_hmm_null2 / gs_hmm_null2_dev) against the numpy restatement tests/pyref_hmm_null2.py. Every comparison is `==` on int32 or on bytes,
through the host form and the device form: the slot words {corr, dom_bias, seg_raw, mass}, seq_bias, the n2 vectors and the occM / occI rows; every
device output sits between canaries. The expected values are computed once per module.

What is chosen here: the envelopes are inputs, so the segments are put where the kernels can go wrong - Forward loads residues 64 at a time from the
segment's start and Backward from its end, so Ld sits on both sides of that edge and one segment is a single row, each as a whole record and inside a
longer one; the slots of a call are cut into blocks and grouped by profile, so the pair lists are shuffled and hold repeats, pairs with two and three
envelopes, one whose n_env is above max_env, and the three kinds of pair that get nothing; a profile of one node has no insert state at all."""
import numpy as np
import pytest

import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_null2 as N
import pyref_hmm_posterior as P
import pyref_orf as O
from test_gpu_hmm import CANARY, FIXTURES, GUARD, _Dev, _write_faa, fixture_path  # noqa: F401
from test_gpu_hmm_posterior import pack

pytestmark = pytest.mark.gpu
GS_OK, GS_ERR_INVALID, GS_ERR_UNSUPPORTED = 0, -1, -3
MAX_ENV = 3


def occ_offsets(models, pr, pp, ne, max_env):
    """occ_off as HmmDb.null2_packed lays the rows out: the listed slots of a pair one after the other, M words each"""
    words = [min(int(n), max_env) * (models[int(p)]["M"] if int(p) < len(models) else 0) for n, p in zip(ne, pp)]
    return np.concatenate([[0], np.cumsum(words)]).astype(np.uint64)


def null2_dev(ctx, d_b, models, pair_rec, pair_prof, n_env, env, packed, max_block_cells=0, rc_want=GS_OK, extras=True, occ_off=None):
    """gs_hmm_null2_dev on guarded outputs -> (slots, seq_bias, n2, occM rows, occI rows) in the shapes of HmmDb.null2_packed; with rc_want another code:
    that code is returned and the outputs hold the canary"""
    d = _Dev(ctx, packed=packed)
    try:
        pr, pp = np.ascontiguousarray(pair_rec, np.uint32), np.ascontiguousarray(pair_prof, np.uint32)
        ne, env = np.ascontiguousarray(n_env, np.uint32), np.ascontiguousarray(env, np.int32)
        n, max_env = len(pr), env.shape[1]
        oo = occ_offsets(models, pr, pp, ne, max_env) if occ_off is None else np.ascontiguousarray(occ_off, np.uint64)
        ups = []
        for a in (pr, pp, ne, env, oo):
            d.outs.append(ctx.alloc(max(a.nbytes, 16)))
            if a.nbytes:
                ctx.upload(d.outs[-1], a)
            ups.append(d.outs[-1])
        nrow = int(oo[-1])
        p_s, p_b, p_v, p_m, p_i = d.out(n * max_env * N.N2_WORDS), d.out(n), d.out(n * max_env * 20), d.out(nrow), d.out(nrow)
        g = 4 * GUARD
        rc = ctx.L.gs_hmm_null2_dev(ctx.h, d_b.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, ups[0], ups[1], n, max_env, max_block_cells, ups[2], ups[3], p_s + g, p_b + g,
                                    (p_v + g) if extras else None, ups[4] if extras else None, (p_m + g) if extras else None, (p_i + g) if extras else None)
        assert rc == rc_want, rc
        slots, sb, v = d.read(p_s, (n, max_env, N.N2_WORDS)), d.read(p_b, (n,)), d.read(p_v, (n, max_env, 20))
        om, oi = d.read(p_m, (nrow,)), d.read(p_i, (nrow,))
        if rc != GS_OK or not extras:
            assert (v == CANARY).all() and (om == CANARY).all() and (oi == CANARY).all()
        if rc != GS_OK:
            assert (slots == CANARY).all() and (sb == CANARY).all()
        return slots, sb, v, om, oi, oo
    finally:
        d.free()


def rows_equal(flat, oo, models, pp, want_rows, untouched):
    """the flat row buffer of a device form against the restatement's per-pair lists; the words of a pair that gets none keep what was there"""
    for j, rows in enumerate(want_rows):
        got = flat[int(oo[j]):int(oo[j + 1])]
        if rows:
            if not np.array_equal(got, np.concatenate(rows)):
                return False
        elif not (got == untouched).all():
            return False
    return True


def both_forms(ctx, d_b, models, records, pr, pp, ne, env, want, max_block_cells=0):
    """the host form and the device form, n2 vectors and rows included, against the restatement"""
    packed = pack(records)
    w_slots, w_sb, w_n2, w_om, w_oi = want
    host = d_b.null2_packed(*packed, pr, pp, ne, env, n2=True, occ=True, max_block_cells=max_block_cells)
    bad = np.flatnonzero((host[0] != w_slots).any(axis=(1, 2)) | (host[1] != w_sb))
    assert len(bad) == 0, [(int(pr[j]), int(pp[j]), int(ne[j]), env[j, :, :2].tolist(), host[0][j].tolist(), w_slots[j].tolist(), int(host[1][j]), int(w_sb[j])) for j in bad[:3]]
    assert host[0].dtype == np.int32 and host[1].dtype == np.int32 and np.array_equal(host[2], w_n2)
    for got_rows, want_rows in ((host[3], w_om), (host[4], w_oi)):
        for j, (g, w) in enumerate(zip(got_rows, want_rows)):
            assert g.dtype == np.int32 and g.shape == (len(w), models[int(pp[j])]["M"]) and (len(w) == 0 or np.array_equal(g, np.stack(w))), j
    slots, sb, v, om, oi, oo = null2_dev(ctx, d_b, models, pr, pp, ne, env, packed, max_block_cells=max_block_cells)
    assert np.array_equal(slots, w_slots) and np.array_equal(sb, w_sb) and np.array_equal(v, w_n2)
    assert rows_equal(om, oo, models, pp, w_om, CANARY) and rows_equal(oi, oo, models, pp, w_oi, CANARY)
    plain = d_b.null2_packed(*packed, pr, pp, ne, env, max_block_cells=max_block_cells)                      # without the optional outputs
    assert len(plain) == 2 and np.array_equal(plain[0], w_slots) and np.array_equal(plain[1], w_sb)
    slots, sb = null2_dev(ctx, d_b, models, pr, pp, ne, env, packed, max_block_cells=max_block_cells, extras=False)[:2]
    assert np.array_equal(slots, w_slots) and np.array_equal(sb, w_sb)
    return host


@pytest.fixture(scope="module")
def small():
    """the two real profiles and synthetic ones of 1, 2, 65 and 129 nodes; segments of 1, 63, 64, 65 and 130 rows as whole records and inside a record of
    200; the envelopes SPEC 13.4 finds in records with two copies; an empty record, one with a byte that is no residue, GS_HMM_NO_HIT; shuffled, with
    repeats"""
    rng = np.random.default_rng(1353)
    texts = [open(fixture_path(n), "rb").read() for n in FIXTURES] + [R.write_hmm(R.synth_model(rng, M)) for M in (1, 2, 65, 129)]
    models = [m for t in texts for m in R.parse_hmm(t)]
    c0, c1 = (R.consensus(m["tables"]) for m in models[:2])
    bg = lambda n: R.background(rng, n)                                                         # noqa: E731
    records = [bg(1), bg(63), bg(64), bg(65), bg(130), bg(200), c0 + c0, c1 + bg(30) + c1, b"", c0[:40] + b"\xff" + c0[41:]]
    entries = []                                                                                # (record, n_env as given, the envelopes given)
    for r in range(5):
        entries.append((r, 1, [(1, len(records[r]))]))
    entries += [(5, 4, [(3, 3), (5, 67), (7, 70)]),                                             # n_env above max_env: three are listed
                (5, 2, [(9, 73), (11, 140)]), (5, 1, [(200, 200)]), (6, None, None), (7, None, None), (8, 0, []), (9, 1, [(1, 10)]), (R.NO_HIT, 2, [(1, 5), (7, 9)])]
    pr, pp, ne, env = [], [], [], []
    for p in range(len(models)):
        for r, n, lst in entries:
            if lst is None:                                                                     # what gs_hmm_envelopes lists for the pair
                _, _, n_, e_ = P.envelope_pairs(models, records, [r], [p], MAX_ENV)
                n, e = int(n_[0]), e_[0]
            else:
                e = np.zeros((MAX_ENV, 4), np.int32)
                for d, (a, b) in enumerate(lst):
                    e[d] = (a, b, 12345, -500)                                                  # env_raw and peak are not read
            pr.append(r); pp.append(p); ne.append(n); env.append(e)
    order = rng.permutation(len(pr))
    order = np.concatenate([order, order[:9]])
    pr, pp, ne, env = np.array(pr, np.uint32)[order], np.array(pp, np.uint32)[order], np.array(ne, np.uint32)[order], np.stack(env).astype(np.int32)[order]
    want = N.null2_pairs(models, records, pr, pp, ne, env, MAX_ENV)
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "ne": ne, "env": env, "want": want}


@pytest.fixture(scope="module")
def small_db(small, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(small["texts"], gpu_ctx, texts=True)
    yield d
    d.close()


def test_segment_lengths_positions_and_pair_list_rules(small, small_db, gpu_ctx):
    s = small
    slots, sb = s["want"][:2]
    by = {(int(r), int(p), int(n)): j for j, (r, p, n) in enumerate(zip(s["pr"], s["pp"], s["ne"]))}
    # what the restatement says about these inputs
    j = by[5, 0, 4]
    assert slots[j, :, 2].all() and (slots[j, :, 1] >= 0).all() and sb[j] == N.seq_bias(slots[j, :, 0])       # three listed of four: the bias counts those
    assert not slots[by[9, 0, 1]].any() and sb[by[9, 0, 1]] == 0 and sb[by[8, 1, 0]] == 0 and (sb[s["pr"] == R.NO_HIT] == 0).all()
    two = [j for j in range(len(s["pr"])) if s["pr"][j] == 6 and s["pp"][j] == 0][0]
    assert s["ne"][two] == 2 and np.array_equal(slots[two, :2, 2], s["env"][two, :2, 2]) and not slots[two, 2].any()      # seg_raw == env_raw on the integers
    whole = by[2, 1, 1]
    assert slots[whole, 0, 2] == F.forward(s["models"][1]["tables"], s["records"][2])                                     # a whole record: the pair's Forward raw
    assert s["want"][4][by[4, 2, 1]][0][0] == R.NEG and len(s["want"][3][by[4, 2, 1]][0]) == 1                            # one node: no insert state
    host = both_forms(gpu_ctx, small_db, s["models"], s["records"], s["pr"], s["pp"], s["ne"], s["env"], s["want"])
    assert (host[0][:, :, 1] >= 0).all() and (host[1] >= 0).all()
    # through gs_hmm_envelopes, the records-as-bytes forms and no pair at all
    live = s["records"][:8]
    got = small_db.envelopes(live, [(6, 0), (7, 1), (5, 0)], max_env=2, bias=True)
    assert len(got) == 6 and got[2].tolist()[:2] == [2, 2] and np.array_equal(got[4][:2, :, 2], got[3][:2, :, 2])
    want = N.null2_pairs(s["models"], live, [6, 7, 5], [0, 1, 0], got[2], got[3], 2)
    assert np.array_equal(got[4], want[0]) and np.array_equal(got[5], want[1])
    again = small_db.null2(live, [(6, 0), (7, 1), (5, 0)], got[2], got[3])
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    none = small_db.null2(live, np.zeros((0, 2), np.int64), np.zeros(0, np.uint32), np.zeros((0, 8, 4), np.int32))
    assert none[0].shape == (0, 8, 4) and none[1].shape == (0,)


def test_a_cut_list_and_no_slots(small, small_db, gpu_ctx):
    """max_env = 1 against pairs with two and three envelopes: only the first is listed; max_env = 0: seq_bias alone"""
    s = small
    keep = np.flatnonzero(np.isin(s["pr"], (5, 6, 7, 9)))[:24]
    for m in (1, 0):
        pr, pp, ne, env = s["pr"][keep], s["pp"][keep], s["ne"][keep], np.ascontiguousarray(s["env"][keep, :m])
        want = N.null2_pairs(s["models"], s["records"], pr, pp, ne, env, m)
        assert want[0].shape == (len(keep), m, 4) and (m == 1 or (want[1][pr != 9] == N.seq_bias([])).all())
        both_forms(gpu_ctx, small_db, s["models"], s["records"], pr, pp, ne, env, want)


def test_max_block_cells_changes_nothing(small, small_db, gpu_ctx):
    """a block per slot and a block of a few against the default: the same bytes"""
    s = small
    for cells in (1, 40000):
        both_forms(gpu_ctx, small_db, s["models"], s["records"], s["pr"], s["pp"], s["ne"], s["env"], s["want"], max_block_cells=cells)


@pytest.fixture(scope="module")
def cset():
    """every kernel class at both edges: the profiles of hmm_classes_case.SET_ORDER (profile number and class differ), each against its own consensus
    as one segment of M rows; the shorter profiles also inside a longer record"""
    rng = np.random.default_rng(1355)
    texts = [K.model_text(M) for M in K.SET_ORDER]
    models = [m for t in texts for m in R.parse_hmm(t)]
    records, pr, pp, ne, env = [], [], [], [], []
    for p, m in enumerate(models):
        c = R.consensus(m["tables"])
        inside = m["M"] <= 257
        records.append(R.background(rng, 5) + c + R.background(rng, 3) if inside else c)
        pr.append(len(records) - 1); pp.append(p); ne.append(1)
        env.append([(6, 5 + m["M"], 0, 0) if inside else (1, m["M"], 0, 0)])
    order = rng.permutation(len(pr))
    pr, pp, ne, env = np.array(pr, np.uint32)[order], np.array(pp, np.uint32)[order], np.array(ne, np.uint32)[order], np.array(env, np.int32)[order]
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "ne": ne, "env": env, "want": N.null2_pairs(models, records, pr, pp, ne, env, 1)}


def test_every_class(cset, gpu_ctx):
    import gsearch_amd as G
    c = cset
    assert {F.group_size(m["M"]) for m in c["models"]} == set(F.CLASS_G) and c["want"][0][:, 0, 2].all()
    d = G.HmmDb(c["texts"], gpu_ctx, texts=True)
    try:
        both_forms(gpu_ctx, d, c["models"], c["records"], c["pr"], c["pp"], c["ne"], c["env"], c["want"])
    finally:
        d.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_on_poisoned_scratch(small, gpu_ctx, byte):
    """host and device form twice on scratch and allocations filled with a chosen byte: nothing reads what nothing wrote"""
    import gsearch_amd as G
    s = small
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        d = G.HmmDb(s["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                both_forms(gpu_ctx, d, s["models"], s["records"], s["pr"], s["pp"], s["ne"], s["env"], s["want"], max_block_cells=100000)
        finally:
            d.close()
    finally:
        G.debug_mem_fill(None)


def test_refusals_write_nothing(small, small_db, gpu_ctx):
    import gsearch_amd as G
    L, db, models = gpu_ctx.L, small_db, small["models"]
    aa = np.frombuffer(b"ACDEFGHIKL" * 4, np.uint8)
    rs, rl = np.array([0, 0, 10], np.uint64), np.array([10, F.FWD_MAX_L + 1, 10], np.uint64)          # a faked length: nothing reads record 1
    n_prof = len(db)

    def envs(lists):
        e = np.zeros((len(lists), 2, 4), np.int32)
        for j, lst in enumerate(lists):
            for d, (a, b) in enumerate(lst):
                e[j, d, :2] = (a, b)
        return np.array([len(lst) for lst in lists], np.uint32), e

    def host(pr, pp, lists, ctx=gpu_ctx, occ_off=None):
        pr, pp = np.array(pr, np.uint32), np.array(pp, np.uint32)
        ne, env = envs(lists)
        outs = [np.full((len(pr), 2, 4), 77, np.int32), np.full(len(pr), 77, np.int32), np.full((len(pr), 2, 20), 77, np.int32), np.full(4000, 77, np.int32),
                np.full(4000, 77, np.int32)]
        oo = None if occ_off is None else np.array(occ_off, np.uint64)
        rc = L.gs_hmm_null2(ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, pr.ctypes.data, pp.ctypes.data, len(pr), 2, 0, ne.ctypes.data, env.ctypes.data,
                            outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, None if oo is None else oo.ctypes.data,
                            None if oo is None else outs[3].ctypes.data, None if oo is None else outs[4].ctypes.data)
        return rc, all((o == 77).all() for o in outs)

    one = [(1, 10)]
    for pr, pp, lists, code in (([0, 3], [0, 0], [one, one], GS_ERR_INVALID), ([0, 2], [0, n_prof], [one, one], GS_ERR_INVALID), ([R.NO_HIT], [n_prof], [[]], GS_ERR_INVALID),
                                ([0, 1, 2], [0, 0, 0], [one, one, one], GS_ERR_UNSUPPORTED),
                                ([0, 2], [0, 1], [one, [(5, 4)]], GS_ERR_INVALID),                      # i_from > i_to
                                ([0, 2], [0, 1], [[(0, 4)], one], GS_ERR_INVALID),                      # a bound below 1
                                ([0, 2], [0, 1], [one, [(2, 3), (4, 11)]], GS_ERR_INVALID)):            # a bound above L
        assert host(pr, pp, lists) == (code, True), (pr, pp, lists)
        ne, env = envs(lists)
        null2_dev(gpu_ctx, db, models, pr, pp, ne, env, (aa, rs, rl), rc_want=code, extras=False)     # asserts the code and the canaries
    # occ_off that leaves a pair fewer words than its listed envelopes times M, or that decreases
    M0 = models[0]["M"]
    for oo in ([0, 2 * M0 - 1, 3 * M0], [0, 2 * M0, 2 * M0 - 1]):
        assert host([0, 2], [0, 0], [[(1, 4), (6, 10)], one], occ_off=oo) == (GS_ERR_INVALID, True)
        ne, env = envs([[(1, 4), (6, 10)], one])
        null2_dev(gpu_ctx, db, models, [0, 2], [0, 0], ne, env, (aa, rs, rl), rc_want=GS_ERR_INVALID, occ_off=oo)
    other = G.Context(0)
    try:
        assert host([0], [0], [one], other) == (GS_ERR_INVALID, True)
        ne, env = envs([one])
        null2_dev(other, db, models, [0], [0], ne, env, (aa, rs, rl), rc_want=GS_ERR_INVALID, extras=False)
    finally:
        other.close()
    # an over-long record that no pair names is accepted, and the words of a pair without a record are not read
    pr, pp = np.array([2, 0, R.NO_HIT], np.uint32), np.array([1, 0, 0], np.uint32)
    ne, env = envs([[(2, 9)], one, [(7, 3)]])
    want = N.null2_pairs(models, [b"ACDEFGHIKL", b"", b"ACDEFGHIKL"], pr, pp, ne, env, 2)
    got = db.null2_packed(aa, rs, rl, pr, pp, ne, env)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0][0, 0, 2] != 0
    got = null2_dev(gpu_ctx, db, models, pr, pp, ne, env, (aa, rs, rl))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_tables_of_hmmsearch_and_universal_genes_with_bias(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(1357)
    paths = [fixture_path(n) for n in FIXTURES]
    texts = [open(p, "rb").read() for p in paths]
    models = [m for t in texts for m in R.parse_hmm(t)]
    stats = [F.stats_lines(t)[0] for t in texts]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    bg = lambda n: R.background(rng, n)                                                         # noqa: E731
    poly = b"K" * 121                                                                           # 39.65 bits against PF00380.20, GA 22.10; 126.83 bits of bias
    seqs = [bg(150), bg(40) + c0 + bg(25), c1 + bg(30) + c1, poly, c0[:60] + b"K" * 40 + c0[60:], bg(40)]
    ids = ["prot%d" % i for i in range(len(seqs))]
    faa = str(tmp_path / "p.faa")
    _write_faa(faa, ids, seqs, False)
    fwd = F.search_forward(models, seqs, floor=F.floors(models))[1]
    cand = [(r, p) for r in range(len(seqs)) for p in range(2) if fwd[r, p] != R.NO_SCORE and fwd[r, p] >= 0]
    pr, pp = np.array([r for r, _ in cand], np.uint32), np.array([p for _, p in cand], np.uint32)
    _, _, ne, env = P.envelope_pairs(models, seqs, pr, pp, 8)
    slots, sb = N.null2_pairs(models, seqs, pr, pp, ne, env, 8)[:2]
    sbias = np.zeros(fwd.shape, np.int64)
    sbias[pr, pp] = sb
    want = N.table_bytes(models, stats, ids, fwd, sbias)
    listed = N.listed_pairs(models, fwd, sbias)
    at = {rp: j for j, rp in enumerate(cand)}
    j = [at[rp] for rp in listed]
    want_env = N.envelope_table_bytes(models, ids, listed, ne[j], env[j], slots[j])
    eout, out = str(tmp_path / "env.tsv"), str(tmp_path / "out.tsv")
    res = G.hmmsearch(faa, paths, out, ctx=gpu_ctx, score="forward", envelopes=eout, bias=True)
    assert res[0] == ids and np.array_equal(res[1], fwd)                                         # the matrix stays the uncorrected one
    assert res[2] == want and open(out, "rb").read() == want and res[3] == want_env and open(eout, "rb").read() == want_env
    assert b"prot3\tRibosomal_S9\tPF00380.20\t-87.18\t" in want and want.split(b"\n")[0].endswith(b"\tbias") and b"\t126.83\n" in want_env
    assert G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward", bias=True)[2] == want
    plain = G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward")
    assert plain[2] == F.table_bytes(models, stats, ids, fwd) and b"prot3\tRibosomal_S9\tPF00380.20\t39.65\t" in plain[2]       # the default is what it was
    with pytest.raises(ValueError):
        G.hmmsearch(faa, paths, ctx=gpu_ctx, bias=True)
    with pytest.raises(ValueError):
        G.universal_genes([faa], paths, ctx=gpu_ctx, bias=True)
    # universal genes: the homopolymer is genome 0's only hit of PF00380.20 without the correction and no hit with it; genome 1 keeps its consensus
    genomes = [[bg(100), poly, seqs[2]], [poly, seqs[1], bg(60)], [bg(80)]]
    files = []
    for g, gs in enumerate(genomes):
        files.append(str(tmp_path / ("g%d.faa" % g)))
        _write_faa(files[-1], ["g%d_%d" % (g, i) for i in range(len(gs))], gs)
    kept, local = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward")
    corr, local_b = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward", bias=True)
    assert local.tolist() == [[1, 2], [1, R.NO_HIT], [R.NO_HIT, R.NO_HIT]] and kept[0] == [poly, seqs[2]]
    assert local_b.tolist() == [[R.NO_HIT, 2], [1, R.NO_HIT], [R.NO_HIT, R.NO_HIT]] and corr == [[seqs[2]], [seqs[1]], []]
    for g, gs in enumerate(genomes):                                                            # and that is what the restatement chooses
        f_g = F.search_forward(models, gs, floor=F.floors(models))[1]
        for p, m in enumerate(models):
            best = [(-(int(f_g[r, p]) - N.pair(m["tables"], gs[r])["seq_bias"]), r) for r in range(len(gs)) if f_g[r, p] != R.NO_SCORE and f_g[r, p] >= m["ga_units"]]
            best = [b for b in best if -b[0] >= m["ga_units"]]
            assert local_b[g, p] == (min(best)[1] if best else R.NO_HIT)
    cut, local_e = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward", bias=True, region="envelope")
    e1 = P.posterior(models[0]["tables"], seqs[1])["env"]
    assert np.array_equal(local_e, local_b) and cut[1] == [seqs[1][e1[0][0] - 1:e1[-1][1]]] and cut[0] == [c1 + seqs[2][57:87] + c1]
    # the same on a genome given as nucleotides: the homopolymer between two stop codons is an ORF of its own
    rng2 = np.random.default_rng(1359)
    codes = np.concatenate([O.planted_genome(rng2, b"*" + poly + b"*", 0, 1)[0], O.planted_genome(rng2, b"*" + c1 + b"*", 1, 2)[0]])
    fna = str(tmp_path / "g.fna")
    with open(fna, "wb") as f:
        f.write(b">ctg1\n" + bytes(b"ACGT"[c] for c in codes) + b"\n")
    for translate in (True, "genes"):                                                           # (a genome this small does not train the gene caller: no targets)
        _, loc, _ = G.universal_genes([fna], paths, ctx=gpu_ctx, score="forward", translate=translate)
        hits_b, loc_b, where_b = G.universal_genes([fna], paths, ctx=gpu_ctx, score="forward", translate=translate, bias=True)
        if translate is True:
            assert loc[0, 0] != R.NO_HIT and loc[0, 1] != R.NO_HIT and hits_b[0] == [c1]
        assert loc_b[0, 0] == R.NO_HIT and loc_b[0, 1] == loc[0, 1] and (where_b[0, 0] == -1).all()
    ids_t, _, table_t = G.hmmsearch(fna, paths, ctx=gpu_ctx, score="forward", translate=True, bias=True)
    rows = [ln.split(b"\t") for ln in table_t.split(b"\n")[1:] if ln]
    assert [r for r in rows if r[1] == b"Ribosomal_S9" and float(r[6]) > 100 and r[5] == b"0"] and [r for r in rows if r[1] == b"TIGR00964" and r[5] == b"1"]
