"""The optimal-accuracy alignment of SPEC 13.6 on the device (k_hmm_n2_forward<Q>, k_hmm_ali_backward<Q>, k_hmm_ali_rows<Q>, k_hmm_ali_walk and
k_hmm_ali_fill of gs_hmm.hip, gs_hmm_align / gs_hmm_align_dev) against the numpy restatement tests/pyref_hmm_align.py. Every comparison is `==` on
int32 or on bytes, through the host form and the device form: the eight slot words and both words of every column; every device output sits between
canaries, and the columns a slot owns but does not write keep the canary. The expected values are computed once per module.

What is chosen here: the envelopes are inputs, so the segments are put where the kernels can go wrong - Forward and the row kernel read from the
segment's start, Backward loads residues 64 at a time from its end, so Ld sits on both sides of that edge and one segment is a single row, each as a
whole record and inside a longer one; the slots of a call are cut into blocks and grouped by profile, so the pair lists are shuffled and hold repeats,
pairs with two and three envelopes, one whose n_env is above max_env, and the three kinds of pair that get nothing; a profile of one node has no
insert and no delete state at all; every kernel class runs a record that deletes across most of its lanes; and the profiles of
tests/hmm_align_case.py hold `*` in transitions between valid nodes - every m->d, or one d->d inside a lane's group or on a lane's edge - under a
deletion that would cross it, so that the masks, their prefix minima, the minimum scan over lanes and the edge nibble each decide output words: the
fixture asserts that a program without the masks would write other words."""
import numpy as np
import pytest

import hmm_align_case as HC
import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_align as A
import pyref_hmm_forward as F
import pyref_hmm_null2 as N
import pyref_hmm_posterior as P
import pyref_orf as O
from test_gpu_hmm import CANARY, FIXTURES, GUARD, _Dev, _write_faa, fixture_path  # noqa: F401
from test_gpu_hmm_posterior import pack

pytestmark = pytest.mark.gpu
GS_OK, GS_ERR_INVALID, GS_ERR_UNSUPPORTED = 0, -1, -3
MAX_ENV = 3


def col_offsets(models, rl, pr, pp, ne, env):
    """col_off as HmmDb.align_packed lays the columns out: the listed slots of a pair one after the other, Ld + M columns each"""
    max_env = env.shape[1]
    cols = []
    for j, (r, p) in enumerate(zip(pr, pp)):
        has = int(r) != R.NO_HIT and int(r) < len(rl) and int(rl[int(r)]) > 0
        cols.append(sum(int(env[j, e, 1]) - int(env[j, e, 0]) + 1 + models[int(p)]["M"] for e in range(min(int(ne[j]), max_env))) if has and int(p) < len(models) else 0)
    return np.concatenate([[0], np.cumsum(cols)]).astype(np.uint64)


def flat_columns(models, pp, env, co, want_cols, fill):
    """the column buffer the restatement expects: every slot's words from its first column on, `fill` in the columns it owns and does not write"""
    flat = np.full((int(co[-1]), 2), fill, np.int32)
    for j, per in enumerate(want_cols):
        at = int(co[j])
        for e, c in enumerate(per):
            flat[at:at + len(c)] = A.column_words(c)
            at += int(env[j, e, 1]) - int(env[j, e, 0]) + 1 + models[int(pp[j])]["M"]
    return flat


def align_dev(ctx, d_b, models, pair_rec, pair_prof, n_env, env, packed, max_block_cells=0, rc_want=GS_OK, columns=True, col_off=None):
    """gs_hmm_align_dev on guarded outputs -> (slots, flat columns, col_off); with rc_want another code: that code is returned and the outputs hold the canary"""
    d = _Dev(ctx, packed=packed)
    try:
        pr, pp = np.ascontiguousarray(pair_rec, np.uint32), np.ascontiguousarray(pair_prof, np.uint32)
        ne, env = np.ascontiguousarray(n_env, np.uint32), np.ascontiguousarray(env, np.int32)
        n, max_env = len(pr), env.shape[1]
        co = col_offsets(models, packed[2], pr, pp, ne, env) if col_off is None else np.ascontiguousarray(col_off, np.uint64)
        ups = []
        for a in (pr, pp, ne, env, co):
            d.outs.append(ctx.alloc(max(a.nbytes, 16)))
            if a.nbytes:
                ctx.upload(d.outs[-1], a)
            ups.append(d.outs[-1])
        ncol = int(co[-1])
        p_s, p_c = d.out(n * max_env * A.ALI_WORDS), d.out(2 * ncol)
        g = 4 * GUARD
        rc = ctx.L.gs_hmm_align_dev(ctx.h, d_b.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, ups[0], ups[1], n, max_env, max_block_cells, ups[2], ups[3], p_s + g,
                                    ups[4] if columns else None, (p_c + g) if columns else None)
        assert rc == rc_want, rc
        slots, cols = d.read(p_s, (n, max_env, A.ALI_WORDS)), d.read(p_c, (ncol, 2))
        if rc != GS_OK or not columns:
            assert (cols == CANARY).all()
        if rc != GS_OK:
            assert (slots == CANARY).all()
        return slots, cols, co
    finally:
        d.free()


def both_forms(ctx, d_b, models, records, pr, pp, ne, env, want, max_block_cells=0):
    """the host form and the device form, with the columns and without, against the restatement"""
    packed = pack(records)
    w_slots, w_cols = want
    slots, cols = d_b.align_packed(*packed, pr, pp, ne, env, columns=True, max_block_cells=max_block_cells)
    bad = np.flatnonzero((slots != w_slots).any(axis=(1, 2)))
    assert len(bad) == 0, [(int(pr[j]), int(pp[j]), int(ne[j]), env[j, :, :2].tolist(), slots[j].tolist(), w_slots[j].tolist()) for j in bad[:3]]
    assert slots.dtype == np.int32 and len(cols) == len(w_cols)
    for j, (got, exp) in enumerate(zip(cols, w_cols)):
        assert len(got) == len(exp), j
        for g, w in zip(got, exp):
            assert all(a.dtype == np.int32 for a in g) and np.array_equal(np.stack(g, axis=1), w), j
    d_slots, d_cols, co = align_dev(ctx, d_b, models, pr, pp, ne, env, packed, max_block_cells=max_block_cells)
    assert np.array_equal(d_slots, w_slots) and np.array_equal(d_cols, flat_columns(models, pp, env, co, w_cols, CANARY))
    assert np.array_equal(d_b.align_packed(*packed, pr, pp, ne, env, max_block_cells=max_block_cells), w_slots)          # without the columns
    assert np.array_equal(align_dev(ctx, d_b, models, pr, pp, ne, env, packed, max_block_cells=max_block_cells, columns=False)[0], w_slots)
    return slots, cols


@pytest.fixture(scope="module")
def small():
    """the two real profiles and synthetic ones of 1, 2, 65 and 129 nodes; segments of 1, 63, 64, 65 and 130 rows as whole records and inside a record of
    200; the envelopes SPEC 13.4 finds in records with two copies; an empty record, one with a byte that is no residue, GS_HMM_NO_HIT; shuffled, with
    repeats"""
    rng = np.random.default_rng(1363)
    texts = [open(fixture_path(n), "rb").read() for n in FIXTURES] + [R.write_hmm(R.synth_model(rng, M)) for M in (1, 2, 65, 129)]
    models = [m for t in texts for m in R.parse_hmm(t)]
    c0, c1 = (R.consensus(m["tables"]) for m in models[:2])
    bg = lambda n: R.background(rng, n)                                                         # noqa: E731
    records = [bg(1), bg(20) + c1[:23] + bg(20), c0[:64], bg(4) + c1 + bg(4), c0[:30] + c0[70:] + bg(49), bg(60) + c0[:50] + bg(8) + c0[50:] + bg(11), c0 + c0,
               c1 + bg(30) + c1, b"", c0[:40] + b"\xff" + c0[41:]]
    assert [len(r) for r in records[:6]] == [1, 63, 64, 65, 130, 200]
    entries = []                                                                                # (record, n_env as given, the envelopes given)
    for r in range(5):
        entries.append((r, 1, [(1, len(records[r]))]))
    entries += [(5, 4, [(3, 3), (5, 67), (61, 124)]),                                           # n_env above max_env: three are listed; 1, 63 and 64 rows
                (5, 2, [(58, 122), (50, 179)]), (5, 1, [(200, 200)]),                           # 65 and 130 rows inside the record of 200, and its last row
                (6, None, None), (7, None, None), (8, 0, []), (9, 1, [(1, 10)]), (R.NO_HIT, 2, [(1, 5), (7, 9)])]
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
    want = A.align_pairs(models, records, pr, pp, ne, env, MAX_ENV)
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "ne": ne, "env": env, "want": want}


@pytest.fixture(scope="module")
def small_db(small, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(small["texts"], gpu_ctx, texts=True)
    yield d
    d.close()


def test_segment_lengths_positions_and_pair_list_rules(small, small_db, gpu_ctx):
    s = small
    slots, cols = s["want"]
    by = {(int(r), int(p), int(n)): j for j, (r, p, n) in enumerate(zip(s["pr"], s["pp"], s["ne"]))}
    # what the restatement says about these inputs
    j = by[5, 0, 4]
    assert slots[j, :, 5].all() and len(cols[j]) == 3 and slots[j, 0, :4].tolist()[:2] == [3, 3]                  # three listed of four; a segment of one row
    assert not slots[by[9, 0, 1]].any() and not cols[by[9, 0, 1]] and not slots[by[8, 1, 0]].any() and not slots[s["pr"] == R.NO_HIT].any()
    two = [j for j in range(len(s["pr"])) if s["pr"][j] == 6 and s["pp"][j] == 0][0]
    assert s["ne"][two] == 2 and slots[two, :2, 2:4].tolist() == [[1, 121], [1, 121]] and not slots[two, 2].any()  # 13.4's two envelopes: each aligns (.., 1, M)
    assert A.cigar(cols[by[4, 0, 1]][0]).startswith("30M40D51M")                                                   # the deletion case inside a longer record
    ins = cols[by[5, 0, 2]][1]
    assert "8I" in A.cigar(ins) and slots[by[5, 0, 2], 1, 6] >= 8                                                  # the planted insertion of record 5
    one = by[4, 2, 1]
    assert slots[one, 0, 2:4].tolist() == [1, 1] and slots[one, 0, 5:].tolist() == [1, 0, 0]                       # one node: one match cell
    for j in range(len(s["pr"])):                                                                                  # the identities of the section
        for e, c in enumerate(cols[j]):
            w = slots[j, e]
            assert w[5] + w[6] == w[1] - w[0] + 1 and w[5] + w[7] == w[3] - w[2] + 1 and s["env"][j, e, 0] <= w[0] <= w[1] <= s["env"][j, e, 1] and len(c) == w[5:].sum()
    both_forms(gpu_ctx, small_db, s["models"], s["records"], s["pr"], s["pp"], s["ne"], s["env"], s["want"])
    # through gs_hmm_envelopes, the records-as-bytes forms and no pair at all
    live = s["records"][:8]
    _, _, ne, env = small_db.envelopes(live, [(6, 0), (7, 1), (5, 0)], max_env=2)
    want = A.align_pairs(s["models"], live, [6, 7, 5], [0, 1, 0], ne, env, 2)
    got = small_db.align(live, [(6, 0), (7, 1), (5, 0)], ne, env, columns=True)
    assert ne.tolist()[:2] == [2, 2] and np.array_equal(got[0], want[0]) and [len(c) for c in got[1]] == [len(c) for c in want[1]]
    none = small_db.align(live, np.zeros((0, 2), np.int64), np.zeros(0, np.uint32), np.zeros((0, 8, 4), np.int32), columns=True)
    assert none[0].shape == (0, 8, 8) and none[1] == []


def test_a_cut_list_and_no_slots(small, small_db, gpu_ctx):
    """max_env = 1 against pairs with two and three envelopes: only the first is listed; max_env = 0: nothing to write"""
    s = small
    keep = np.flatnonzero(np.isin(s["pr"], (5, 6, 7, 9)))[:24]
    for m in (1, 0):
        pr, pp, ne, env = s["pr"][keep], s["pp"][keep], s["ne"][keep], np.ascontiguousarray(s["env"][keep, :m])
        want = A.align_pairs(s["models"], s["records"], pr, pp, ne, env, m)
        assert want[0].shape == (len(keep), m, 8) and all(len(c) <= m for c in want[1])
        both_forms(gpu_ctx, small_db, s["models"], s["records"], pr, pp, ne, env, want)


def test_max_block_cells_changes_nothing(small, small_db, gpu_ctx):
    """a block per slot and a block of a few against the default: the same bytes"""
    s = small
    for cells in (1, 40000):
        both_forms(gpu_ctx, small_db, s["models"], s["records"], s["pr"], s["pp"], s["ne"], s["env"], s["want"], max_block_cells=cells)


CLASS_M = (64, 128, 192, 256, 384, 512, 768, 1024, 1280)                                        # one profile per kernel class, every lane in use


@pytest.fixture(scope="module")
def cset():
    """every kernel class: a deletion-friendly profile of 64 Q nodes (profile number and class differ) against about 70 rows - 35 nodes from either end
    of its consensus, a deletion across most of the wavefront, inside a few background residues - and against its whole consensus where that is short"""
    rng = np.random.default_rng(1365)
    order = rng.permutation(len(CLASS_M))
    texts = [K.model_text(CLASS_M[i]) for i in order]
    models = [m for t in texts for m in R.parse_hmm(t)]
    records, pr, pp, ne, env = [], [], [], [], []
    for p, m in enumerate(models):
        c, M = R.consensus(m["tables"]), m["M"]
        rec = c if M == 64 else c[:35] + c[M - 35:]
        records.append(R.background(rng, 3) + rec + R.background(rng, 2))
        pr.append(len(records) - 1); pp.append(p); ne.append(1)
        env.append([(4, 3 + len(rec), 0, 0)])
    order = rng.permutation(len(pr))
    pr, pp, ne, env = np.array(pr, np.uint32)[order], np.array(pp, np.uint32)[order], np.array(ne, np.uint32)[order], np.array(env, np.int32)[order]
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "ne": ne, "env": env, "want": A.align_pairs(models, records, pr, pp, ne, env, 1)}


def test_every_class(cset, gpu_ctx):
    import gsearch_amd as G
    c = cset
    assert {F.group_size(m["M"]) for m in c["models"]} == set(F.CLASS_G) and c["want"][0][:, 0, 5].all()
    dels = {c["models"][int(p)]["M"]: int(c["want"][0][j, 0, 7]) for j, p in enumerate(c["pp"])}
    assert all(dels[M] == M - 70 for M in CLASS_M[1:]), dels                                    # the deletion crosses the lanes: the scan carries the path
    d = G.HmmDb(c["texts"], gpu_ctx, texts=True)
    try:
        both_forms(gpu_ctx, d, c["models"], c["records"], c["pr"], c["pp"], c["ne"], c["env"], c["want"])
    finally:
        d.close()


def test_universal_genes_from_called_genes_cut_by_the_alignment(gpu_ctx, tmp_path):
    """translate="genes" with targets: a genome with enough coding sequence to train the caller (the recipe of tests/test_gpu_gene.py), in which the gene
    of PF00380.20 is its consensus without nodes 31 .. 70 and the gene of TIGR00964 its whole consensus. region="alignment" gives the rows the
    restatement aligns in the called gene's own residues, which region="protein" returns"""
    import gene_cases as GC
    import gsearch_amd as G
    paths = [fixture_path(n) for n in FIXTURES]
    models = [R.parse_hmm(open(p, "rb").read())[0] for p in paths]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    planted = {1: b"M" + c0[:30] + c0[70:], 2: b"M" + c1}
    rng = np.random.default_rng(1375)
    aas = R.AA.encode()
    contigs = []
    for ci in range(3):
        parts = [rng.integers(0, 4, 300).astype(np.uint8)]
        for k in range(16):                                                                             # 16 genes of 450 residues a contig: training material
            prot = planted[ci] if k == 7 and ci in planted else b"M" + bytes(aas[i] for i in rng.integers(0, 20, 450))
            gene = np.concatenate([O.back_translate(prot), GC.bases([48])])
            parts += [GC.revcomp(gene) if (k + ci) % 2 else gene, rng.integers(0, 4, int(rng.integers(30, 200))).astype(np.uint8)]
        contigs.append(O.ascii_of(np.concatenate(parts)))
    fna = str(tmp_path / "genes.fna")
    with open(fna, "wb") as f:
        for i, c in enumerate(contigs):
            f.write(b">c%d\n" % i + c + b"\n")
    whole, local, _ = G.universal_genes([fna], paths, ctx=gpu_ctx, score="forward", translate="genes")
    cut, local_a, where = G.universal_genes([fna], paths, ctx=gpu_ctx, score="forward", translate="genes", region="alignment")
    assert (local != R.NO_HIT).all() and np.array_equal(local, local_a) and (where[0, :, 0] == [1, 2]).all()
    for p, (gene, got) in enumerate(zip(whole[0], cut[0])):
        x = R.encode(gene)
        env = P.posterior(models[p]["tables"], gene)["env"]
        first, last = (A.segment(models[p]["tables"], x[a - 1:b], len(x), a)[0] for a, b, _, _ in (env[0], env[-1]))
        assert got == gene[first[0] - 1:last[1]] and len(env) == 1
    assert c0[12:30] + c0[70:] in cut[0][0] and c1[6:] in cut[0][1] and len(cut[0][0]) <= 81 and len(cut[0][1]) <= 57      # (the caller chooses the start)


@pytest.fixture(scope="module")
def mset():
    """the starred profiles of hmm_align_case (classes Q = 2, 3, 6, 8, 20), each against its record as one envelope, shuffled; and what a program that
    forgot the rule of allowed transitions would write for them"""
    rng = np.random.default_rng(1373)
    texts, models, records = HC.build()
    order = rng.permutation(len(models))
    pr, pp, ne = order.astype(np.uint32), order.astype(np.uint32), np.ones(len(order), np.uint32)
    env = np.array([[(4, len(records[r]) - 2, 0, 0)] for r in order], np.int32)
    want = A.align_pairs(models, records, pr, pp, ne, env, 1)
    loose = A.align_pairs(models, records, pr, pp, ne, env, 1, use_masks=False)
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "ne": ne, "env": env, "want": want, "loose": loose}


def test_starred_transitions_between_valid_nodes(mset, gpu_ctx):
    import gsearch_amd as G
    s = mset
    for j, p in enumerate(s["pp"]):
        kind, M, nodes = HC.CASES[int(p)]
        tab, w, c, lw, lc = s["models"][int(p)]["tables"], s["want"][0][j, 0], s["want"][1][j][0], s["loose"][0][j, 0], s["loose"][1][j][0]
        assert A.steps_allowed(tab, c) and not A.steps_allowed(tab, lc) and not np.array_equal(w, lw) and lw[4] > w[4], HC.CASES[int(p)]
        assert A.cigar(lc) == ("30M40D51M" if M == 121 else "35M%dD35M" % (M - 70))                     # without the masks: straight across the star
        if kind == "md":
            assert w[7] == 0 and w[6] == 0                                                              # no way into D: one end of the record is aligned
        else:                                                                                           # D steps out through M of node k + 1 and in again
            k = nodes[0]
            assert w[7] == M - 70 and w[5] == 70 and ((c[:, 0] == 0) & (c[:, 1] == k + 1)).any() and not ((c[:, 0] == 2) & (c[:, 1] == k + 1)).any()
    assert {HC.where(M, nodes[0]) for kind, M, nodes in HC.CASES if kind == "dd"} == {"inside", "edge"}
    assert {F.group_size(M) for _, M, _ in HC.CASES} == {2, 3, 6, 8, 20}
    d = G.HmmDb(s["texts"], gpu_ctx, texts=True)
    try:
        for cells in (0, 1):
            both_forms(gpu_ctx, d, s["models"], s["records"], s["pr"], s["pp"], s["ne"], s["env"], s["want"], max_block_cells=cells)
        assert [d.consensus(p) for p in range(len(d))] == [R.consensus(m["tables"]) for m in s["models"]]
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
    long_l = A.ALI_MAX_LD + 1
    aa = np.frombuffer(b"ACDEFGHIKL" * 4 + b"A" * long_l, np.uint8)
    rs, rl = np.array([0, 0, 10, 40], np.uint64), np.array([10, F.FWD_MAX_L + 1, 10, long_l], np.uint64)         # a faked length: nothing reads record 1
    n_prof = len(db)
    assert G._lib.HMM_ALI_MAX_LD == A.ALI_MAX_LD == 8192

    def envs(lists):
        e = np.zeros((len(lists), 2, 4), np.int32)
        for j, lst in enumerate(lists):
            for d, (a, b) in enumerate(lst):
                e[j, d, :2] = (a, b)
        return np.array([len(lst) for lst in lists], np.uint32), e

    def host(pr, pp, lists, ctx=gpu_ctx, col_off=None):
        pr, pp = np.array(pr, np.uint32), np.array(pp, np.uint32)
        ne, env = envs(lists)
        outs = [np.full((len(pr), 2, 8), 77, np.int32), np.full((40000, 2), 77, np.int32)]
        co = None if col_off is None else np.array(col_off, np.uint64)
        rc = L.gs_hmm_align(ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 4, pr.ctypes.data, pp.ctypes.data, len(pr), 2, 0, ne.ctypes.data, env.ctypes.data,
                            outs[0].ctypes.data, None if co is None else co.ctypes.data, None if co is None else outs[1].ctypes.data)
        return rc, all((o == 77).all() for o in outs)

    one = [(1, 10)]
    for pr, pp, lists, code in (([0, 4], [0, 0], [one, one], GS_ERR_INVALID), ([0, 2], [0, n_prof], [one, one], GS_ERR_INVALID), ([R.NO_HIT], [n_prof], [[]], GS_ERR_INVALID),
                                ([0, 1, 2], [0, 0, 0], [one, one, one], GS_ERR_UNSUPPORTED),
                                ([0, 3], [0, 1], [one, [(1, long_l)]], GS_ERR_UNSUPPORTED),             # Ld = 8193
                                ([0, 2], [0, 1], [one, [(5, 4)]], GS_ERR_INVALID),                      # i_from > i_to
                                ([0, 2], [0, 1], [[(0, 4)], one], GS_ERR_INVALID),                      # a bound below 1
                                ([0, 2], [0, 1], [one, [(2, 3), (4, 11)]], GS_ERR_INVALID)):            # a bound above L
        assert host(pr, pp, lists) == (code, True), (pr, pp, lists)
        ne, env = envs(lists)
        align_dev(gpu_ctx, db, models, pr, pp, ne, env, (aa, rs, rl), rc_want=code, columns=False)      # asserts the code and the canaries
    # col_off that leaves a pair fewer columns than its listed envelopes' residues and nodes, or that decreases; columns without their offsets
    M0 = models[0]["M"]
    need = 4 + 5 + 2 * M0
    for co in ([0, need - 1, need + 10 + M0], [0, need, need - 1]):
        assert host([0, 2], [0, 0], [[(1, 4), (6, 10)], one], col_off=co) == (GS_ERR_INVALID, True)
        ne, env = envs([[(1, 4), (6, 10)], one])
        align_dev(gpu_ctx, db, models, [0, 2], [0, 0], ne, env, (aa, rs, rl), rc_want=GS_ERR_INVALID, col_off=co)
    other = G.Context(0)
    try:
        assert host([0], [0], [one], other) == (GS_ERR_INVALID, True)
        ne, env = envs([one])
        align_dev(other, db, models, [0], [0], ne, env, (aa, rs, rl), rc_want=GS_ERR_INVALID, columns=False)
    finally:
        other.close()
    # the longest envelope the call takes, an over-long record that no pair names, and the words of a pair without a record are not read
    recs = [b"ACDEFGHIKL", b"", b"ACDEFGHIKL", b"A" * long_l]
    pr, pp = np.array([2, 0, R.NO_HIT, 3], np.uint32), np.array([1, 0, 0, 2], np.uint32)
    ne, env = envs([[(2, 9)], one, [(7, 3)], [(2, long_l)]])
    want = A.align_pairs(models, recs, pr, pp, ne, env, 2)
    got = db.align_packed(aa, rs, rl, pr, pp, ne, env)
    assert np.array_equal(got, want[0]) and want[0][0, 0, 5] != 0 and want[0][3, 0, 1] - want[0][3, 0, 0] >= 0
    d_slots, d_cols, co = align_dev(gpu_ctx, db, models, pr, pp, ne, env, (aa, rs, rl))
    assert np.array_equal(d_slots, want[0]) and np.array_equal(d_cols, flat_columns(models, pp, env, co, want[1], CANARY))


def test_alignments_of_hmmsearch_and_universal_genes(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(1367)
    paths = [fixture_path(n) for n in FIXTURES]
    texts = [open(p, "rb").read() for p in paths]
    models = [m for t in texts for m in R.parse_hmm(t)]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    bg = lambda n: R.background(rng, n)                                                         # noqa: E731
    seqs = [bg(150), bg(40) + c0[:30] + c0[70:] + bg(25), c1 + bg(30) + c1, c0[:60] + bg(6) + c0[60:], bg(40)]
    ids = ["prot%d" % i for i in range(len(seqs))]
    faa = str(tmp_path / "p.faa")
    _write_faa(faa, ids, seqs, False)

    def expected(seqs, ids, scores, sbias=None):
        listed = P.listed_pairs(models, scores) if sbias is None else N.listed_pairs(models, scores, sbias)
        pr, pp = np.array([r for r, _ in listed], np.uint32), np.array([p for _, p in listed], np.uint32)
        _, _, ne, env = P.envelope_pairs(models, seqs, pr, pp, 8)
        slots, cols = A.align_pairs(models, seqs, pr, pp, ne, env, 8)
        return A.alignment_bytes(models, ids, seqs, listed, ne, env, slots, cols), (pr, pp, ne, env)

    fwd = F.search_forward(models, seqs, floor=F.floors(models))[1]
    want, (pr, pp, ne, env) = expected(seqs, ids, fwd)
    aout = str(tmp_path / "ali.txt")
    res = G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward", alignments=aout)
    assert len(res) == 4 and res[3] == want and open(aout, "rb").read() == want
    assert want.count(b"\n==\t") >= 4 and b"  PP     " in want and want.startswith(b"# == target\t")
    assert b"-" * 40 in want and b"\t81\t0\t40\n" in want                                        # 30M 40D 51M of prot1, written out
    # with the bias correction the order is the corrected table's; with the envelope and domain tables the text comes last
    cand = [(r, p) for r in range(len(seqs)) for p in range(2) if fwd[r, p] != R.NO_SCORE and fwd[r, p] >= 0]
    cr, cp = np.array([r for r, _ in cand], np.uint32), np.array([p for _, p in cand], np.uint32)
    _, _, c_ne, c_env = P.envelope_pairs(models, seqs, cr, cp, 8)
    sbias = np.zeros(fwd.shape, np.int64)
    sbias[cr, cp] = N.null2_pairs(models, seqs, cr, cp, c_ne, c_env, 8)[1]
    want_b = expected(seqs, ids, fwd, sbias)[0]
    res = G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward", bias=True, envelopes=str(tmp_path / "e.tsv"), domains=str(tmp_path / "d.tsv"), alignments=aout)
    assert len(res) == 6 and res[5] == want_b and open(aout, "rb").read() == want_b
    vit = R.search(models, seqs)
    assert G.hmmsearch(faa, paths, ctx=gpu_ctx, alignments=aout)[3] == expected(seqs, ids, vit)[0]
    assert len(G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward")) == 3                       # the default is what it was
    # universal genes: the alignment's rows, not the envelope's
    genomes = [[bg(100), seqs[1], seqs[2]], [seqs[3], bg(60)], [bg(80)]]
    files = []
    for g, gs in enumerate(genomes):
        files.append(str(tmp_path / ("g%d.faa" % g)))
        _write_faa(files[-1], ["g%d_%d" % (g, i) for i in range(len(gs))], gs)
    cut, local = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward", region="alignment")
    plain, local_p = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward")
    assert np.array_equal(local, local_p) and local.tolist() == [[1, 2], [0, R.NO_HIT], [R.NO_HIT, R.NO_HIT]]

    def span(tab, rec):
        e = P.posterior(tab, rec)["env"]
        if not e:
            return rec
        x = R.encode(rec)
        first, last = (A.segment(tab, x[a - 1:b], len(x), a)[0] for a, b, _, _ in (e[0], e[-1]))
        return rec[first[0] - 1:last[1]]

    assert cut == [[span(models[0]["tables"], seqs[1]), span(models[1]["tables"], seqs[2])], [span(models[0]["tables"], seqs[3])], []]
    assert cut[0][0] == c0[:30] + c0[70:] and cut[0][1] == seqs[2] and cut[1][0] == seqs[3]
    with pytest.raises(ValueError):
        G.universal_genes(files, paths, ctx=gpu_ctx, region="alignments")
    # the same on a genome given as nucleotides
    rng2 = np.random.default_rng(1369)
    codes = np.concatenate([O.planted_genome(rng2, b"*" + c0[:30] + c0[70:] + b"*", 0, 1)[0], O.planted_genome(rng2, b"*" + c1 + b"*", 1, 2)[0]])
    fna = str(tmp_path / "g.fna")
    with open(fna, "wb") as f:
        f.write(b">ctg1\n" + bytes(b"ACGT"[c] for c in codes) + b"\n")
    hits, loc, _ = G.universal_genes([fna], paths, ctx=gpu_ctx, score="forward", translate=True, region="alignment")
    assert (loc[0] != R.NO_HIT).all() and hits[0] == [c0[:30] + c0[70:], c1]
    assert G.universal_genes([fna], paths, ctx=gpu_ctx, score="forward", translate="genes", region="alignment")[1].shape == (1, 2)      # (too small to train: no targets)
    ids_t, sc_t, _, text_t = G.hmmsearch(fna, paths, ctx=gpu_ctx, score="forward", translate=True, alignments=aout)
    ref = O.contig_orfs([bytes(b"ACGT"[c] for c in codes)])
    names = [O.orf_name("ctg1", b, e, s) for b, e, s, _ in ref[0]]
    prots = [p for _, _, _, p in ref[0]]
    fwd_t = F.search_forward(models, prots, floor=F.floors(models))[1]
    assert ids_t == names and np.array_equal(sc_t, fwd_t)
    assert text_t == expected(prots, names, fwd_t)[0] == open(aout, "rb").read() and b"\t81\t0\t40\n" in text_t
