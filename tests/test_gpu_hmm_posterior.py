"""Backward scores and posterior envelopes of SPEC 13.4 on the device (k_hmm_forward_rows<Q>, k_hmm_backward<Q>, k_hmm_envelopes and k_hmm_env_score<Q> of
gs_hmm.hip, gs_hmm_envelopes / gs_hmm_envelopes_dev) against the numpy restatement tests/pyref_hmm_posterior.py. Every comparison is `==` on int32 or on
bytes, through the host form and the device form; every device output sits between canaries. The expected values are computed once per module; those of
the length limit against the largest profile come from tests/golden/hmm_posterior_limits.json.

What is chosen here: Backward loads residues 64 at a time from the record's end, so the record lengths sit on both sides of that edge and one record is
a single row; the D scan runs down the lanes, which the deletion-friendly profiles of every class exercise; a profile of one node is first and last
node at once; the pairs of a call are cut into blocks by max_block_rows and grouped by profile, so the pair lists are shuffled and hold repeats."""
import hashlib
import json
import os

import numpy as np
import pytest

import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_posterior as P
from test_gpu_hmm import CANARY, FIXTURES, GUARD, _Dev, _write_faa, fixture_path  # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GS_OK, GS_ERR_INVALID, GS_ERR_UNSUPPORTED = 0, -1, -3


def pack(records):
    """records as they are (no byte is filtered away) -> aa, rec_start, rec_len"""
    rl = np.array([len(r) for r in records], np.uint64)
    rs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(bytes(r) for r in records) + bytes(8), np.uint8), rs, rl


def env_dev(ctx, d_b, pair_rec, pair_prof, packed, max_env=4, max_block_rows=0, rows=True, rc_want=GS_OK):
    """gs_hmm_envelopes_dev on guarded outputs -> (fwd, bck, n_env, env, out rows, cont rows); with rc_want another code: that code is returned and the
    outputs hold the canary"""
    d = _Dev(ctx, packed=packed)
    try:
        pr, pp = np.ascontiguousarray(pair_rec, np.uint32), np.ascontiguousarray(pair_prof, np.uint32)
        n, rl = len(pr), packed[2]
        lens = np.array([int(rl[r]) if r < len(rl) else 0 for r in pr], np.uint64)
        ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ups = []
        for a in (pr, pp, ro):
            d.outs.append(ctx.alloc(max(a.nbytes, 16)))
            ctx.upload(d.outs[-1], a)
            ups.append(d.outs[-1])
        nrow = int(ro[-1])
        p_f, p_b, p_n, p_e, p_o, p_c = d.out(n), d.out(n), d.out(n), d.out(n * max_env * P.ENV_WORDS), d.out(nrow), d.out(nrow)
        rc = ctx.L.gs_hmm_envelopes_dev(ctx.h, d_b.h, d.ptrs[0], d.ptrs[1], d.ptrs[2], d.n_rec, ups[0], ups[1], n, max_env, max_block_rows, p_f + 4 * GUARD, p_b + 4 * GUARD,
                                        p_n + 4 * GUARD, (p_e + 4 * GUARD) if max_env else None, ups[2] if rows else None, (p_o + 4 * GUARD) if rows else None,
                                        (p_c + 4 * GUARD) if rows else None)
        assert rc == rc_want, rc
        got = [d.read(p_f, (n,)), d.read(p_b, (n,)), d.read(p_n, (n,), np.uint32), d.read(p_e, (n, max_env, P.ENV_WORDS))]
        o, c = d.read(p_o, (nrow,)), d.read(p_c, (nrow,))
        if rc != GS_OK:
            assert all((g.view(np.int32) == CANARY).all() for g in got) and (o == CANARY).all() and (c == CANARY).all()
        has = got[0] != R.NO_SCORE
        cut = lambda a: [a[int(ro[j]):int(ro[j + 1])] if has[j] else a[:0] for j in range(n)]      # noqa: E731
        return got + [cut(o), cut(c)]
    finally:
        d.free()


def same(got, want):
    """(fwd, bck, n_env, env[, out rows, cont rows]) against the restatement's"""
    for g, w in zip(got[:4], want[:4]):
        if not (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)):
            return False
    for g_rows, w_rows in zip(got[4:6], want[4:6]):
        for g, w in zip(g_rows, w_rows):
            if (w is None and len(g)) or (w is not None and not (g.dtype == np.int32 and np.array_equal(g, w))):
                return False
    return True


def both_forms(ctx, d_b, records, pair_rec, pair_prof, want, max_env=4, max_block_rows=0):
    """the host form and the device form, rows included, against the restatement"""
    packed = pack(records)
    host = d_b.envelopes_packed(*packed, pair_rec, pair_prof, max_env=max_env, rows=True, max_block_rows=max_block_rows)
    bad = np.flatnonzero((host[0] != want[0]) | (host[1] != want[1]) | (host[2] != want[2]) | (host[3] != want[3]).any(axis=(1, 2)))
    assert len(bad) == 0, [(int(pair_rec[j]), int(pair_prof[j]), [int(h[j]) for h in host[:3]], [int(w[j]) for w in want[:3]], host[3][j].tolist(), want[3][j].tolist())
                           for j in bad[:3]]
    assert same(host, want)
    assert same(env_dev(ctx, d_b, pair_rec, pair_prof, packed, max_env=max_env, max_block_rows=max_block_rows), want)
    assert same(d_b.envelopes_packed(*packed, pair_rec, pair_prof, max_env=max_env, max_block_rows=max_block_rows), want[:4])       # without rows
    return host


@pytest.fixture(scope="module")
def small():
    """the two real profiles and synthetic ones of 1, 2 and 65 nodes against records on both sides of the 64-residue edge, records with several copies
    of a consensus, an empty record and records with a byte that is no residue; all pairs in a shuffled order with repeats and GS_HMM_NO_HIT entries"""
    rng = np.random.default_rng(1343)
    texts = [open(fixture_path(n), "rb").read() for n in FIXTURES] + [R.write_hmm(R.synth_model(rng, M)) for M in (1, 2, 65)]
    models = [m for t in texts for m in R.parse_hmm(t)]
    c0, c1 = (R.consensus(m["tables"]) for m in models[:2])
    bg = lambda n: R.background(rng, n)                                                         # noqa: E731
    records = [bg(L) for L in (1, 2, 63, 64, 65, 128, 129, 200)]
    records += [c0, c0 + c0, c1 + bg(30) + c1, c0 + c0 + c0, c1 + c1 + c1, b"", c0[:40] + b"\xff" + c0[41:], c1 + b"*"]
    n_rec, n_prof = len(records), len(models)
    idx = rng.permutation(n_rec * n_prof)
    idx = np.concatenate([idx, idx[:12]])
    pr, pp = (idx // n_prof).astype(np.uint32), (idx % n_prof).astype(np.uint32)
    pr[[5, 40]] = R.NO_HIT
    want = P.envelope_pairs(models, records, pr, pp, 4, rows=True)
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "want": want, "c0": c0, "c1": c1}


@pytest.fixture(scope="module")
def small_db(small, gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb(small["texts"], gpu_ctx, texts=True)
    yield d
    d.close()


def test_record_lengths_copies_and_pair_list_rules(small, small_db, gpu_ctx):
    fwd, bck, ne, env = small["want"][:4]
    pr, pp = small["pr"], small["pp"]
    by = {(int(r), int(p)): j for j, (r, p) in enumerate(zip(pr, pp))}
    # what the restatement says about these inputs: the copies are separate envelopes, the empty pairs are empty
    assert env[by[9, 0], :2, :2].tolist() == [[1, 121], [122, 242]] and env[by[10, 1], :2, :2].tolist() == [[1, 57], [88, 144]]
    assert ne[by[11, 0]] == 3 == ne[by[12, 1]] and env[by[8, 0], 0, 2] == fwd[by[8, 0]]
    for r in (13, 14, 15):
        assert fwd[by[r, 0]] == R.NO_SCORE == bck[by[r, 1]] and ne[by[r, 0]] == 0 and small["want"][4][by[r, 0]] is None
    assert (fwd[pr == R.NO_HIT] == R.NO_SCORE).all() and (np.abs(fwd.astype(np.int64) - bck)[fwd != R.NO_SCORE] <= 64).all()
    host = both_forms(gpu_ctx, small_db, small["records"], pr, pp, small["want"])
    live = [r for r in small["records"][:13]]
    assert np.array_equal(host[0][pr < 13], small_db.search_forward(live, filter_p=None)[1][pr[pr < 13], pp[pr < 13]])        # fwd is gs_hmm_search_forward's
    # the records-as-bytes form and no pair at all
    got = small_db.envelopes(live, [(9, 0), (10, 1)], max_env=2)
    assert got[3][:, :, :2].tolist() == [[[1, 121], [122, 242]], [[1, 57], [88, 144]]]
    assert small_db.envelopes(live, np.zeros((0, 2), np.int64))[3].shape == (0, 8, 4)


def test_a_cut_list_and_no_slots(small, small_db, gpu_ctx):
    """max_env = 1 against the three-copy records: n_env stays 3; max_env = 0 with no env_out"""
    pr, pp = np.array([11, 12, 8], np.uint32), np.array([0, 1, 0], np.uint32)
    want = P.envelope_pairs(small["models"], small["records"], pr, pp, 1, rows=True)
    assert want[2].tolist() == [3, 3, 1] and want[3][:, 0, :2].tolist() == [[1, 121], [1, 57], [1, 121]]
    both_forms(gpu_ctx, small_db, small["records"], pr, pp, want, max_env=1)
    both_forms(gpu_ctx, small_db, small["records"], pr, pp, P.envelope_pairs(small["models"], small["records"], pr, pp, 0, rows=True), max_env=0)


def test_max_block_rows_changes_nothing(small, small_db, gpu_ctx):
    """a block per pair against the default: the same bytes"""
    both_forms(gpu_ctx, small_db, small["records"], small["pr"], small["pp"], small["want"], max_block_rows=1)
    both_forms(gpu_ctx, small_db, small["records"], small["pr"], small["pp"], small["want"], max_block_rows=300)


@pytest.fixture(scope="module")
def cset():
    """every kernel class at both edges: the profiles of hmm_classes_case.SET_ORDER (profile number and class differ) and profiles of 1 and 2 nodes,
    each against pieces of its own consensus with nodes left out between them (the D scan across lanes) and with background between them"""
    rng = np.random.default_rng(1345)
    texts = [K.model_text(M) for M in K.SET_ORDER] + [R.write_hmm(R.synth_model(rng, M)) for M in (1, 2)]
    models = [m for t in texts for m in R.parse_hmm(t)]
    records, pr, pp = [], [], []
    for p, m in enumerate(models):
        c = R.consensus(m["tables"])
        if m["name"].startswith("DEL"):
            recs = K.deletion_records(c, m["M"])[:2] + [c[:40] + R.background(rng, 20) + c[-40:]]
        elif m["M"] <= 2:
            recs = [c, c + c + c, R.background(rng, 70)]
        else:
            recs = [c[:40] + R.background(rng, 20) + c[100:160]]
        pr += list(range(len(records), len(records) + len(recs)))
        pp += [p] * len(recs)
        records += recs
    order = rng.permutation(len(pr))
    pr, pp = np.array(pr, np.uint32)[order], np.array(pp, np.uint32)[order]
    return {"texts": texts, "models": models, "records": records, "pr": pr, "pp": pp, "want": P.envelope_pairs(models, records, pr, pp, 4, rows=True)}


def test_every_class_and_the_one_node_profile(cset, gpu_ctx):
    import gsearch_amd as G
    assert sorted(F.group_size(m["M"]) for m in cset["models"]).count(20) >= 2 and {F.group_size(m["M"]) for m in cset["models"]} == set(F.CLASS_G)
    assert (cset["want"][0] != R.NO_SCORE).all() and (cset["want"][2] >= 1).sum() > 50 and cset["want"][2].max() == 3
    d = G.HmmDb(cset["texts"], gpu_ctx, texts=True)
    try:
        both_forms(gpu_ctx, d, cset["records"], cset["pr"], cset["pp"], cset["want"])
    finally:
        d.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_on_poisoned_scratch(small, gpu_ctx, byte):
    """host and device form twice on scratch and allocations filled with a chosen byte: nothing reads what nothing wrote"""
    import gsearch_amd as G
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        d = G.HmmDb(small["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                both_forms(gpu_ctx, d, small["records"], small["pr"], small["pp"], small["want"], max_block_rows=500)
        finally:
            d.close()
    finally:
        G.debug_mem_fill(None)


def test_refusals_write_nothing(small, small_db, gpu_ctx):
    import gsearch_amd as G
    L, db = gpu_ctx.L, small_db
    aa = np.frombuffer(b"ACDEFGHIKL" * 4, np.uint8)
    rs, rl = np.array([0, 0, 10], np.uint64), np.array([10, F.FWD_MAX_L + 1, 10], np.uint64)          # a faked length: nothing reads record 1
    n_prof = len(db)

    def host(pr, pp, ctx=gpu_ctx):
        pr, pp = np.array(pr, np.uint32), np.array(pp, np.uint32)
        outs = [np.full(len(pr), 77, np.int32), np.full(len(pr), 77, np.int32), np.full(len(pr), 77, np.uint32), np.full((len(pr), 2, 4), 77, np.int32)]
        rc = L.gs_hmm_envelopes(ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 3, pr.ctypes.data, pp.ctypes.data, len(pr), 2, 0, outs[0].ctypes.data,
                                outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data, None, None, None)
        return rc, all((o == 77).all() for o in outs)

    for pr, pp, code in (([0, 3], [0, 0], GS_ERR_INVALID), ([0, 2], [0, n_prof], GS_ERR_INVALID), ([R.NO_HIT], [n_prof], GS_ERR_INVALID),
                         ([0, 1, 2], [0, 0, 0], GS_ERR_UNSUPPORTED)):
        assert host(pr, pp) == (code, True), (pr, pp)
        env_dev(gpu_ctx, db, pr, pp, (aa, rs, rl), max_env=2, rows=False, rc_want=code)               # asserts the code and the canaries
    other = G.Context(0)
    try:
        assert host([0], [0], other) == (GS_ERR_INVALID, True)
        env_dev(other, db, [0], [0], (aa, rs, rl), max_env=2, rows=False, rc_want=GS_ERR_INVALID)
    finally:
        other.close()
    # an over-long record that no pair names is accepted
    pr, pp = np.array([2, 0, R.NO_HIT], np.uint32), np.array([1, 0, 0], np.uint32)
    want = P.envelope_pairs(small["models"], [b"ACDEFGHIKL", b"", b"ACDEFGHIKL"], pr, pp, 2)
    assert same(db.envelopes_packed(aa, rs, rl, pr, pp, max_env=2), want) and same(env_dev(gpu_ctx, db, pr, pp, (aa, rs, rl), max_env=2, rows=False)[:4], want)


def test_one_long_record(gpu_ctx):
    """65 536 residues of background with one planted consensus against 1 280 nodes: the range of both passes, and row buffers behind a pair whose rows
    push the offsets of the long one; the expected words come from the golden file (the restatement takes minutes at this size)"""
    import gsearch_amd as G
    with open(os.path.join(HERE, "golden", "hmm_posterior_limits.json")) as f:
        (gold,) = json.load(f)["cases"]
    text = K.model_text(gold["M"])
    assert K.sha256(text) == gold["sha256"], "the profile text is not the one the golden file was computed from"
    model = R.parse_hmm(text)[0]
    rng = np.random.default_rng(gold["seed"])
    c = R.consensus(model["tables"])
    at = gold["planted_at"] - 1
    rec = R.background(rng, at) + c + R.background(rng, gold["L"] - at - gold["M"])
    assert len(rec) == gold["L"] == F.FWD_MAX_L and gold["env"][0][:2] == [gold["planted_at"], at + gold["M"]]
    short = c[:50]
    w_short = P.envelope_pairs([model], [short], [0], [0], 2, rows=True)
    d = G.HmmDb([text], gpu_ctx, texts=True)
    try:
        pr, pp = np.array([1, 0], np.uint32), np.zeros(2, np.uint32)
        for got in (d.envelopes_packed(*pack([rec, short]), pr, pp, max_env=2, rows=True), env_dev(gpu_ctx, d, pr, pp, pack([rec, short]), max_env=2)):
            assert [int(got[0][1]), int(got[1][1]), int(got[2][1])] == [gold["fwd"], gold["bck"], len(gold["env"])]
            assert got[3][1, :len(gold["env"])].tolist() == gold["env"]
            assert hashlib.sha256(got[4][1].tobytes()).hexdigest() == gold["out_sha256"] and hashlib.sha256(got[5][1].tobytes()).hexdigest() == gold["cont_sha256"]
            assert same([g[:1] for g in got], w_short)
        assert d.search_forward([rec], filter_p=None)[1][0, 0] == gold["fwd"]
    finally:
        d.close()


def test_tables_of_hmmsearch_and_envelope_universal_genes(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(1347)
    paths = [fixture_path(n) for n in FIXTURES]
    models = [m for n in FIXTURES for m in R.parse_hmm(open(fixture_path(n), "rb").read())]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    bg = lambda n: R.background(rng, n)                                                         # noqa: E731
    seqs = [bg(150), bg(40) + c0 + bg(25), c1 + bg(30) + c1, c0[:80], bg(90) + c1[10:], c0[:30] + c0[70:], bg(40)]
    ids = ["prot%d" % i for i in range(len(seqs))]
    faa = str(tmp_path / "p.faa")
    _write_faa(faa, ids, seqs, False)
    for score in ("viterbi", "forward"):
        eout = str(tmp_path / ("env_%s.tsv" % score))
        res = G.hmmsearch(faa, paths, ctx=gpu_ctx, score=score, envelopes=eout)
        assert len(res) == 4 and res[0] == ids
        listed = P.listed_pairs(models, res[1])
        pr, pp = np.array([r for r, _ in listed], np.uint32), np.array([p for _, p in listed], np.uint32)
        _, _, ne, env = P.envelope_pairs(models, seqs, pr, pp, 8)
        want = P.envelope_table_bytes(models, ids, listed, ne, env)
        assert res[3] == want and open(eout, "rb").read() == want
        assert b"prot1\tRibosomal_S9\tPF00380.20\t1\t1\t41\t161\t" in want and b"\t2\t2\t88\t144\t" in want
    both = G.hmmsearch(faa, paths, ctx=gpu_ctx, score="forward", domains=str(tmp_path / "d.tsv"), envelopes=str(tmp_path / "e.tsv"))
    assert len(both) == 5 and both[4] == res[3] and both[3].startswith(b"target\tprofile\tacc\tdom\t")
    assert len(G.hmmsearch(faa, paths, ctx=gpu_ctx)) == 3                              # without envelopes= the return value is what it was
    # universal genes: from the first envelope through the last of every best hit, and the default still the whole protein
    genomes = [[bg(100), seqs[2], c0[:100], seqs[1]], [bg(60)], [seqs[5]]]
    files = []
    for g, gs in enumerate(genomes):
        files.append(str(tmp_path / ("g%d.faa" % g)))
        _write_faa(files[-1], ["g%d_%d" % (g, i) for i in range(len(gs))], gs)
    whole, local = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward")
    cut, local2 = G.universal_genes(files, paths, ctx=gpu_ctx, score="forward", region="envelope")
    assert np.array_equal(local, local2) and whole == [[seqs[1], seqs[2]], [], [seqs[5]]]
    want = []
    for g, gs in enumerate(genomes):
        want.append([])
        for p, r in enumerate(local[g]):
            if r != R.NO_HIT:
                env = P.posterior(models[p]["tables"], gs[r])["env"]
                want[-1].append(gs[r][env[0][0] - 1:env[-1][1]] if env else gs[r])
    assert cut == want and cut[0] == [c0, c1 + seqs[2][57:87] + c1]
