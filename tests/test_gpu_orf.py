"""orfs on the device (gs_orf.hip) against the restatement of SPEC 14 (tests/pyref_orf.py): `==` on every array a call writes (descriptors,
residues, aa_start, aa_len, rec_orf_off) and on its counts. The shapes are chosen from what the kernels do: a wavefront takes GS_ORF_TILE = 192 bases
of one record (64 lanes x one codon of each class), a pair's carry crosses tiles through a prefix maximum, the scans take 1024 tiles a workgroup
(one random record of 200 000 bases has 1042), offsets are prefix sums over (record, tile), and every byte of the packed buffer is addressed by base,
so record starts that are no multiple of 4 or 32 matter. The constructed cases are the table of tests/orf_cases.py (tests/test_orf_cpu.py checks
without a device that each holds what its name promises). End to end: the planted genomes of tests/test_orf_cpu.py through gs_hmm_search_dev,
hmmsearch(translate=True) and universal_genes(translate=True)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import pyref_hmm as R
import pyref_hmm_trace as T
import pyref_orf as P
from orf_cases import SMALL, TILE

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3


def fixture_path(name):
    return os.path.join(HERE, "golden", "hmm", name)


def _same(got, want):
    for k in ("orf", "aa", "aa_start", "aa_len", "rec_orf_off"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["n_long"] == want["n_long"]


def _starts(records, first=1, gap=(2, 5, 1, 0, 3)):
    """base offsets that leave gaps and are no multiple of 4 as a rule"""
    out, at = [], first
    for i, r in enumerate(records):
        out.append(at)
        at += len(r) + gap[i % len(gap)]
    return np.array(out, np.uint64)


def run(ctx, records, starts=None, **kw):
    """records: code arrays -> (device result, restatement) of one host-form call"""
    import gsearch_amd as G
    starts = _starts(records) if starts is None else np.asarray(starts, np.uint64)
    seq = P.pack_at(records, starts)
    lens = np.array([len(r) for r in records], np.uint64)
    got = G.orf_translate_packed(seq, starts, lens, ctx=ctx, **kw)
    want = P.translate_records(records, **{"min_aa": P.MIN_AA, **kw})
    _same(got, want)
    return got, want


@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_small_cases(gpu_ctx, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for name, records, kw in SMALL:
            got, want = run(gpu_ctx, records, **kw)
            if fill is None:
                print("%-70s %4d ORFs %6d residues %3d long" % (name, len(got["orf"]), len(got["aa"]), got["n_long"]))
    finally:
        G.debug_mem_fill(None)


def test_many_records_and_one_long(gpu_ctx):
    rng = np.random.default_rng(15)
    many = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(50, 401, 300)]
    got, _ = run(gpu_ctx, many, min_aa=20)
    assert len(got["orf"]) > 300
    starts = np.cumsum([3] + [len(r) for r in many[:-1]]).astype(np.uint64)                               # back to back: every start mod 4 and mod 32 occurs
    assert len(set(int(s) % 32 for s in starts)) == 32
    run(gpu_ctx, many, starts=starts, min_aa=20)
    long = [rng.integers(0, 4, 200000).astype(np.uint8)]
    got, _ = run(gpu_ctx, long, starts=[3])
    assert len(got["orf"]) > 1000
    got, _ = run(gpu_ctx, long, starts=[33], min_aa=30, max_aa=60)
    assert got["n_long"] > 0


class _Dev:
    """packed records on the device and canary-guarded outputs of the device form"""
    GUARD = 256

    def __init__(self, ctx, records, starts=None):
        self.ctx = ctx
        starts = _starts(records) if starts is None else np.asarray(starts, np.uint64)
        self.seq = P.pack_at(records, starts)
        lens = np.array([len(r) for r in records], np.uint64)
        self.n_rec = len(records)
        self.ptrs = [ctx.alloc(max(a.nbytes, 16)) for a in (self.seq, starts, lens)]
        for p, a in zip(self.ptrs, (self.seq, starts, lens)):
            if a.nbytes:
                ctx.upload(p, a)

    def outputs(self, cap_orf, cap_aa):
        sizes = [16 * cap_orf, cap_aa, 8 * cap_orf, 8 * cap_orf, 8 * (self.n_rec + 1)]
        outs = []
        for n in sizes:
            p = self.ctx.alloc(n + 2 * self.GUARD)
            self.ctx.memset(p, 0xC5, n + 2 * self.GUARD)
            outs.append(p)
        self.ptrs += outs
        return sizes, outs

    def translate(self, cap_orf, cap_aa, outs, **kw):
        import gsearch_amd as G
        args = [None] * 5 if outs is None else [p + self.GUARD for p in outs]
        return G.orf_translate_dev(self.ctx, self.ptrs[0], self.seq.nbytes, self.ptrs[1], self.ptrs[2], self.n_rec, cap_orf, cap_aa, *args, **kw)

    def raw(self, sizes, outs):
        return [self.ctx.download(p, (n + 2 * self.GUARD,), np.uint8) for n, p in zip(sizes, outs)]

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)


def test_device_form_counts_caps_and_guards(gpu_ctx):
    import gsearch_amd as G
    rng = np.random.default_rng(16)
    records = [rng.integers(0, 4, n).astype(np.uint8) for n in (900, 0, 2 * TILE + 1, 5000)]
    kw = {"min_aa": 12, "max_aa": 50}
    want = P.translate_records(records, **kw)
    no, na = len(want["orf"]), len(want["aa"])
    assert no > 20 and want["n_long"] > 0
    d = _Dev(gpu_ctx, records)
    try:
        assert d.translate(0, 0, None, **kw) == (no, na, want["n_long"])                                   # count only
        # exact capacities: everything written, nothing around it
        sizes, outs = d.outputs(no, na)
        assert d.translate(no, na, outs, **kw) == (no, na, want["n_long"])
        gpu_ctx.sync()
        raws = d.raw(sizes, outs)
        for r in raws:
            assert (r[:d.GUARD] == 0xC5).all() and (r[-d.GUARD:] == 0xC5).all()
        body = [r[d.GUARD:len(r) - d.GUARD] for r in raws]
        assert np.array_equal(body[0].view(P.ORF_DTYPE), want["orf"]) and np.array_equal(body[1], want["aa"])
        assert np.array_equal(body[2].view(np.uint64), want["aa_start"]) and np.array_equal(body[3].view(np.uint64), want["aa_len"])
        assert np.array_equal(body[4].view(np.uint64), want["rec_orf_off"])
        # a capacity one too small: GS_ERR_INVALID, the counts filled, nothing written
        for co, ca in ((no - 1, na), (no, na - 1)):
            sizes, outs = d.outputs(no, na)
            with pytest.raises(G.GsError) as e:
                d.translate(co, ca, outs, **kw)
            assert e.value.code == GS_ERR_INVALID and e.value.counts == (no, na, want["n_long"])
            gpu_ctx.sync()
            assert all((r == 0xC5).all() for r in d.raw(sizes, outs))
        # a partial set of outputs, capacities without outputs
        sizes, outs = d.outputs(no, na)
        L = gpu_ctx.L
        prm = G._lib.OrfParamsC(12, 50, 11, 0)
        n = (C.c_uint64 * 3)()
        full = [p + d.GUARD for p in outs]
        for miss in range(5):
            a = list(full)
            a[miss] = None
            assert L.gs_orf_translate_dev(gpu_ctx.h, C.byref(prm), d.ptrs[0], d.seq.nbytes, d.ptrs[1], d.ptrs[2], d.n_rec, no, na, *a, n) == GS_ERR_INVALID
        assert L.gs_orf_translate_dev(gpu_ctx.h, C.byref(prm), d.ptrs[0], d.seq.nbytes, d.ptrs[1], d.ptrs[2], d.n_rec, no, 0, None, None, None, None, None, n) == GS_ERR_INVALID
        # the validation of SPEC 14
        for prm_bad, code in (((0, 0, 11, 0), GS_ERR_INVALID), ((10, 9, 11, 0), GS_ERR_INVALID), ((10, 0, 11, 1), GS_ERR_UNSUPPORTED), ((10, 0, 1, 0), GS_ERR_UNSUPPORTED)):
            pb = G._lib.OrfParamsC(*prm_bad)
            assert L.gs_orf_translate_dev(gpu_ctx.h, C.byref(pb), d.ptrs[0], d.seq.nbytes, d.ptrs[1], d.ptrs[2], d.n_rec, 0, 0, None, None, None, None, None, n) == code
            assert L.gs_orf_translate(gpu_ctx.h, C.byref(pb), d.seq.ctypes.data_as(C.c_void_p), d.seq.nbytes, None, None, 0, 0, 0, None, None, None, None, None, n) == code
        assert L.gs_orf_translate_dev(gpu_ctx.h, C.byref(prm), d.ptrs[0], d.seq.nbytes, d.ptrs[1], d.ptrs[2], 1 << 32, 0, 0, None, None, None, None, None, n) == GS_ERR_UNSUPPORTED
        # a record that does not lie inside seq: GS_ERR_INVALID and nothing read outside (seq_bytes one byte short of the last record's end)
        short = int(_starts(records)[-1] + len(records[-1])) // 4 - 1
        assert L.gs_orf_translate_dev(gpu_ctx.h, C.byref(prm), d.ptrs[0], short, d.ptrs[1], d.ptrs[2], d.n_rec, 0, 0, None, None, None, None, None, n) == GS_ERR_INVALID
        with pytest.raises(G.GsError):
            G.orf_translate_packed(d.seq, [0], [10], min_aa=0, ctx=gpu_ctx)
        # no record at all
        assert L.gs_orf_translate_dev(gpu_ctx.h, C.byref(prm), None, 0, None, None, 0, 0, 0, None, None, None, None, None, n) == 0 and list(n) == [0, 0, 0]
    finally:
        d.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    models = [R.parse_hmm(open(fixture_path(n), "rb").read())[0] for n in FIXTURES]
    cases = P.planted_cases(models, seed=7)
    want = P.translate_records([cs["genome"] for cs in cases])
    scores = R.search(models, want["proteins"])
    return {"models": models, "cases": cases, "want": want, "scores": scores}


def _write_fa(path, ids, contigs, width=70):
    text = b"".join(b">" + i.encode() + b" planted\n" + b"\n".join(c[j:j + width] for j in range(0, len(c), width)) + b"\n" for i, c in zip(ids, contigs))
    with (gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(text)


def test_device_orfs_feed_hmm_search(gpu_ctx, planted):
    """gs_hmm_search_dev fed straight from the device outputs of gs_orf_translate_dev"""
    import gsearch_amd as G
    want, models = planted["want"], planted["models"]
    no, na = len(want["orf"]), len(want["aa"])
    d = _Dev(gpu_ctx, [cs["genome"] for cs in planted["cases"]], starts=None)
    db = G.HmmDb([fixture_path(n) for n in FIXTURES], gpu_ctx)
    try:
        sizes, outs = d.outputs(no, na)
        assert d.translate(no, na, outs) == (no, na, 0)
        g = d.GUARD
        d_score = gpu_ctx.alloc(4 * no * len(models))
        d.ptrs.append(d_score)
        db.search_dev(outs[1] + g, outs[2] + g, outs[3] + g, no, d_score)
        got = gpu_ctx.download(d_score, (no, len(models)), np.int32)
        assert np.array_equal(got, planted["scores"])
        # and the planted ORF is every genome's only hit at GA
        off = want["rec_orf_off"]
        for i, cs in enumerate(planted["cases"]):
            col = got[int(off[i]):int(off[i + 1]), cs["model"]]
            assert (col >= models[cs["model"]]["ga_units"]).sum() == 1
    finally:
        db.close()
        d.close()


def test_hmmsearch_translated(gpu_ctx, planted, tmp_path):
    import gsearch_amd as G
    cases, models = planted["cases"], planted["models"]
    paths = [fixture_path(n) for n in FIXTURES]
    # contigs: two planted genomes each, an N run between them (a segment boundary: coordinates stay the contig's), lower case in places
    ids, contigs = [], []
    for k in range(0, len(cases), 2):
        a, b = P.ascii_of(cases[k]["genome"]), P.ascii_of(cases[k + 1]["genome"])
        ids.append("ctg%d" % (k // 2))
        contigs.append(a[:500] + a[500:].lower() + b"NNRN" + b)
    ref = P.contig_orfs(contigs)
    names = [P.orf_name(i, b, e, s) for i, lst in zip(ids, ref) for b, e, s, _ in lst]
    prots = [p for lst in ref for _, _, _, p in lst]
    scores = R.search(models, prots)
    for fn in ("g.fa", "g.fa.gz"):
        _write_fa(tmp_path / fn, ids, contigs)
        got_ids, got_scores, table = G.hmmsearch(str(tmp_path / fn), paths, output=str(tmp_path / "out.tsv"), ctx=gpu_ctx, translate=True)
        assert got_ids == names and np.array_equal(got_scores, scores)
        assert table == R.table_bytes(models, names, scores) == open(tmp_path / "out.tsv", "rb").read()
    assert table.count(b"\t1\n") == len(cases)                                                          # every planted gene passes GA, nothing else does
    # the domain table of the translated targets
    res = G.hmmsearch(str(tmp_path / "g.fa"), paths, ctx=gpu_ctx, translate=True, domains=str(tmp_path / "dom.tsv"))
    listed = [(r, p) for p in range(2) for r in np.lexsort((np.arange(len(names)), -scores[:, p].astype(np.int64))) if scores[r, p] != R.NO_SCORE and scores[r, p] >= 0]
    pr, pp = np.array([r for r, _ in listed], np.uint32), np.array([p for _, p in listed], np.uint32)
    nd = T.trace_pairs(models, prots, pr, pp, 8)[1]
    assert res[3] == T.domain_table_bytes(models, names, scores, *T.trace_pairs(models, prots, pr, pp, max(8, int(nd.max()))), pr, pp)
    # the orf_translate / write_orf_faa pair writes the same targets, byte for byte
    per_contig, flat = G.orf_translate(contigs, ctx=gpu_ctx)
    assert per_contig == ref and flat["n_long"] == 0
    G.write_orf_faa(str(tmp_path / "orfs.faa"), ids, per_contig)
    assert open(tmp_path / "orfs.faa", "rb").read() == P.faa_bytes(ids, ref)
    # translate=False on that protein file: the call as it was, the same scores by another road
    ids_f, scores_f, table_f = G.hmmsearch(str(tmp_path / "orfs.faa"), paths, ctx=gpu_ctx)
    assert ids_f == names and np.array_equal(scores_f, scores) and table_f == table
    with pytest.raises(G.GsError):
        G.hmmsearch(str(tmp_path / "g.fa"), paths, ctx=gpu_ctx, translate=True, table=1)


def test_universal_genes_translated(gpu_ctx, planted, tmp_path):
    import gsearch_amd as G
    cases, models = planted["cases"], planted["models"]
    paths = [fixture_path(n) for n in FIXTURES]
    pick = lambda model, strand, f: next(c for c in cases if (c["model"], c["strand"], c["f"]) == (model, strand, f))      # noqa: E731
    rng = np.random.default_rng(17)
    files, expect = [], []
    for g, (strand, f, fn) in enumerate(((0, 1, "a.fa"), (1, 2, "b.fa.gz"), (1, 0, "c.fa"))):
        # contig 0: random bases only; contig 1: profile 1's gene; contig 2: profile 0's gene
        chosen = [pick(1, strand, f), pick(0, strand, f)]
        contigs = [P.ascii_of(rng.integers(0, 4, 400))] + [P.ascii_of(c["genome"]) for c in chosen]
        _write_fa(tmp_path / fn, ["g%d_c%d" % (g, i) for i in range(3)], contigs)
        files.append(str(tmp_path / fn))
        ref = P.contig_orfs(contigs)
        flat = [(ci, b, e, s, p) for ci, lst in enumerate(ref) for b, e, s, p in lst]
        row = {}
        for prof, ci in ((0, 2), (1, 1)):
            cs = chosen[0] if prof == 1 else chosen[1]
            j = [k for k, (c, b, e, s, p) in enumerate(flat) if c == ci and cs["cons"] in p]
            assert len(j) == 1 and flat[j[0]][3] == strand
            row[prof] = (j[0],) + flat[j[0]]
        expect.append(row)
    files.append(str(tmp_path / "empty.fa"))                                                             # a genome without a hit
    _write_fa(files[-1], ["e0"], [P.ascii_of(rng.integers(0, 4, 600))])
    genomes, local, where = G.universal_genes(files, paths, ctx=gpu_ctx, translate=True)
    assert where.shape == (4, 2, 4) and where.dtype == np.int64 and local.dtype == np.uint32
    for g, row in enumerate(expect):
        assert genomes[g] == [row[0][5], row[1][5]]
        for prof in (0, 1):
            assert int(local[g, prof]) == row[prof][0] and tuple(int(v) for v in where[g, prof]) == row[prof][1:5]
    assert genomes[3] == [] and (local[3] == R.NO_HIT).all() and (where[3] == -1).all()
    # the aligned region: what the trace of the ORF gives, inside the ORF, holding the consensus but for its ends
    aligned, local2, where2 = G.universal_genes(files, paths, ctx=gpu_ctx, translate=True, region="aligned")
    assert np.array_equal(local, local2) and np.array_equal(where, where2) and aligned[3] == []
    for g, row in enumerate(expect):
        for prof in (0, 1):
            prot, hit = row[prof][5], aligned[g][prof]
            cons = R.consensus(models[prof]["tables"])
            _, doms = T.trace(models[prof]["tables"], prot)
            assert hit == prot[doms[0][0] - 1:doms[-1][1]] and hit in prot
            k = len(cons) // 10                     # a local alignment may leave out end nodes whose consensus residue scores below the entry; a tenth is generous
            assert cons[k:len(cons) - k] in hit and len(hit) <= len(cons) + 2 * k
    # Forward scores choose the same ORFs
    g3 = G.universal_genes(files, paths, ctx=gpu_ctx, translate=True, score="forward")
    assert g3[0] == genomes and np.array_equal(g3[1], local)
    # translate=False still returns two values
    G.write_orf_faa(str(tmp_path / "p.faa"), ["x"], [[(0, 3 * len(expect[0][0][5]), 0, expect[0][0][5])]])
    res = G.universal_genes([str(tmp_path / "p.faa")], paths, ctx=gpu_ctx)
    assert len(res) == 2 and res[0] == [[expect[0][0][5]]]
