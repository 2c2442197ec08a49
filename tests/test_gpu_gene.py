"""genes on the device (gs_gene.hip) against the restatement of SPEC 15 (tests/pyref_gene.py): `==` on every array of every call. The shapes come from
what the kernels do: the scoring kernel gives a wavefront to an ORF and walks it in trips of 256 codons from the 3' end, four codons a lane (ORFs of 30
to 5000 codons, edges at 64, 128 and 256); the chain kernel gives a wavefront to a record and stages 64 candidates at a time (records with none, more
than 64 and more than 4096) whose range it finds by bisection of sort keys built on tiles of 192 bases (records of whole tiles with genes that end at
their high edge, in front of a record with and one without candidates); the histograms flush LDS tables per genome (two genomes, 300 records over three). The constructed cases are the tables of
tests/gene_cases.py, whose properties tests/test_gene_cpu.py checks without a device. Every device-resident entry is held to its host twin too."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import gene_cases as GC
import pyref_gene as R
import pyref_hmm as RH
import pyref_orf as RO

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("PF00380.20.HMM", "TIGR00964.HMM")
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3
KEYS = ("gene", "aa", "aa_start", "aa_len", "rec_gene_off", "info", "tables")


def _same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _packed(records):
    """records at base offsets that are no multiple of 4 as a rule"""
    starts, at = [], 1
    for i, r in enumerate(records):
        starts.append(at)
        at += len(r) + (2, 5, 1, 0, 3)[i % 5]
    starts = np.array(starts, np.uint64)
    return RO.pack_at(records, starts), starts, np.array([len(r) for r in records], np.uint64)


def _score_case(ctx, case, host=False):
    import gsearch_amd as G
    seq, rs, rl = GC.packed(case)
    orf = np.array([(b, r, s) for r, b, n, s in case["orfs"]], G.ORF_DTYPE)
    return G.gene_score(seq, rs, rl, case["goff"], case["tables"], orf, [n for _, _, n, _ in case["orfs"]], ctx=ctx, host=host, min_aa=case["min_aa"],
                        min_score=case["min_score"], max_overlap=min(60, 3 * case["min_aa"] - 1))


@pytest.fixture(scope="module")
def scoring():
    cases = GC.scoring_cases()
    return [(c, R.score(c["records"], c["goff"], c["tables"], c["orfs"], c["min_aa"], c["min_score"])) for c in cases]


@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_scoring_cases(gpu_ctx, scoring, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for case, want in scoring:
            got = _score_case(gpu_ctx, case)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and np.array_equal(a, b), case["name"]
            if fill is None:
                for a, b in zip(got, _score_case(gpu_ctx, case, host=True)):                       # the host twin
                    assert np.array_equal(a, b), case["name"]
    finally:
        G.debug_mem_fill(None)


@pytest.mark.parametrize("fill", [None, 0xFF])
def test_train_equals_restatement_and_host_twin(gpu_ctx, fill):
    import gsearch_amd as G
    records, goff, iv = GC.training_input()
    want_t, want_i = R.train(records, goff, iv, min_train_codons=18000)
    seq, rs, rl = _packed(records)
    ivs = np.array([(b, n, r, s) for r, b, n, s in iv], G.GENE_INTERVAL_DTYPE)
    G.debug_mem_fill(fill)
    try:
        got_t, got_i = G.gene_train(seq, rs, rl, goff, ivs, ctx=gpu_ctx, min_train_codons=18000)
    finally:
        G.debug_mem_fill(None)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_t, want_t)
    host_t, host_i = G.gene_train(seq, rs, rl, goff, ivs, host=True, min_train_codons=18000)
    assert np.array_equal(got_i, host_i) and np.array_equal(got_t, host_t)
    # more than one workgroup of intervals, a genome change inside one: 700 short intervals over two genomes
    rng = np.random.default_rng(3)
    many = sorted((int(rng.integers(0, 2)) * 3, int(rng.integers(0, 9000)), int(rng.integers(0, 40)), int(rng.integers(0, 2))) for _ in range(700))
    want_t, want_i = R.train(records, goff, many, min_train_codons=100)
    got_t, got_i = G.gene_train(seq, rs, rl, goff, np.array([(b, n, r, s) for r, b, n, s in many], G.GENE_INTERVAL_DTYPE), ctx=gpu_ctx, min_train_codons=100)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_t, want_t)
    # no interval at all: the prior alone, every entry log2(A / A) = 0
    got_t, got_i = G.gene_train(seq, rs, rl, goff, ivs[:0], ctx=gpu_ctx)
    assert not got_t.any() and not got_i.any()


def _call(ctx, case, **kw):
    import gsearch_amd as G
    seq, rs, rl = _packed(case["records"])
    return G.gene_call_packed(seq, rs, rl, case["goff"], ctx=ctx, tables=True, **dict(case["params"], **kw))


@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_pipeline_cases(gpu_ctx, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for case in GC.pipeline_cases():
            got = _call(gpu_ctx, case)
            _same(got, GC.pipeline_result(case))
            if fill is None:
                print("%-45s %5d genes %7d residues" % (case["name"], len(got["gene"]), len(got["aa"])))
    finally:
        G.debug_mem_fill(None)


class _Dev:
    """packed records on the device and canary-guarded outputs of gs_gene_call_dev"""
    GUARD = 256

    def __init__(self, ctx, records, goff):
        self.ctx = ctx
        self.seq, rs, rl = _packed(records)
        self.n_rec, self.ng = len(records), len(goff) - 1
        arrs = (self.seq, rs, rl, np.array(goff, np.uint64))
        self.ptrs = [ctx.alloc(max(a.nbytes, 16)) for a in arrs]
        for p, a in zip(self.ptrs, arrs):
            if a.nbytes:
                ctx.upload(p, a)
        self.info, self.tab = ctx.alloc(16 * self.ng), ctx.alloc(4 * 4096 * self.ng)
        self.ptrs += [self.info, self.tab]

    def outputs(self, cap_gene, cap_aa):
        sizes = [32 * cap_gene, cap_aa, 8 * cap_gene, 8 * cap_gene, 8 * (self.n_rec + 1)]
        outs = []
        for n in sizes:
            p = self.ctx.alloc(n + 2 * self.GUARD)
            self.ctx.memset(p, 0xC5, n + 2 * self.GUARD)
            outs.append(p)
        self.ptrs += outs
        return sizes, outs

    def call(self, cap_gene, cap_aa, outs, tables=True, **kw):
        import gsearch_amd as G
        args = [None] * 5 if outs is None else [p + self.GUARD for p in outs]
        return G.gene_call_dev(self.ctx, self.ptrs[0], self.seq.nbytes, self.ptrs[1], self.ptrs[2], self.n_rec, self.ptrs[3], self.ng, self.info, cap_gene, cap_aa, *args,
                               tables_out_dev=self.tab if tables else None, **kw)

    def raw(self, sizes, outs):
        return [self.ctx.download(p, (n + 2 * self.GUARD,), np.uint8) for n, p in zip(sizes, outs)]

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)


def test_device_form_counts_caps_and_errors(gpu_ctx):
    import gsearch_amd as G
    case = next(c for c in GC.pipeline_cases() if c["name"] == "two_genomes_tables_differ")
    want = GC.pipeline_result(case)
    kw = case["params"]
    ng, na = len(want["gene"]), len(want["aa"])
    d = _Dev(gpu_ctx, case["records"], case["goff"])
    try:
        assert d.call(0, 0, None, **kw) == (ng, na)                                              # count only; info and tables are written
        assert np.array_equal(gpu_ctx.download(d.info, (2, 2), np.uint64), want["info"]) and np.array_equal(gpu_ctx.download(d.tab, (2, 4096), np.int32), want["tables"])
        sizes, outs = d.outputs(ng, na)
        assert d.call(ng, na, outs, tables=False, **kw) == (ng, na)                              # exact capacities, no tables asked for
        gpu_ctx.sync()
        raws = d.raw(sizes, outs)
        for r in raws:
            assert (r[:d.GUARD] == 0xC5).all() and (r[-d.GUARD:] == 0xC5).all()
        body = [r[d.GUARD:len(r) - d.GUARD] for r in raws]
        assert np.array_equal(body[0].view(R.GENE_DTYPE), want["gene"]) and np.array_equal(body[1], want["aa"])
        assert np.array_equal(body[2].view(np.uint64), want["aa_start"]) and np.array_equal(body[3].view(np.uint64), want["aa_len"])
        assert np.array_equal(body[4].view(np.uint64), want["rec_gene_off"])
        for cg, ca in ((ng - 1, na), (ng, na - 1)):                                              # a capacity one short: the counts, nothing written
            sizes, outs = d.outputs(ng, na)
            with pytest.raises(G.GsError) as e:
                d.call(cg, ca, outs, **kw)
            assert e.value.code == GS_ERR_INVALID and e.value.counts == (ng, na)
            gpu_ctx.sync()
            assert all((r == 0xC5).all() for r in d.raw(sizes, outs))
        # a partial pointer set, capacities without outputs
        sizes, outs = d.outputs(ng, na)
        L, prm, n = gpu_ctx.L, G.gene_params(**kw), (C.c_uint64 * 2)()
        full = [p + d.GUARD for p in outs]
        head = (gpu_ctx.h, C.byref(prm), d.ptrs[0], d.seq.nbytes, d.ptrs[1], d.ptrs[2], d.n_rec, d.ptrs[3], d.ng)
        for miss in range(5):
            a = list(full)
            a[miss] = None
            assert L.gs_gene_call_dev(*head, ng, na, *a, d.info, None, n) == GS_ERR_INVALID
        assert L.gs_gene_call_dev(*head, ng, 0, None, None, None, None, None, d.info, None, n) == GS_ERR_INVALID
        # max_overlap = 3 * min_aa, and the other parameter checks, in every entry
        for bad, code in ((dict(max_overlap=90), GS_ERR_INVALID), (dict(min_aa=0), GS_ERR_INVALID), (dict(rounds=0), GS_ERR_INVALID), (dict(table=1), GS_ERR_UNSUPPORTED),
                          (dict(flags=1), GS_ERR_UNSUPPORTED)):
            pb = G.gene_params(**bad)
            bhead = (gpu_ctx.h, C.byref(pb)) + head[2:]
            assert L.gs_gene_call_dev(*bhead, 0, 0, None, None, None, None, None, d.info, None, n) == code
            assert L.gs_gene_train_dev(*bhead, None, 0, d.tab, d.info) == code
            assert L.gs_gene_score_dev(*bhead, d.tab, None, None, 0, None, None, None) == code
        G.gene_call_packed(d.seq, [0], [400], [0, 1], ctx=gpu_ctx, max_overlap=89)
        # a record outside seq, genome offsets that do not end at n_rec
        assert L.gs_gene_call_dev(gpu_ctx.h, C.byref(prm), d.ptrs[0], 100, *head[4:], 0, 0, None, None, None, None, None, d.info, None, n) == GS_ERR_INVALID
        assert L.gs_gene_train_dev(gpu_ctx.h, C.byref(prm), d.ptrs[0], d.seq.nbytes, d.ptrs[1], d.ptrs[2], 1, d.ptrs[3], 2, None, 0, d.tab, d.info) == GS_ERR_INVALID
    finally:
        d.close()


def test_stage_entries_reject_bad_inputs(gpu_ctx):
    import gsearch_amd as G
    records, goff, iv = GC.training_input()
    seq, rs, rl = _packed(records)
    for wrong in ([(0, 7000, 0, 0)], [(19999, 1, 0, 0)], [(0, 5, 0, 2)], [(0, 5, 9, 0)], [(0, 5, 1, 0), (0, 5, 0, 0)], [(0, 5, 3, 0), (0, 5, 0, 0)]):
        with pytest.raises(G.GsError) as e:
            G.gene_train(seq, rs, rl, goff, np.array(wrong, G.GENE_INTERVAL_DTYPE), ctx=gpu_ctx)
        assert e.value.code == GS_ERR_INVALID, wrong
    tables = np.zeros((2, 4096), np.int32)
    orf = np.array([(0, 0, 0)], G.ORF_DTYPE)
    j, s, f = G.gene_score(seq, rs, rl, goff, tables, orf, [40], ctx=gpu_ctx)
    assert s[0] == 0
    tables[1, 77] = 32769                                                                       # a bad table
    with pytest.raises(G.GsError) as e:
        G.gene_score(seq, rs, rl, goff, tables, orf, [40], ctx=gpu_ctx)
    assert e.value.code == GS_ERR_INVALID
    tables[1, 77] = -32768
    for o, n in (((0, 0, 0), 0), ((0, 0, 0), 6667), ((19999, 0, 0), 1), ((0, 4, 0), 1), ((0, 0, 2), 5)):
        with pytest.raises(G.GsError) as e:
            G.gene_score(seq, rs, rl, goff, tables, np.array([o], G.ORF_DTYPE), [n], ctx=gpu_ctx)
        assert e.value.code == GS_ERR_INVALID, (o, n)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, 11])
def test_planted_genomes_end_to_end(gpu_ctx, seed):
    import gsearch_amd as G
    g, planted = GC.planted_genome(seed, 100000)
    want = R.call([g], [0, 1], train_min_aa=150)
    genes, flat = G.gene_call([[RO.ascii_of(g)]], ctx=gpu_ctx, train_min_aa=150)
    _same(flat, want, KEYS[:-1])
    assert GC.accuracy(planted, flat["gene"])[0] >= 0.95
    assert [(t[0], t[1], t[2], t[3]) for t in genes[0][0]] == [(int(x["begin"]), int(x["end"]), int(x["flags"]) & 1, p) for x, p in zip(want["gene"], want["proteins"])]


def _write_fa(path, ids, contigs, width=70):
    text = b"".join(b">" + i.encode() + b" planted\n" + b"\n".join(c[j:j + width] for j in range(0, len(c), width)) + b"\n" for i, c in zip(ids, contigs))
    with (gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(text)


def test_genecall_files(gpu_ctx, tmp_path):
    """genecall() on .fna and .fna.gz against the files the restatement writes, byte for byte: two contigs, an N run inside one (a segment boundary),
    lower case in places"""
    import gsearch_amd as G
    g, _ = GC.planted_genome(7, 100000)
    a = RO.ascii_of(g)
    contigs = [a[:30000] + b"NNNN" + a[30000:60000].lower(), a[60000:]]
    ids = ["ctgA", "ctgB"]
    ref, info = R.contig_genes(contigs, train_min_aa=150)
    assert int(info[0, 1]) == 1 and sum(len(x) for x in ref) > 60
    for fn in ("g.fna", "g.fna.gz"):
        _write_fa(tmp_path / fn, ids, contigs)
        out = G.genecall(str(tmp_path / fn), str(tmp_path / "out"), ctx=gpu_ctx, train_min_aa=150)
        assert out == {"n_genes": sum(len(x) for x in ref), "trained": True, "Nc": int(info[0, 0])}
        assert open(tmp_path / "out.faa", "rb").read() == R.faa_bytes(ids, ref)
        assert open(tmp_path / "out.ffn", "rb").read() == R.ffn_bytes(ids, contigs, ref)
        assert open(tmp_path / "out.gff", "rb").read() == R.gff_bytes(ids, ref)
    # a genome too small to train: empty files, no error
    _write_fa(tmp_path / "s.fna", ["s"], [a[:20000]])
    out = G.genecall(str(tmp_path / "s.fna"), str(tmp_path / "small"), ctx=gpu_ctx)
    assert out["n_genes"] == 0 and out["trained"] is False
    assert open(tmp_path / "small.faa", "rb").read() == b"" and open(tmp_path / "small.gff", "rb").read() == b"##gff-version 3\n"


def test_universal_genes_from_called_genes(gpu_ctx, tmp_path):
    """the planted-profile genes of tests/test_orf_cpu.py (a profile's consensus, back-translated) in genomes that hold enough coding sequence of the same
    codon choice to train: universal_genes(translate="genes") finds each planted profile's gene, at the gene's own coordinates"""
    import gsearch_amd as G
    paths = [os.path.join(HERE, "golden", "hmm", n) for n in FIXTURES]
    models = [RH.parse_hmm(open(p, "rb").read())[0] for p in paths]
    cons = [RH.consensus(m["tables"]) for m in models]
    rng = np.random.default_rng(21)
    aas = b"ACDEFGHIKLMNPQRSTVWY"
    files, expect = [], []
    for g, fn in enumerate(("a.fna", "b.fna.gz")):
        contigs, where = [], {}
        for ci in range(3):
            parts, at = [rng.integers(0, 4, 300).astype(np.uint8)], 300
            for k in range(16):                                                                     # 16 genes of 450 residues a contig: training material
                if k == 7 and ci in (1, 2):
                    prof = ci - 1
                    prot = b"M" + cons[prof]
                else:
                    prof, prot = None, b"M" + bytes(aas[i] for i in rng.integers(0, 20, 450))
                gene = np.concatenate([RO.back_translate(prot), GC.bases([48])])
                strand = int(rng.integers(0, 2)) if prof is None else (g + prof) % 2
                parts.append(GC.revcomp(gene) if strand else gene)
                if prof is not None:
                    where[prof] = (ci, at, at + len(gene), strand)
                at += len(gene)
                gap = rng.integers(0, 4, int(rng.integers(30, 200))).astype(np.uint8)
                parts.append(gap)
                at += len(gap)
            contigs.append(RO.ascii_of(np.concatenate(parts)))
        _write_fa(tmp_path / fn, ["g%d_c%d" % (g, i) for i in range(3)], contigs)
        files.append(str(tmp_path / fn))
        expect.append(where)
    genomes, local, where = G.universal_genes(files, paths, ctx=gpu_ctx, translate="genes")
    assert where.shape == (2, 2, 4) and (local != RH.NO_HIT).all()
    for g in range(2):
        for prof in (0, 1):
            ci, b, e, s = expect[g][prof]
            got = tuple(int(v) for v in where[g, prof])
            assert got[0] == ci and got[3] == s and (got[1] == b if s else got[2] == e), (g, prof, got, expect[g][prof])       # the contig, the strand, the 3' end
            assert cons[prof][len(cons[prof]) // 10:] in genomes[g][prof]
    # hmmsearch on the first file: its targets are that genome's genes, named by their coordinates
    ids, scores, table = G.hmmsearch(files[0], paths, ctx=gpu_ctx, translate="genes")
    genes, _ = G.gene_call([[c for _, c in G.api._fna_contigs(files[0])]], ctx=gpu_ctx)
    names = [RO.orf_name("g0_c%d" % ci, t[0], t[1], t[2]) for ci, lst in enumerate(genes[0]) for t in lst]
    assert ids == names and scores.shape == (len(names), 2)
    for prof in (0, 1):
        assert (scores[:, prof] >= models[prof]["ga_units"]).sum() == 1
