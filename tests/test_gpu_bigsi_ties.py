"""bigsig's tied top hits on the device (the TIES form of k_bigsi_query, k_bigsi_verdict; SPEC.md 11.2): every array == the numpy restatement
tests/pyref_bigsi_ties.py, and tied[0] == the best_colour of the existing query on the same reads.

Ties are planted by adding one genome as several colours. Colour counts 1, 2, 63, 64, 65, 130 and 4097 give W = 1, 1, 1, 1, 2, 3 (lane groups of 1, 2
and 4 words) and 65 words (two chunks: colours 0..4095 and colour 4096). The 4097-colour index holds every chunk case: the same genome in two words of the
first chunk and in the second (append), a first-chunk tie beaten by colour 4096 (restart), colour 4096 below a first-chunk tie (ignored), and one genome as
m colours for every m in {1, 2, 3, 4, 16, 17, 41, 43, 56} = max_ties, max_ties + 1 and max_ties + 40 for max_ties in {1, 3, 16}.

scenario() builds an index's genomes, its reads and the restatement's answers with no device; the conditions that keep the test honest (all five verdicts,
n_tied == 2, n_tied > max_ties, a tie across both chunks, a sig_colour that is not tied[0]) are asserted there."""
import functools
import gzip

import numpy as np
import pytest

import gsearch_amd as G
import pyref_bigsi as R
import pyref_bigsi_mini as RM
import pyref_bigsi_ties as RT

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
GLEN = 2000                                         # bases of a genome
MULT = (3, 4, 16, 17, 41, 43, 56)                   # with the unique and the doubled genomes: max_ties, + 1, + 40 for max_ties in (1, 3, 16)
MAX_TIES = (1, 3, 16)
BLOOM = {1: 4099, 2: 1 << 14, 63: 1 << 16, 64: 1 << 16, 65: 1 << 16, 130: 1 << 17, 4097: 1 << 18}
FP = 1e-3


def _seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def _plan(n, rng):
    """(genomes: one list of records per colour, groups: name -> the colours that hold that genome whole, named: name -> genome)"""
    named = {x: _seq(rng, GLEN) for x in ("A", "B", "C", "S", "X")}
    put = {}                                                            # colour -> records
    if n == 1:
        put[0] = [named["A"]]
    elif n == 2:
        put[0], put[1] = [named["A"]], [named["A"]]
    elif n <= 64:
        for c in (3, n - 1):
            put[c] = [named["A"]]                                       # inside one word
        for c in (10, 11, 40):
            put[c] = [named["B"]]
        put[20], put[50] = [named["S"], named["X"]], [named["S"]]       # the earlier colour has more bits set: sig_colour is the later one
    elif n <= 130:
        for c in ([3, 64] if n == 65 else [3, 70, 129]):
            put[c] = [named["A"]]                                       # in two / three words of a chunk (a narrow matrix: lane groups)
        for c in (10, 40):
            put[c] = [named["B"]]                                       # inside one word
        put[20], put[50] = [named["S"], named["X"]], [named["S"]]
    else:
        assert n == 4097
        half = GLEN // 2
        put[5], put[70] = [named["A"]], [named["A"]]
        put[7], put[8] = [named["B"][:half]], [named["B"][:half]]
        put[9], put[10] = [named["C"]], [named["C"]]
        put[4096] = [named["A"], named["B"], named["C"][:half]]         # the second chunk
        put[20], put[50] = [named["S"], named["X"]], [named["S"]]
        c = 100
        for m in MULT:
            named["M%d" % m] = _seq(rng, GLEN)
            for _ in range(m):
                put[c] = [named["M%d" % m]]
                c += 1
        assert c < 4096
    genomes = [put[c] if c in put else [_seq(rng, GLEN)] for c in range(n)]
    groups = {x: [c for c in range(n) if genomes[c] == [g]] for x, g in named.items()}
    return genomes, groups, named


@functools.lru_cache(maxsize=None)
def scenario(n, k=21, m=0, h=3, down_sample=1):
    """no device: the genomes of an index of n colours, its reads, and per max_ties the restatement's (n_kmers, best_hits, n_tied, tied, sig_colour, tail,
    verdict, best_colour of the plain query)"""
    rng = np.random.default_rng(1000 + n)
    B = BLOOM[n]
    genomes, groups, named = _plan(n, rng)
    ref = RM.Index(k, m, h, B) if m else R.Index(k, h, B)
    for g in genomes:
        ref.add(g)
    cut = lambda g, s, l: g[s:s + l]                                                     # noqa: E731
    reads = []
    for x in sorted(named):
        if x != "X":
            reads += [[cut(named[x], 100, 200)], [cut(named[x], 901, 199)]]              # inside the first half; across the middle
    reads.append([cut(named["A"], 100, 150), cut(named["A"], 1500, 100)])                # a pair: two records
    reads.append([cut(named["A"], 300, 60) + b"N" + cut(named["A"], 361, 120)])
    for _ in range(8):                                                                   # single colours
        c = int(rng.integers(n))
        reads.append([cut(genomes[c][0], int(rng.integers(0, len(genomes[c][0]) - 300)), int(rng.integers(100, 301)))])
    reads += [[_seq(rng, int(rng.integers(100, 301)))] for _ in range(6)]                # chance hits alone
    reads += [[_seq(rng, k + int(rng.integers(0, 3)))] for _ in range(6)]                # one to three k-mers: mostly no hit
    reads += [[named["A"][:k - 1]], [b"N" * 150], [b""], []]                             # too short
    nk, dense = np.zeros(len(reads), np.uint32), np.zeros((len(reads), n), np.uint32)
    for r, read in enumerate(reads):
        nk[r], dense[r] = ref.counts(read, down_sample=down_sample)
    want = {}
    for mt in MAX_TIES:
        bh, nt, td, sc = RT.ties_from_dense(dense, ref.t(), mt)
        tl, vd = RT.verdict(ref, nk, bh, nt, sc, FP)
        want[mt] = (nk, bh, nt, td, sc, tl, vd, np.array([R.best(d)[0] for d in dense], np.uint32))
    # what keeps the test honest
    nk, bh, nt, td, sc, tl, vd, _ = want[16]
    assert (nk[-4:] == 0).all() and (vd[-4:] == RT.TOO_SHORT).all()
    if n >= 2:
        assert (nt == 2).any() and RT.TIED in vd and len(groups["A"]) >= 2 and set(groups["A"]) <= set(td[0][:nt[0]].tolist())
        assert (want[1][2] > 1).any()                                                    # n_tied > max_ties
    if n >= 63:
        assert any(s != t[0] and s != NONE for s, t in zip(sc, td)), "no read whose sig_colour is not tied[0]"
        assert ((bh > 0) & (nt == 1)).any() and RT.UNIQUE in vd
    if n == 4097 and m == 0 and down_sample == 1:
        assert set(vd.tolist()) == {RT.TOO_SHORT, RT.NO_HITS, RT.NOT_SIGNIFICANT, RT.UNIQUE, RT.TIED}
        seen = set(nt.tolist())
        assert {1, 2} | set(MULT) <= seen, sorted(seen)
        for mt in MAX_TIES:
            assert {mt, mt + 1, mt + 40} <= seen and (want[mt][3][nt > mt] != NONE).all() and (want[mt][3][nt == 0] == NONE).all()
        assert any(nt[r] >= 3 and td[r][nt[r] - 1] == 4096 and td[r][0] < 4096 for r in range(len(nt))), "no tie in both chunks"       # append
        assert any(nt[r] == 1 and td[r][0] == 4096 and dense[r][7] == dense[r][8] > 0 for r in range(len(nt))), "no restart"
        assert any(nt[r] == 2 and td[r][:2].tolist() == [9, 10] and 0 < dense[r][4096] < bh[r] for r in range(len(nt))), "no ignored second chunk"
    return genomes, reads, ref, want


def _index(ctx, genomes, n, k=21, m=0, h=3):
    bx = G.Bigsi(k, h, BLOOM[n], n, ctx=ctx, minimizer_len=m)
    bx.add_genomes(genomes)
    return bx


def _check(bx, reads, want, down_sample=1):
    for mt in MAX_TIES:
        nk, bh, nt, td, sc = bx.query_ties(reads, down_sample=down_sample, max_ties=mt)
        wnk, wbh, wnt, wtd, wsc, wtl, wvd, wbc = want[mt]
        assert td.shape == (len(reads), mt) and td.dtype == np.uint32
        assert np.array_equal(nk, wnk) and np.array_equal(bh, wbh), mt
        assert np.array_equal(nt, wnt), (mt, nt.tolist(), wnt.tolist())
        assert np.array_equal(td, wtd), mt
        assert np.array_equal(sc, wsc), mt
        tl, vd = bx.verdict(nk, bh, nt, sc, FP)
        assert np.array_equal(tl.view(np.uint64), wtl.view(np.uint64)) and np.array_equal(vd, wvd), mt
    qnk, qbc, qbh = bx.query(reads, down_sample=down_sample)                             # the existing call on the same reads
    assert np.array_equal(qnk, nk) and np.array_equal(qbh, bh) and np.array_equal(qbc, wbc)
    assert np.array_equal(td[:, 0][bh > 0], qbc[bh > 0]) and (td[:, 0][bh == 0] == NONE).all()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 4097])
def test_colour_counts(gpu_ctx, n):
    genomes, reads, ref, want = scenario(n)
    bx = _index(gpu_ctx, genomes, n)
    assert bx.info()["row_words"] == (n + 63) // 64
    _check(bx, reads, want)
    bx.close()


@pytest.mark.parametrize("kw", [dict(down_sample=3), dict(h=1), dict(h=5), dict(k=31, m=21), dict(k=31, m=21, down_sample=3)], ids=str)
def test_down_sample_hashes_and_minimizer_index(gpu_ctx, kw):
    n = 65
    genomes, reads, ref, want = scenario(n, **kw)
    idx = {x: kw[x] for x in ("k", "m", "h") if x in kw}
    bx = _index(gpu_ctx, genomes, n, **idx)
    _check(bx, reads, want, down_sample=kw.get("down_sample", 1))
    bx.close()


def test_long_read_takes_the_32_plane_launch(gpu_ctx):
    """more than 4096 k-mers: the other launch of the pair; the genome is planted as colours 0 and 2, and once more with extra sequence in front"""
    rng = np.random.default_rng(9)
    k, h, B = 21, 3, 1 << 18
    L, other, extra = _seq(rng, 6000), _seq(rng, 6000), _seq(rng, 3000)
    genomes = [[L], [other], [L], [extra, L]]
    ref = R.Index(k, h, B)
    for g in genomes:
        ref.add(g)
    reads = [[L[100:100 + 4200 + k - 1]], [L[:150]], [other[1000:1000 + 4100 + k - 1]]]
    bx = G.Bigsi(k, h, B, 4, ctx=gpu_ctx)
    bx.add_genomes(genomes)
    for d in (1, 3):
        wnk, _, _, _, _, dense = RT.query_ties(ref, reads, down_sample=d)
        for mt in (1, 2, 16):
            got = bx.query_ties(reads, down_sample=d, max_ties=mt)
            for g, w in zip(got, (wnk,) + RT.ties_from_dense(dense, ref.t(), mt)):
                assert np.array_equal(g, w), (d, mt)
        assert got[0][0] == (4200 + d - 1) // d > (4096 if d == 1 else 0) and got[2].tolist() == [3, 3, 1] and got[4].tolist() == [0, 0, 1]
    bx.close()


def test_on_poisoned_memory():
    """a context of its own; the scratch slots of the host form and the caller's device buffers start as 0x00, 0x01 and 0xFF: the slots behind a list are the
    kernel's to write"""
    n = 65
    genomes, reads, ref, want = scenario(n)
    ctx = G.Context(0)
    try:
        for fill in (None, 0x00, 0x01, 0xFF):
            G.debug_mem_fill(fill)
            bx = _index(ctx, genomes, n)
            _check(bx, reads, want)
            bx.close()
    finally:
        G.debug_mem_fill(None)
        ctx.close()


def _dev(ctx, a):
    a = np.ascontiguousarray(a)
    p = ctx.alloc(max(a.nbytes, 8))
    ctx.upload(p, a)
    return p


def test_device_forms_match_host_forms(gpu_ctx):
    n, mt = 130, 3
    genomes, reads, ref, want = scenario(n)
    reads = [r for r in reads if len(r) == 1 and b"N" not in r[0] and len(r[0]) >= 21]  # packed records hold bases only
    ctx = gpu_ctx
    bx = _index(ctx, genomes, n)
    nr = len(reads)
    seq, rs, rl = G.pack_dna_records([r[0] for r in reads])
    q = [_dev(ctx, x) for x in (seq, rs, rl, np.arange(nr + 1, dtype=np.uint64))]
    out = [ctx.alloc(4 * nr) for _ in range(3)] + [ctx.alloc(4 * nr * mt), ctx.alloc(4 * nr), ctx.alloc(8 * nr), ctx.alloc(nr)]
    ctx.memset(out[3], 0xA5, 4 * nr * mt)
    bx.query_ties_dev(q[0], len(seq), q[1], q[2], nr, q[3], nr, out[0], out[1], out[2], out[3], out[4], down_sample=2, max_ties=mt)
    bx.verdict_dev(nr, out[0], out[1], out[2], out[4], FP, out[5], out[6])
    ctx.sync()
    nk, bh, nt, td, sc = bx.query_ties(reads, down_sample=2, max_ties=mt)
    tl, vd = bx.verdict(nk, bh, nt, sc, FP)
    assert (nt > mt).any() or (nt == 2).any()
    for ptr, shape, dt, w in ((out[0], nr, np.uint32, nk), (out[1], nr, np.uint32, bh), (out[2], nr, np.uint32, nt), (out[3], (nr, mt), np.uint32, td),
                              (out[4], nr, np.uint32, sc), (out[5], nr, np.uint64, tl.view(np.uint64)), (out[6], nr, np.uint8, vd)):
        assert np.array_equal(ctx.download(ptr, shape, dt), w)
    for p in q + out:
        ctx.free(p)
    bx.close()


def test_validation_codes(gpu_ctx):
    def code(f):
        with pytest.raises(G.GsError) as e:
            f()
        return e.value.code
    bx = G.Bigsi(21, 3, 4099, 2, ctx=gpu_ctx)
    rd = [[b"ACGT" * 10]]
    assert code(lambda: bx.query_ties(rd)) == -4                       # no colour yet
    assert code(lambda: bx.verdict([1], [1], [1], [0], FP)) == -4
    bx.add_genomes([rd[0]])
    assert code(lambda: bx.query_ties(rd, down_sample=0)) == -1
    assert code(lambda: bx.query_ties(rd, max_ties=0)) == -1 and code(lambda: bx.query_ties(rd, max_ties=1025)) == -1
    nk, bh, nt, td, sc = bx.query_ties(rd, max_ties=1024)
    assert (nk[0], bh[0], nt[0], sc[0]) == (20, 20, 1, 0) and td[0].tolist() == [0] + [NONE] * 1023
    assert all(len(x) == 0 for x in bx.query_ties([]))
    bx.close()


def _fastq(ids, seqs):
    return b"".join(b"@%s some text\n%s\n+\n%s\n" % (i.encode(), s, b"I" * len(s)) for i, s in zip(ids, seqs))


def test_identify_writes_the_six_field_report(gpu_ctx, tmp_path):
    n, mt = 65, 3
    genomes, reads, ref, want = scenario(n)
    accs = ["GCF_%03d.1" % (n - i) for i in range(n)]
    bx = _index(gpu_ctx, genomes, n)
    bx.set_accessions(accs)
    single = [r for r in reads if len(r) == 1 and len(r[0]) > 0]
    pairs = [r for r in reads if len(r) == 2]
    keep = [i for i, r in enumerate(reads) if len(r) == 1 and len(r[0]) > 0]
    ids = ["read%d" % i for i in range(len(single))]
    (tmp_path / "q.fq.gz").write_bytes(gzip.compress(_fastq(ids, [r[0] for r in single])))
    (tmp_path / "q.fa").write_bytes(b"".join(b">%s\n%s\n" % (i.encode(), r[0]) for i, r in zip(ids, single)))
    wnk, wbh, wnt, wtd, wsc, wtl, wvd, wbc = (x[keep] for x in want[mt])
    for name in ("q.fq.gz", "q.fa"):
        prefix = str(tmp_path / ("ties_" + name))
        got = G.bigsig_identify(bx, tmp_path / name, prefix, fp_correct=3.0, batch=7, ctx=gpu_ctx, report="ties", max_ties=mt)
        assert np.array_equal(got["n_tied"], wnt) and np.array_equal(got["tied"], wtd) and np.array_equal(got["verdict"], wvd)
        assert open(prefix + "_reads.txt", "rb").read() == RT.reads_txt(accs, ids, wnk, wbh, wnt, wtd, wvd)
        assert open(prefix + "_counts.txt", "rb").read() == RT.counts_txt(accs, wtd, wvd)
        assert RT.TIED in wvd and (wnt > mt).any()
        # report="best" is the path of before: the files bigsig_write_reads writes from the plain query
        best = str(tmp_path / ("best_" + name))
        old = G.bigsig_identify(bx, tmp_path / name, best, fp_correct=3.0, batch=7, ctx=gpu_ctx)
        nk, bc, bh = bx.query(single)
        _, acc = bx.classify(nk, bc, bh, FP)
        G.bigsig_write_reads(str(tmp_path / "direct"), accs, ids, bc, bh, nk, acc)
        assert np.array_equal(old["best_colour"], bc) and "n_tied" not in old
        for ext in ("_reads.txt", "_counts.txt"):
            assert open(best + ext, "rb").read() == open(str(tmp_path / "direct") + ext, "rb").read()
    # mates of pairs: two files
    pid = ["pair%d" % i for i in range(len(pairs))]
    (tmp_path / "p1.fa").write_bytes(b"".join(b">%s\n%s\n" % (i.encode(), r[0]) for i, r in zip(pid, pairs)))
    (tmp_path / "p2.fa").write_bytes(b"".join(b">%s\n%s\n" % (i.encode(), r[1]) for i, r in zip(pid, pairs)))
    got = G.bigsig_identify(bx, [tmp_path / "p1.fa", tmp_path / "p2.fa"], str(tmp_path / "pairs"), ctx=gpu_ctx, report="ties", max_ties=mt)
    kp = [i for i, r in enumerate(reads) if len(r) == 2]
    assert len(kp) >= 1 and np.array_equal(got["n_tied"], want[mt][2][kp]) and np.array_equal(got["n_kmers"], want[mt][0][kp])
    with pytest.raises(G.GsError) as e:
        G.bigsig_identify(bx, tmp_path / "q.fa", str(tmp_path / "x"), ctx=gpu_ctx, report="all")
    assert e.value.code == -1
    bx.close()
