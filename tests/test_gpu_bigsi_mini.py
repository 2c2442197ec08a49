"""bigsig minimizer indexes and the coverage filter on the device (gs_bigsi.hip; SPEC.md 11.1): the index (rows, t_c, nk_c), the per-read counts, the best
colour, the report files and the index file, every one compared with == against the numpy restatement tests/pyref_bigsi_mini.py. Shapes: the smallest at
which each part can go wrong - window widths 2, 17 and 32 (the widest halo), a colour of records mostly shorter than the window, a record of many tiles,
a build call that starts inside a colour word, a read on either side of the 12- / 32-plane split of the query kernel, values whose counts sit at the filter's
threshold and on either side of it, filters whose sort takes an odd and an even number of passes (the sorted list ends in the other or in the same buffer),
a colour whose occurrence list spans three tiles of the sort with a run of equal values across the first tile edge."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

import gsearch_amd as G
import pyref_bigsi_mini as RM

pytestmark = pytest.mark.gpu

KM = [(22, 21), (31, 15), (32, 1)]


def _seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def _cut(rng, genome, n):
    s = int(rng.integers(0, len(genome) - n + 1))
    return genome[s:s + n]


def _mutate(rng, read, n_sub):
    r = bytearray(read)
    for p in rng.choice(len(r), n_sub, replace=False):
        r[p] = b"ACGT"[(b"ACGT".index(r[p]) + 1 + int(rng.integers(3))) % 4]
    return bytes(r)


def _build(ctx, genomes, k, m, h, B, cap=None, data_t="dna", calls=1, min_count=1):
    bx = G.Bigsi(k, h, B, cap or max(len(genomes), 1), data_t=data_t, ctx=ctx, minimizer_len=m)
    ref = RM.Index(k, m, h, B, fwd_only=data_t == "dna_fwd")
    step = max((len(genomes) + calls - 1) // calls, 1)
    for i in range(0, len(genomes), step):
        bx.add_genomes(genomes[i:i + step], min_count=min_count)
    for g in genomes:
        ref.add(g, min_count=min_count)
    return bx, ref


def _rows_of(ref, B, rng):
    if B <= 4099:
        return np.arange(B)
    return np.unique(np.concatenate(ref.cols + [rng.integers(0, B, 500).astype(np.uint64)]))


def _check_index(bx, ref, rows):
    W = bx.info()["row_words"]
    assert np.array_equal(bx.rows(rows), ref.row_words(rows, W))
    t, nk = bx.bits_set(return_kmers=True)
    assert np.array_equal(t, ref.t()) and nk.tolist() == ref.nk


def _check_query(bx, ref, reads, quals=None, down_sample=1, min_phred=15):
    nk, bc, bh, cnt = bx.query(reads, quals=quals, min_phred=min_phred, down_sample=down_sample, dense=True)
    rnk, rbc, rbh, rcnt = ref.query(reads, quals=quals, min_phred=min_phred, down_sample=down_sample)
    assert np.array_equal(nk, rnk)
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(bh, rbh) and np.array_equal(bc, rbc)
    nk2, bc2, bh2 = bx.query(reads, quals=quals, min_phred=min_phred, down_sample=down_sample)          # without the dense matrix
    assert np.array_equal(nk2, nk) and np.array_equal(bc2, bc) and np.array_equal(bh2, bh)
    return nk, bc, bh, cnt


# ---- build ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colours", [1, 65, 130])
@pytest.mark.parametrize("k,m", KM)
def test_build_rows_bits_and_occurrences(gpu_ctx, k, m, n_colours):
    rng = np.random.default_rng(100 * k + m + n_colours)
    genomes = [[_seq(rng, 200)] for _ in range(n_colours)]
    for B in (64, 4099, 1 << 20):
        bx, ref = _build(gpu_ctx, genomes, k, m, 3, B)
        assert bx.info()["minimizer_len"] == m and bx.info()["k"] == k and bx.info()["n_colours"] == n_colours
        _check_index(bx, ref, _rows_of(ref, B, rng))
        bx.close()


@pytest.mark.parametrize("k,m", [(22, 21), (31, 15)])
def test_short_records_a_record_of_many_tiles_and_two_calls(gpu_ctx, k, m):
    rng = np.random.default_rng(k)
    h, B = 3, 1 << 16
    shorts = [_seq(rng, int(n)) for n in rng.integers(20, 61, 400)]          # about one in four below k = 31, one in twenty below k = 22: no occurrence
    long_one = [_seq(rng, 300000)]
    assert len(long_one[0]) >= 3 * G.BIGSI_MINI_TILE and sum(len(s) < k for s in shorts) >= 10 and sum(len(s) == k for s in shorts) >= 1
    mixed = [_seq(rng, 37), _seq(rng, 20) + b"N" + _seq(rng, 64), b"", _seq(rng, k), b"acgtnnACGT" * 9, _seq(rng, 300) + b"\n" + _seq(rng, 33)]
    genomes = [[_seq(rng, 150)] for _ in range(33)] + [shorts, [], [b"NNNN"], mixed, long_one] + [[_seq(rng, 150)] for _ in range(33)]
    bx, ref = _build(gpu_ctx, genomes, k, m, h, B)
    _check_index(bx, ref, np.arange(B))
    t, nk = bx.bits_set(return_kmers=True)
    assert t[34] == 0 and t[35] == 0 and nk[34] == 0 and nk[33] > 0
    # the long record alone (its tiles spread over many wavefronts) gives the same column
    alone, ref1 = _build(gpu_ctx, [long_one], k, m, h, B)
    _check_index(alone, ref1, np.arange(B))
    assert alone.bits_set()[0] == t[37]
    # two calls: the second starts at colour 36, inside a word
    two, _ = _build(gpu_ctx, genomes, k, m, h, B, calls=2)
    assert np.array_equal(two.rows(np.arange(B)), bx.rows(np.arange(B)))
    for a, b in zip(two.bits_set(return_kmers=True), (t, nk)):
        assert np.array_equal(a, b)
    for x in (bx, alone, two):
        x.close()


def test_forward_only_minimizers(gpu_ctx):
    rng = np.random.default_rng(2)
    genomes = [[_seq(rng, 400)] for _ in range(3)]
    bx, ref = _build(gpu_ctx, genomes, 21, 11, 3, 4099, data_t="dna_fwd")
    _check_index(bx, ref, np.arange(4099))
    read = genomes[1][0][50:200]
    nk, bc, bh, cnt = _check_query(bx, ref, [[read], [read[::-1]]])
    assert bc[0] == 1 and bh[0] == nk[0] > 0
    bx.close()


# ---- query ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=KM, ids=lambda p: "k%d_m%d" % p)
def read_index(request, gpu_ctx):
    k, m = request.param
    rng = np.random.default_rng(11 + k)
    genomes = [[_seq(rng, 2000)] for _ in range(6)] + [[_seq(rng, 7500)]]
    bx, ref = _build(gpu_ctx, genomes, k, m, 3, 1 << 18)
    yield rng, genomes, bx, ref, k, m
    bx.close()


def test_reads(read_index):
    rng, genomes, bx, ref, k, m = read_index
    g0, g1 = genomes[0][0], genomes[1][0]
    exact = [[_cut(rng, genomes[i % 7][0], 150)] for i in range(7)]
    subs = [[_mutate(rng, _cut(rng, genomes[i % 7][0], 150), 3)] for i in range(7)]
    pairs = [[g0[500:650], g0[900:1050][::-1]], [_mutate(rng, g1[100:250], 2), g1[700:800]]]
    special = [[g0[:k - 1]], [g0[100:100 + k]], [b"N" * 150], [g0[200:260] + b"N" + g0[261:350]], [b""], []]
    reads = exact + subs + pairs + special
    quals = [[b"I" * len(r) for r in rd] for rd in reads]
    quals[1] = [b"I" * 40 + b"/" + b"I" * 39 + b"0" + b"I" * 30 + b"#" * 5 + b"I" * 34]       # one below, one at the threshold, a run
    for d in (1, 2, 7):
        nk, bc, bh, cnt = _check_query(bx, ref, reads, quals=quals, down_sample=d)
        n0 = len(reads) - len(special)
        assert nk[n0] == 0 and nk[n0 + 1] == 1 and nk[n0 + 2] == 0 and nk[n0 + 4] == 0 and nk[n0 + 5] == 0 and bh[n0 + 2] == 0 and bc[n0 + 2] == 0
        assert all(cnt[i, i % 7] == nk[i] > 0 for i in (0, 2, 3, 4, 5, 6))             # no false negatives (read 1 has the low-quality bases)
        if d == 1:
            assert nk[n0 + 3] == len(RM.minimizers(reads[n0 + 3][0], k, m)[0])
    for n_reads in (1, 5):
        _check_query(bx, ref, reads[:n_reads])
    _check_query(bx, ref, reads[:16], quals=None)


def test_a_contig_as_a_read_takes_the_32_plane_launch(gpu_ctx):
    """(22, 21): two of three positions are occurrences, so 7 kbp give about 4 600 - past the 2^12 of the short launch"""
    rng = np.random.default_rng(33)
    k, m = 22, 21
    genomes = [[_seq(rng, 2000)], [_seq(rng, 7500)]]
    bx, ref = _build(gpu_ctx, genomes, k, m, 3, 1 << 18)
    contig = genomes[1][0][100:100 + 7200]
    n_ref = len(RM.minimizers(contig, k, m)[0])
    assert n_ref >= 4096
    for d in (1, 2):
        nk, bc, bh, cnt = _check_query(bx, ref, [[contig], [genomes[0][0][:150]]], down_sample=d)
        assert nk[0] == (n_ref + d - 1) // d and bh[0] == nk[0] and bc[0] == 1
        assert (nk[0] >= 4096) == (d == 1) and nk[1] < 4096            # d = 2 brings the same contig back under the split
    bx.close()


def _dev(ctx, a):
    a = np.ascontiguousarray(a)
    p = ctx.alloc(max(a.nbytes, 8))
    ctx.upload(p, a)
    return p


@pytest.mark.parametrize("k,m", [(31, 15), (21, 0)])
def test_device_forms_match_host_forms(gpu_ctx, k, m):
    ctx = gpu_ctx
    rng = np.random.default_rng(40 + m)
    h, B, n_g = 3, 1 << 16, 5
    genomes = [[_seq(rng, 3000) * 2] for _ in range(n_g)]              # every value twice: min_count = 2 keeps them
    # reads from inside the first copy: every one of their values occurs twice (those across the joint of the copies occur once and are filtered)
    reads = [[_cut(rng, genomes[i % n_g][0][:2900], 150)] for i in range(40)] + [[_seq(rng, 150)] for _ in range(8)]
    seq, rs, rl = G.pack_dna_records([g[0] for g in genomes])
    ptrs = [_dev(ctx, x) for x in (seq, rs, rl, np.arange(n_g + 1, dtype=np.uint64))]
    rows = np.arange(B)
    for f in (1, 2):
        host = G.Bigsi(k, h, B, n_g, ctx=ctx, minimizer_len=m)
        host.add_genomes(genomes, min_count=f)
        dv = G.Bigsi(k, h, B, n_g, ctx=ctx, minimizer_len=m)
        dv.add_genomes_dev(ptrs[0], len(seq), ptrs[1], ptrs[2], n_g, ptrs[3], n_g, min_count=f)
        ctx.sync()
        assert np.array_equal(dv.rows(rows), host.rows(rows))
        for a, b in zip(dv.bits_set(return_kmers=True), host.bits_set(return_kmers=True)):
            assert np.array_equal(a, b) and a.min() > 0
        n = len(reads)
        rseq, rrs, rrl = G.pack_dna_records([r[0] for r in reads])
        q = [_dev(ctx, x) for x in (rseq, rrs, rrl, np.arange(n + 1, dtype=np.uint64))]
        out = [ctx.alloc(4 * n) for _ in range(3)] + [ctx.alloc(4 * n * n_g)]
        dv.query_dev(q[0], len(rseq), q[1], q[2], n, q[3], n, out[0], out[1], out[2], d_counts=out[3], down_sample=2)
        ctx.sync()
        nk, bc, bh, cnt = host.query(reads, down_sample=2, dense=True)
        assert np.array_equal(ctx.download(out[0], n, np.uint32), nk) and np.array_equal(ctx.download(out[1], n, np.uint32), bc)
        assert np.array_equal(ctx.download(out[2], n, np.uint32), bh) and np.array_equal(ctx.download(out[3], (n, n_g), np.uint32), cnt)
        assert (bh[:40] == nk[:40]).all() and nk[:40].min() > 0
        for p in q + out:
            ctx.free(p)
        host.close()
        dv.close()
    for p in ptrs:
        ctx.free(p)


# ---- coverage filter ------------------------------------------------------------------------------------------------------------------------------
def _read_set(rng, genome, f):
    """reads over the genome, every stretch of 150 bases once, and three stretches planted f - 1, f and f + 1 times in all"""
    tiles = [genome[i:i + 150] for i in range(0, len(genome) - 149, 150)]
    planted = {3: f - 1, 11: f, 20: f + 1}
    reads = []
    for i, t in enumerate(tiles):
        reads += [t] * planted.get(i, 1)
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], [tiles[i] for i in planted]


def _sort_passes(k, m):
    """8-bit digits the filter's sort walks: the values of a plain index hold 2 k bits, those of a minimizer index 2 m"""
    return (2 * (m or k) + 7) // 8


@pytest.mark.parametrize("f", [2, 3])
@pytest.mark.parametrize("k,m", [(21, 0), (31, 15), (12, 0), (32, 11), (32, 0)])
def test_coverage_filter(gpu_ctx, k, m, f):
    """the sort of the occurrence list walks ceil(2 k / 8) digits (2 m for a minimizer index): (21, 0) six and (31, 15) four, which leave the sorted list in the
    buffer it came in; (12, 0) and (32, 11) three, which leave it in the second buffer, so that the runs go back into the first; (32, 0) eight, with values that
    use the top digit. At k = 12 a value can recur by chance: the planted counts below hold at these seeds"""
    assert _sort_passes(k, m) == {(21, 0): 6, (31, 15): 4, (12, 0): 3, (32, 11): 3, (32, 0): 8}[(k, m)]
    rng = np.random.default_rng(10 * k + f)
    h, B = 3, 1 << 16
    genome = _seq(rng, 5000)
    reads, (below, at, above) = _read_set(rng, genome, f)
    # the planted counts, on the restatement first
    u, c = np.unique(RM.occurrences(reads, k, m), return_counts=True)
    count = dict(zip(u.tolist(), c.tolist()))
    assert (k, m) != (32, 0) or (u >> np.uint64(56) > 0).sum() > len(u) // 2        # the eighth digit is in use
    for stretch, want in ((below, f - 1), (at, f), (above, f + 1)):
        vals = RM.occurrences([stretch], k, m)
        assert len(vals) > 0 and all(count[int(v)] == want for v in vals)
    unique_colour = [_seq(rng, 3000)]                                  # every value once: all of it falls below f
    # a colour of 20 000 bases given f times: thousands of values at the threshold. Where the sort has three passes, the list after two of them (ordered
    # on 16 bits) still has equal values apart - what a filter that reads the wrong one of the two sort buffers would count
    repeated = [_seq(rng, 20000)] * f
    if _sort_passes(k, m) == 3:
        v = RM.occurrences(repeated, k, m)
        two_passes = v[np.argsort(v & np.uint64(0xFFFF), kind="stable")]
        assert (two_passes[1:] != two_passes[:-1]).sum() + 1 > len(np.unique(v)) > 1000
    genomes = [reads, unique_colour, reads[::-1], [], [below] * f, repeated]
    bx, ref = _build(gpu_ctx, genomes, k, m, h, B, min_count=f)
    _check_index(bx, ref, np.arange(B))
    t, nk = bx.bits_set(return_kmers=True)
    assert t[1] == 0 and nk[1] == 0 and t[3] == 0 and t[0] == t[2] > 0 and nk[0] == nk[2] > 0 and t[4] > 0
    assert nk[5] == len(RM.occurrences(repeated, k, m))
    want_nk = sum(n * len(RM.occurrences([s], k, m)) for s, n in ((at, f), (above, f + 1)))
    assert nk[0] == want_nk
    col = bx.rows(np.arange(B))[:, 0]
    assert np.array_equal((col >> np.uint64(2)) & np.uint64(1), col & np.uint64(1))          # colour 2 = colour 0: the order of the reads does not matter
    nkq, bc, bh, cnt = _check_query(bx, ref, [[at], [below], [above]])
    assert cnt[0, 0] == nkq[0] and cnt[2, 0] == nkq[2] and cnt[1, 4] == nkq[1]
    # min_count = 1 is add_genomes bit for bit
    one, _ = _build(gpu_ctx, genomes, k, m, h, B, min_count=1)
    plain = G.Bigsi(k, h, B, len(genomes), ctx=gpu_ctx, minimizer_len=m)
    plain.add_genomes(genomes)
    L = gpu_ctx.L
    text, qual, b, e, off = G.api._text_records(genomes)
    raw = G.Bigsi(k, h, B, len(genomes), ctx=gpu_ctx, minimizer_len=m)
    for mc in (0, 1):
        G._lib.check(L.gs_bigsi_add_batch_min_count(raw.h, text.ctypes.data_as(C.c_void_p), None, 15, b.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(b),
                                                    off.ctypes.data_as(C.c_void_p), len(genomes) if mc == 0 else 0, mc))
    for x in (one, raw):
        assert np.array_equal(x.rows(np.arange(B)), plain.rows(np.arange(B)))
        for a, b_ in zip(x.bits_set(return_kmers=True), plain.bits_set(return_kmers=True)):
            assert np.array_equal(a, b_)
    for x in (bx, one, plain, raw):
        x.close()


SORT_TILE = 16384                       # keys a wavefront owns in the sort and the run-length passes of the filter (gs_radix.hip)
TILE_EDGE_SEED = {(21, 0): 2, (12, 0): 2}      # seeds at which positions 16383 and 16384 of the sorted occurrence list hold one value (about every second seed does)


def _tile_edge_colour(seed, k, m):
    """a genome of 12 000 bases given twice, four stretches of 800 of its bases three times each and a record given once, in a fixed shuffle"""
    rng = np.random.default_rng(seed)
    genome = _seq(rng, 12000)
    stretches = [genome[s:s + 800] for s in (700, 3900, 6100, 10400)]
    once = _seq(rng, 1500)
    records = [genome, genome, once] + stretches * 3
    return genome, stretches, once, [records[i] for i in rng.permutation(len(records))]


@pytest.mark.parametrize("k,m", [(21, 0), (12, 0)])
def test_coverage_filter_across_sort_tiles(gpu_ctx, k, m):
    """one colour of more than two sort tiles of occurrences, a run of equal values across the first tile edge: the head counts of the tiles and the
    heads written have to agree there. (21, 0) sorts in six passes, (12, 0) in three (the sorted list in the second buffer)"""
    h, B, f = 3, 1 << 16, 2
    assert _sort_passes(k, m) == {(21, 0): 6, (12, 0): 3}[(k, m)]
    genome, stretches, once, colour = _tile_edge_colour(TILE_EDGE_SEED[(k, m)], k, m)
    # on the restatement first: the size, the run on the edge, and counts on either side of the threshold
    occ = np.sort(RM.occurrences(colour, k, m))
    assert len(occ) > 2 * SORT_TILE and occ[SORT_TILE - 1] == occ[SORT_TILE]
    u, c = np.unique(occ, return_counts=True)
    count = dict(zip(u.tolist(), c.tolist()))
    assert all(count[int(v)] >= 5 for v in RM.occurrences([stretches[0]], k, m)) and (c == 1).sum() > 1000 and (c == 2).sum() > 5000
    genomes = [[_seq(np.random.default_rng(5), 900) * 2], colour, []]
    bx, ref = _build(gpu_ctx, genomes, k, m, h, B, min_count=f)
    _check_index(bx, ref, np.arange(B))
    t, nk = bx.bits_set(return_kmers=True)
    assert nk[1] == int(c[c >= f].sum()) and t[1] > 0 and nk[2] == 0
    reads = [[stretches[1][100:250]], [genome[5000:5150]], [once[300:450]], [once[:100], genome[200:300]]]
    nkq, bc, bh, cnt = _check_query(bx, ref, reads)
    assert cnt[0, 1] == nkq[0] > 0 and cnt[1, 1] == nkq[1] > 0 and bc[0] == 1
    if k == 21:
        assert cnt[2, 1] < nkq[2] // 4                               # the record given once was dropped: what it still hits are false positives
    bx.close()


# ---- files ----------------------------------------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_and_versions(gpu_ctx, tmp_path):
    rng = np.random.default_rng(9)
    k, m, h, B = 31, 15, 3, 1 << 14
    genomes = [[_seq(rng, 1500)] for _ in range(5)]
    reads = [[_cut(rng, genomes[i % 5][0], 150)] for i in range(12)]
    names = ["GCF_%03d.1" % i for i in range(5)]
    bx, _ = _build(gpu_ctx, genomes, k, m, h, B)
    bx.set_accessions(names)
    path = str(tmp_path / "index.gsmx")
    bx.save(path)
    head = open(path, "rb").read(28)
    assert head[:8] == b"GSBIGSI1" and struct.unpack("<5I", head[8:28]) == (2, k, h, 0, m)
    for cap in (0, 70):
        back = G.Bigsi.load(path, ctx=gpu_ctx, capacity=cap)
        info = back.info()
        assert (info["k"], info["minimizer_len"], info["num_hash"], info["bloom_size"], info["n_colours"], info["colour_capacity"]) == (k, m, h, B, 5, max(cap, 5))
        assert back.accessions() == names
        for a, b in zip(back.bits_set(return_kmers=True), bx.bits_set(return_kmers=True)):
            assert np.array_equal(a, b)
        for a, b in zip(back.query(reads, down_sample=2, dense=True), bx.query(reads, down_sample=2, dense=True)):
            assert np.array_equal(a, b)
        back.close()
    # a plain index still writes version 1, and a version-1 file loads as a plain index
    plain, _ = _build(gpu_ctx, genomes, 21, 0, h, B)
    ppath = str(tmp_path / "index.gsbx")
    plain.save(ppath)
    raw = open(ppath, "rb").read()
    assert struct.unpack("<I", raw[8:12])[0] == 1 and struct.unpack("<4I", raw[8:24]) == (1, 21, h, 0) and struct.unpack("<2Q", raw[24:40]) == (B, 5)
    back = G.Bigsi.load(ppath, ctx=gpu_ctx)
    assert back.info()["minimizer_len"] == 0 and gpu_ctx.L.gs_bigsi_minimizer_len(back.h) == 0
    for a, b in zip(back.query(reads, dense=True), plain.query(reads, dense=True)):
        assert np.array_equal(a, b)
    back.close()
    # any other version, and a minimizer length that is none, are refused as a bad header is
    for patch in (struct.pack("<I", 3), None):
        bad = bytearray(open(path, "rb").read())
        if patch is not None:
            bad[8:12] = patch
        else:
            bad[24:28] = struct.pack("<I", k)
        (tmp_path / "bad.gsmx").write_bytes(bytes(bad))
        with pytest.raises(G.GsError) as e:
            G.Bigsi.load(str(tmp_path / "bad.gsmx"), ctx=gpu_ctx)
        assert e.value.code == -5
    bx.close()
    plain.close()


def _fastq(ids, seqs, quals):
    return b"".join(b"@%s some text\n%s\n+\n%s\n" % (i.encode(), s, q) for i, s, q in zip(ids, seqs, quals))


def test_construct_and_identify_files(gpu_ctx, tmp_path):
    rng = np.random.default_rng(23)
    k, m, h, B = 31, 21, 3, 1 << 18
    accs = ["GCF_B", "GCF_A", "GCF_C"]
    contigs = [[_seq(rng, 3000), _seq(rng, 1200) + b"NNNN" + _seq(rng, 800)] for _ in accs]
    lines = []
    for a, cs in zip(accs, contigs):
        text = b"".join(b">%s_%d contig\n%s\n" % (a.encode(), i, b"\n".join(c[j:j + 70] for j in range(0, len(c), 70))) for i, c in enumerate(cs))
        p = tmp_path / (a + ".fna.gz")
        p.write_bytes(gzip.compress(text))
        lines.append("%s\t%s\n" % (a, p))
    (tmp_path / "refs.txt").write_text("".join(lines))
    bx = G.bigsig_construct(tmp_path / "refs.txt", tmp_path / "idx", k, h, B, ctx=gpu_ctx, minimizer=True)          # value: the default, 21
    assert (tmp_path / "idx.gsmx").exists() and not (tmp_path / "idx.gsbx").exists() and bx.info()["minimizer_len"] == 21
    ref = RM.Index(k, m, h, B)
    for cs in contigs:
        ref.add(cs)
    t, nk = bx.bits_set(return_kmers=True)
    assert bx.accessions() == accs and np.array_equal(t, ref.t()) and nk.tolist() == ref.nk
    n = 24
    ids = ["read%d" % i for i in range(n)]
    seqs = [_cut(rng, contigs[i % 3][0], 150) if i % 4 else _seq(rng, 150) for i in range(n)]
    seqs[5] = seqs[5][:70] + b"N" + seqs[5][71:]
    quals = [bytearray(b"I" * 150) for _ in range(n)]
    for i in range(1, n, 2):
        for j in rng.integers(0, 150, 3):
            quals[i][int(j)] = 33 + int(rng.integers(2, 15))
        quals[i][int(rng.integers(0, 150))] = 33 + 15
    quals = [bytes(q) for q in quals]
    mates = [_cut(rng, contigs[i % 3][0], 100) for i in range(n)]
    (tmp_path / "r1.fastq.gz").write_bytes(gzip.compress(_fastq(ids, seqs, quals)))
    (tmp_path / "r2.fastq.gz").write_bytes(gzip.compress(_fastq(ids, mates, [b"I" * 100] * n)))
    for name, paths, reads, rq in (("single", [tmp_path / "r1.fastq.gz"], [[s] for s in seqs], [[q] for q in quals]),
                                   ("pairs", [tmp_path / "r1.fastq.gz", tmp_path / "r2.fastq.gz"], [[s, mt] for s, mt in zip(seqs, mates)],
                                    [[q, b"I" * 100] for q in quals])):
        prefix = str(tmp_path / name)
        got = G.bigsig_identify(str(tmp_path / "idx.gsmx"), paths, prefix, down_sample=1, fp_correct=3.0, quality=15, batch=16, ctx=gpu_ctx)
        rnk, rbc, rbh, _ = ref.query(reads, quals=rq, min_phred=15)
        _, racc = ref.classify(rnk, rbc, rbh, 10.0 ** -3.0)
        assert np.array_equal(got["n_kmers"], rnk) and np.array_equal(got["best_hits"], rbh) and np.array_equal(got["accept"], racc)
        assert open(prefix + "_reads.txt", "rb").read() == RM.R.reads_txt(accs, ids, rbc, rbh, rnk, racc)
        assert open(prefix + "_counts.txt", "rb").read() == RM.R.counts_txt(accs, rbc, rbh, racc)
        assert racc.sum() >= 10
    bx.close()
    # the filter through the command's own keyword: every value of these assemblies occurs once
    fx = G.bigsig_construct(tmp_path / "refs.txt", tmp_path / "idx_f", 21, h, B, ctx=gpu_ctx, filter=2)
    assert (tmp_path / "idx_f.gsbx").exists() and fx.info()["minimizer_len"] == 0 and (fx.bits_set() == 0).all() and fx.info()["n_colours"] == 3
    fx.close()


# ---- validation -----------------------------------------------------------------------------------------------------------------------------------
def test_validation_codes(gpu_ctx, tmp_path):
    def code(f):
        with pytest.raises(G.GsError) as e:
            f()
        return e.value.code
    mk = lambda **kw: G.Bigsi(**{**dict(k=21, num_hash=3, bloom_size=4099, capacity=2, ctx=gpu_ctx, minimizer_len=11), **kw})      # noqa: E731
    for m in (21, 22, 100):
        assert code(lambda: mk(minimizer_len=m)) == -1, m
    assert code(lambda: mk(minimizer=1)) == -3 and code(lambda: mk(coverage_filter=1)) == -3
    assert code(lambda: mk(k=33)) == -1 and code(lambda: mk(num_hash=0)) == -1
    # minimizer_len = 0 through the entry point itself (the Python keyword 0 means a plain index)
    from gsearch_amd._lib import BigsiParamsC
    h = C.c_void_p()
    prm = BigsiParamsC(21, 3, 4099, 0, 0, 0)
    assert gpu_ctx.L.gs_bigsi_create_mini(gpu_ctx.h, C.byref(prm), 0, 2, C.byref(h)) == -1
    assert gpu_ctx.L.gs_bigsi_create_mini(gpu_ctx.h, C.byref(prm), 21, 2, C.byref(h)) == -1
    prm.minimizer = 1
    assert gpu_ctx.L.gs_bigsi_create_mini(gpu_ctx.h, C.byref(prm), 11, 2, C.byref(h)) == -3
    (tmp_path / "refs.txt").write_text("")
    assert code(lambda: G.bigsig_construct(tmp_path / "refs.txt", tmp_path / "x", 21, 3, 4099, ctx=gpu_ctx, minimizer=True, value=21)) == -1
    assert code(lambda: G.bigsig_construct(tmp_path / "refs.txt", tmp_path / "x", 21, 3, 4099, ctx=gpu_ctx, minimizer=True)) == -1      # the default value is 21
    bx = mk()
    assert bx.info()["minimizer_len"] == 11 and gpu_ctx.L.gs_bigsi_minimizer_len(bx.h) == 11
    assert code(lambda: bx.query([[b"ACGT" * 10]])) == -4              # no colour yet
    bx.add_genomes([[b"ACGT" * 10]], min_count=2)
    assert code(lambda: bx.query([[b"ACGT" * 10]], down_sample=0)) == -1
    assert code(lambda: bx.add_genomes([[b"A"], [b"C"]], min_count=2)) == -4        # past the capacity
    assert bx.info()["n_colours"] == 1
    bx.close()


# ---- poisoned scratch -----------------------------------------------------------------------------------------------------------------------------
def test_build_filter_and_query_on_poisoned_scratch():
    """as tests/test_gpu_stale_scratch.py does for the plain index: a context of its own, the fill off, then 0x00, 0x01 and 0xFF; every output == the
    reference. The larger shapes come first, so the later ones run in slots larger than they need."""
    rng = np.random.default_rng(77)
    k, m, h, B = 31, 15, 3, 4099
    big = [[_seq(rng, 6000) * 2]]
    genomes = [[_seq(rng, 300)] for _ in range(66)] + [[_seq(rng, 700) * 2]]
    reads = [[_cut(rng, genomes[int(rng.integers(67))][0], 100)] for _ in range(24)] + [[_seq(rng, 100)] for _ in range(8)] + [[genomes[66][0]]]
    refs = {}
    for f in (1, 2):
        ref = RM.Index(k, m, h, B)
        for g in big + genomes:
            ref.add(g, min_count=f)
        refs[f] = (ref.row_words(np.arange(B), 2), np.asarray(ref.t(), np.uint64), np.asarray(ref.nk, np.uint64)) + tuple(ref.query(reads, down_sample=2))
    ctx = G.Context(0)
    try:
        for fill in (None, 0x00, 0x01, 0xFF):
            G.debug_mem_fill(fill)
            for f in (1, 2):
                bx = G.Bigsi(k, h, B, 68, ctx=ctx, minimizer_len=m)
                bx.add_genomes(big, min_count=f)
                bx.add_genomes(genomes, min_count=f)
                t, nk = bx.bits_set(return_kmers=True)
                got = (bx.rows(np.arange(B)), t, nk) + tuple(bx.query(reads, down_sample=2, dense=True))
                bx.close()
                for i, (g, r) in enumerate(zip(got, refs[f])):
                    assert np.array_equal(g, np.asarray(r, g.dtype)), (fill, f, i)
    finally:
        G.debug_mem_fill(None)
        ctx.close()
