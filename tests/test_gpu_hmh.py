"""hypermash on the device: HyperMinHash registers (k_sketch_hmh), cardinality and all-pairs similarity (gs_hmh.hip), the files path and the
end-to-end TSV, against the independent numpy reference of SPEC 7 (tests/pyref_hmh.py)."""
import bz2
import ctypes as C
import gzip
import lzma
import os

import numpy as np
import pytest

import helpers as H
import pyref_hmh as PR

pytestmark = pytest.mark.gpu
KS = [1, 2, 5, 14, 15, 16, 17, 21, 31, 32]


def _genome(rng, k, n):
    """one genome of n bases as records: mixed case, an N run, a short record"""
    s = bytearray(H.dna_ascii(H.rand_dna(rng, n)))
    if n > 50:
        s[n // 3:n // 3 + 7] = b"NNNNNNN"
        s[n // 2:n // 2 + 40] = bytes(s[n // 2:n // 2 + 40]).lower()
        cut = n * 2 // 3
        return [bytes(s[:cut]), bytes(s[cut:]), b"ACGTN"[: max(1, k - 1)]]
    return [bytes(s)]


def _sketch(G, genomes, k):
    return G.HyperMinHashSketch.for_k(k).sketch_genomes(genomes)


@pytest.mark.parametrize("k", KS)
def test_registers_bit_exact(gpu_ctx, k):
    import gsearch_amd as G
    rng = np.random.default_rng(100 + k)
    lens = [0, k - 1, k, k + 1, 1000, 200_000]
    genomes = [_genome(rng, k, n) for n in lens]
    genomes.append([b""])
    sig = _sketch(G, genomes, k)
    assert sig.dtype == np.uint16 and sig.shape == (len(genomes), 16384)
    for i, g in enumerate(genomes):
        assert np.array_equal(sig[i], PR.sketch(g, k)), (k, lens[i] if i < len(lens) else "empty")
    assert not sig[0].any() and not sig[1].any() and not sig[-1].any()
    info = gpu_ctx.last_sketch_info()
    assert info["table_in_lds"] and info["launches"] >= 1


def test_three_mbp_genome_and_mixed_batch(gpu_ctx):
    import gsearch_amd as G
    rng = np.random.default_rng(7)
    for k in (15, 21):
        genomes = [_genome(rng, k, 3_000_000), _genome(rng, k, 10), _genome(rng, k, 50_000), [b"acgtNNacgt" * 3]]
        sig = _sketch(G, genomes, k)
        for i, g in enumerate(genomes):
            assert np.array_equal(sig[i], PR.sketch(g, k)), (k, i)
        card = G.hmh_cardinality(sig)
        assert [int(c) for c in card] == [PR.cardinality(s) for s in sig]


def test_split_genome_equals_max_of_pieces(gpu_ctx):
    """a 1.05 Gbp genome synthesised on the device, sketched whole (split over many workgroups) and as pieces cut with k - 1 bases of overlap"""
    import gsearch_amd as G
    ctx, L, k = gpu_ctx, 1_050_000_000, 21
    prm = G.SeqSketcherParams(k, 16384, "hmh")
    words = (L + 31) // 32
    d_seq = ctx.alloc(words * 8 + 64)
    npieces = 700
    piece = (L + npieces - 1) // npieces
    starts = np.array([max(0, i * piece - (k - 1)) for i in range(npieces)], np.uint64)
    ends = np.array([min(L, (i + 1) * piece) for i in range(npieces)], np.uint64)
    rs = np.concatenate([[0], starts]).astype(np.uint64)
    rl = np.concatenate([[L], ends - starts]).astype(np.uint64)
    d_rs, d_rl, d_go1, d_go2 = ctx.alloc(rs.nbytes), ctx.alloc(rl.nbytes), ctx.alloc(16), ctx.alloc(8 * (npieces + 1))
    d_sig1, d_sig2 = ctx.alloc(2 * 16384), ctx.alloc(2 * 16384 * npieces)
    try:
        G._lib.check(ctx.L.gs_synth_dna_dev(ctx.h, 99, 0, 1, L, d_seq))
        ctx.memset(d_seq + words * 8, 0, 64)
        ctx.upload(d_rs, rs); ctx.upload(d_rl, rl)
        ctx.upload(d_go1, np.array([0, 1], np.uint64)); ctx.upload(d_go2, np.arange(1, npieces + 2, dtype=np.uint64))
        G._lib.check(ctx.L.gs_sketch_batch_dev(ctx.h, C.byref(prm.c), d_seq, words * 8 + 64, d_rs, d_rl, 1, d_go1, 1, d_sig1))
        ctx.sync()
        info = ctx.last_sketch_info()
        whole = ctx.download(d_sig1, (16384,), np.uint16)
        G._lib.check(ctx.L.gs_sketch_batch_dev(ctx.h, C.byref(prm.c), d_seq, words * 8 + 64, d_rs, d_rl, npieces + 1, d_go2, npieces, d_sig2))
        ctx.sync()
        pieces = ctx.download(d_sig2, (npieces, 16384), np.uint16)
        # the first piece checked against the reference as well: a piece is an ordinary genome
        head = ctx.download(d_seq, (piece // 4 + 8,), np.uint8)
    finally:
        for p in (d_seq, d_rs, d_rl, d_go1, d_go2, d_sig1, d_sig2):
            ctx.free(p)
    assert info["workgroups_per_genome"] > 1, info
    assert whole.any() and np.array_equal(whole, pieces.max(axis=0))
    codes = np.stack([(head >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[:piece]
    assert np.array_equal(pieces[0], PR.sketch([H.dna_ascii(codes)], k))


def _random_sketches(rng, n_small, n_big):
    """sketches of the sizes the two branches need: small genomes (cards <= 2^19), 5 Mbp-like ones from the register distribution, an
    empty sketch, a one-k-mer sketch, near copies (C large) and unrelated ones (C < ec)"""
    rows = []
    base_small = PR.sketch([H.dna_ascii(H.rand_dna(rng, 60_000))], 21)
    for i in range(n_small):
        g = H.dna_ascii(H.rand_dna(rng, int(rng.integers(2_000, 120_000))))
        rows.append(PR.sketch([g], 21) if i % 3 else np.maximum(base_small, PR.sketch([g[:5000]], 21)))
    big = PR.sketch([H.dna_ascii(H.rand_dna(rng, 1_500_000))], 21)
    for i in range(n_big):
        g = H.dna_ascii(H.rand_dna(rng, 700_000))
        rows.append(np.maximum(big, PR.sketch([g], 21)) if i % 2 else PR.sketch([g], 21))
    rows.append(np.zeros(16384, np.uint16))
    rows.append(PR.sketch([b"ACGTACGTACGTACGTACGTA"], 21))
    return np.stack(rows)


def test_cardinality_and_similarity(gpu_ctx):
    import gsearch_amd as G
    rng = np.random.default_rng(11)
    S = _random_sketches(rng, 12, 6)
    Q, R = S[::2].copy(), S[1::2].copy()
    Q = np.concatenate([Q, S[-2:]])                      # the empty and one-k-mer sketches on both sides
    cq, cr = G.hmh_cardinality(Q), G.hmh_cardinality(R)
    assert [int(c) for c in cq] == [PR.cardinality(s) for s in Q]
    assert [int(c) for c in cr] == [PR.cardinality(s) for s in R]
    assert int(G.hmh_cardinality(np.zeros((1, 16384), np.uint16))[0]) == 0
    sim = G.hmh_similarity_qxc(Q, R)
    assert sim.shape == (len(Q), len(R))
    branches = set()
    for i in range(len(Q)):
        for j in range(len(R)):
            ref = PR.similarity(Q[i], R[j], int(cq[i]), int(cr[j]))
            C_, _ = PR.counts(Q[i], R[j])
            small = max(int(cq[i]), int(cr[j])) <= PR.SMALL
            tol = 1e-9 if small else 1e-12
            assert abs(sim[i, j] - ref) <= tol, (i, j, sim[i, j], ref)
            branches.add(("small" if small else "closed", C_ == 0, ref == 0.0))
    assert ("small", False, False) in branches and ("closed", False, False) in branches
    assert any(b[1] for b in branches) and any(b[2] and not b[1] for b in branches)        # C == 0, and C < ec


def test_counts_exact_on_uneven_shapes(gpu_ctx):
    """C and N exactly (through the similarity of the closed branch: all sketches large) on Q x R shapes that are not tile multiples"""
    import gsearch_amd as G
    rng = np.random.default_rng(5)
    big = PR.sketch([H.dna_ascii(H.rand_dna(rng, 3_000_000))], 21)
    rows = []
    for i in range(203):
        x = big.copy()
        flip = rng.random(16384) < rng.uniform(0.0, 0.9)
        x[flip] = rng.integers(1 << 10, 12 << 10, int(flip.sum()), dtype=np.uint16)
        if i % 7 == 0:
            x[rng.random(16384) < 0.05] = 0
        rows.append(x)
    S = np.stack(rows)
    Q, R = S[:131], S[131:]
    cq, cr = G.hmh_cardinality(Q), G.hmh_cardinality(R)
    sim = G.hmh_similarity_qxc(Q, R)
    for i in range(0, len(Q), 5):
        for j in range(len(R)):
            assert abs(sim[i, j] - PR.similarity(Q[i], R[j], int(cq[i]), int(cr[j]))) <= 1e-12, (i, j)
    # the _dev forms give the same answers
    ctx = gpu_ctx
    dq, dr, ds, dc = ctx.alloc(Q.nbytes), ctx.alloc(R.nbytes), ctx.alloc(8 * len(Q) * len(R)), ctx.alloc(8 * len(Q))
    try:
        ctx.upload(dq, Q); ctx.upload(dr, R)
        G.hmh_similarity_qxc_dev(ctx, dq, len(Q), dr, len(R), ds)
        G.hmh_cardinality_dev(ctx, dq, len(Q), dc)
        ctx.sync()
        sd, cd = ctx.download(ds, (len(Q), len(R)), np.float64), ctx.download(dc, (len(Q),), np.uint64)
    finally:
        for p in (dq, dr, ds, dc):
            ctx.free(p)
    assert np.array_equal(sd, sim) and np.array_equal(cd, cq)


def _write(path, text):
    if path.endswith(".gz"):
        data = gzip.compress(text)
    elif path.endswith(".bz2"):
        data = bz2.compress(text)
    elif path.endswith(".xz"):
        data = lzma.compress(text)
    else:
        data = text
    with open(path, "wb") as f:
        f.write(data)


def _fasta(recs):
    out = b""
    for i, (name, s) in enumerate(recs):
        out += b">" + name + b"\n" + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n"
    return out


def _fastq(recs, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    out = b""
    for name, s in recs:
        out += b"@" + name + nl + s[: len(s) // 2] + nl + s[len(s) // 2:] + nl + b"+" + nl + b"I" * len(s) + nl
    return out


def test_files_fasta_fastq_all_codecs(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(21)
    k = 21
    paths, expect, nrec = [], [], []
    for fi, suf in enumerate([".fa", ".fa.gz", ".fa.bz2", ".fa.xz", ".fq", ".fq.gz", ".fq.bz2", ".fq.xz"]):
        recs = [(b"r%d capsid protein" % fi, H.dna_ascii(H.rand_dna(rng, 5000 + 100 * fi))),     # kept: hypermash has no capsid filter
                (b"short", H.dna_ascii(H.rand_dna(rng, k))),                                       # len <= k: dropped
                (b"edge", H.dna_ascii(H.rand_dna(rng, k + 1))),                                     # kept
                (b"n_run", b"ACGTNNNNNNNNNNNNNNNNACGTAC" + H.dna_ascii(H.rand_dna(rng, 300)))]
        text = _fasta(recs) if ".fa" in suf else _fastq(recs, crlf=fi % 2 == 1)
        p = str(tmp_path / ("f%d%s" % (fi, suf)))
        _write(p, text)
        paths.append(p)
        kept = [s for _, s in recs if len(s) > k]
        expect.append(PR.sketch(kept, k))
        nrec.append(len(kept))
    sk = G.HyperMinHashSketch.for_k(k)
    sig, nr, nb, st = sk.sketch_files(paths, threads=4)
    for i in range(len(paths)):
        assert np.array_equal(sig[i], expect[i]), paths[i]
    assert list(nr) == nrec
    # the packed path on the same records gives the same sketches
    recs0 = [H.dna_ascii(H.rand_dna(np.random.default_rng(1), 900))]
    assert st["wall_s"] > 0
    p0 = str(tmp_path / "same.fq")
    _write(p0, _fastq([(b"a", recs0[0])]))
    assert np.array_equal(sk.sketch_files([p0])[0][0], sk.sketch_genomes([recs0])[0])
    # zstd is refused
    pz = str(tmp_path / "x.fq.zst")
    _write(pz, b"\x28\xb5\x2f\xfd" + b"\0" * 32)
    with pytest.raises(G.GsError) as e:
        sk.sketch_files([pz])
    assert e.value.code == -3


def test_files_one_large_fastq_gz(gpu_ctx, tmp_path):
    """one file of 64 Mbp of reads (FASTQ.gz): the whole file is one sketch"""
    import gsearch_amd as G
    rng = np.random.default_rng(4)
    k, n_reads, rl = 21, 426_667, 150
    genome = H.dna_ascii(H.rand_dna(rng, 2_000_000))
    starts = rng.integers(0, len(genome) - rl, n_reads)
    qual = b"I" * rl
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, genome[s:s + rl], qual) for i, s in enumerate(starts))
    p = str(tmp_path / "big.fq.gz")
    with open(p, "wb") as f:
        f.write(gzip.compress(text, compresslevel=1))
    sig, nr, nb, _ = G.HyperMinHashSketch.for_k(k).sketch_files([p])
    assert int(nr[0]) == n_reads and int(nb[0]) == n_reads * rl and int(nb[0]) >= 64_000_000
    # the reference over all reads: the k-mers of every read at once (reads x windows), in blocks
    codes = H.rand_dna(np.random.default_rng(4), 2_000_000).astype(np.uint64)      # (the genome above: same generator state)
    assert H.dna_ascii(codes[:1000]) == genome[:1000]
    full = np.zeros(16384, np.uint64)
    nw = rl - k + 1
    for b0 in range(0, n_reads, 40000):
        st = starts[b0:b0 + 40000].astype(np.int64)
        fwd = np.zeros((len(st), nw), np.uint64)
        rc = np.zeros((len(st), nw), np.uint64)
        for t in range(k):
            fwd = (fwd << np.uint64(2)) | codes[st[:, None] + t + np.arange(nw)[None, :]]
            rc = (rc << np.uint64(2)) | (np.uint64(3) - codes[st[:, None] + k - 1 - t + np.arange(nw)[None, :]])
        v = np.minimum(fwd, rc).reshape(-1) & np.uint64((1 << (2 * k)) - 1)
        idx, reg = PR.register_updates(v)
        np.maximum.at(full, idx.astype(np.int64), reg)
    assert np.array_equal(sig[0], full.astype(np.uint16))


def test_hypermash_end_to_end(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(8)
    k = 17
    root = H.dna_ascii(H.rand_dna(rng, 400_000))
    files = {}
    for name, g in (("q1.fa", root), ("q2.fq", H.dna_ascii(H.rand_dna(rng, 30_000))), ("r1.fa.gz", root[:300_000]), ("sub/q1.fa", root[100_000:])):
        p = str(tmp_path / name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        _write(p, _fastq([(b"x", g)]) if ".fq" in name else _fasta([(b"x", g)]))
        files[name] = p
    ql = tmp_path / "q.txt"; rl_ = tmp_path / "r.txt"
    ql.write_text("%s\n\n%s\n" % (files["q1.fa"], files["q2.fq"]))
    rl_.write_text("%s\n%s\n\n" % (files["r1.fa.gz"], files["sub/q1.fa"]))
    qp, rp = G.read_path_list(str(ql)), G.read_path_list(str(rl_))
    out = tmp_path / "out.tsv"
    G.hypermash(qp, rp, k, str(out), threads=2)
    lines = out.read_text().split("\n")
    assert lines[0] == "Query\tReference\tDistance" and lines[-1] == ""
    rows = [x.split("\t") for x in lines[1:-1]]
    assert [(a, b) for a, b, _ in rows] == [(q, r) for q in qp for r in rp]
    sk = {p: PR.sketch([open(p, "rb").read().split(b"\n", 1)[1].split(b"\n+")[0]] if p.endswith(".fq") else
                       [b"".join((gzip.decompress(open(p, "rb").read()) if p.endswith(".gz") else open(p, "rb").read()).split(b"\n")[1:])], k)
          for p in qp + rp}
    for q, r, d in rows:
        ref = 0.0 if os.path.basename(q) == os.path.basename(r) else PR.distance(PR.similarity(sk[q], sk[r]), k)
        assert abs(float(d) - ref) <= 1e-6 + 5e-7, (q, r, d, ref)
    assert float(rows[1][2]) == 0.0                                # q1.fa against sub/q1.fa: same file name
