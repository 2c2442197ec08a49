"""superaai on the device: FracMinHash sketches (k_frac_hash, k_frac_seg_sort and the radix path), all-pairs similarity (k_frac_pairs), the
files path and the end-to-end text, against the independent numpy reference of SPEC 9 (tests/pyref_aai.py)."""
import bz2
import gzip
import lzma
import os

import numpy as np
import pytest

import pyref_aai as PR

pytestmark = pytest.mark.gpu
KS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32]
CASES = [(100, 5120), (0, 64), (1, 5120), (100, 0), (7, 1), (0, 0)]
AA = b"ACDEFGHIKLMNPQRSTVWY"


def _protein(rng, n, alphabet=AA):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])


def _genome(rng, k, n):
    """records of a proteome: mixed case, '*' and 'X', CRLF and LF line breaks, records shorter than k, a repeated stretch"""
    s = bytearray(_protein(rng, n))
    if n > 100:
        s[n // 4:n // 4 + 30] = bytes(s[n // 4:n // 4 + 30]).lower()
        s[n // 3] = ord("*")
        s[n // 3 + 5] = ord("X")
        s[n // 2:n // 2 + 60] = s[10:70]                          # repeats: deduplication
    cut = len(s) * 2 // 3
    a = bytes(s[:cut])
    a = b"\r\n".join(a[i:i + 61] for i in range(0, len(a), 61))
    b = b"\n".join(bytes(s[cut:])[i:i + 50] for i in range(0, len(s) - cut, 50))
    return [a, b, AA[: max(0, k - 1)], b"MK*"]


def _check(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint64 and np.array_equal(g, w), "genome %d: %d vs %d values" % (i, len(g), len(w))


@pytest.mark.parametrize("k", KS)
def test_sketch_bit_exact_every_k(gpu_ctx, k):
    import gsearch_amd as G
    rng = np.random.default_rng(300 + k)
    genomes = [_genome(rng, k, n) for n in (0, k, 500, 40_000, 300_000)] + [[]] + [[b""]]
    for scaled, num in CASES:
        got = G.FracMinHashSketch(k, scaled, num).sketch_genomes(genomes)
        _check(got, [PR.sketch(g, k, scaled, num) for g in genomes])


def test_sketch_large_proteome_split_and_mixed_batch(gpu_ctx):
    """a 12 M-residue proteome (thousands of workgroups) beside small ones, defaults and scaled = 1 (every hash survives the filter)"""
    import gsearch_amd as G
    rng = np.random.default_rng(12)
    big = [_protein(rng, 3_000_000) for _ in range(4)]
    genomes = [big, [_protein(rng, 5000)], [b"MKVL"], [_protein(rng, 200_000), _protein(rng, 7)]]
    for scaled, num in [(100, 5120), (1, 5120), (1, 0), (0, 100)]:
        got = G.FracMinHashSketch(7, scaled, num).sketch_genomes(genomes)
        _check(got, [PR.sketch(g, 7, scaled, num) for g in genomes])


def _sim_check(G, Q, R, num):
    sim, com, uni = G.frac_similarity_qxc(Q, R, num, return_counts=True)
    for i, a in enumerate(Q):
        for j, b in enumerate(R):
            c, u = PR.similarity_counts(a, b, num)
            assert com[i, j] == c and uni[i, j] == u, (i, j)
            assert sim[i, j] == float(c) / float(max(1, u))


def _family(rng, n, size, num, share):
    base = np.unique(rng.integers(0, 2 ** 64, size * 2, dtype=np.uint64))
    out = []
    for _ in range(n):
        m = int(rng.integers(0, size + 1))
        keep = base[rng.random(len(base)) < share]
        own = rng.integers(0, 2 ** 64, m, dtype=np.uint64)
        s = np.unique(np.concatenate([keep, own]))
        out.append(s[: min(len(s), int(rng.integers(0, num + 1)))] if num else s)
    return out


@pytest.mark.parametrize("nq,nr", [(1, 1), (3, 257), (130, 70)])
def test_similarity_counts_exact(gpu_ctx, nq, nr):
    import gsearch_amd as G
    rng = np.random.default_rng(nq * 1000 + nr)
    num = 64
    Q = _family(rng, nq, 80, num, 0.4)
    R = _family(rng, nr, 80, num, 0.4)
    Q[0] = np.zeros(0, np.uint64)
    if nq > 2:
        Q[1] = R[0].copy()                                           # identical sketches
        Q[2] = R[min(2, nr - 1)][:num].copy()
    _sim_check(G, Q, R, num)


def test_similarity_long_sketches(gpu_ctx):
    """num = 0 sketches longer than any LDS tile, and num = 5120 at the defaults' lengths"""
    import gsearch_amd as G
    rng = np.random.default_rng(77)
    Q = _family(rng, 5, 12_000, 0, 0.5) + [np.zeros(0, np.uint64)]
    R = _family(rng, 9, 12_000, 0, 0.5)
    Q[0] = np.unique(np.concatenate([Q[0], rng.integers(0, 2 ** 64, 20_000, dtype=np.uint64)]))   # > 8192: searched in global memory
    _sim_check(G, Q, R, 0)
    Q2 = [x[:5120] for x in Q] + [np.sort(rng.choice(R[0], min(len(R[0]), 3000), replace=False))]
    R2 = [x[:5120] for x in R]
    _sim_check(G, Q2, R2, 5120)
    _sim_check(G, Q2, R2, 100)


def _write(path, text):
    data = gzip.compress(text) if path.endswith(".gz") else bz2.compress(text) if path.endswith(".bz2") else lzma.compress(text) if path.endswith(".xz") else text
    with open(path, "wb") as f:
        f.write(data)


def _fasta(recs, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    return b"".join(b">" + name + nl + nl.join(s[j:j + 60] for j in range(0, len(s), 60)) + nl for name, s in recs)


def _fastq(recs, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    return b"".join(b"@" + name + nl + s[: len(s) // 2] + nl + s[len(s) // 2:] + nl + b"+" + nl + b"I" * len(s) + nl for name, s in recs)


def test_files_fasta_fastq_all_codecs(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(31)
    k, scaled, num = 7, 10, 500
    paths, expect = [], []
    for fi, suf in enumerate([".faa", ".faa.gz", ".faa.bz2", ".faa.xz", ".fq", ".fq.gz", ".fq.bz2", ".fq.xz"]):
        recs = [(b"p%d capsid protein" % fi, _protein(rng, 3000 + 100 * fi)), (b"short", b"MKV"), (b"odd", b"mkvXX*ab" + _protein(rng, 50)),
                (b"empty", b"")]
        if ".fq" in suf:
            recs = recs[:3]
        text = _fastq(recs, crlf=fi % 2 == 1) if ".fq" in suf else _fasta(recs, crlf=fi % 2 == 1)
        p = str(tmp_path / ("f%d%s" % (fi, suf)))
        _write(p, text)
        paths.append(p)
        expect.append(PR.sketch([s for _, s in recs], k, scaled, num))
    sk = G.FracMinHashSketch(k, scaled, num)
    got, nrec, nb, st = sk.sketch_files(paths, threads=4, return_stats=True)
    _check(got, expect)
    assert st["wall_s"] > 0
    pz = str(tmp_path / "x.faa.zst")
    _write(pz, b"\x28\xb5\x2f\xfd" + b"\0" * 32)
    with pytest.raises(G.GsError) as e:
        sk.sketch_files([pz])
    assert e.value.code == -3


def test_superaai_end_to_end(gpu_ctx, tmp_path):
    import gsearch_amd as G
    rng = np.random.default_rng(5)
    base = [_protein(rng, 20_000) for _ in range(3)]
    files = []
    for i in range(5):
        s = bytearray(base[i % 3])
        pos = rng.integers(0, len(s), 200 * (i + 1))
        for p in pos:
            s[p] = AA[int(rng.integers(0, 20))]
        p = str(tmp_path / ("g%d.faa%s" % (i, ".gz" if i % 2 else "")))
        _write(p, _fasta([(b"a", bytes(s[:9000])), (b"b", bytes(s[9000:]))]))
        files.append(p)
    ql, rl = tmp_path / "q.txt", tmp_path / "r.txt"
    ql.write_text("\n".join([files[0], files[1], files[0]]) + "\n")
    rl.write_bytes(("\r\n".join(files[2:] + [files[0]])).encode())
    out = tmp_path / "out.txt"
    k, scaled, num = 7, 20, 400
    sim = G.superaai(str(ql), str(rl), str(out), k=k, scaled=scaled, sketch=num, threads=2)
    qp, rp = PR.read_list(ql.read_bytes()), PR.read_list(rl.read_bytes())
    sk = {}
    for p in set(qp + rp):
        data = gzip.decompress(open(p, "rb").read()) if p.endswith(".gz") else open(p, "rb").read()
        recs = [r.split(b"\n", 1)[1] for r in data.split(b">")[1:]]
        sk[p] = PR.sketch(recs, k, scaled, num)
    want = [[PR.similarity(sk[q], sk[r], num) for r in rp] for q in qp]
    assert np.array_equal(sim, np.array(want))
    assert out.read_bytes() == PR.output_text(qp, rp, want, k).encode()
    assert sim[0, 3] == 1.0 and 0 < sim[1, 2] < 1                    # the same file; two members of one family
