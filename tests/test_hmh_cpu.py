"""hypermash on the host side: the hmh parameter rules, known answers of the independent reference (tests/pyref_hmh.py), the FASTQ scanner,
the list-file reader and the TSV writer. Nothing here launches a kernel; without a GPU the compute calls must refuse."""
import io
import os

import numpy as np
import pytest

import pyref_hmh as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hypermash")


def test_hmh_parameter_rules():
    import gsearch_amd as G
    P = G.SeqSketcherParams
    for k in (1, 14, 15, 16, 17, 21, 32):
        assert P(k, 16384, "hmh").sig_dtype() == np.uint16
    with pytest.raises(G.GsError) as e:
        P(15, 16384, "optdens")                                     # still refused for gsearch's sketchers
    assert e.value.code == -1
    for args in ((21, 16000, "hmh"), (21, 32768, "hmh"), (5, 16384, "hmh", "aa"), (21, 16384, "hmh", "dna_fwd"), (33, 16384, "hmh"), (0, 16384, "hmh")):
        with pytest.raises(G.GsError) as e:
            P(*args)
        assert e.value.code == -1, args
    assert G.ALGO["hmh"] == 6


def test_register_update_known_answers():
    # value 0 (the k-mer AAA...A): fx64(0) = 0, h1 = the first SplitMix64 output from state 0 = 0xE220A8397B1DCDAF: index = its top 14 bits
    # (0x3888 = 14472); the 50 bits below start 0b0010... -> two leading zeros, lz = 3; register = 3 << 10 | (h2 & 0x3FF) = 3072 + 500
    assert PR.register_update_scalar(0) == (14472, 3572)
    assert PR.register_update_scalar(0x1B) == (8778, 2227)
    assert PR.register_update_scalar((1 << 64) - 1) == (13793, 5682)
    # the vectorised path agrees with the scalar one, and every register holds lz in [1, 51]
    rng = np.random.default_rng(3)
    v = rng.integers(0, 2 ** 63, 5000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 5000, dtype=np.uint64)
    idx, reg = PR.register_updates(v)
    for i in range(0, 5000, 97):
        assert (int(idx[i]), int(reg[i])) == PR.register_update_scalar(int(v[i]))
    lz = reg >> np.uint64(10)
    assert lz.min() >= 1 and lz.max() <= 51 and idx.max() < 16384


def test_canonical_kmers_and_empty_sketch():
    assert PR.cardinality(np.zeros(16384, np.uint16)) == 0
    # GAT = 0b100011 = 35 and its reverse complement ATC = 0b001101 = 13 -> 13; N is dropped before windowing, lower case folded
    assert list(PR.canonical_kmers(b"GAT", 3)) == [13]
    assert list(PR.canonical_kmers(b"gNaT", 3)) == [13]
    assert list(PR.canonical_kmers(b"GA", 3)) == []
    s = PR.sketch([b"ACGTACGTTGCA"], 5)
    assert s.dtype == np.uint16 and (s != 0).sum() <= 8
    assert 1 <= PR.cardinality(s) <= 40


def _parse_fastq(text):
    """plain-Python FASTQ parse: (id, sequence without line breaks) per record"""
    lines = [x[:-1] if x.endswith(b"\r") else x for x in text.split(b"\n")]
    out, i = [], 0
    while i < len(lines):
        if not lines[i]:
            i += 1
            continue
        assert lines[i].startswith(b"@")
        rid = lines[i][1:].split()[0].decode()
        i += 1
        seq = b""
        while not lines[i].startswith(b"+"):
            seq += lines[i]
            i += 1
        i += 1
        q = 0
        while q < len(seq):
            q += len(lines[i])
            i += 1
        out.append((rid, seq))
    return out


def test_fastq_scan_matches_a_plain_parse():
    import gsearch_amd as G
    txt = (b"@r1 first read\nACGT\nAC\n+\nIIII\nII\n"
           b"@r2\r\nGGGNNN\r\n+r2\r\n@@@@@@\r\n"                            # CRLF, a '+' line repeating the header, quality that starts with '@'
           b"\n@r3 empty\n\n+\n\n"                                        # a blank line between records, an empty record
           b"@r4\nTTTT\n+\n+III")                                         # quality starting with '+', no final newline
    recs = G.fastq_scan(txt)
    ref = _parse_fastq(txt)
    assert [r[0] for r in recs] == [x[0] for x in ref] == ["r1", "r2", "r3", "r4"]
    for (_, b, e), (_, seq) in zip(recs, ref):
        assert txt[b:e].replace(b"\r", b"").replace(b"\n", b"") == seq
    for bad in (b"@r1\nACGT\n+\nIII", b"@r1\nACGT\n", b"@r1\nACGT\n+\nIIIII\n", b"r1\nACGT\n+\nIIII\n", b"@r1"):
        with pytest.raises(G.GsError) as e:
            G.fastq_scan(bad)
        assert e.value.code == -5, bad
    assert G.fastq_scan(b"") == [] and G.fastq_scan(b"\n\n") == []


def test_path_list_and_tsv_writer_match_the_fixture():
    import gsearch_amd as G
    q = G.read_path_list(os.path.join(GOLD, "query_list.txt"))
    r = G.read_path_list(os.path.join(GOLD, "ref_list.txt"))
    assert q == ["data/q1.fna", "data/sub/shared.fq.gz"] and r == ["ref/r1.fa", "ref/shared.fq.gz"]
    dist = np.array([[0.1234567, 1.0], [0.0000004, 0.77]])
    out = io.StringIO()
    G.write_hypermash_tsv(q, r, dist, out)
    assert out.getvalue() == open(os.path.join(GOLD, "expected.tsv")).read()


def test_distance_helper():
    import gsearch_amd as G
    for s in (0.0, 0.01, 0.5, 0.999, 1.0):
        for k in (15, 21, 32):
            assert abs(G.hypermash_distance(s, k) - PR.distance(s, k)) < 1e-15


def test_hmh_compute_refuses_without_a_gpu():
    """no CPU fallback: without a device the new compute calls refuse; with one this test is skipped"""
    import gsearch_amd as G
    try:
        ctx = G.Context(0)
    except G.GsError as e:
        assert e.code == -2
        with pytest.raises(G.GsError):
            G.hmh_cardinality(np.zeros((1, 16384), np.uint16))
        with pytest.raises(G.GsError):
            G.hmh_similarity_qxc(np.zeros((1, 16384), np.uint16), np.zeros((1, 16384), np.uint16))
        with pytest.raises(G.GsError):
            G.HyperMinHashSketch.for_k(21)
        return
    ctx.close()
    pytest.skip("a GPU is present")
