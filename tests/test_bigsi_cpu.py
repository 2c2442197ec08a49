"""bigsig (SPEC.md 11) without a device: the host arithmetic of the library - row positions, segmenting, the tail, the report files - against Python
big integers, exact fractions, the numpy restatement (tests/pyref_bigsi.py) and a hand-written fixture (tests/golden/bigsig)."""
import json
import os
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import gsearch_amd as G
import pyref_bigsi as R

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = (1 << 64) - 1


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _positions_bigint(v, h, B):
    x = (v * 0x517CC1B727220A95) & M64
    h1, st = _mix((x + 0x9E3779B97F4A7C15) & M64), _mix((x + 2 * 0x9E3779B97F4A7C15) & M64) | 1
    return [(((h1 + i * st) & M64) * B) >> 64 for i in range(h)]


@pytest.mark.parametrize("v", [0, M64, 0x0123456789ABCDEF, 1])
@pytest.mark.parametrize("B", [1, 64, 4099, 1 << 20, (1 << 40) - 1])
def test_position_known_answers(v, B):
    """k = 1 with value 0 (v = 0), the all-ones value of k = 32, B = 1 and the largest B, against Python big-integer arithmetic"""
    want = _positions_bigint(v, 16, B)
    assert [int(x) for x in G.bigsi_positions(v, 16, B)] == want
    assert [int(x) for x in R.positions(np.array([v], np.uint64), 16, B)[0]] == want
    assert all(p < B for p in want)
    if B == 1:
        assert want == [0] * 16


def test_kmer_values_of_the_edge_cases():
    assert R.kmers([b"A"], 1).tolist() == [0] and R.kmers([b"T"], 1).tolist() == [0]          # canonical: T = rc(A)
    assert R.kmers([b"T" * 32], 32, fwd_only=True).tolist() == [M64]
    assert R.kmers([b"T" * 32], 32).tolist() == [0]


def test_position_parameters_are_checked():
    for args in ((0, 0, 10), (0, 17, 10), (0, 3, 0), (0, 3, 1 << 40)):
        with pytest.raises(G.GsError) as e:
            G.bigsi_positions(*args)
        assert e.value.code == -1


SEG_CASES = [
    (b"NACGTACGTN", None),                       # an N at each end
    (b"ACGTNNNNNACGTAC", None),                  # a run of N
    (b"acgtACgtnACGT", None),                    # lower case
    (b"ACGT\nACGT\r\nAC-GT", None),              # line breaks end nothing, any other byte does
    (b"", None), (b"NNNN", None), (b"A", None),
    (b"ACGTACGTAC", b"IIII0/IIII"),              # '0' = 15: exactly at the threshold, kept; '/' = 14: one below, ends the segment
    (b"ACGTACGTAC", b"//////////"),
    (b"ACGNACGTAC", b"IIIIIII!II"),
]


@pytest.mark.parametrize("text,qual", SEG_CASES)
def test_segmenting(text, qual):
    want = [(b, len(c)) for b, c in R.segments(text, qual, 15)]
    assert G.bigsi_split(text, qual, 15, 1) == want
    assert G.bigsi_split(text, qual, 15, 4) == [s for s in want if s[1] >= 4]
    if qual == b"IIII0/IIII":
        assert want == [(0, 5), (6, 4)]
    if text == b"NACGTACGTN":
        assert want == [(1, 8)]


TAIL_B = 10 ** 9
TAIL_GRID = [(n, x0, t) for n in (1, 2, 31, 150, 300) for x0 in sorted({1, n // 2, n}) for t in (1, 10 ** 6, 3 * 10 ** 8)]
TAIL_MEASURED = 5.7e-14        # the largest relative error over the grid, measured on the CPU (SPEC 11)


def test_tail_against_the_exact_binomial_tail():
    """p = t / 10^9 in {1e-9, 1e-3, 0.3} with num_hash = 1. The bound is 16 x the measured error and never above 1e-9. Where the exact tail lies below half
    the smallest positive f64 (2^-1075: n >= 150 with x0 >= n / 2 at the two small p) a relative error is not defined - the correctly rounded
    answer is 0 - and the library must return exactly 0."""
    bound = min(16 * TAIL_MEASURED, 1e-9)
    worst = 0.0
    for n, x0, t in TAIL_GRID:
        p = Fraction(t, TAIL_B)
        exact = sum(comb(n, x) * p ** x * (1 - p) ** (n - x) for x in range(x0, n + 1))
        lib = G.bigsi_tail(t, TAIL_B, 1, n, x0)
        assert lib == R.tail(t, TAIL_B, 1, n, x0), (n, x0, t)
        if exact < Fraction(1, 2 ** 1075):
            assert lib == 0.0, (n, x0, t, lib)
            continue
        assert exact >= Fraction(1, 2 ** 1022)          # no case of the grid is subnormal
        err = float(abs(Fraction(lib) - exact) / exact)
        worst = max(worst, err)
        print("tail n=%d x0=%d p=%g lib=%.17g rel.err=%.3g" % (n, x0, t / TAIL_B, lib, err))
        assert err <= bound, (n, x0, t, lib, err)
    print("largest relative error %.3g" % worst)


def test_tail_special_cases():
    assert G.bigsi_tail(5, 100, 3, 150, 0) == 1.0                       # no hit
    assert G.bigsi_tail(0, 100, 3, 150, 7) == 0.0                       # an empty genome
    assert G.bigsi_tail(100, 100, 3, 150, 7) == 1.0                     # a full column
    assert G.bigsi_tail(1, (1 << 40) - 1, 16, 150, 1) == R.tail(1, (1 << 40) - 1, 16, 150, 1)
    for h in (1, 3, 16):
        for n, x0 in ((150, 150), (150, 3), (70000, 70000), (70000, 12)):
            assert G.bigsi_tail(123456, 1 << 20, h, n, x0) == R.tail(123456, 1 << 20, h, n, x0)


def test_report_files_match_the_fixture(tmp_path):
    case = json.load(open(os.path.join(HERE, "golden", "bigsig", "case.json")))
    prefix = str(tmp_path / "out")
    G.bigsig_write_reads(prefix, case["accessions"], case["read_ids"], case["best_colour"], case["best_hits"], case["n_kmers"], case["accept"])
    reads, counts = open(prefix + "_reads.txt", "rb").read(), open(prefix + "_counts.txt", "rb").read()
    assert reads == open(os.path.join(HERE, "golden", "bigsig", "expected_reads.txt"), "rb").read()
    assert counts == open(os.path.join(HERE, "golden", "bigsig", "expected_counts.txt"), "rb").read()
    # the restatement writes the same bytes
    assert reads == R.reads_txt(case["accessions"], case["read_ids"], case["best_colour"], case["best_hits"], case["n_kmers"], case["accept"])
    assert counts == R.counts_txt(case["accessions"], case["best_colour"], case["best_hits"], case["accept"])


def test_reference_list(tmp_path):
    p = tmp_path / "refs.txt"
    p.write_text("GCF_1\t/data/a.fna.gz\nGCF_2\t/data/b.fna\n\n")
    assert G.read_ref_list(p) == [("GCF_1", "/data/a.fna.gz"), ("GCF_2", "/data/b.fna")]
    p.write_text("GCF_1\t/data/a.fna.gz\nGCF_1\t/data/b.fna\n")
    with pytest.raises(G.GsError) as e:
        G.read_ref_list(p)
    assert e.value.code == -1


def test_parameter_validation_needs_no_device():
    L = G.load()
    from gsearch_amd._lib import BigsiParamsC
    import ctypes as C

    def rc(k=31, h=3, B=1 << 20, data_t=0, mini=0, cov=0):
        return L.gs_bigsi_check_params(C.byref(BigsiParamsC(k, h, B, data_t, mini, cov)))
    assert rc() == 0 and rc(k=15) == 0 and rc(k=1) == 0 and rc(k=32, h=16, B=(1 << 40) - 1, data_t=2) == 0
    for kw in (dict(k=0), dict(k=33), dict(h=0), dict(h=17), dict(B=0), dict(B=1 << 40), dict(data_t=1)):
        assert rc(**kw) == -1, kw
    assert rc(mini=1) == -3 and rc(cov=1) == -3
