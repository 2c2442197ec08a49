"""bigsig's tied top hits and six-field report (SPEC.md 11.2) without a device: the writer of the library and the numpy restatement
(tests/pyref_bigsi_ties.py) against the seven sample lines of the reference's README (tests/golden/bigsig_reads_readme.txt), the `,...` marker, the counts
file, the writer's validation codes and the verdict table."""
import os

import numpy as np
import pytest

import gsearch_amd as G
import pyref_bigsi as R
import pyref_bigsi_ties as RT

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
ACC = ["Ecoli_CE98", "Ecoli_224", "Ecoli_tEPEC", "Ecoli_OB20"]                  # colours 0..3
IDS = ["@m84137_250807_202000_s4/%d/ccs" % i for i in (244911914, 244911147, 256971887, 245240131, 245503310, 245765017, 244846078)]
# the seven reads of the README, arrays written out by hand. Read 1 is not significant: its hits, ties and listed colour must not reach the file.
NK = [891, 4226, 762, 1454, 510, 1578, 1786]
BH = [29, 7, 152, 27, 503, 42, 20]
NT = [3, 1, 1, 4, 1, 1, 2]
VD = [RT.TIED, RT.NOT_SIGNIFICANT, RT.UNIQUE, RT.TIED, RT.UNIQUE, RT.UNIQUE, RT.TIED]
LISTS = [[0, 1, 3], [2], [0], [0, 1, 2, 3], [0], [1], [0, 3]]


def _tied(lists, max_ties):
    td = np.full((len(lists), max_ties), NONE, np.uint32)
    for i, l in enumerate(lists):
        td[i, :min(len(l), max_ties)] = l[:max_ties]
    return td


def _files(tmp_path, name, acc, ids, nk, bh, nt, td, vd):
    prefix = str(tmp_path / name)
    G.bigsig_write_report(prefix, acc, ids, nk, bh, nt, td, vd)
    return open(prefix + "_reads.txt", "rb").read(), open(prefix + "_counts.txt", "rb").read()


@pytest.mark.parametrize("max_ties", [4, 16])
def test_the_readme_sample_byte_for_byte(tmp_path, max_ties):
    golden = open(os.path.join(HERE, "golden", "bigsig_reads_readme.txt"), "rb").read()
    assert golden.count(b"\n") == 7 and golden.endswith(b"\n")
    td = _tied(LISTS, max_ties)
    reads, counts = _files(tmp_path, "readme", ACC, IDS, NK, BH, NT, td, VD)
    assert reads == golden
    assert RT.reads_txt(ACC, IDS, NK, BH, NT, td, VD) == golden
    assert counts == b"Ecoli_CE98\t2\nEcoli_224\t1\nreject\t4\nno_hits\t0\ntoo_short\t0\n" == RT.counts_txt(ACC, td, VD)


def test_the_marker_behind_a_cut_list(tmp_path):
    acc = ["g%d" % i for i in range(8)]
    for max_ties, n_tied, want in ((3, 3, b"g0,g1,g2"), (3, 4, b"g0,g1,g2,..."), (1, 2, b"g0,..."), (1, 41, b"g0,..."), (4, 3, b"g0,g1,g2")):
        td = _tied([list(range(min(n_tied, 8)))], max_ties)
        reads, counts = _files(tmp_path, "cut", acc, ["r"], [100], [9], [n_tied], td, [RT.TIED])
        assert reads == b"r\t" + want + b"\t9\t100\treject\t%d\n" % n_tied
        assert reads == RT.reads_txt(acc, ["r"], [100], [9], [n_tied], td, [RT.TIED])
        assert counts == b"reject\t1\nno_hits\t0\ntoo_short\t0\n" == RT.counts_txt(acc, td, [RT.TIED])


def test_counts_file_order_and_trailing_lines(tmp_path):
    """descending count, then accession bytes ("B" < "a" < "b"); unique reads alone are credited; every other verdict lands in its trailing line"""
    acc = ["b", "a", "B", "never"]
    vd = [RT.UNIQUE] * 5 + [RT.TIED, RT.NOT_SIGNIFICANT, RT.NOT_SIGNIFICANT, RT.NO_HITS, RT.TOO_SHORT, RT.TOO_SHORT, RT.TOO_SHORT]
    first = [0, 1, 2, 1, 0, 3, 3, 3, NONE, NONE, NONE, NONE]
    n = len(vd)
    td = _tied([[c, 3][:2 if v == RT.TIED else 1] if c != NONE else [] for c, v in zip(first, vd)], 2)
    nt = [2 if v == RT.TIED else (1 if v in (RT.UNIQUE, RT.NOT_SIGNIFICANT) else 0) for v in vd]
    nk = [0 if v == RT.TOO_SHORT else 50 for v in vd]
    bh = [0 if v in (RT.TOO_SHORT, RT.NO_HITS) else 5 for v in vd]
    ids = ["r%d" % i for i in range(n)]
    reads, counts = _files(tmp_path, "cnt", acc, ids, nk, bh, nt, td, vd)
    assert counts == b"a\t2\nb\t2\nB\t1\nreject\t3\nno_hits\t1\ntoo_short\t3\n" == RT.counts_txt(acc, td, vd)
    assert reads == RT.reads_txt(acc, ids, nk, bh, nt, td, vd)
    lines = reads.split(b"\n")
    assert lines[8] == b"r8\tno_hits\t0\t50\taccept\t0" and lines[9] == b"r9\ttoo_short\t0\t0\taccept\t0"
    assert lines[6] == b"r6\tno_significant_hits\t0\t50\treject\t0" and lines[5] == b"r5\tnever,never\t5\t50\treject\t2"
    # no read at all
    reads, counts = _files(tmp_path, "none", acc, [], [], [], [], np.zeros((0, 2), np.uint32), [])
    assert reads == b"" and counts == b"reject\t0\nno_hits\t0\ntoo_short\t0\n"


def test_writer_validation_codes(tmp_path):
    def code(nt, td, vd, acc=ACC):
        with pytest.raises(G.GsError) as e:
            G.bigsig_write_report(str(tmp_path / "bad"), acc, ["r"], [10], [3], nt, np.asarray(td, np.uint32), vd)
        return e.value.code
    assert code([1], [[4]], [RT.UNIQUE]) == -1                        # a listed colour past the accessions
    assert code([2], [[0, 4]], [RT.TIED]) == -1
    assert code([3], [[0, NONE]], [RT.TIED]) == -1                    # a listed slot left unused
    assert code([1], [[0]], [5]) == -1                                # no such verdict
    assert code([0], [[0]], [RT.UNIQUE]) == -1 and code([0], [[0]], [RT.TIED]) == -1
    assert code([1], np.zeros((1, 0)), [RT.UNIQUE]) == -1             # max_ties 0
    assert code([1], np.zeros((1, 1025)), [RT.UNIQUE]) == -1          # max_ties past 1024
    assert not os.path.exists(str(tmp_path / "bad_reads.txt"))        # refused before anything is written
    # slots behind the list, and every slot of a read that names no colour, are not looked at
    G.bigsig_write_report(str(tmp_path / "ok"), ACC, ["r", "s"], [10, 10], [3, 3], [1, 7], np.array([[0, 99], [99, 99]], np.uint32), [RT.UNIQUE, RT.NOT_SIGNIFICANT])
    assert open(str(tmp_path / "ok_reads.txt"), "rb").read() == b"r\tEcoli_CE98\t3\t10\taccept\t1\ns\tno_significant_hits\t0\t10\treject\t0\n"
    with pytest.raises(G.GsError) as e:
        G.bigsig_write_report(str(tmp_path / "no_such_dir" / "x"), ACC, ["r"], [10], [3], [1], np.array([[0]], np.uint32), [RT.UNIQUE])
    assert e.value.code == -5


def test_verdict_table():
    """each of the five rows, in the order of the table; a tail equal to the threshold is not significant"""
    B, h, n, x0, t_c = 1 << 20, 3, 130, 2, 58000
    tail = R.tail(t_c, B, h, n, x0)
    assert 0.0 < tail < 1e-3 and G.bigsi_tail(t_c, B, h, n, x0) == tail
    below = float(np.nextafter(tail, 0.0))
    cases = [((0, 0, 0, 1.0, 1e-3), RT.TOO_SHORT), ((0, 5, 2, 0.0, 1e-3), RT.TOO_SHORT),          # n = 0 comes first
             ((n, 0, 0, 1.0, 1e-3), RT.NO_HITS), ((n, 0, 3, 0.0, 1e-3), RT.NO_HITS),
             ((n, x0, 1, tail, tail), RT.NOT_SIGNIFICANT), ((n, x0, 2, tail, below), RT.NOT_SIGNIFICANT), ((n, x0, 1, 1.0, 1.0), RT.NOT_SIGNIFICANT),
             ((n, x0, 1, float("nan"), 1e-3), RT.NOT_SIGNIFICANT),
             ((n, x0, 1, below, tail), RT.UNIQUE), ((n, x0, 1, tail, 1e-3), RT.UNIQUE), ((n, x0, 1, 0.0, 1e-300), RT.UNIQUE),
             ((n, x0, 2, below, tail), RT.TIED), ((n, x0, 4097, tail, 1e-3), RT.TIED)]
    for args, want in cases:
        assert G.bigsi_verdict_code(*args) == want == RT.verdict_code(*args), args
    assert {w for _, w in cases} == set(range(5))
    assert G.BIGSI_VERDICTS == ("too_short", "no_hits", "no_significant_hits", "unique", "tied")
    assert [G.BIGSI_VERDICTS[v] for v in (RT.TOO_SHORT, RT.NO_HITS, RT.NOT_SIGNIFICANT)] == [RT.STATUS[v] for v in (RT.TOO_SHORT, RT.NO_HITS, RT.NOT_SIGNIFICANT)]


def test_ties_of_the_restatement():
    """the restatement on hits written out by hand: the list is ascending and cut, n_tied is not, sig_colour looks past the cut"""
    t = np.array([50, 40, 40, 30, 60], np.uint64)
    bh, nt, td, sig = RT.ties_of(np.array([3, 7, 7, 7, 2], np.uint32), t, 2)
    assert (bh, nt, td.tolist(), sig) == (7, 3, [1, 2], 3)
    bh, nt, td, sig = RT.ties_of(np.array([3, 7, 7, 1, 2], np.uint32), t, 4)
    assert (bh, nt, td.tolist(), sig) == (7, 2, [1, 2, NONE, NONE], 1)                  # equal t_c: the smaller colour
    bh, nt, td, sig = RT.ties_of(np.zeros(5, np.uint32), t, 3)                          # no hit: no tie
    assert (bh, nt, td.tolist(), sig) == (0, 0, [NONE] * 3, NONE)
