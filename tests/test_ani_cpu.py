"""superani (SPEC 12) without a GPU: the numpy restatement (tests/pyref_ani.py) against a hand-worked chaining example, its invariants on planted
pairs, the accuracy of the method against the planted truth, and the writer and the host closed form of the library against the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import pyref_ani as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superani")
N = PR.NONE
# (rpos, qpos, qcontig, strand), every anchor on r contig 0. Worked by hand with W = 20, B = 64, G = 2500:
HAND = [(100, 100, 0, 0),      # 0  nothing in front                                         f = 20
        (200, 200, 0, 0),      # 1  from 0: 20 + 20 - 0                                      f = 40
        (300, 310, 0, 0),      # 2  from 1: 40 + 20 - 10 (from 0: 30)                        f = 50
        (400, 50, 0, 0),       # 3  q runs backwards against every anchor in front           f = 20
        (450, 460, 0, 0),      # 4  from 2: 50 + 20 - 0 (from 1: 50, from 3: 40 - 360)       f = 70
        (450, 900, 0, 0),      # 5  dr = 0 against 4 (a repeated r seed), the others < W     f = 20
        (3100, 3100, 0, 0),    # 6  dr = 2650 > G against 4 and 5                            f = 20
        (3200, 5000, 0, 1),    # 7  first anchor of strand 1                                 f = 20
        (3300, 4900, 0, 1),    # 8  strand 1, dq = 5000 - 4900: from 7                       f = 40
        (3400, 3400, 0, 0),    # 9  from 6: dr = dq = 300                                    f = 40
        (3400, 4800, 0, 1),    # 10 from 8: 40 + 20 (from 7: 40)                             f = 60
        (3500, 100, 1, 0),     # 11 first anchor on q contig 1                               f = 20
        (3600, 220, 1, 0),     # 12 from 11: 20 + 20 - 20 = W, not strictly greater          f = 20
        (3700, 1000, 2, 0),    # 13 first anchor on q contig 2                               f = 20
        (3720, 1040, 2, 0),    # 14 from 13: 20 + 20 - 20 = W, not taken                     f = 20
        (3800, 1110, 2, 0)]    # 15 from 13: 40 - 10, from 14: 40 - 10: the larger j wins    f = 30
HAND_F = [20, 40, 50, 20, 70, 20, 20, 20, 40, 40, 60, 20, 20, 20, 20, 30]
HAND_PRED = [N, 0, 1, N, 2, N, N, N, 7, 6, 8, N, N, N, N, 14]
HAND_ROOT = [0, 0, 0, 3, 0, 5, 6, 7, 7, 6, 7, 11, 12, 13, 14, 14]


def hand_anchors():
    a = np.array(HAND, np.int64)
    return {"rcontig": np.zeros(len(a), np.int64), "rpos": a[:, 0], "qcontig": a[:, 2], "qpos": a[:, 1], "strand": a[:, 3]}


def test_hand_worked_chaining():
    f, pred, root = PR.chain(hand_anchors())
    assert f.tolist() == HAND_F
    assert pred.tolist() == HAND_PRED
    assert root.tolist() == HAND_ROOT
    # root 0 ends at 4 (f = 70): 4 anchors; root 7 ends at 10: 3 anchors; roots 6 and 14 have 2 anchors and are dropped, the others 1
    assert PR.kept_chains(f, pred, root) == [[4, 2, 1, 0], [10, 8, 7]]


def test_seed_rule_literals():
    """k = 8: the window ACGTACGT is its own reverse complement (fwd = 1), AAAAAAAC has the forward value 1 < its reverse complement"""
    s = PR.seeds([b"ACGTACGT", b"aaaNaaaac", b"ACG"], 8, 1)
    assert s.tolist() == [[0x1B1B, 0, 0, 1], [1, 1, 0, 1]]
    s = PR.seeds([b"GTTTTTTT"], 8, 1)                     # reverse complement AAAAAAAC = 1 is the smaller: fwd = 0
    assert s.tolist() == [[1, 0, 0, 0]]
    assert int(PR.mix(np.array([0], np.uint64))[0]) == 0 and int(PR.mix(np.array([1], np.uint64))[0]) == 0x5692161D100B05E5


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(12)
    base = PR.random_genome(rng, 200_000)
    return rng, base, PR.seeds([base])


def test_identical_genomes(planted):
    _, base, s = planted
    c = PR.pair_counts(s, s)
    assert c[2] == c[3] and c[5] == c[6] and c[2:5] == c[5:8]
    ani, afq, afr = PR.estimate(c, len(base), len(base))
    assert ani == 1 and afq == afr and afq > 0.99
    assert c[4] <= len(base)


def test_reverse_complemented_contig_gives_the_same_integers(planted):
    _, base, _ = planted
    cut = 120_000
    two = PR.seeds([base[:cut], base[cut:]])
    flipped = PR.seeds([base[:cut], PR.revcomp(base[cut:])])
    same = PR.pair_counts(two, two)
    assert PR.pair_counts(two, flipped) == same
    assert PR.pair_counts(flipped, two) == same


@pytest.mark.parametrize("p", [0.01, 0.05, 0.10])
def test_accuracy_against_the_planted_truth(planted, p):
    """|ani - (1 - p)| <= 6 sigma, sigma = the binomial error of the matched share carried through the k-th root"""
    rng, base, s = planted
    k = 16
    mut = PR.substitute(np.random.default_rng(int(p * 1000)), base, p)
    ms = PR.seeds([mut[:90_000], mut[90_000:]])
    c = PR.pair_counts(ms, s)
    mq, cq, aq = c[2], c[3], c[4]
    assert mq <= cq and aq <= len(mut) and c[7] <= len(base)
    ani = float(PR.estimate(c, len(mut), len(base))[0])
    f = mq / cq
    sigma = ani * np.sqrt(f * (1 - f) / cq) / (k * f)
    print("p = %g: ani = %.5f, truth %.5f, deviation %.2f sigma (sigma = %.2e), C_q = %d, chains = %d" % (p, ani, 1 - p, (ani - (1 - p)) / sigma, sigma, cq, c[1]))
    assert abs(ani - (1 - p)) <= 6 * sigma


def test_unrelated_genomes(planted):
    _, base, s = planted
    other = PR.seeds([PR.random_genome(np.random.default_rng(99), 100_000)])
    c = PR.pair_counts(other, s)
    assert c[1] == 0 and c[2:] == [0] * 6
    assert [float(x) for x in PR.estimate(c, 100_000, len(base))] == [0, 0, 0]


EST = [[(0.0, 0.0, 0.0), (1.0, 1.0, 0.5)], [(np.float32(0.1), np.float32(0.95), np.float32(0.999)), (np.float32(0.9473), np.float32(1e-7), 0.25)]]


def test_writer_against_the_literal_fixture(tmp_path):
    """0, 1, values whose f32 shortest form differs from the f64 form of the same number (f32 0.1 is 0.10000000149011612 as an f64), a small
    value that must not turn into an exponent; reference-major order"""
    import gsearch_amd as G
    want = open(os.path.join(GOLD, "writer_expected.tsv"), "rb").read()
    q, r = ["q1.fa", "q2.fa"], ["r1.fa", "r2 b.fa"]
    assert repr(float(np.float32(0.1))) != "0.1"
    assert PR.superani_text(q, r, EST) == want
    G.write_superani(tmp_path / "o.tsv", q, r, np.array(EST, np.float32))
    assert open(tmp_path / "o.tsv", "rb").read() == want


def test_fmt_f32_round_trips():
    rng = np.random.default_rng(5)
    import gsearch_amd.api as A
    for x in np.concatenate([rng.random(300), 10.0 ** rng.integers(-9, 3, 50) * rng.random(50)]).astype(np.float32):
        s = PR.fmt_f32(x)
        assert "e" not in s and np.float32(float(s)) == x and s == A._rust_f32(x)


def test_estimate_of_the_library_equals_the_restatement():
    import gsearch_amd as G
    rng = np.random.default_rng(3)
    rows = [[10, 1, 0, 0, 0, 0, 0, 0], [5, 1, 7, 7, 500, 7, 7, 400], [9, 2, 3, 10, 99, 3, 11, 2000], [9, 2, 3, 10, 90, 3, 11, 90]]
    for _ in range(40):
        c = int(rng.integers(1, 5000))
        rows.append([0, 1, int(rng.integers(0, c + 1)), c, int(rng.integers(0, 3000)), 0, c, int(rng.integers(0, 3000))])
    bq = [0, 1000, 1000, 1000] + [int(x) for x in rng.integers(1, 6000, 40)]
    br = [0, 1000, 1000, 1000] + [int(x) for x in rng.integers(1, 6000, 40)]
    for k in (11, 16):
        got = G.ani_estimate(np.array(rows, np.uint64), bq, br, k)
        L = G.load()
        assert L.gs_ani_estimate(None, None, None, 1, k, None) == -1
        for i, row in enumerate(rows):
            want = PR.estimate(row, bq[i], br[i], k)
            assert got[i].tolist() == [float(x) for x in want], (k, row)
    assert float(G.ani_estimate([rows[3]], 1000, 1000)[0, 0]) == 0.0          # both aligned fractions below 0.10
