"""SPEC.md 8.1 without a device: the numpy restatement tests/pyref_embed_quality.py against its own two definitions, a case worked by hand, the
identity behind "conserved", and what the measure is for: it tells an embedding that keeps the neighbourhoods from one that does not. The library's
part that needs no device (the report text, the exported names) is held to the same literal."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import embed_quality_cases as K
import pyref_embed_quality as R


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_the_two_definitions_agree(case):
    ids, dist, cnt, pos, kq = K.make(case)
    assert not R.refusals(ids, dist, cnt, pos, kq)
    a, b = R.arrays_sort(ids, cnt, pos, kq), R.arrays_count(ids, cnt, pos, kq)
    for x, y, name in zip(a, b, ("rank", "e2", "rad2")):
        assert x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), name
    n, knbn = ids.shape
    used = np.arange(knbn)[None, :] < cnt[:, None].astype(np.int64)
    assert (a[0][~used] == R.UNUSED).all() and (_bits(a[1])[~used] == 0).all() and (a[0][used] < n - 1).all()


def test_the_case_table_covers_what_it_promises():
    ns, dims, knbns, kinds = ({c[i] for c in K.CASES} for i in (1, 2, 4, 5))
    assert {2, 3, 4097} | {t + d for t in (K.TILE_Q, K.TILE_P) for d in (-1, 0, 1)} <= ns
    assert dims == {1, 2, 3, 4} and knbns == {1, 8, 17} and kinds == set(K.KINDS)
    kq = {("n-1" if c[3] == c[1] - 1 else "n+5" if c[3] == c[1] + 5 else "knbn" if c[3] == c[4] else c[3]) for c in K.CASES}
    assert {1, 2, 200, "n-1", "n+5", "knbn"} <= kq
    assert len(K.KNOB_CASES) >= 3
    for case in K.CASES:
        ids, dist, cnt, pos, _ = K.make(case)
        if case[1] <= 3:
            continue
        assert cnt[0] == 0 and (cnt < min(case[4], case[1] - 1)).any() and (cnt == min(case[4], case[1] - 1)).any()
        d2 = R.d2_rows(pos, np.arange(64))
        if case[5] == "clumps":
            assert np.isinf(d2).any()
        if case[5] == "tiny":
            assert ((d2 > 0) & (d2 < np.finfo(np.float32).tiny)).any()
        if case[5] == "negzero":
            assert (np.signbit(pos) & (pos == 0)).any()


def test_conserved_is_within_the_radius_on_a_lattice():
    """an 8 x 8 integer lattice: every row has ties at its radius, and rank < kq_eff is the same as e2 <= rad2"""
    n = 64
    pos = K.positions("lattice", n, 2, 0)
    assert len(np.unique(pos, axis=0)) == n
    for kq in (1, 2, 4, 9, 20):             # (at 3 or 8 a corner's radius is a diagonal neighbour that has no twin)
        ids, dist, cnt = K.graph(n, 17, kq)
        rank, e2, rad2 = R.arrays_sort(ids, cnt, pos, kq)
        D = R.d2_rows(pos, np.arange(n))
        np.fill_diagonal(D, np.inf)
        assert ((D == rad2[:, None]).sum(axis=1) >= 2).all()                      # ties at the radius, in every row
        used = np.arange(17)[None, :] < cnt[:, None].astype(np.int64)
        assert np.array_equal((rank < kq)[used], (e2 <= rad2[:, None])[used])
        assert (rank < kq)[used].any() and not (rank < kq)[used].all()


HAND_TEXT = ("embedding quality of 5 nodes, knbn 2: 4 rows with neighbours, 7 edges, kq 2\n"
             "neighbourhoods without a match: 1\n"
             "neighbours conserved per matched row: mean 1.33333\n"
             "edges conserved: 4, fraction 0.571429\n"
             "embedded edge length quantiles: 0.01:2 0.05:2 0.25:2 0.5:12 0.75:15 0.95:15 0.99:15\n"
             "embedded radius quantiles: 0.01:2 0.05:2 0.25:2 0.5:3 0.75:3 0.95:3 0.99:3\n"
             "edge / radius quantiles: 0.01:1 0.05:1 0.25:1 0.5:1.25 0.75:4 0.95:4 0.99:4\n")


def hand_case():
    """five points on a line at 0, 1, 3, 7, 15; kq = 2. Squared distances: 0: 1 9 49 225; 1: 1 4 36 196; 2: 9 4 16 144; 3: 49 36 16 64;
    4: 225 196 144 64, so rad2 = 9, 4, 9, 36, 144. Rows: 0 -> (1, 4): e2 1, 225, ranks 0, 3; 1 -> (0, 2): e2 1, 4, ranks 0, 1; 2 -> (4): e2 144, rank 3;
    3 -> nothing; 4 -> (3, 0): e2 64, 225, ranks 0, 3."""
    X = K.U64MAX
    ids = np.array([[1, 4], [0, 2], [4, X], [X, X], [3, 0]], np.uint64)
    dist = np.array([[.1, .2], [.1, .2], [.3, np.inf], [np.inf, np.inf], [.25, .5]], np.float32)
    cnt = np.array([2, 2, 1, 0, 2], np.uint32)
    pos = np.array([[0], [1], [3], [7], [15]], np.float32)
    U = 0xFFFFFFFF
    want = dict(rank=[[0, 3], [0, 1], [3, U], [U, U], [0, 3]], e2=[[1, 225], [1, 4], [144, 0], [0, 0], [64, 225]], rad2=[9, 4, 9, 36, 144],
                n=5, knbn=2, kq_eff=2, n_rows=4, n_edges=7, n_conserved=4, n_nomatch=1, mean_conserved=4 / 3, frac_conserved=4 / 7, hist_conserved=[1, 2, 1],
                q_edge=[2, 2, 2, 12, 15, 15, 15], q_radius=[2, 2, 2, 3, 3, 3, 3], q_ratio=[1, 1, 1, 1.25, 4, 4, 4])
    return ids, dist, cnt, pos, 2, want


def check_hand(s, want):
    for key, v in want.items():
        got = s[key]
        assert (np.array_equal(np.asarray(got, np.float64), np.asarray(v, np.float64)) if np.ndim(v) else got == v), (key, got, v)


def test_summary_and_report_of_a_case_worked_by_hand():
    import gsearch_amd as G
    ids, dist, cnt, pos, kq, want = hand_case()
    for arrays in (R.arrays_sort, R.arrays_count):
        s = R.quality(ids, dist, cnt, pos, kq, arrays)
        check_hand(s, want)
        assert R.text(s) == HAND_TEXT
        assert G.embed_quality_text(s) == HAND_TEXT                 # the library's writer, which needs no device
    empty = R.summary(np.zeros(3, np.uint32), np.full((3, 2), R.UNUSED), np.zeros((3, 2), np.float32), np.ones(3, np.float32), 2)
    assert empty["n_rows"] == 0 and empty["mean_conserved"] == 0.0 and np.isnan(empty["frac_conserved"]) and np.isnan(empty["q_ratio"]).all()
    assert "fraction nan" in G.embed_quality_text(empty)
    # the special quotients: 0/0 = 1, x/0 = inf, inf/inf = 1, x/inf = 0
    s = R.summary(np.ones(4, np.uint32), np.zeros((4, 1), np.uint32), np.array([[0], [2], [np.inf], [3]], np.float32),
                  np.array([0, 0, np.inf, np.inf], np.float32), 1)
    assert s["q_ratio"][[0, 3, 6]].tolist() == [0.0, 1.0, 1.0]          # sorted 0, 1, 1, +inf: the elements 0, 1 and 2
    assert R._quantiles([np.inf, 1.0, np.inf]).tolist() == [1.0, 1.0, 1.0, np.inf, np.inf, np.inf, np.inf]      # +inf sorts last


def test_refusals_of_the_restatement():
    ids, dist, cnt, pos, kq, _ = hand_case()
    assert R.refusals(ids, dist, cnt, pos, 0) == ["kq"] and R.refusals(ids[:1], dist[:1], cnt[:1] * 0, pos[:1], 2) == ["n"]
    assert R.refusals(ids, dist, cnt, np.zeros((5, 0), np.float32), 2) == ["dim"] and R.refusals(ids, dist, cnt, np.zeros((5, 5), np.float32), 2) == ["dim"]
    for v in (np.nan, np.inf, -np.inf):
        p = pos.copy()
        p[3, 0] = v
        assert R.refusals(ids, dist, cnt, p, 2) == ["coordinate"]
    i2 = ids.copy()
    i2[0, 1] = 0
    assert R.refusals(i2, dist, cnt, pos, 2)


def test_the_measure_tells_a_good_embedding_from_a_random_one(capsys):
    """40 families x 25 nodes, every row 8 random members of its family, kq = 24. Planted positions (family centre uniform in [-10, 10]^2 plus
    N(0, 0.05)) conserve nearly everything; uniform random positions conserve what chance gives, kq / (n - 1) = 0.0240 (the standard deviation of
    8000 such edges is 0.0017). Measured on this restatement, numpy seed 1: 0.999875 (7999 of 8000 edges) with no row without a match, and 0.0215."""
    rng = np.random.default_rng(1)
    nf, per, knbn, kq = 40, 25, 8, 24
    n = nf * per
    fam = np.repeat(np.arange(nf), per)
    ids = np.zeros((n, knbn), np.uint64)
    for i in range(n):
        members = np.flatnonzero((fam == fam[i]) & (np.arange(n) != i))
        ids[i] = rng.choice(members, knbn, replace=False)
    dist = np.tile(np.linspace(0.1, 0.5, knbn, dtype=np.float32), (n, 1))
    cnt = np.full(n, knbn, np.uint32)
    centre = rng.uniform(-10, 10, (nf, 2))
    planted = (centre[fam] + rng.normal(0, 0.05, (n, 2))).astype(np.float32)
    random = rng.uniform(-10, 10, (n, 2)).astype(np.float32)
    good, bad = R.quality(ids, dist, cnt, planted, kq), R.quality(ids, dist, cnt, random, kq)
    with capsys.disabled():
        print("\nplanted: frac_conserved %.5f, n_nomatch %d; random: frac_conserved %.4f (chance %.4f)"
              % (good["frac_conserved"], good["n_nomatch"], bad["frac_conserved"], kq / (n - 1)))
    assert good["frac_conserved"] >= 0.99
    assert bad["frac_conserved"] <= 1.5 * kq / (n - 1)


def test_the_package_exports_the_feature():
    import gsearch_amd as G
    from gsearch_amd import _lib
    for name in ("gs_embed_quality", "gs_embed_quality_dev", "gs_index_embed_quality", "gs_embed_quality_last_ms"):
        assert name in G.SYMBOLS
    for name in ("embed_quality", "embed_quality_dev", "embed_quality_text", "embed_quality_last_ms"):
        assert callable(getattr(G, name))
    assert callable(G.Hnsw.embed_quality)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsearch_amd.h")).read()
    assert int(re.search(r"#define GS_EMBQ_TILE_Q (\d+)u", hdr).group(1)) == G.EMBQ_TILE_Q == K.TILE_Q
    assert int(re.search(r"#define GS_EMBQ_TILE_P (\d+)u", hdr).group(1)) == G.EMBQ_TILE_P == K.TILE_P
    assert int(re.search(r"#define GS_EMBQ_TIMES (\d+)u", hdr).group(1)) == _lib.EMBQ_TIMES
    # the summary structure as the header lays it out: five u64, two u32, two doubles, three rows of seven doubles
    assert C.sizeof(_lib.EmbedQualityC) == 5 * 8 + 2 * 4 + 2 * 8 + 3 * 7 * 8
    assert inspect.signature(G.ann).parameters["quality"].default is None
