"""The case table of tests/ani_pair_cases.py against itself: every edge it is there for is present - asserted by counting, so that a later edit cannot
drop one unnoticed -, the rows of eight integers worked out by hand from SPEC 12 are what tests/pyref_ani.py gives, and on the small cases its anchors and
its per-side counts equal a plain double loop and a per-seed walk written here. No GPU."""
import numpy as np
import pytest

import ani_pair_cases as AC
import pyref_ani as PR

N_CU = 256          # for the assertion on many_segments only; the GPU test takes the device's own number
BIG = [n for n in AC.RANDOM_SIZES if n >= 2047]


def test_constants_are_the_restatements():
    assert (AC.W, AC.B, AC.G, AC.MAX_OCC, AC.MIN_ANCHORS) == (PR.W, PR.B, PR.G, PR.MAX_OCC, PR.MIN_ANCHORS)


class Stages:
    """every stage of the restatement for one pair"""

    def __init__(self, qs, rs):
        self.qs, self.rs = qs, rs
        self.a = PR.anchors(qs, rs)
        self.f, self.pred, self.root = PR.chain(self.a)
        self.chains = PR.kept_chains(self.f, self.pred, self.root)
        self.row = [len(self.f), len(self.chains), *PR.side(qs, self.a["qidx"], self.chains, AC.K), *PR.side(rs, self.a["ridx"], self.chains, AC.K)]

    def reach(self):
        """the largest i - pred[i]"""
        has = self.pred != PR.NONE
        return int((np.arange(len(self.pred))[has] - self.pred[has]).max()) if has.any() else 0

    def heads(self):
        """segment heads as SPEC 12 cuts them: the first anchor, another r contig, an r step above G"""
        rc, rp = self.a["rcontig"], self.a["rpos"]
        h = np.ones(len(rp), bool)
        h[1:] = (rc[1:] != rc[:-1]) | (rp[1:] - rp[:-1] > AC.G)
        return h

    def intervals(self, side):
        idx = self.a["qidx" if side == "q" else "ridx"]
        return sorted((int(idx[p].min()), int(idx[p].max())) for p in self.chains)

    def covered(self, side):
        n = len(self.qs if side == "q" else self.rs)
        cov = np.zeros(n, bool)
        for lo, hi in self.intervals(side):
            cov[lo:hi + 1] = True
        return cov


@pytest.fixture(scope="module")
def st():
    return {name: Stages(q, r) for name, (q, r) in AC.all_cases().items()}


def test_the_table_stays_small(st):
    assert sum(s.row[0] for s in st.values()) < 150_000


def test_both_lists_of_every_case_are_in_order(st):
    for name, s in st.items():
        for side in (s.qs, s.rs):
            assert side.dtype == np.uint32 and side.ndim == 2 and side.shape[1] == 4 and AC.in_order(side), name
            assert set(np.unique(side[:, 3]).tolist()) <= {0, 1}, name


def test_rows_worked_out_by_hand(st):
    for name, row in AC.LITERAL.items():
        assert st[name].row == row, name
    for name, n in AC.LITERAL_CHAINS.items():
        assert st[name].row[1] == n, name
    assert st["braid(33,5)"].row[2] == st["braid(33,5)"].row[3] == 165
    assert st["fork"].row[3] != 4 and st["fork_mirror"].row[3] != 4          # what the wrong end of the tie would give


# ---- the loop yardstick ----------------------------------------------------------------------------------------------------------------------------
def loop_anchors(qs, rs):
    """SPEC 12 word for word: by r seed index, then q seed index, no anchor from a value that more than MAX_OCC seeds of either side carry"""
    q, r = qs.tolist(), rs.tolist()
    occ_q, occ_r = {}, {}
    for v, _, _, _ in q:
        occ_q[v] = occ_q.get(v, 0) + 1
    for v, _, _, _ in r:
        occ_r[v] = occ_r.get(v, 0) + 1
    out = []
    for i, (v, rc, rp, rf) in enumerate(r):
        if occ_r[v] > 4 or occ_q.get(v, 0) > 4:
            continue
        for j, (w, qc, qp, qf) in enumerate(q):
            if w == v:
                out.append((rc, rp, qc, qp, rf ^ qf, i, j))
    return out


def loop_side(sd, idx, chains, k):
    """M, C, A by walking the seeds"""
    sd = sd.tolist()
    n = len(sd)
    cov, mat = [False] * n, [False] * n
    for path in chains:
        on = [int(idx[a]) for a in path]
        for i in on:
            mat[i] = True
        for i in range(min(on), max(on) + 1):
            cov[i] = True
    M = C = A = 0
    i = 0
    while i < n:
        if not cov[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and cov[j + 1] and sd[j + 1][1] == sd[j][1]:
            j += 1
        A += sd[j][2] - sd[i][2] + k
        C += j - i + 1
        M += sum(1 for x in range(i, j + 1) if mat[x])
        i = j + 1
    return M, C, A


def test_small_cases_equal_the_loops(st):
    small = [name for name, s in st.items() if len(s.qs) * len(s.rs) <= 70_000]
    assert len(small) >= 35 and {"occ_grid", "occ_grid_tandem", "fork", "fork_mirror", "braid(64,4)", "side_n(129)", "side_intervals_q", "range_values_occ5",
                                 "random(65)"} <= set(small)
    for name in small:
        s = st[name]
        want = loop_anchors(s.qs, s.rs)
        got = list(zip(*(s.a[x].tolist() for x in ("rcontig", "rpos", "qcontig", "qpos", "strand", "ridx", "qidx"))))
        assert got == want, name
        assert loop_side(s.qs, s.a["qidx"], s.chains, AC.K) == tuple(s.row[2:5]), name
        assert loop_side(s.rs, s.a["ridx"], s.chains, AC.K) == tuple(s.row[5:8]), name


def test_anchors_asked_for_are_the_anchors_found():
    for L in (AC.band(63), AC.braid(64, 4), AC.many_segments(30), AC.singles(10), AC.range_diagonals(), AC.range_step(AC.G), AC.side_intervals(True)):
        a = PR.anchors(*L.done())
        got = list(zip(*(a[x].tolist() for x in ("rcontig", "rpos", "qcontig", "qpos", "strand"))))
        assert got == AC.wanted_in_order(L)


# ---- the edges, counted ----------------------------------------------------------------------------------------------------------------------------
def _occ(side):
    v, c = np.unique(side[:, 0], return_counts=True)
    return dict(zip(v.tolist(), c.tolist()))


def test_occ_grid_has_every_cell(st):
    for name, per_cell in (("occ_grid", 1), ("occ_grid_tandem", 3)):
        s = st[name]
        oq, orr = _occ(s.qs), _occ(s.rs)
        assert set(oq) == set(orr)
        cells = {}
        for v in oq:
            cells[(oq[v], orr[v])] = cells.get((oq[v], orr[v]), 0) + 1
        assert cells == {(a, b): per_cell for a in range(1, 6) for b in range(1, 6)}, name
        assert s.row[0] == per_cell * sum(a * b for a in range(1, 5) for b in range(1, 5)) == per_cell * 100
    assert st["occ_grid"].row[1] == 0 and st["occ_grid"].reach() == 0
    t = st["occ_grid_tandem"]
    assert t.row[1] >= 25 and t.row[2] < t.row[0]                              # the copies chain, and not every anchor lies on a kept chain
    # a wrong order of the anchors of one r seed changes the program: some anchor's predecessor is an anchor of the r seed just in front, not the last of them
    ridx, has = t.a["ridx"], t.pred != PR.NONE
    i = np.arange(len(ridx))[has]
    p = t.pred[has]
    assert ((ridx[p + 1] == ridx[p]) & (p + 1 < i)).any()


def test_random_lists_hold_the_occ_edges_and_enough_chains(st):
    for n in BIG:
        s = st["random(%d)" % n]
        oq, orr = _occ(s.qs), _occ(s.rs)
        common = set(oq) & set(orr)
        for side, other in ((oq, orr), (orr, oq)):
            assert sum(1 for v in common if side[v] == 4 and other[v] <= 4) >= 3, n    # kept at the edge
            assert sum(1 for v in common if side[v] == 5) >= 5, n                      # dropped at the edge
            assert sum(1 for v in common if side[v] >= 5) >= 20, n
        assert sum(1 for v in common if max(oq[v], orr[v]) == 4) >= 5 and sum(1 for v in common if max(oq[v], orr[v]) >= 5) > 30, n
        assert {2, 3, 4, 5, 6} <= set(oq.values()) | set(orr.values()), n
        assert 1000 <= s.row[0] <= 5000 and s.row[1] >= 20, (n, s.row)
        has = s.pred != PR.NONE
        assert int((s.a["strand"][has] == 1).sum()) >= 100, n
        assert s.row[2] < s.row[3] and s.row[5] < s.row[6], n
        for side in (s.qs, s.rs):
            assert {0, 0xFFFFFFFF} <= set(side[:, 0].tolist()), n
            assert len(np.unique(side[:, 1])) == 3, n
    assert [len(st["random(%d)" % n].rs) for n in AC.RANDOM_SIZES] == list(AC.RANDOM_SIZES)


def test_band_and_braid_reach_exactly_the_band(st):
    assert st["band(62)"].reach() == 63 and st["band(63)"].reach() == 64 and st["band(64)"].reach() == 1
    assert int(st["band(63)"].pred[65]) == 1 and int(st["band(64)"].pred[66]) == PR.NONE
    for name, reach in (("braid(33,5)", 33), ("braid(63,4)", 63), ("braid(64,4)", 64), ("braid(64,3)", 64), ("braid(64,2)", 64), ("braid(65,4)", 0)):
        s = st[name]
        has = s.pred != PR.NONE
        assert s.reach() == reach, name
        assert reach == 0 or (np.arange(len(s.pred))[has] - s.pred[has] == reach).all(), name       # every predecessor is exactly D back
        assert len(s.heads().nonzero()[0]) == 1, name                                             # one segment
    s = st["braid(64,4)"]
    assert sorted(len(p) for p in s.chains) == [4] * 64 and sorted(p[0] % 64 for p in s.chains) == list(range(64))      # an end in every slot of the ring
    assert sorted(len(p) for p in st["braid(64,3)"].chains) == [3] * 64                      # exactly MIN_ANCHORS
    assert (np.bincount(st["braid(64,2)"].root) == 2).all()                                   # exactly MIN_ANCHORS - 1
    assert set(s.a["strand"].tolist()) == {0, 1}


def test_fork_ties_are_real(st):
    for name, chunks in (("fork", False), ("fork_mirror", True)):
        s = st[name]
        r0 = s.root == 0
        top = np.flatnonzero(r0 & (s.f == s.f[r0].max()))
        assert len(top) == 2, name
        assert s.chains[0][0] == top[0] and len(s.chains) == 1, name
        assert (top[0] // 64 != top[1] // 64) == chunks, name
        assert s.heads().sum() == 1, name
        assert (s.pred[top] != PR.NONE).all() and (s.pred[s.pred[top]] != PR.NONE).all()       # either end would be kept


def test_many_segments_and_tiles(st):
    s = st["many_segments"]
    h = s.heads()
    assert int(h.sum()) == AC.N_RUNS > 32 * N_CU and bool(h[AC.AN_TILE])
    assert np.array_equal(np.diff(np.flatnonzero(h))[:6], [1, 3, 2, 1, 3, 2])
    assert sorted(set(len(p) for p in s.chains)) == [3] and int((s.pred != PR.NONE).sum()) == 3 * (AC.N_RUNS // 3)
    beyond = [p for p in s.chains if np.searchsorted(np.flatnonzero(h), p[0], "right") - 1 >= 32 * N_CU]
    assert len(beyond) >= 200                                                                  # chains in segments of the second trip
    d = st["long_diagonal"]
    h = d.heads()
    assert len(h) >= 3 * AC.AN_TILE and int(h.sum()) == 1 and not h[AC.AN_TILE:2 * AC.AN_TILE].any()
    assert len(d.chains) == 1 and len(d.chains[0]) == len(h)
    for n in (AC.AN_TILE, AC.AN_TILE + 1, 2 * AC.AN_TILE):
        x = st["singles(%d)" % n]
        assert x.row[0] == n and x.heads().all() and x.reach() == 0
        assert len(np.unique(x.a["rcontig"])) == 2


def test_slice_edges(st):
    E = AC.AN_SLICE
    for n in (2047, 2048, 2049, 4097):
        d, o = st["slice_diag(%d)" % n], st["slice_occ4(%d)" % n]
        assert len(d.rs) == len(o.rs) == n
        on = set(d.a["ridx"].tolist())
        assert on == set(range(2040, min(2056, n))) | (set(range(4090, 4096)) if n > 4096 else set())
        per_r = np.bincount(o.a["ridx"], minlength=n)
        assert set(np.flatnonzero(per_r).tolist()) == {i for i in (2046, 2047, 2048, 2049, 4094, 4095, 4096) if i < n} and set(per_r[per_r > 0].tolist()) == {4}
        assert d.row[2] < d.row[3]                                                              # a covered q seed that no anchor touches
    for n in (2049, 4097):
        for s in (st["slice_diag(%d)" % n], st["slice_occ4(%d)" % n]):
            assert any(s.a["ridx"][p].min() < E <= s.a["ridx"][p].max() for p in s.chains)      # a chain across the slice edge
    assert max(st["slice_diag(2049)"].a["ridx"]) == 2048 and max(st["slice_diag(2048)"].a["ridx"]) == 2047
    s = st["slice_diag(4097)"]
    assert int(s.a["ridx"].max()) == 2 * E - 1 < len(s.rs) - 1                                  # an r seed, a whole slice, behind the last anchor-bearing one
    assert int(st["slice_occ4(4097)"].a["ridx"].max()) == 4096 and int(st["slice_diag(2047)"].a["ridx"].max()) == 2046


def test_side_edges(st):
    for n in AC.SIDE_NS:
        s = st["side_n(%d)" % n]
        assert len(s.qs) == len(s.rs) == n
        if n >= 3:
            for side in "qr":
                cov = s.covered(side)
                assert cov.all() and cov[n - 1] and s.intervals(side) == [(0, n - 1)]              # the run reaches the last seed
            assert s.row[2] == 3 < s.row[3] == n
    for name, nq, nr in (("side_n(0,5)", 0, 5), ("side_n(5,0)", 5, 0), ("side_n(1,5)", 1, 5), ("side_n(5,1)", 5, 1)):
        assert (len(st[name].qs), len(st[name].rs)) == (nq, nr) and st[name].row[0] == min(nq, nr)
    for at in (64, 65):
        s = st["side_contig_change(%d)" % at]
        for side, sd in (("q", s.qs), ("r", s.rs)):
            cov = s.covered(side)
            assert cov[at - 1] and cov[at] and sd[at - 1, 1] == 0 and sd[at, 1] == 1            # the change lies inside a covered stretch
            assert (at - 1, at) in [(a[1], b[0]) for a, b in zip(s.intervals(side), s.intervals(side)[1:])]
        assert s.row[4] == 2 * (12 * 20 + AC.K)                                                 # two runs, cut at the change
    for name, side, other in (("side_intervals_q", "q", "r"), ("side_intervals_r", "r", "q")):
        s = st[name]
        iv = s.intervals(side)
        assert iv == [(10, 50), (21, 29), (49, 57), (58, 66)], name                             # nested, overlapping, adjacent (hi + 1 = lo)
        o = s.intervals(other)
        assert all(a[1] + 1 < b[0] for a, b in zip(o, o[1:])), name                             # apart on the other side
        cov = s.covered(side)
        assert int(cov.sum()) == 57 == s.row[3 if side == "q" else 6] and s.row[2] == 12
        assert len(s.qs) == len(s.rs) == 130


def test_range_edges(st):
    for name in ("range_values", "range_values_occ5"):
        s = st[name]
        for sd in (s.qs, s.rs):
            assert {0, 0xFFFFFFFF} <= set(sd[:, 0].tolist())
    s = st["range_values"]
    assert s.row[0] == 4 and s.row[1] == 1 and _occ(s.qs)[0] == _occ(s.rs)[0xFFFFFFFF] == 1
    s = st["range_values_occ5"]
    assert _occ(s.qs)[0] == 5 and _occ(s.rs)[0] == 1 and _occ(s.rs)[0xFFFFFFFF] == 5 and _occ(s.qs)[0xFFFFFFFF] == 1 and s.row[0] == 2
    s = st["range_diagonals"]
    assert sorted(len(p) for p in s.chains) == [4, 5]
    assert s.a["rpos"].min() >= 0xFFFFF000 and (s.a["qpos"] < 1 << 31).any() and (s.a["qpos"] >= 1 << 31).any() and s.a["qpos"].max() == 0xFFFFFFF5
    assert set(s.a["strand"].tolist()) == {0, 1}
    for name, kept in (("range_step(G)", 1), ("range_step(G+1)", 0)):
        s = st[name]
        assert s.row[1] == kept and s.a["rpos"].min() > 0xFFFF0000 and s.a["qpos"].min() < 1 << 31 < s.a["qpos"].max()
        assert set(np.diff(s.a["rpos"]).tolist()) == {AC.G + 1 - kept}
