"""Case table of the superani pair stages (gsearch_amd/csrc/gs_ani.hip: k_ani_anchors, k_ani_seg_*, k_ani_chain, k_ani_ends, k_ani_mark, k_ani_sides and
the block loop of ani_pairs_impl) as constructed seed lists, numpy only: no library call, no GPU. ani_pairs takes plain (n, 4) uint32 seed arrays
{value, contig, pos, fwd}, so every state of SPEC 12 is built directly from the anchors it should give instead of from a genome that happens to give it.
tests/test_ani_pair_cases_cpu.py holds the table to its own names (every edge is counted), tests/test_gpu_ani_pairs.py runs it on the device.

The edges are the kernels' own: GS_ANI_MAX_OCC = 4 on either side, the band of B = 64 anchors and the 64-bit marking ring, chains of MIN_ANCHORS - 1 and
MIN_ANCHORS anchors, equal best ends of one root, more segments than the 32 * n_cu wavefronts of a launch, the tile of 4096 anchors, the slice of 2048
r seeds, sides around one and two chunks of 64 seeds, values 0 and 0xFFFFFFFF, positions at and above 2^31."""
import numpy as np

W, B, G, MAX_OCC, MIN_ANCHORS = 20, 64, 2500, 4, 3          # SPEC 12
AN_TILE, AN_SLICE = 4096, 2048                               # gs_ani.hip
K = 16


class Lists:
    """the two seed lists of a pair in the making. anchor() gives an r seed and a q seed one fresh value (flags fwd_r = 1, fwd_q = 1 ^ strand); seeds that share
    a value with others are added with r_seed() / q_seed() under a value from value(); fill_*() adds a seed whose value exists on that side alone.
    done() orders both lists by (contig, pos) - SPEC 12 requires it - and refuses two seeds of a side at one place."""

    def __init__(self):
        self.q, self.r, self.wanted = [], [], []
        self._next, self._fq, self._fr = 1, 0x80000000, 0x40000000

    def value(self):
        self._next += 1
        return self._next - 1

    def r_seed(self, contig, pos, value, fwd=1):
        self.r.append((contig, pos, value, fwd))

    def q_seed(self, contig, pos, value, fwd=1):
        self.q.append((contig, pos, value, fwd))

    def anchor(self, rcontig, rpos, qcontig, qpos, strand=0):
        v = self.value()
        self.r_seed(rcontig, rpos, v, 1)
        self.q_seed(qcontig, qpos, v, 1 ^ strand)
        self.wanted.append((rcontig, rpos, qcontig, qpos, strand))

    def fill_r(self, contig, pos):
        self._fr += 1
        self.r_seed(contig, pos, self._fr, self._fr & 1)

    def fill_q(self, contig, pos):
        self._fq += 1
        self.q_seed(contig, pos, self._fq, self._fq & 1)

    @staticmethod
    def _array(seeds):
        a = np.array(seeds, np.int64).reshape(-1, 4)
        a = a[np.lexsort((a[:, 1], a[:, 0]))]
        assert ((a >= 0) & (a <= 0xFFFFFFFF)).all()
        same = (a[1:, 0] == a[:-1, 0]) & (a[1:, 1] == a[:-1, 1])
        assert not same.any(), "two seeds of one side at one place"
        return np.ascontiguousarray(a[:, [2, 0, 1, 3]].astype(np.uint32))

    def done(self):
        return self._array(self.q), self._array(self.r)


def in_order(s):
    """the list is in (contig, pos) order, no place twice"""
    c, p = s[:, 1].astype(np.int64), s[:, 2].astype(np.int64)
    return bool(((c[1:] > c[:-1]) | ((c[1:] == c[:-1]) & (p[1:] > p[:-1]))).all())


def wanted_in_order(L):
    """the anchors a case asked for by anchor() alone, in SPEC order (every r seed has one anchor, so r order is anchor order)"""
    return sorted(L.wanted, key=lambda a: (a[0], a[1]))


# ---- occ_grid ------------------------------------------------------------------------------------------------------------------------------------
def occ_grid(tandem=False):
    """one value (tandem: one unit of three values 10 apart) for every (occ_q, occ_r) in 1..5 x 1..5. tandem = False: all seeds 3000 apart, nothing chains,
    100 anchors. tandem = True: the copies of a unit sit 40 apart on either side, so the oq * or diagonals of a cell lie in each other's reach and the
    chains depend on the (r index, q index) order of the anchors; cells are 3000 apart."""
    L = Lists()
    rp = qp = 0
    for oq in range(1, 6):
        for orr in range(1, 6):
            vals = [L.value() for _ in range(3 if tandem else 1)]
            for side, occ in (("r", orr), ("q", oq)):
                p = rp if side == "r" else qp
                for copy in range(occ):
                    for u, v in enumerate(vals):
                        (L.r_seed if side == "r" else L.q_seed)(0, p + 10 * u, v, 1)
                    p += 40 if tandem else 3000
                p += 3000
                if side == "r":
                    rp = p
                else:
                    qp = p
    return L.done()


# ---- band, braid, fork ---------------------------------------------------------------------------------------------------------------------------
def band(between):
    """A0 = (r 100, q 100), A1 = (110, 110), `between` anchors on another q contig with q running backwards (they chain with nobody), A2 = (400, 400):
    with 63 between, A2's only candidate A1 is exactly B = 64 back; with 64 it is out of the band and the chain of two is dropped"""
    L = Lists()
    L.anchor(0, 100, 0, 100)
    L.anchor(0, 110, 0, 110)
    for i in range(between):
        L.anchor(0, 111 + i, 1, 5000 - i)
    L.anchor(0, 400, 0, 400)
    return L


def braid(D, n):
    """D diagonals of n anchors, alternating strand, each on a q contig of its own, interleaved anchor by anchor on one r contig: anchor l of diagonal d
    is anchor l * D + d of the pair, at r = 100 + (D + 5) * l + d, and its only candidate is exactly D back. At D = 64 every slot of the ring holds another
    chain and every predecessor sets the bit that was just cleared."""
    L = Lists()
    S = D + 5
    for l in range(n):
        for d in range(D):
            s = d & 1
            L.anchor(0, 100 + S * l + d, d, (1000 + S * l) if s == 0 else (1000 + S * (n - 1 - l)), s)
    return L


def fork():
    """r: values 1, 2, 3 at 100, 110, 120; q: 1, 2, 3, 3 at 100, 110, 118, 122, an unmatched seed on either side behind them. Anchors 2 and 3 are two ends of
    root 0 with f = 58 each; the smaller index (q 118) is the chain's end."""
    L = Lists()
    L.anchor(0, 100, 0, 100)
    L.anchor(0, 110, 0, 110)
    v = L.value()
    L.r_seed(0, 120, v)
    L.q_seed(0, 118, v)
    L.q_seed(0, 122, v)
    L.fill_r(0, 9000)
    L.fill_q(0, 9000)
    return L


def fork_mirror():
    """the same tie across two chunks of 64 of one segment. Anchors 0..2 = (100, 100), (110, 110), (120, 120), f = 60. Anchor 3 = X (r 130, q 140): f = 70.
    Anchors 4..63: fifteen r seeds 131..145, each with four q seeds on q contig 1 that run backwards (no chain). Anchor 64 = Y (r 149, q 139): its best
    candidate is anchor 2, 62 back, f = 60 + 20 - |29 - 19| = 70 as well, and q 139 < 140 keeps it from following X. X wins: the chain covers q seeds
    100 .. 140, the unmatched 139 among them (C_q = 5, M_q = 4); Y as the end would give C_q = 4."""
    L = Lists()
    for i in range(3):
        L.anchor(0, 100 + 10 * i, 0, 100 + 10 * i)
    L.anchor(0, 130, 0, 140)
    for j in range(15):
        v = L.value()
        L.r_seed(0, 131 + j, v)
        for c in range(4):
            L.q_seed(1, 9000 - 10 * j + c, v)
    L.anchor(0, 149, 0, 139)
    return L


# ---- many segments, tiles --------------------------------------------------------------------------------------------------------------------------
def many_segments(n_runs):
    """runs of 1, 3, 2, 1, 3, 2, ... anchors 10 apart on one diagonal, the runs separated by r (and q) gaps of G + 1: n_runs segments, a chain kept in
    every run of three. Heads sit at anchors 6 j + {0, 1, 4}: one at 4096 = 6 * 682 + 4."""
    L = Lists()
    p = 50
    for run in range(n_runs):
        for i in range((1, 3, 2)[run % 3]):
            L.anchor(0, p, 0, p + 7)
            p += 10
        p += G + 1 - 10
    return L


def long_diagonal(n):
    """one segment and one chain of n anchors: the tiles in the middle have no head"""
    L = Lists()
    for i in range(n):
        L.anchor(0, 10 * i, 0, 10 * i + 3)
    return L


def singles(n):
    """n segments of one anchor each: every anchor of every tile is a head"""
    L = Lists()
    for i in range(n):
        L.anchor(i & 1, (G + 1) * i, 0, (G + 1) * i)
    return L


# ---- slices ------------------------------------------------------------------------------------------------------------------------------------------
def slice_diag(n_r):
    """n_r r seeds 10 apart; a diagonal over the r seeds 2040 .. 2055 (as far as they exist) crosses the slice edge 2047 | 2048, and for n_r > 4096 another
    over 4090 .. 4095 ends on the last seed of the second slice: the only seed of the third, behind the last anchor-bearing one, bears none"""
    L = Lists()
    on = set(range(2040, min(2056, n_r))) | (set(range(4090, 2 * AN_SLICE)) if n_r > 2 * AN_SLICE else set())
    for i in range(n_r):
        if i in on:
            L.anchor(0, 10 * i, 0, 10 * i + 5)
        else:
            L.fill_r(0, 10 * i)
    L.fill_q(0, 3)
    L.fill_q(0, 20447)                                      # a covered q seed no anchor touches
    return L


def slice_occ4(n_r):
    """the r seeds 2046 .. 2049 (as far as they exist) each with occ_q = 4: four q copies 1000 apart, so four diagonals cross the slice edge and the
    multi-anchor seeds sit in the last lane of slice 0 and the first of slice 1; the same at 4094 .. 4096 for n_r > 4096"""
    L = Lists()
    multi = [i for i in (2046, 2047, 2048, 2049, 4094, 4095, 4096) if i < n_r]
    for i in range(n_r):
        if i in multi:
            v = L.value()
            L.r_seed(0, 10 * i, v)
            for c in range(4):
                L.q_seed(c & 1, 1000 * c + 10 * i, v)
        else:
            L.fill_r(0, 10 * i)
    return L


# ---- sides -------------------------------------------------------------------------------------------------------------------------------------------
def side_n(n, other=None):
    """a q side of n seeds against an r side of `other` (default n) seeds, seed i of a side of m at pos (1000 i) // (m - 1). With both sides alike and
    n >= 3, a chain through the seeds 0, n // 2 and n - 1 covers the whole side: the run ends on the last seed. n = 0, 1: whatever can match does."""
    L = Lists()
    m = n if other is None else other
    pos = lambda i, cnt: 1000 * i // max(cnt - 1, 1)                                     # noqa: E731
    if n == m and n >= 3:
        on = {0, n // 2, n - 1}
        for i in range(n):
            if i in on:
                L.anchor(0, pos(i, n), 0, pos(i, n))
            else:
                L.fill_r(0, pos(i, n))
                L.fill_q(0, pos(i, n))
    else:
        for i in range(min(n, m)):
            L.anchor(0, pos(i, m), 0, pos(i, n))
        for i in range(min(n, m), n):
            L.fill_q(0, pos(i, n))
        for i in range(min(n, m), m):
            L.fill_r(0, pos(i, m))
    return L


def side_chains(n_q, n_r, chains, q_break=None, r_break=None):
    """sides of n_q and n_r seeds 20 apart, contig 1 from seed *_break on; chains = [(strand, [(r seed, q seed), ...]), ...]: every listed couple becomes an
    anchor, every other seed a filler"""
    L = Lists()
    qc = lambda i: int(q_break is not None and i >= q_break)                            # noqa: E731
    rc = lambda i: int(r_break is not None and i >= r_break)                            # noqa: E731
    used_q, used_r = set(), set()
    for s, couples in chains:
        for ri, qi in couples:
            assert ri not in used_r and qi not in used_q
            used_r.add(ri); used_q.add(qi)
            L.anchor(rc(ri), 20 * ri, qc(qi), 20 * qi, s)
    for i in range(n_q):
        if i not in used_q:
            L.fill_q(qc(i), 20 * i)
    for i in range(n_r):
        if i not in used_r:
            L.fill_r(rc(i), 20 * i)
    return L


def _fwd(a, b, step, off=0):
    return (0, [(i, i + off) for i in range(a, b + 1, step)])


def _rev(r0, q_hi, n=3, step=4):
    return (1, [(r0 + step * i, q_hi - step * i) for i in range(n)])


def side_intervals(mirror):
    """q side (mirror: r side): chain 1 covers [10, 50]; a chain on the other strand nested in it [21, 29], one overlapping it [49, 57] and one adjacent to
    that [58, 66]; the other side has them apart"""
    if mirror:
        chains = [_fwd(10, 50, 20), _rev(21, 80), _rev(49, 100), _rev(58, 120)]
    else:
        chains = [_fwd(10, 50, 20), _rev(70, 29), _rev(90, 57), _rev(110, 66)]
    return side_chains(130, 130, chains)


def side_contig_change(at):
    """129 seeds a side, contig 1 from seed `at` (64 or 65) on, on both sides: a chain that ends on seed at - 1 and one that starts on seed at - the covered
    stretch goes through the change, which cuts the run at lane 0 (at = 64) or lane 1 (at = 65) of the second chunk"""
    chains = [_fwd(at - 13, at - 1, 6), _fwd(at, at + 12, 6)]
    return side_chains(129, 129, chains, q_break=at, r_break=at)


# ---- range -------------------------------------------------------------------------------------------------------------------------------------------
def _plant(L, value, q_at, r_at):
    for c, p in q_at:
        L.q_seed(c, p, value)
    for c, p in r_at:
        L.r_seed(c, p, value)


def range_diagonals():
    """a 5-anchor diagonal (step 4) at r 0xFFFFF000, q 0x7FFFFFF8 .. 0x80000008 and a 4-anchor one on the other strand (step 7) at r 0xFFFFFF58,
    q 0xFFFFFFF5 down to 0xFFFFFFE0 on q contig 1: [9, 2, 9, 9, 69, 9, 9, 3965]"""
    L = Lists()
    for i in range(5):
        L.anchor(0, 0xFFFFF000 + 4 * i, 0, 0x7FFFFFF8 + 4 * i)
    for i in range(4):
        L.anchor(0, 0xFFFFFF58 + 7 * i, 1, 0xFFFFFFF5 - 7 * i, 1)
    return L


def range_values(occ5):
    """values 0 and 0xFFFFFFFF. occ5 = False: each once on both sides, inside a diagonal of four (value 0 its first anchor, 0xFFFFFFFF its last).
    occ5 = True: value 0 five times on the q side and 0xFFFFFFFF five times on the r side: the diagonal keeps its two middle anchors only."""
    L = Lists()
    _plant(L, 0, [(0, 500)], [(0, 0xFFFFF000)])
    L.anchor(0, 0xFFFFF010, 0, 510)
    L.anchor(0, 0xFFFFF020, 0, 520)
    _plant(L, 0xFFFFFFFF, [(0, 530)], [(0, 0xFFFFF030)])
    if occ5:
        _plant(L, 0, [(1, 100 * i) for i in range(4)], [])
        _plant(L, 0xFFFFFFFF, [], [(1, 100 * i) for i in range(4)])
    L.fill_q(0, 7)
    L.fill_r(0, 7)
    return L


def range_step(step):
    """three anchors `step` apart in r and q (G: a chain; G + 1: none), r up to 0xFFFFF388, q across 2^31"""
    L = Lists()
    for i in range(3):
        L.anchor(0, 0xFFFFE000 + step * i, 0, 0x80000000 - step - 5 + step * i)
    return L


# ---- random lists ------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4097, 6000)


def random_lists(rng, n_r):
    """an r list of n_r seeds over 3 contigs (steps of 6 .. 60, a gap above G every 80 seeds or so) and a q list that is a copy of it with about 30 % of the
    seeds dropped, positions moved by up to 2, one block inverted (positions mirrored, fwd flipped), fresh seeds added and, on either side, about 15 % of the
    values redrawn from a small pool so that occ 2 .. 6 occur; values 0 and 0xFFFFFFFF are planted on both sides."""
    val = rng.choice(np.arange(1, 1 << 24, dtype=np.int64), n_r, replace=False) * 251 + 1000
    step = rng.integers(6, 61, n_r)
    step[rng.random(n_r) < 1 / 80] += G + 1
    ctg = np.sort(rng.integers(0, 3, n_r)) if n_r >= 3 else np.zeros(n_r, np.int64)
    pos = np.zeros(n_r, np.int64)
    for c in range(3):
        m = ctg == c
        pos[m] = np.cumsum(step[m])
    fwd = rng.integers(0, 2, n_r)
    pool = rng.integers(1, 1 << 30, max(1, n_r // 30)) * 4 + 3

    def redraw(v, share):
        v = v.copy()
        hit = rng.random(len(v)) < share
        v[hit] = rng.choice(pool, int(hit.sum()))
        return v

    rv = redraw(val, 0.15)
    qv = redraw(rv, 0.05)
    if n_r >= 2:
        rv[n_r // 3] = qv[n_r // 3] = 0
        rv[n_r - 1] = qv[n_r - 1] = 0xFFFFFFFF
    keep = rng.random(n_r) >= 0.30
    if n_r >= 2:
        keep[[n_r // 3, n_r - 1]] = True
    qc, qp, qf, qv = ctg[keep], pos[keep] + rng.integers(-2, 3, int(keep.sum())), fwd[keep], qv[keep]
    nq = len(qp)
    if nq >= 40:                                            # the inverted block: inside contig 0
        n0 = int((qc == 0).sum())
        a = n0 // 4
        b = min(n0, a + max(10, n0 // 3))
        if b - a >= 2:
            qp[a:b] = (qp[a] + qp[b - 1] - qp[a:b])[::-1]
            qv[a:b] = qv[a:b][::-1]
            qf[a:b] = 1 - qf[a:b][::-1]
    n_new = n_r // 10 + 1                                    # fresh seeds: odd places are free on no side in particular, a clash is dropped below
    fc = rng.integers(0, 3, n_new)
    fp = rng.integers(0, int(pos.max()) + 100 if n_r else 100, n_new)
    fv = 0xC0000000 + np.arange(n_new)
    q = np.stack([np.concatenate([qc, fc]), np.concatenate([qp, fp]), np.concatenate([qv, fv]), np.concatenate([qf, rng.integers(0, 2, n_new)])], 1)
    q = q[np.lexsort((q[:, 1], q[:, 0]))]
    first = np.ones(len(q), bool)
    first[1:] = (q[1:, 0] != q[:-1, 0]) | (q[1:, 1] != q[:-1, 1])
    q = q[first]
    r = np.stack([ctg, pos, rv, fwd], 1)
    return np.ascontiguousarray(q[:, [2, 0, 1, 3]].astype(np.uint32)), np.ascontiguousarray(r[:, [2, 0, 1, 3]].astype(np.uint32))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------
N_RUNS = 9000                # many_segments at n_cu = 256: 9000 > 32 * 256
LONG_N = 3 * AN_TILE + 7
SIDE_NS = (0, 1, 63, 64, 65, 128, 129)

# the eight integers {n_anchors, n_chains_kept, M_q, C_q, A_q, M_r, C_r, A_r} worked out by hand from SPEC 12
LITERAL = {
    "occ_grid": [100, 0, 0, 0, 0, 0, 0, 0],
    "band(62)": [65, 1, 3, 3, 316, 3, 65, 316],
    "band(63)": [66, 1, 3, 3, 316, 3, 66, 316],
    "band(64)": [67, 0, 0, 0, 0, 0, 0, 0],
    "braid(64,4)": [256, 64, 256, 256, 14272, 256, 256, 286],
    "fork": [4, 1, 3, 3, 34, 3, 3, 36],
    "fork_mirror": [65, 1, 4, 5, 56, 4, 4, 46],
    "many_segments": [18000, 3000, 9000, 9000, 108000, 9000, 9000, 108000],
    "side_n(64)": [3, 1, 3, 64, 1016, 3, 64, 1016],
    "range_diagonals": [9, 2, 9, 9, 69, 9, 9, 3965],
}
# chains kept and, where the issue states them, M and C
LITERAL_CHAINS = {"braid(33,5)": 33, "braid(63,4)": 63, "braid(64,4)": 64, "braid(65,4)": 0, "braid(64,2)": 0, "braid(64,3)": 64}


def named_cases(n_runs=N_RUNS):
    """name -> (qs, rs); n_runs: the runs of many_segments (the device test takes more where 32 * n_cu asks for it)"""
    out = {"occ_grid": occ_grid(False), "occ_grid_tandem": occ_grid(True)}
    for b in (62, 63, 64):
        out["band(%d)" % b] = band(b).done()
    for D, n in ((33, 5), (63, 4), (64, 4), (65, 4), (64, 2), (64, 3)):
        out["braid(%d,%d)" % (D, n)] = braid(D, n).done()
    out["fork"] = fork().done()
    out["fork_mirror"] = fork_mirror().done()
    out["many_segments"] = many_segments(n_runs).done()
    out["long_diagonal"] = long_diagonal(LONG_N).done()
    for n in (AN_TILE, AN_TILE + 1, 2 * AN_TILE):
        out["singles(%d)" % n] = singles(n).done()
    for n in (2047, 2048, 2049, 4097):
        out["slice_diag(%d)" % n] = slice_diag(n).done()
        out["slice_occ4(%d)" % n] = slice_occ4(n).done()
    for n in SIDE_NS:
        out["side_n(%d)" % n] = side_n(n).done()
    for n in (0, 1):
        out["side_n(%d,5)" % n] = side_n(n, 5).done()
        out["side_n(5,%d)" % n] = side_n(5, n).done()
    out["side_intervals_q"] = side_intervals(False).done()
    out["side_intervals_r"] = side_intervals(True).done()
    out["side_contig_change(64)"] = side_contig_change(64).done()
    out["side_contig_change(65)"] = side_contig_change(65).done()
    out["range_diagonals"] = range_diagonals().done()
    out["range_values"] = range_values(False).done()
    out["range_values_occ5"] = range_values(True).done()
    out["range_step(G)"] = range_step(G).done()
    out["range_step(G+1)"] = range_step(G + 1).done()
    return out


def random_cases():
    rng = np.random.default_rng(1212)
    return {"random(%d)" % n: random_lists(rng, n) for n in RANDOM_SIZES}


def all_cases(n_runs=N_RUNS):
    out = named_cases(n_runs)
    out.update(random_cases())
    return out
