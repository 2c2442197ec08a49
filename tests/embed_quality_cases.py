"""The case table of SPEC.md 8.1's tests (shared by test_embed_quality_cpu.py and test_gpu_embed_quality.py): graphs, positions and the list of
(name, n, dim, kq, knbn, kind) cases. n: 2, 3, one below / at / one above both tile sizes of the counting kernel, 257 (the block knob of the GPU test),
4097; dim: 1..4; kq: 1, 2, knbn, 200, n - 1, n + 5 (clamped); knbn: 1, 8, 17; rows with count 0 and count < knbn among the full ones; positions: the
integer lattice (ties at every radius), all points equal, two clumps at x = +-3e19 (d2 = +inf across them), coordinates of the order 1e-20 (denormal
squares), negative zeros, a Gaussian cloud. Everything is seeded."""
import numpy as np

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
TILE_Q, TILE_P = 256, 1024          # GS_EMBQ_TILE_Q / GS_EMBQ_TILE_P (the GPU test holds them to the library's)
KINDS = ("lattice", "equal", "clumps", "tiny", "negzero", "gauss")


def graph(n, knbn, seed):
    """a valid graph in node numbers: distinct neighbours other than the node, ascending distances; row 0 is empty when n > 2, about a quarter of the
    rows keep fewer than they could"""
    rng = np.random.default_rng(seed)
    full = min(knbn, n - 1)
    cnt = np.where(rng.random(n) < 0.25, rng.integers(0, full + 1, n), full).astype(np.uint32)
    if n > 2:
        cnt[0] = 0
    cnt[n - 1] = full
    ids = np.full((n, knbn), U64MAX)
    dist = np.full((n, knbn), np.inf, np.float32)
    for i in range(n):
        c = int(cnt[i])
        nb = rng.choice(n - 1, c, replace=False)
        ids[i, :c] = nb + (nb >= i)
        dist[i, :c] = np.sort(rng.integers(0, 1 << 12, c) * np.float32(2.0 ** -12))
    return ids, dist, cnt


def positions(kind, n, dim, seed):
    rng = np.random.default_rng(seed + 1000)
    i = np.arange(n)
    if kind == "lattice":            # 8 points per axis: beyond 8^dim nodes the points repeat
        y = np.stack([(i // 8 ** t) % 8 for t in range(dim)], axis=1)
    elif kind == "equal":
        y = np.full((n, dim), 1.5)
    elif kind == "clumps":
        y = rng.normal(0, 1, (n, dim))
        y[:, 0] = np.where(i % 2 == 0, 3e19, -3e19)
    elif kind == "tiny":
        y = rng.normal(0, 1, (n, dim)) * 1e-20
    elif kind == "negzero":
        y = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), (n, dim))
    else:
        y = rng.normal(0, 1, (n, dim))
    return np.ascontiguousarray(y, dtype=np.float32)


def _table():
    T = []
    # the small ends: every kind at n = 2 and 3
    for k, kind in enumerate(KINDS):
        T.append((2, 1 + k % 4, (1, 2, 7)[k % 3], (1, 8, 17)[k % 3], kind))
        T.append((3, 1 + (k + 1) % 4, (2, 1, 8)[k % 3], (8, 17, 1)[k % 3], kind))
    # the tile edges, over dim, kq and knbn
    for n, dim, kq, knbn, kind in ((TILE_Q - 1, 2, 200, 8, "gauss"), (TILE_Q, 1, 1, 17, "lattice"), (TILE_Q + 1, 3, 8, 8, "lattice"),
                                   (TILE_Q + 1, 4, TILE_Q, 1, "clumps"), (TILE_Q + 1, 2, 2, 17, "negzero"), (TILE_Q + 1, 2, 17, 17, "tiny"),
                                   (TILE_P - 1, 4, 200, 17, "lattice"), (TILE_P, 2, TILE_P - 1, 8, "clumps"), (TILE_P + 1, 3, TILE_P + 6, 1, "tiny"),
                                   (TILE_P + 1, 1, 200, 8, "gauss"), (TILE_P + 1, 2, 8, 8, "equal"), (TILE_Q, 4, 1, 8, "negzero"),
                                   (4097, 2, 200, 8, "gauss"), (4097, 3, 2, 17, "lattice")):
        T.append((n, dim, kq, knbn, kind))
    return [("%s-n%d-d%d-kq%d-k%d" % (kind, n, dim, kq, knbn), n, dim, kq, knbn, kind) for n, dim, kq, knbn, kind in T]


CASES = _table()
# the cases of the block knob: 257 nodes in blocks of 100 rows and 100 points
KNOB_CASES = [c for c in CASES if c[1] == TILE_Q + 1]


def make(case):
    name, n, dim, kq, knbn, kind = case
    seed = sum(name.encode())
    ids, dist, cnt = graph(n, knbn, seed)
    return ids, dist, cnt, positions(kind, n, dim, seed), kq
