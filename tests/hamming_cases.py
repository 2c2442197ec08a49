"""Case table of the DistHamming compare kernels (gsearch_amd/csrc/gs_hamming.hip) with a numpy reference only: no library call, no GPU.
tests/test_hamming_cases_cpu.py holds the table to its own names (every value class and edge is counted, so a later edit cannot drop one
unnoticed), tests/test_gpu_hamming.py runs it on the device, tests/test_hamming_split_cpu.py holds split_rule to the header it restates.

The edges are the kernels' own: the 128 x 128 tile (rows on either side of 127 / 128 / 129, a second and third query tile), the 32-word K-chunk and
the 4-word load (m around 32, 64, 256 and m % 4 in 0..3), the 256-word step of the thin kernel, the 16 query rows of a thin item, ceil(rows / 16)
from 1 to 8 on the tile kernel's THIN path, row pitches that allow or forbid 16-byte loads, garbage behind the row end, and the 256 row words from
which the drivers split a row over blockIdx.z."""
import numpy as np

HT, HKW, HTQ, HTR = 128, 32, 16, 4          # gs_hamming_split.hpp
# The split rule of gs_hamming_split.hpp, restated from its comment. units = tiles (dense form, 0) or items (work-list form, 1); roww = 32-bit words per row.
#   split only if units * A <= n_cu * B and roww >= 8 * HKW;  nz = min(n_cu * F // units, roww // (4 * HKW));  split only if nz > 1;
#   ksplit = ceil(ceil(roww / nz) / HKW) * HKW;  parts = ceil(roww / ksplit).  No split: ksplit = 0, parts = 1.
SPLIT_FORMS = {0: (2, 1, 2), 1: (2, 2, 4)}   # form -> (A, B, F)


def split_rule(n_cu, units, roww, form):
    """(ksplit words, parts) for an int64 array of row-word counts"""
    a, b, f = SPLIT_FORMS[form]
    roww = np.asarray(roww, dtype=np.int64)
    ks, parts = np.zeros_like(roww), np.ones_like(roww)
    if units * a > n_cu * b:
        return ks, parts
    nz = np.minimum(n_cu * f // units, roww // (4 * HKW))
    sp = (roww >= 8 * HKW) & (nz > 1)
    per = -(-roww[sp] // nz[sp])
    ks[sp] = -(-per // HKW) * HKW
    parts[sp] = -(-roww[sp] // ks[sp])
    return ks, parts


def split_parts(n_cu, units, roww, form):
    return int(split_rule(n_cu, units, np.array([roww]), form)[1][0])


def row_words(dtype, m):
    return m * (np.dtype(dtype).itemsize // 4)


# ---- reference -----------------------------------------------------------------------------------------------------------------------------
def counts(q, c, m):
    """mismatch counts of the logical columns [:m], numpy's own `!=` of the element type (IEEE for float32: NaN differs from everything, itself
    included; +0 equals -0; denormals are numbers like any other)"""
    q, c = q[:, :m], c[:, :m]
    out = np.empty((q.shape[0], c.shape[0]), np.int64)
    step = max(1, (1 << 22) // max(1, c.shape[0] * m))
    for i in range(0, q.shape[0], step):
        out[i:i + step] = (q[i:i + step, None, :] != c[None, :, :]).sum(-1)
    return out


def distances(cnt, m):
    return np.float32(cnt) / np.float32(m)


def counts_python(q, c, m):
    """the same with plain Python scalars (float32 -> Python float is exact)"""
    ql, cl = q[:, :m].tolist(), c[:, :m].tolist()
    return np.array([[sum(1 for x, y in zip(a, b) if x != y) for b in cl] for a in ql], np.int64).reshape(len(ql), len(cl))


def pair_counts(a, b, ia, ib):
    return (a[ia] != b[ib]).sum(-1).astype(np.int64)


# ---- values --------------------------------------------------------------------------------------------------------------------------------
SPECIAL_COLS = (0, 31, 32, 255, 256)         # and m - 1
F_POS0, F_NEG0, F_NAN_A, F_NAN_B, F_SNAN, F_PINF, F_NINF, F_DEN1, F_DEN2, F_NDEN1, F_ONE = (
    0x00000000, 0x80000000, 0x7FC00000, 0x7FC00123, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001, 0x00000002, 0x80000001, 0x3F800000)
F32_POOL = np.array([F_POS0, F_NEG0, F_NAN_A, F_NAN_B, F_SNAN, F_PINF, F_NINF, F_DEN1, F_DEN2, F_NDEN1, F_ONE], np.uint32)
_V32, _V64, _V16 = 0x5A3C96E1, 0x5A3C96E1C3A50F69, 0x5A3C
# xor masks of the integer pools: equal; bit 31 (u64: bit 63) alone; bit 0 alone; for u64 also: only above bit 31, only below it, bit 32, bit 31
U32_MASKS = np.array([0, 1 << 31, 1, 0x00010000, 0x80000001, 0], np.uint32)
U64_MASKS = np.array([0, 1 << 63, 1, 0x00F0000100000000, 0x00000000F0010002, 1 << 32, 1 << 31, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF, 0], np.uint64)
U16_MASKS = np.array([0, 1 << 15, 1, 0x0100, 0x8001, 0], np.uint16)


def special_cols(m):
    return sorted(set(c for c in SPECIAL_COLS + (m - 1,) if c < m))


def _pool(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return F32_POOL.view(np.float32)
    if dtype == np.uint32:
        return np.uint32(_V32) ^ U32_MASKS
    if dtype == np.uint64:
        return np.uint64(_V64) ^ U64_MASKS
    return np.uint16(_V16) ^ U16_MASKS


def make_rows(seed, dtype, nq, nc, m, plain_rows=True):
    """(q, c): nq and nc rows of m elements over one alphabet of three values per column, so that about a third of the slots match. The three differ
    in ways half a compare would miss: u64 in the high word only and in the low word only, u32 in bit 31 and bit 0, f32 in the last mantissa bit and in
    the sign. The special columns hold the pool of the type instead (every pair of pool values once nq, nc >= the pool's length). With plain_rows and
    enough rows: c[0] = q[0] without NaN (count 0), q[nq - 1] differs from every row in every slot (count m), for f32 c[nc - 1] is all NaN (count m)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        base = (rng.integers(0x30000000, 0x4F000000, m, dtype=np.uint32) | np.uint32(2)).astype(np.uint32)      # finite, normal, not the special ones
        alpha = np.stack([base, base ^ np.uint32(1), base ^ np.uint32(0x80000000)]).view(np.float32)
    elif dtype == np.uint32:
        base = rng.integers(0, 1 << 31, m, dtype=np.uint32)                                                      # (bit 31 clear: the all-different row sets it)
        alpha = np.stack([base, base ^ np.uint32(1 << 30), base ^ np.uint32(1)])
    elif dtype == np.uint64:
        base = rng.integers(0, 1 << 62, m, dtype=np.uint64)
        hi = rng.integers(1, 1 << 29, m, dtype=np.uint64) << np.uint64(32)
        lo = rng.integers(1, 1 << 31, m, dtype=np.uint64)
        alpha = np.stack([base, base ^ hi, base ^ lo])
    else:
        base = rng.integers(0, 1 << 14, m, dtype=np.uint16)
        alpha = np.stack([base, base ^ np.uint16(1 << 13), base ^ np.uint16(1)])
    cols = np.arange(m)
    q = alpha[rng.integers(0, 3, (nq, m)), cols]
    c = alpha[rng.integers(0, 3, (nc, m)), cols]
    pool = _pool(dtype)
    for k, col in enumerate(special_cols(m)):
        q[:, col] = pool[(np.arange(nq) + 3 * k) % len(pool)]
        c[:, col] = pool[(np.arange(nc) * 7 + k) % len(pool)]
    if plain_rows:
        if nq >= 2 and nc >= 2:
            q[0] = alpha[0]
            c[0] = q[0]
        if nq >= 3:                                                           # a negative number of an exponent of its own, or the top bit and bit 1 flipped: in no alphabet
            if dtype == np.float32:
                q[nq - 1] = (np.uint32(0xD0000000) + np.arange(m, dtype=np.uint32)).view(np.float32)
            else:
                q[nq - 1] = alpha[0] ^ dtype.type((1 << (dtype.itemsize * 8 - 1)) | 2)
        if nc >= 3 and dtype == np.float32:
            c[nc - 1] = np.where(cols % 2 == 0, np.uint32(F_NAN_A), np.uint32(F_SNAN)).astype(np.uint32).view(np.float32)
    return np.ascontiguousarray(q), np.ascontiguousarray(c)


STRIDES = ("row", "r16", "r256", "plus4")


def stride_bytes(mode, dtype, m):
    row = np.dtype(dtype).itemsize * m
    return {"row": row, "r16": (row + 15) // 16 * 16, "r256": (row + 255) // 256 * 256, "plus4": row + 4}[mode]


def padded_words(rows, stride, seed):
    """the rows as a matrix of uint32 words of `stride` bytes per row; what lies behind a row's end is random non-zero garbage, different in every row"""
    n, m = rows.shape
    roww = rows.dtype.itemsize * m // 4
    w = np.random.default_rng(seed ^ 0x9E3779B9).integers(1, 1 << 32, (n, stride // 4), dtype=np.uint32)
    w[:, :roww] = rows.view(np.uint32).reshape(n, roww)
    return np.ascontiguousarray(w)


# ---- the dense form ------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 129), (127, 129), (128, 128), (129, 127), (257, 130), (16, 128), (17, 1))
MS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 515, 1023)
KINDS = (np.dtype(np.float32), np.dtype(np.uint32), np.dtype(np.uint64))
SHIFTS = {4: (0, 4, 8), 8: (0, 8)}
SPLIT_MS = {4: (256, 257, 300, 515, 1023), 8: (128, 150)}
SPLIT_SHAPES = ((128, 128), (129, 130))       # one tile, 2 x 2 tiles


def _dense(name, i, dtype, nq, nc, m, mode, shift, plain_rows=True):
    q, c = make_rows(1000 + i, dtype, nq, nc, m, plain_rows)
    sq = stride_bytes(mode, dtype, m)
    return {"name": name, "dtype": np.dtype(dtype), "m": m, "nq": nq, "nc": nc, "stride": mode, "stride_bytes": sq, "shift": shift, "q": q, "c": c,
            "qw": padded_words(q, sq, 2 * i), "cw": padded_words(c, sq, 2 * i + 1)}


def dense_cases():
    """a covering selection, not the full cross: every m at two shapes or more, every shape at m = 33 and 257, each of those in the three kinds; pitch and
    shift rotate so that each kind meets every pitch and every shift; then the split cases and m = 65535"""
    combos = []
    for i, m in enumerate(MS):
        for s in {SHAPES[i % 8], SHAPES[(i + 3) % 8]} | (set(SHAPES) if m in (33, 257) else set()):
            combos.append((m, s))
    combos.sort()
    out, i = [], 0
    for m, (nq, nc) in combos:
        for dtype in KINDS:
            mode = STRIDES[(i + i // 4) % 4]
            sh = SHIFTS[dtype.itemsize]
            shift = sh[(i // 3 + i // 12) % len(sh)]
            out.append(_dense("%s_%dx%d_m%d_%s_s%d" % (dtype.name, nq, nc, m, mode, shift), i, dtype, nq, nc, m, mode, shift))
            i += 1
    for dtype in KINDS:
        for m in SPLIT_MS[dtype.itemsize]:
            for nq, nc in SPLIT_SHAPES:
                mode = STRIDES[i % 4]
                out.append(_dense("split_%s_%dx%d_m%d_%s" % (dtype.name, nq, nc, m, mode), i, dtype, nq, nc, m, mode, 0))
                i += 1
    # the 16-bit form at its largest m, every slot different: q = 2 j + 1, c = 2 j (+ 2^20 in the second row of each)
    m = 65535
    j = np.arange(m, dtype=np.uint32)
    q, c = np.stack([2 * j + 1, 2 * j + 1 + (1 << 20)]), np.stack([2 * j, 2 * j + (1 << 21)])
    out.append({"name": "uint32_2x2_m65535_all_different", "dtype": np.dtype(np.uint32), "m": m, "nq": 2, "nc": 2, "stride": "row", "stride_bytes": 4 * m, "shift": 0,
                "q": q, "c": c, "qw": padded_words(q, 4 * m, 1), "cw": padded_words(c, 4 * m, 2)})
    return out


def dense_tiles(case):
    return -(-case["nq"] // HT) * -(-case["nc"] // HT)


def dense_vec4(case):
    return case["stride_bytes"] % 16 == 0 and case["shift"] % 16 == 0


# ---- the work-list form --------------------------------------------------------------------------------------------------------------------
ITEM_SHAPES = ((1, 1), (1, 128), (15, 17), (16, 16), (16, 128), (17, 128), (40, 127), (112, 128), (113, 3), (128, 128))
EXTRA_SHAPES = ((50, 5), (70, 64), (90, 33))                    # ceil(rows / 16) = 4, 5, 6: with ITEM_SHAPES every value 1..8
SMALL_SHAPES = ((2, 3), (16, 1), (3, 70), (9, 9), (16, 31), (5, 128), (12, 2), (1, 15), (8, 16), (16, 127), (7, 33), (4, 4), (14, 65), (10, 5), (6, 100))
THIN_MS = (4, 255, 256, 257, 515, 802, 1001, 1003)
NC_ROWS, PAIR_COLS = 300, 20
LDS = (NC_ROWS, NC_ROWS + 1)


def _lists(seed, shapes, with_pair):
    """items (thin-eligible ones first), qlist, clist, the number of query rows. Every item has query rows of its own, except the pair: two items on the
    same PAIR rows (16), one with PAIR_COLS even columns 2 k and one with the odd columns 2 k + 1 - every cell of either has its 32-bit partner in the other
    item. clist is a shuffled strict subset of the columns with those two stretches in it, qlist a shuffled strict subset of the rows."""
    rng = np.random.default_rng(seed)
    ks = np.sort(rng.choice(NC_ROWS // 2, PAIR_COLS, replace=False))
    rest = np.setdiff1d(np.arange(NC_ROWS), np.concatenate([2 * ks, 2 * ks + 1]))
    rest = rng.permutation(rest)[:215]
    cut = int(rng.integers(10, 60))
    clist = np.concatenate([rest[:cut], rng.permutation(2 * ks), rng.permutation(2 * ks + 1), rest[cut:]]).astype(np.uint32)
    shapes = sorted(shapes, key=lambda s: s[0] > HTQ)          # stable: the thin-eligible ones first
    items, qpos = [], 0
    if with_pair:
        items += [(0, HTQ, cut, PAIR_COLS), (0, HTQ, cut + PAIR_COLS, PAIR_COLS)]
        qpos = HTQ
    for qr, cr in shapes:
        items.append((qpos, qr, int(rng.integers(0, len(clist) - cr + 1)), cr))
        qpos += qr
    items.sort(key=lambda it: it[1] > HTQ)
    nq_rows = qpos + 7
    qlist = rng.permutation(nq_rows)[:qpos].astype(np.uint32)
    return np.array(items, np.uint32).reshape(-1, 4), qlist, clist, nq_rows


def _blocks(name, i, dtype, m, mode, shapes, with_pair):
    items, qlist, clist, nq_rows = _lists(5000 + i, shapes, with_pair)
    q, c = make_rows(3000 + i, dtype, nq_rows, NC_ROWS, m, plain_rows=False)
    sq = stride_bytes(mode, dtype, m)
    eligible = int((items[:, 1] <= HTQ).sum())
    return {"name": name, "dtype": np.dtype(dtype), "m": m, "stride": mode, "stride_bytes": sq, "q": q, "c": c, "qw": padded_words(q, sq, 2 * i),
            "cw": padded_words(c, sq, 2 * i + 1), "items": items, "qlist": qlist, "clist": clist, "nq_rows": nq_rows, "nc_rows": NC_ROWS,
            "n_thin": sorted({0, min(2, eligible), eligible}), "eligible": eligible}


LIST_30 = ITEM_SHAPES + EXTRA_SHAPES + SMALL_SHAPES           # + the pair = 30 items
LIST_3 = ((40, 127),)                                         # + the pair = 3 items
LIST_1 = ((16, 128),)


def blocks_cases():
    out, i = [], 0
    for m in THIN_MS:                                          # the thin kernel: 4-byte elements, rows that allow 16-byte loads
        for dtype in KINDS[:2]:
            mode = ("r16", "r256")[(i + i // 2) % 2]
            out.append(_blocks("thin_%s_m%d_%s_30" % (dtype.name, m, mode), i, dtype, m, mode, LIST_30, True))
            i += 1
    for dtype, m, mode in ((KINDS[2], 33, "r16"), (KINDS[2], 128, "row"), (KINDS[2], 150, "plus4"), (KINDS[2], 257, "r256"),       # u64 and pitches without
                           (KINDS[0], 33, "plus4"), (KINDS[1], 257, "plus4"), (KINDS[0], 300, "plus4"), (KINDS[1], 255, "row")):    # 16-byte loads: the tile kernel's THIN path
        out.append(_blocks("tile_%s_m%d_%s_30" % (dtype.name, m, mode), i, dtype, m, mode, LIST_30, True))
        i += 1
    for dtype, m, mode in ((KINDS[0], 257, "r16"), (KINDS[1], 515, "r256"), (KINDS[2], 150, "row"), (KINDS[1], 5, "plus4")):
        out.append(_blocks("three_%s_m%d_%s_3" % (dtype.name, m, mode), i, dtype, m, mode, LIST_3, True))
        out.append(_blocks("one_%s_m%d_%s_1" % (dtype.name, m, mode), i + 1, dtype, m, mode, LIST_1, False))
        i += 2
    return out


def long_list_case(n_items, m, dtype=np.uint32):
    """more items than the device has compute units (the caller knows how many): n_items items of 2 x 2, each with rows of its own"""
    rng = np.random.default_rng(n_items * 131 + m)
    nq_rows = nc_rows = 2 * n_items + 3
    qlist, clist = rng.permutation(nq_rows)[:2 * n_items].astype(np.uint32), rng.permutation(nc_rows)[:2 * n_items].astype(np.uint32)
    items = np.array([(2 * k, 2, 2 * k, 2) for k in range(n_items)], np.uint32)
    q, c = make_rows(n_items + m, dtype, nq_rows, nc_rows, m, plain_rows=False)
    sq = stride_bytes("r16", dtype, m)
    return {"name": "long_%d_m%d" % (n_items, m), "dtype": np.dtype(dtype), "m": m, "stride": "r16", "stride_bytes": sq, "q": q, "c": c, "qw": padded_words(q, sq, 7),
            "cw": padded_words(c, sq, 8), "items": items, "qlist": qlist, "clist": clist, "nq_rows": nq_rows, "nc_rows": nc_rows, "n_thin": [0], "eligible": n_items}


def blocks_vec4(case):
    return case["stride_bytes"] % 16 == 0


def blocks_left(case, n_thin, thin_off=False):
    """the items the tile kernel gets: the thin kernel takes the first n_thin where it applies"""
    thin = n_thin > 0 and blocks_vec4(case) and case["dtype"].itemsize == 4 and not thin_off
    return len(case["items"]) - (n_thin if thin else 0)


CANARY16 = np.uint16(0xFFFF)


def blocks_expected(case, ld_out):
    """the matrix a canary-filled (nq_rows, ld_out) output must come back as: the cells the items name hold numpy's counts, every other the canary"""
    want = np.full((case["nq_rows"], ld_out), CANARY16, np.uint16)
    named = np.zeros(want.shape, bool)
    m = case["m"]
    for q0, qr, c0, cr in case["items"].tolist():
        rows, cols = case["qlist"][q0:q0 + qr], case["clist"][c0:c0 + cr]
        cell = np.ix_(rows, cols)
        assert not named[cell].any(), "two items name one cell"
        named[cell] = True
        want[cell] = counts(case["q"][rows], case["c"][cols], m)
    return want, named


# ---- the public calls ----------------------------------------------------------------------------------------------------------------------
ALL_KINDS = KINDS + (np.dtype(np.uint16),)
PAIR_MS = (1, 63, 64, 65, 129)


def qxc_cases():
    out = []
    for i, ((nq, nc), m) in enumerate((((129, 257), 65), ((257, 129), 257))):
        for dtype in ALL_KINDS:
            q, c = make_rows(7000 + 10 * i + dtype.itemsize, dtype, nq, nc, m)
            out.append({"name": "qxc_%s_%dx%d_m%d" % (dtype.name, nq, nc, m), "dtype": dtype, "m": m, "q": q, "c": c})
    return out


def pairs_cases():
    out = []
    for m in PAIR_MS:
        for dtype in ALL_KINDS:
            a, b = make_rows(8000 + m + dtype.itemsize, dtype, 23, 29, m)
            rng = np.random.default_rng(m)
            ia, ib = np.repeat(np.arange(23), 29), np.tile(np.arange(29), 23)          # every pair, so every pair of pool values
            p = rng.permutation(len(ia))
            out.append({"name": "pairs_%s_m%d" % (dtype.name, m), "dtype": dtype, "m": m, "a": a, "b": b, "ia": ia[p].astype(np.uint64), "ib": ib[p].astype(np.uint64)})
    return out


def many_pairs_case(n_cu, dtype):
    """8 * n_cu * 4 + 5 pairs of m = 5 within one array: more pairs than the grid has wavefronts, repeated pairs and self pairs among them"""
    n, m, rows = 8 * n_cu * 4 + 5, 5, 61
    a, _ = make_rows(9000 + n_cu, dtype, rows, 1, m)
    rng = np.random.default_rng(n)
    ia, ib = rng.integers(0, rows, n).astype(np.uint64), rng.integers(0, rows, n).astype(np.uint64)
    ib[::7] = ia[::7]                                          # self pairs
    ia[-40:], ib[-40:] = ia[:40], ib[:40]                      # repeated pairs, the last wavefronts' among them
    return {"name": "pairs_%s_%d" % (np.dtype(dtype).name, n), "dtype": np.dtype(dtype), "m": m, "a": a, "b": a, "ia": ia, "ib": ib}
