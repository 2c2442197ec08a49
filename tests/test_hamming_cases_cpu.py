"""The case table of tests/hamming_cases.py against itself: every value class and every edge it is there for is present - asserted by counting, so that
a later edit cannot drop one unnoticed -, its numpy reference equals a plain Python loop on the small cases, and equals the CPU oracle bit for bit on
the unpadded ones. No GPU."""
import numpy as np
import pytest

import hamming_cases as HC

N_CU = 256          # for the assertions on the split cases only; the GPU test takes the device's own number


@pytest.fixture(scope="module")
def dense():
    return HC.dense_cases()


@pytest.fixture(scope="module")
def blocks():
    return HC.blocks_cases()


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def class_counts(q, c, m):
    """how many (query, candidate) pairs of one special column realise each value class"""
    cols = HC.special_cols(m)
    x, y = _bits(np.ascontiguousarray(q[:, cols]))[:, None, :], _bits(np.ascontiguousarray(c[:, cols]))[None, :, :]
    n = {}
    if q.dtype == np.float32:
        def pair(a, b):
            return int(((x == a) & (y == b)).sum() + ((x == b) & (y == a)).sum())
        n = {"+0/-0": pair(HC.F_POS0, HC.F_NEG0), "nan/same nan": pair(HC.F_NAN_A, HC.F_NAN_A), "nan/other payload": pair(HC.F_NAN_A, HC.F_NAN_B),
             "snan/snan": pair(HC.F_SNAN, HC.F_SNAN), "snan/nan": pair(HC.F_SNAN, HC.F_NAN_A), "+inf/-inf": pair(HC.F_PINF, HC.F_NINF), "+inf/+inf": pair(HC.F_PINF, HC.F_PINF),
             "denormal/0": pair(HC.F_DEN1, HC.F_POS0), "denormal/next": pair(HC.F_DEN1, HC.F_DEN2), "denormal/itself": pair(HC.F_DEN1, HC.F_DEN1),
             "denormal/-denormal": pair(HC.F_DEN1, HC.F_NDEN1)}
    else:
        d = x ^ y
        top = d.dtype.type(1 << (8 * d.dtype.itemsize - 1))
        n = {"top bit only": int((d == top).sum()), "bit 0 only": int((d == 1).sum()), "equal": int((d == 0).sum())}
        if q.dtype == np.uint64:
            lo = np.uint64(0xFFFFFFFF)
            n.update({"above bit 31 only": int(((d != 0) & (d & lo == 0)).sum()), "below bit 32 only": int(((d != 0) & (d >> np.uint64(32) == 0)).sum()),
                      "bit 32 only": int((d == np.uint64(1 << 32)).sum()), "bit 31 only": int((d == np.uint64(1 << 31)).sum())})
    return n


def _sum(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


CLASSES = {2: {"top bit only", "bit 0 only", "equal"}, 4: {"top bit only", "bit 0 only", "equal"}, 8: {"top bit only", "bit 0 only", "equal", "above bit 31 only", "below bit 32 only", "bit 32 only", "bit 31 only"}}
F32_CLASSES = {"+0/-0", "nan/same nan", "nan/other payload", "snan/snan", "snan/nan", "+inf/-inf", "+inf/+inf", "denormal/0", "denormal/next", "denormal/itself",
               "denormal/-denormal"}


def _want_classes(dtype):
    return F32_CLASSES if dtype == np.float32 else CLASSES[dtype.itemsize]


def test_reference_semantics():
    """numpy's `!=` is the operation: IEEE on float32 bit patterns, denormals kept apart"""
    f = HC.F32_POOL.view(np.float32)
    ne = f[:, None] != f[None, :]
    i = {v: k for k, v in enumerate(HC.F32_POOL.tolist())}
    for a in (HC.F_NAN_A, HC.F_NAN_B, HC.F_SNAN):
        assert ne[i[a]].all() and ne[:, i[a]].all()
    assert not ne[i[HC.F_POS0], i[HC.F_NEG0]] and ne[i[HC.F_DEN1], i[HC.F_POS0]] and ne[i[HC.F_DEN1], i[HC.F_DEN2]] and not ne[i[HC.F_DEN1], i[HC.F_DEN1]]
    assert ne[i[HC.F_DEN1], i[HC.F_NDEN1]] and ne[i[HC.F_PINF], i[HC.F_NINF]] and not ne[i[HC.F_PINF], i[HC.F_PINF]]
    assert HC.distances(np.array([3]), 7)[0] == np.float32(3) / np.float32(7) and HC.distances(np.array([3]), 7).dtype == np.float32


def test_dense_table_covers_shapes_sizes_pitches_and_shifts(dense):
    main = [c for c in dense if not c["name"].startswith("split_") and c["m"] != 65535]
    for m in HC.MS:
        assert len({(c["nq"], c["nc"]) for c in main if c["m"] == m}) >= 2, m
    for dtype in HC.KINDS:
        mine = [c for c in main if c["dtype"] == dtype]
        for s in HC.SHAPES:
            assert {33, 257} <= {c["m"] for c in mine if (c["nq"], c["nc"]) == s}, (dtype, s)
        assert {m for c in mine for m in [c["m"]]} == set(HC.MS)
        assert {c["stride"] for c in mine} == set(HC.STRIDES) and {c["shift"] for c in mine} == set(HC.SHIFTS[dtype.itemsize]), dtype
        # 16-byte loads with a word tail (aligned rows, m no multiple of 4), and both ways of forbidding them
        assert sum(1 for c in mine if HC.dense_vec4(c) and HC.row_words(dtype, c["m"]) % 4) >= 3, dtype
        assert any(c["stride"] == "plus4" and c["shift"] == 0 for c in mine) and any(c["stride"] in ("r16", "r256") and c["shift"] for c in mine), dtype
        assert any(c["stride_bytes"] > c["m"] * dtype.itemsize for c in mine if c["stride"] == "r256")
        assert any(c["nq"] > 2 * HC.HT for c in mine) and any(c["nc"] > HC.HT for c in mine)
    assert max(c["nq"] * c["nc"] * c["m"] for c in dense) <= 260 * 260 * 515
    assert len({c["name"] for c in dense}) == len(dense)
    big = [c for c in dense if c["m"] == 65535]
    assert len(big) == 1 and (HC.counts(big[0]["q"], big[0]["c"], 65535) == 65535).all() and big[0]["nq"] == big[0]["nc"] == 2


def test_dense_table_holds_every_value_class(dense):
    for dtype in HC.KINDS:
        mine = [c for c in dense if c["dtype"] == dtype and c["m"] != 65535]
        got = _sum(class_counts(c["q"], c["c"], c["m"]) for c in mine)
        assert set(got) == _want_classes(dtype) and all(v >= 20 for v in got.values()), (dtype, got)
        for col in (0, 31, 32, 255, 256):
            assert any(col in HC.special_cols(c["m"]) and c["m"] - 1 != col for c in mine), col
        # identical rows, all-different rows, all-NaN rows
        ident = diff = nan = 0
        for c in mine:
            cnt = HC.counts(c["q"], c["c"], c["m"])
            if c["nq"] >= 2 and c["nc"] >= 2:
                assert cnt[0, 0] == 0, c["name"]
                ident += 1
            if c["nq"] >= 3:
                assert (cnt[-1] == c["m"]).all(), c["name"]
                diff += 1
            if c["nc"] >= 3 and dtype == np.float32:
                assert (cnt[:, -1] == c["m"]).all() and np.isnan(c["c"][-1]).all(), c["name"]
                nan += 1
            assert 0 < cnt.sum() or c["nq"] * c["nc"] == 1
        assert ident >= 10 and diff >= 10 and (nan >= 10 or dtype != np.float32)
    # the alphabets themselves: u64 values of one column differ in one word only, so that half a compare shows in every slot
    c = next(c for c in dense if c["dtype"] == np.uint64 and c["m"] == 257 and c["nq"] == 128)
    d = c["q"][:, None, 1:31] ^ c["c"][None, :, 1:31]
    lo = np.uint64(0xFFFFFFFF)
    assert ((d != 0) & (d & lo == 0)).sum() > 1000 and ((d != 0) & (d >> np.uint64(32) == 0)).sum() > 1000


def test_padding_is_garbage_and_rows_are_in_place(dense):
    for c in dense:
        roww = HC.row_words(c["dtype"], c["m"])
        for rows, words in ((c["q"], c["qw"]), (c["c"], c["cw"])):
            assert words.dtype == np.uint32 and words.shape == (len(rows), c["stride_bytes"] // 4) and c["stride_bytes"] % 4 == 0
            assert np.array_equal(words[:, :roww], _bits(rows).view(np.uint32).reshape(len(rows), roww))
            pad = words[:, roww:]
            assert (pad != 0).all()
            if pad.shape[1] and len(rows) > 1:
                assert (pad[0] != pad[1]).any()


def test_split_cases_split(dense):
    split = [c for c in dense if c["name"].startswith("split_")]
    assert len(split) == 2 * (5 + 5 + 2)
    shorter = 0
    for c in split:
        roww, tiles = HC.row_words(c["dtype"], c["m"]), HC.dense_tiles(c)
        assert tiles in (1, 4) and roww in (256, 257, 300, 515, 1023)
        ks, parts = HC.split_rule(N_CU, tiles, np.array([roww]), 0)
        assert parts[0] > 1
        shorter += roww % ks[0] != 0
    assert shorter >= 1 and {HC.dense_tiles(c) for c in split} == {1, 4}
    # under 256 row words nothing splits; the main table has such cases and ones that do
    main = [c for c in dense if not c["name"].startswith("split_")]
    parts = [HC.split_parts(N_CU, HC.dense_tiles(c), HC.row_words(c["dtype"], c["m"]), 0) for c in main]
    assert all(p == 1 for c, p in zip(main, parts) if HC.row_words(c["dtype"], c["m"]) < 256)
    assert sum(p == 1 for p in parts) > 20 and sum(p > 1 for p in parts) > 5


def test_work_lists(blocks):
    assert len({c["name"] for c in blocks}) == len(blocks)
    assert {len(c["items"]) for c in blocks} == {1, 3, 30}
    thin_ms, tile_thin = set(), 0
    for c in blocks:
        items, ql, cl = c["items"], c["qlist"], c["clist"]
        for lst, n in ((ql, c["nq_rows"]), (cl, c["nc_rows"])):
            assert len(np.unique(lst)) == len(lst) < n and lst.max() < n and (np.diff(lst.astype(np.int64)) < 0).any()       # a strict subset, each row once, not sorted
        assert (items[:, 0] + items[:, 1] <= len(ql)).all() and (items[:, 2] + items[:, 3] <= len(cl)).all()
        assert (items[:, 1] >= 1).all() and (items[:, 1] <= HC.HT).all() and (items[:, 3] >= 1).all() and (items[:, 3] <= HC.HT).all()
        e = c["eligible"]
        assert (items[:e, 1] <= HC.HTQ).all() and (items[e:, 1] > HC.HTQ).all() and max(c["n_thin"]) == e and min(c["n_thin"]) == 0
        want, named = HC.blocks_expected(c, HC.LDS[1])                      # asserts that no two items name one cell
        assert named.sum() == int((items[:, 1] * items[:, 3]).sum())
        if len(items) == 30:
            assert set(HC.ITEM_SHAPES) <= {(int(a), int(b)) for a, b in items[:, [1, 3]]}
            assert {-(-int(r) // 16) for r in items[:, 1]} == set(range(1, 9))
            assert len(c["n_thin"]) == 3
        if len(items) >= 3:
            # the pair: every cell of one item has its neighbour (column ^ 1) in the other; and cells whose neighbour no item names
            owner = np.full(named.shape, -1)
            for k, (q0, qr, c0, cr) in enumerate(items.tolist()):
                owner[np.ix_(ql[q0:q0 + qr], cl[c0:c0 + cr])] = k
            cols = np.arange(named.shape[1] - 1) ^ 1
            nb = owner[:, :-1][:, cols]
            mine = owner[:, :-1]
            assert ((mine >= 0) & (nb >= 0) & (mine != nb)).sum() >= 2 * HC.HTQ * HC.PAIR_COLS
            assert ((mine >= 0) & (nb < 0)).sum() > 50
        if c["name"].startswith("thin_"):
            assert HC.blocks_vec4(c) and c["dtype"].itemsize == 4
            thin_ms.add((c["dtype"].name, c["m"]))
            rows = np.concatenate([ql[q0:q0 + qr] for q0, qr, _, _ in items[:e].tolist()])
            cols_ = np.concatenate([cl[c0:c0 + cr] for _, _, c0, cr in items[:e].tolist()])
            got = class_counts(c["q"][rows], c["c"][cols_], c["m"])
            assert set(got) == _want_classes(c["dtype"]) and all(v >= 5 for v in got.values()), (c["name"], got)
        if c["name"].startswith("tile_"):
            assert not HC.blocks_vec4(c) or c["dtype"].itemsize == 8 or c["stride"] == "row"
            tile_thin += HC.blocks_left(c, e) == len(items)
    assert thin_ms == {(k, m) for k in ("float32", "uint32") for m in HC.THIN_MS}
    assert {m % 4 for m in HC.THIN_MS} == {0, 1, 2, 3} and {m <= 256 for m in HC.THIN_MS} == {True, False} and 256 in HC.THIN_MS and 257 in HC.THIN_MS
    assert tile_thin >= 6 and HC.LDS[0] % 2 == 0 and HC.LDS[1] % 2 == 1 and min(HC.LDS) >= HC.NC_ROWS
    # with 256 compute units: lists of 1, 3 and 30 items split from 256 row words on, and what is left after the thin kernel decides
    for c in blocks:
        roww = HC.row_words(c["dtype"], c["m"])
        for nt in c["n_thin"]:
            left = HC.blocks_left(c, nt)
            parts = HC.split_parts(N_CU, left, roww, 1) if left else 1
            assert (parts > 1) == (left > 0 and roww >= 256), (c["name"], nt)
    long = HC.long_list_case(N_CU + 1, 256)
    assert len(long["items"]) == N_CU + 1 and HC.split_parts(N_CU, N_CU + 1, 256, 1) == 1 and HC.split_parts(N_CU, N_CU, 256, 1) > 1
    HC.blocks_expected(long, long["nc_rows"] + 1)


def test_public_call_cases():
    qx, pr = HC.qxc_cases(), HC.pairs_cases()
    assert {(c["q"].shape[0], c["c"].shape[0]) for c in qx} == {(129, 257), (257, 129)} and {c["dtype"] for c in qx} == set(HC.ALL_KINDS)
    assert {(c["dtype"], c["m"]) for c in pr} == {(d, m) for d in HC.ALL_KINDS for m in HC.PAIR_MS}
    for dtype in HC.ALL_KINDS:                              # u16 among them: bit 15 alone, bit 0 alone
        for c in pr:                                        # every pair of rows is asked for, so every pair of pool values at a special column is
            if c["dtype"] == dtype:
                assert len(set(zip(c["ia"].tolist(), c["ib"].tolist()))) == len(c["a"]) * len(c["b"])
        for table, rows in ((pr, ("a", "b")), (qx, ("q", "c"))):
            got = _sum(class_counts(c[rows[0]], c[rows[1]], c["m"]) for c in table if c["dtype"] == dtype)
            assert set(got) == _want_classes(dtype) and all(v >= 5 for v in got.values()), (dtype, got)
    many = HC.many_pairs_case(N_CU, np.uint32)
    n = len(many["ia"])
    assert n == 8 * N_CU * 4 + 5 and many["m"] == 5 and (many["ia"] == many["ib"]).sum() >= n // 7
    assert len(set(zip(many["ia"].tolist(), many["ib"].tolist()))) < n and many["a"] is many["b"]


def test_numpy_reference_equals_a_python_loop(dense, blocks):
    n = 0
    for c in dense:
        if c["nq"] * c["nc"] * c["m"] <= 40000:
            assert np.array_equal(HC.counts(c["q"], c["c"], c["m"]), HC.counts_python(c["q"], c["c"], c["m"])), c["name"]
            n += 1
    assert n >= 40
    c = blocks[0]
    rows, cols = c["qlist"][:20], c["clist"][:30]
    assert np.array_equal(HC.counts(c["q"][rows], c["c"][cols], c["m"]), HC.counts_python(c["q"][rows], c["c"][cols], c["m"]))
    for c in HC.pairs_cases()[:8]:
        ia, ib = c["ia"].astype(np.int64), c["ib"].astype(np.int64)
        full = HC.counts_python(c["a"], c["b"], c["m"])
        assert np.array_equal(HC.pair_counts(c["a"], c["b"], ia, ib), full[ia, ib]), c["name"]


def test_numpy_reference_equals_the_oracle(dense):
    import oracle_lib as O
    n = 0
    for c in dense:
        if c["stride"] == "row":
            want = HC.distances(HC.counts(c["q"], c["c"], c["m"]), c["m"])
            got = O.hamming_qxc(c["q"], c["c"])
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)), c["name"]
            n += 1
    assert n >= 20
    for c in HC.qxc_cases():
        want = HC.distances(HC.counts(c["q"], c["c"], c["m"]), c["m"])
        assert np.array_equal(O.hamming_qxc(c["q"], c["c"]).view(np.uint32), want.view(np.uint32)), c["name"]
    for c in HC.pairs_cases() + [HC.many_pairs_case(N_CU, np.float32)]:
        ia, ib = c["ia"].astype(np.int64), c["ib"].astype(np.int64)
        want = HC.distances(HC.pair_counts(c["a"], c["b"], ia, ib), c["m"])
        assert np.array_equal(O.hamming_pairs(c["a"], c["b"], c["ia"], c["ib"]).view(np.uint32), want.view(np.uint32)), c["name"]
