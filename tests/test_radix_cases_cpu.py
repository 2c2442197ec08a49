"""The tables of tests/radix_cases.py without a device: every case holds the property its name promises (so that the GPU test which runs the same
table, tests/test_gpu_radix.py, cannot drift off the edge it is there for), the tables hold the sizes and widths they are meant to, and the references of
tests/pyref_radix.py agree with second definitions."""
import numpy as np

import pyref_radix as R
import radix_cases as RC

U64 = np.uint64


def _by_name(cases):
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return dict(zip(names, cases))


# ---- the references ---------------------------------------------------------------------------------------------------------------------------------
def test_references_against_second_definitions():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 64, 5000, dtype=np.uint64) & U64(0xFFFF00000000FF03)
    for e in (1, 8, 9, 16, 63, 64):
        mask = int(R.sort_mask(e))
        assert mask == (1 << 8 * ((e + 7) // 8)) - 1
        want = [int(k) for _, _, k in sorted(((int(k) & mask), i, int(k)) for i, k in enumerate(keys))]       # by masked key, then by input position
        assert R.sort(keys, e).tolist() == want
    a = np.sort(rng.integers(0, 40, 300).astype(np.uint64))
    u, c = np.unique(a, return_counts=True)
    ru, rl = R.run_lengths(a)
    assert ru.dtype == np.uint64 and rl.dtype == np.uint32 and np.array_equal(ru, u) and np.array_equal(rl, c)
    b = np.array([5, 5, 3, 5, 5, 5], np.uint64)                               # run lengths need no order: neighbours only
    assert [x.tolist() for x in R.run_lengths(b)] == [[5, 3, 5], [2, 1, 3]]
    v = rng.integers(0, 1 << 20, 77).astype(np.uint32)
    s, total = R.scan(v)
    assert s.dtype == np.uint32 and s.tolist() == [int(v[:i].sum()) for i in range(77)] and total == int(v.sum())
    s, total = R.scan(np.zeros(0, np.uint32))
    assert len(s) == 0 and total == 0


# ---- sort ---------------------------------------------------------------------------------------------------------------------------------------------
def test_sort_table_covers_sizes_widths_and_both_result_buffers():
    cases = _by_name(RC.sort_cases())
    assert RC.ENDBITS == (8, 24, 32, 40, 64) and [R.passes(e) for e in RC.ENDBITS] == [1, 3, 4, 5, 8]
    assert {R.passes(e) % 2 for e in RC.ENDBITS} == {0, 1}                       # the result in the second buffer and in the first
    assert RC.SORT_SIZES == (0, 1, 2, 63, 64, 65, 16383, 16384, 16385, 32768, 3 * 16384 + 17)
    for e in RC.ENDBITS:
        for n in RC.SORT_SIZES:
            c = cases["size_%d_e%d" % (n, e)]
            assert len(c["keys"]) == n and c["endbit"] == e and not (c["keys"] & ~R.sort_mask(e)).any()
            if n >= 64:
                assert len(np.unique(c["keys"])) > n // 300                         # uniform over the width (8 bits hold 256 values)
        for group in ("all_equal", "same_digit_pass0", "step_of_64_digits_pass0", "two_digits_alternating", "already_sorted", "reverse_sorted", "extremes_among_others"):
            assert "%s_e%d" % (group, e) in cases
        for group in ("same_digit_top_pass", "step_of_64_digits_top_pass"):
            assert ("%s_e%d" % (group, e) in cases) == (e > 8)
    assert {c["endbit"] for c in cases.values() if "zero_from_endbit" in c["props"]} == {13, 33, 42, 62}
    assert {(len(c["keys"]), c["endbit"]) for c in cases.values() if "index_shift" in c["props"]} == {(n, e) for n in (16385, 3 * 16384 + 17) for e in (32, 8)}
    for c in cases.values():
        assert c["keys"].dtype == np.uint64 and c["keys"].ndim == 1 and c["keys"].flags.c_contiguous and len(c["keys"]) <= 300000
        assert 1 <= c["endbit"] <= 64


def test_sort_cases_hold_their_properties():
    seen = set()
    for c in RC.sort_cases():
        k, e, p, n = c["keys"], c["endbit"], c["props"], len(c["keys"])
        P = R.passes(e)
        seen |= set(p)
        for q in p.get("one_digit_passes", ()):                                    # one LDS counter takes every tile whole, whatever the earlier passes did
            assert q < P and len(np.unique(RC.digit(k, q))) == 1 and n > 2 * RC.TILE
        if "one_digit_passes" in p and len(p["one_digit_passes"]) < P:
            assert len(np.unique(k & R.sort_mask(e))) > 1 and len(np.unique(k)) == n   # different elsewhere, every key its own payload
        if "constant_below" in p:                                                   # the earlier passes are stable sorts of equal digits: the order stays
            low = U64((1 << (8 * p["constant_below"])) - 1)
            assert len(np.unique(k & low)) == 1
        if "distinct_step_pass" in p:
            q = p["distinct_step_pass"]
            assert q == 0 or p.get("constant_below") == q
            d = RC.digit(k, q)
            assert n > RC.TILE + RC.STEP and n % RC.STEP not in (0, 1)              # more than one tile, a ragged last step
            for s in range(0, n, RC.STEP):
                step = d[s:s + RC.STEP]
                assert len(np.unique(step)) == len(step)
            assert len(np.unique(d)) == 64
        if "two_digits" in p:
            for q in range(P):
                assert set(np.unique(RC.digit(k, q)).tolist()) == {0, 255}
            d = RC.digit(k, 0)
            assert (d[1:] != d[:-1]).all() and n > RC.TILE
        if "ascending" in p:
            m = k & R.sort_mask(e)
            assert (m[1:] >= m[:-1]).all() and n > RC.TILE
        if "descending" in p:
            m = k & R.sort_mask(e)
            assert (m[1:] <= m[:-1]).all() and (m[1:] < m[:-1]).any()
        if "extremes" in p:
            lo, hi = p["extremes"]
            assert hi == (1 << (8 * P)) - 1 and lo == 0 and (e != 64 or hi == 2 ** 64 - 1)
            assert (k == U64(lo)).sum() > 10 and (k == U64(hi)).sum() > 10 and len(np.unique(k)) > 250
        if "index_shift" in p:
            sh = p["index_shift"]
            assert sh == e and sh % 8 == 0
            idx, v = k >> U64(sh), k & R.sort_mask(e)
            assert np.array_equal(idx, np.arange(n, dtype=np.uint64))
            vals = np.unique(v)
            assert len(vals) == 7
            # the expected result, said a second way: by value, then by index
            order = np.lexsort((idx, v))
            assert np.array_equal(R.sort(k, e), k[order])
            # one value at least occurs in every tile, and in every tile in both halves of some step
            ok = []
            for val in vals:
                hit = np.zeros(RC.tiles(n) * RC.TILE, bool)
                hit[:n] = v == val
                halves = hit.reshape(-1, 2, RC.STEP // 2).any(axis=2).all(axis=1)       # per step: in both halves
                ok.append(hit.reshape(-1, RC.TILE).any(axis=1).all() and halves.reshape(-1, RC.TILE // RC.STEP)[:n // RC.TILE].any(axis=1).all())
            assert any(ok) and n // RC.TILE >= 1
        if "zero_from_endbit" in p:
            assert e % 8 and not (k >> U64(e)).any() and (k >> U64(e - 1)).any() and n > 2 * RC.TILE
            assert np.array_equal(R.sort(k, e), np.sort(k))                         # with the bits above zero, the order on whole digits is the order on [0, endbit)
        if "hist_stretch" in p:
            assert (n, e) == (17 * 16384 + 5, 16) and RC.tiles(n) == 18 and RC.scan_stretch(256 * RC.tiles(n)) == p["hist_stretch"] == 8
    assert seen == {"one_digit_passes", "distinct_step_pass", "constant_below", "two_digits", "ascending", "descending", "extremes", "index_shift", "zero_from_endbit", "hist_stretch"}


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------------------------
def test_run_length_cases_hold_their_properties():
    cases = _by_name(RC.rle_cases())
    assert RC.RLE_SIZES == (1, 2, 64, 65, 16384, 16385, 65537) and RC.tiles(65537) == 5
    for n in RC.RLE_SIZES:
        assert len(cases["size_%d" % n]["a"]) == n
    seen = set()
    E = RC.TILE
    for c in cases.values():
        a, p, n = c["a"], c["props"], len(c["a"])
        seen |= set(p)
        assert a.dtype == np.uint64 and n >= 1 and (a[1:] >= a[:-1]).all()
        u, ln = R.run_lengths(a)
        assert int(ln.sum()) == n and (len(u) < 2 or (u[1:] > u[:-1]).all())
        if "all_distinct" in p:
            assert len(u) == n == 65537
        if "all_equal" in p:
            assert len(u) == 1 and ln[0] == n == 65537
        if "alternating" in p:
            assert (ln[0::2] == 1).all() and (ln[1::2] >= 2).all() and ln.max() > 250 and n > E
        if "ends_at_edge" in p:
            assert a[E - 1] != a[E] and a[E - 2] == a[E - 1] and a[E] == a[E + 1]
        if "straddles_edge" in p:
            assert a[E - 1] == a[E] and a[E - 101] != a[E - 100] and a[E + 99] != a[E + 100]
        if "straddles_steps" in p:
            assert n == E and all(a[j - 1] == a[j] for j in range(RC.STEP, E, RC.STEP)) and len(u) == E // RC.STEP + 1
        if "long_run" in p:
            heads = np.flatnonzero(a[1:] != a[:-1]) + 1
            assert ln.max() > E and not ((heads >= E) & (heads < 2 * E)).any() and n > 3 * E      # a tile without a single head
        if "high_bits_only" in p:
            assert len(np.unique(a & U64(0xFFFFFFFF))) == 1 and len(u) == 400 and n > E
    assert seen == {"all_distinct", "all_equal", "alternating", "ends_at_edge", "straddles_edge", "straddles_steps", "long_run", "high_bits_only"}


# ---- scan -----------------------------------------------------------------------------------------------------------------------------------------------
def test_scan_cases_reach_the_stretches_they_name():
    cases = _by_name(RC.scan_cases())
    assert RC.SCAN_SIZES == (0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 4100, 256 * 18)
    for n in RC.SCAN_SIZES:
        v = cases["size_%d" % n]["v"]
        assert v.dtype == np.uint32 and len(v) == n and (n == 0 or int(v.max()) < 1 << 20) and int(v.astype(np.uint64).sum()) < 1 << 32
        assert n < 64 or len(np.unique(v)) > n // 2
    assert not cases["all_zeros"]["v"].any() and len(cases["all_zeros"]["v"]) > 4096
    assert (cases["all_ones"]["v"] == 1).all() and len(cases["all_ones"]["v"]) == 256 * 18
    # the stretch of a lane: 4 up to 4096 counts, 8 from 4097 on; at 5 counts (five tiles of run heads) lane 0 has one whole group, lane 1 a ragged one
    assert [RC.scan_stretch(n) for n in (1, 5, 4096, 4097, 4100, 256 * 18)] == [4, 4, 4, 8, 8, 8]
    assert RC.scan_stretch(0) == 0 and RC.scan_stretch(256 * 18) * 576 == 256 * 18          # 576 lanes with work, 448 without
    assert all(RC.scan_stretch(n) * RC.SCAN_LANES >= n for n in range(0, 70000, 7))
