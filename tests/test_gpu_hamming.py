"""The DistHamming compare kernels of gs_hamming.hip against numpy (tests/hamming_cases.py), == on every cell: the dense driver with its three output
forms and its K-split of the 32-bit count form (gs_debug_hamming_strided), the work-list driver with the thin kernel, the tile kernel's THIN path and
the K-split that takes matches off through 32-bit containers (gs_debug_hamming_blocks), and the public calls (eval_qxc, eval_pairs). Every distance of
the library comes from these kernels, and the index reaches them only at the shapes its clustering happens to produce. The shapes here are the
kernels' own edges, built and held to their names in tests/hamming_cases.py / tests/test_hamming_cases_cpu.py. Every output starts as 0xFF bytes in
its whole pitch: a cell the call does not own must come back as it was. The number of K parts each call reports is held to the rule restated in
hamming_cases.split_rule, with the device's own number of compute units. Every table runs with the fill off and on scratch filled with 0x00 and 0xFF."""
import ctypes as C
import os

import numpy as np
import pytest

import hamming_cases as HC

pytestmark = pytest.mark.gpu
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3
KIND_U16, KIND_U32, KIND_U64, KIND_F32 = 0, 1, 2, 3
FILLS = [None, 0x00, 0xFF]
FORM_DTYPE = (np.float32, np.uint32, np.uint16)


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    g, w = got.reshape(-1).view("u%d" % got.dtype.itemsize), want.reshape(-1).view("u%d" % want.dtype.itemsize)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d cells differ, the first at row %d column %d (got %#x, want %#x)" % (tag, len(bad), len(w), i // got.shape[-1], i % got.shape[-1],
                                                                                                            int(g[i]), int(w[i])))


class Tally:
    """runs every case before it fails: the list of the cases that differ says which kernel and which edge broke"""
    def __init__(self):
        self.n, self.bad = 0, []

    def check(self, fn, *a):
        self.n += 1
        try:
            fn(*a)
        except AssertionError as e:
            self.bad.append(str(e).split("\n")[0][:160])

    def done(self):
        assert not self.bad, "%d of %d runs differ: %s" % (len(self.bad), self.n, "; ".join(self.bad[:40]))


def _eq(got, want, tag):
    assert got == want, "%s: %r, want %r" % (tag, got, want)


def _canary(shape, dtype):
    return np.full(shape, 0xFF, np.uint8).repeat(np.dtype(dtype).itemsize, axis=-1).view(dtype).reshape(shape)


def _dense_want(cnt, m, form, ld):
    want = _canary((cnt.shape[0], ld), FORM_DTYPE[form])
    want[:, :cnt.shape[1]] = HC.distances(cnt, m) if form == 0 else cnt.astype(FORM_DTYPE[form])
    return want


@pytest.fixture(scope="module")
def n_cu(gpu_ctx):
    return gpu_ctx.device_info()["n_cu"]


@pytest.fixture(scope="module")
def dense_table():
    return [(c, HC.counts(c["q"], c["c"], c["m"])) for c in HC.dense_cases()]


@pytest.fixture(scope="module")
def blocks_table():
    return [(c, [HC.blocks_expected(c, ld)[0] for ld in HC.LDS]) for c in HC.blocks_cases()]


@pytest.mark.parametrize("fill", FILLS)
def test_dense_cases(gpu_ctx, n_cu, dense_table, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    parts_seen, t = {0: set(), 1: set(), 2: set()}, Tally()
    try:
        for case, cnt in dense_table:
            m, nc = case["m"], case["nc"]
            qw, cw = case["qw"].copy(), case["cw"].copy()
            for form in (0, 1, 2):
                for ld in (nc, nc + 3):
                    out = _canary((case["nq"], ld), FORM_DTYPE[form])
                    parts = G.debug_hamming_strided(qw, cw, m, out, form, shift_bytes=case["shift"], dtype=case["dtype"], ctx=gpu_ctx)
                    tag = "%s form %d ld %d" % (case["name"], form, ld)
                    t.check(_same, out, _dense_want(cnt, m, form, ld), tag)
                    want_parts = HC.split_parts(n_cu, HC.dense_tiles(case), HC.row_words(case["dtype"], m), 0) if form == 1 else 1
                    t.check(_eq, parts, want_parts, tag + " parts")
                    if HC.row_words(case["dtype"], m) < 8 * HC.HKW:
                        assert parts == 1, tag
                    if case["name"].startswith("split_") and form == 1:
                        assert parts > 1, tag
                    parts_seen[form].add(parts > 1)
            assert np.array_equal(qw, case["qw"]) and np.array_equal(cw, case["cw"]), case["name"]       # the inputs are left alone
    finally:
        G.debug_mem_fill(None)
    t.done()
    assert parts_seen == {0: {False}, 1: {False, True}, 2: {False}}          # the split and the unsplit form of the 32-bit counts both ran


def _run_blocks(G, ctx, case, n_thin, ld):
    out = _canary((case["nq_rows"], ld), np.uint16)
    parts = G.debug_hamming_blocks(case["qw"], case["cw"], case["m"], case["items"], case["qlist"], case["clist"], n_thin, out, dtype=case["dtype"], ctx=ctx)
    return out, parts


@pytest.mark.parametrize("fill", FILLS)
def test_work_list_cases(gpu_ctx, n_cu, blocks_table, fill):
    import gsearch_amd as G
    assert "GS_BLOCKS_THIN_OFF" not in os.environ
    G.debug_mem_fill(fill)
    seen, t = set(), Tally()
    try:
        for case, wants in blocks_table:
            roww = HC.row_words(case["dtype"], case["m"])
            for n_thin in case["n_thin"]:
                for ld, want in zip(HC.LDS, wants):             # an even and an odd pitch: the parity of a cell's index flips from row to row, or does not
                    tag = "%s n_thin %d ld %d" % (case["name"], n_thin, ld)
                    out, parts = _run_blocks(G, gpu_ctx, case, n_thin, ld)
                    t.check(_same, out, want, tag)
                    left = HC.blocks_left(case, n_thin)
                    want_parts = HC.split_parts(n_cu, left, roww, 1) if left else 1
                    t.check(_eq, parts, want_parts, tag + " parts")
                    seen.add((len(case["items"]), left < len(case["items"]), parts > 1, ld % 2))
                    if n_thin:                      # the same list without the thin kernel: the same matrix
                        os.environ["GS_BLOCKS_THIN_OFF"] = "1"
                        try:
                            out_off, parts_off = _run_blocks(G, gpu_ctx, case, n_thin, ld)
                        finally:
                            del os.environ["GS_BLOCKS_THIN_OFF"]
                        t.check(_same, out_off, want, tag + " thin off")
                        t.check(_eq, parts_off, HC.split_parts(n_cu, len(case["items"]), roww, 1), tag + " thin off parts")
        # more items than compute units: no split, whatever the row length
        for m in (4, 256):
            case = HC.long_list_case(n_cu + 1, m)
            for ld in (case["nc_rows"], case["nc_rows"] + 1):
                out, parts = _run_blocks(G, gpu_ctx, case, 0, ld)
                t.check(_same, out, HC.blocks_expected(case, ld)[0], case["name"])
                t.check(_eq, parts, 1, case["name"] + " parts")
    finally:
        G.debug_mem_fill(None)
    t.done()
    # lists of 1, 3 and 30 items ran split, the thin kernel ran in front of a split and of an unsplit tile run, with an even and an odd pitch
    for n in (1, 3, 30):
        assert {(n, False, True, 0), (n, False, True, 1)} <= seen, (n, seen)
    assert {(30, True, True), (30, True, False)} <= {s[:3] for s in seen}, seen


@pytest.mark.parametrize("fill", FILLS)
def test_public_calls(gpu_ctx, n_cu, fill):
    """eval_qxc and eval_pairs stage through slots of their own, the u16 forms through the widened copies besides"""
    import gsearch_amd as G
    D, t = G.DistHamming(gpu_ctx), Tally()
    many = [HC.many_pairs_case(n_cu, dt) for dt in HC.ALL_KINDS]
    assert all(len(c["ia"]) > n_cu * 8 * 4 for c in many)                   # more pairs than the grid of k_hamming_pairs has wavefronts
    G.debug_mem_fill(fill)
    try:
        for c in HC.qxc_cases():
            q, cc = c["q"].copy(), c["c"].copy()
            t.check(_same, D.eval_qxc(q, cc), HC.distances(HC.counts(c["q"], c["c"], c["m"]), c["m"]), c["name"])
            assert np.array_equal(q.view(np.uint8), c["q"].view(np.uint8)) and np.array_equal(cc.view(np.uint8), c["c"].view(np.uint8)), c["name"]
        for c in HC.pairs_cases() + many:
            ia, ib = c["ia"].astype(np.int64), c["ib"].astype(np.int64)
            t.check(_same, D.eval_pairs(c["a"], c["b"], c["ia"], c["ib"]), HC.distances(HC.pair_counts(c["a"], c["b"], ia, ib), c["m"]), c["name"])
    finally:
        G.debug_mem_fill(None)
    t.done()


def test_error_codes_and_the_empty_calls(gpu_ctx):
    L, h = gpu_ctx.L, gpu_ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    q, c = np.arange(12, dtype=np.uint32).reshape(3, 4), np.arange(8, dtype=np.uint32).reshape(2, 4)
    out = _canary((3, 2), np.uint32)
    parts = C.c_uint32(77)
    pp = C.byref(parts)

    def strided(ctx=h, kind=KIND_U32, m=4, Q=q, nq=3, sq=16, Cm=c, nc=2, sc=16, shift=0, form=1, o=out, ld=2, po=pp):
        return L.gs_debug_hamming_strided(ctx, kind, m, None if Q is None else p(Q), nq, sq, None if Cm is None else p(Cm), nc, sc, shift, form, None if o is None else p(o), ld, po)
    for bad in (dict(ctx=None), dict(Q=None), dict(Cm=None), dict(o=None), dict(po=None), dict(m=0), dict(form=3), dict(form=-1), dict(ld=1), dict(shift=256), dict(shift=2),
                dict(sq=12), dict(sc=12), dict(sq=18), dict(form=2, m=65536, sq=1 << 18, sc=1 << 18)):
        assert strided(**bad) == GS_ERR_INVALID, bad
    assert strided(kind=KIND_U64, shift=4) == GS_ERR_INVALID                 # a shift of half an element
    assert strided(kind=KIND_U16) == GS_ERR_UNSUPPORTED and strided(kind=7) == GS_ERR_UNSUPPORTED
    for big in (dict(nq=1 << 24), dict(nc=1 << 24), dict(ld=1 << 24), dict(sq=1 << 32), dict(sc=1 << 32), dict(sq=1 << 31), dict(sq=(1 << 64) - 4), dict(sc=(1 << 63) + 16)):
        assert strided(**big) == GS_ERR_UNSUPPORTED, big                     # sizes whose products would wrap, or operands beyond 4 GB: refused before anything is read
    assert (out == 0xFFFFFFFF).all()
    # n = 0: GS_OK, one part, nothing written (null operands will do)
    for empty in (dict(nq=0), dict(nc=0), dict(nq=0, Q=None, Cm=None, o=None)):
        parts.value = 77
        assert strided(**empty) == 0 and parts.value == 1 and (out == 0xFFFFFFFF).all(), empty
    assert strided() == 0 and parts.value == 1 and np.array_equal(out, HC.counts(q, c, 4).astype(np.uint32))

    items = np.array([[0, 2, 0, 2]], np.uint32)
    ql, cl = np.array([2, 0], np.uint32), np.array([1, 0], np.uint32)
    out16 = _canary((3, 3), np.uint16)

    def blocks(ctx=h, kind=KIND_U32, m=4, Q=q, nqr=3, sq=16, Cm=c, ncr=2, sc=16, it=items, n=1, qlist=ql, nql=2, clist=cl, ncl=2, n_thin=0, o=out16, ld=3, po=pp):
        f = lambda a: None if a is None else p(a)      # noqa: E731
        return L.gs_debug_hamming_blocks(ctx, kind, m, f(Q), nqr, sq, f(Cm), ncr, sc, f(it), n, f(qlist), nql, f(clist), ncl, n_thin, f(o), ld, po)
    tall = np.array([[0, 17, 0, 1]], np.uint32)
    wide = np.array([[0, 129, 0, 1]], np.uint32)
    many_q = np.zeros(200, np.uint32)
    for bad in (dict(ctx=None), dict(Q=None), dict(Cm=None), dict(it=None), dict(qlist=None), dict(clist=None), dict(o=None), dict(po=None), dict(m=0), dict(m=65536, sq=1 << 18, sc=1 << 18),
                dict(n_thin=2), dict(ld=1), dict(sq=12), dict(sc=18),
                dict(it=np.array([[1, 2, 0, 2]], np.uint32)), dict(it=np.array([[0, 2, 1, 2]], np.uint32)),                     # ranges that leave the lists
                dict(it=np.array([[0xFFFFFFFF, 2, 0, 2]], np.uint32)),
                dict(it=np.array([[0, 0, 0, 2]], np.uint32)), dict(it=np.array([[0, 2, 0, 0]], np.uint32)),                     # no rows
                dict(it=wide, qlist=many_q, nql=200, n_thin=0), dict(it=wide[:, [2, 3, 0, 1]], clist=many_q, ncl=200),          # more than 128 rows
                dict(it=tall, qlist=many_q, nql=200, n_thin=1),                                                                 # a thin item of 17 rows
                dict(qlist=np.array([3, 0], np.uint32)), dict(clist=np.array([1, 2], np.uint32))):                               # list entries that are no rows
        assert blocks(**bad) == GS_ERR_INVALID, bad
    assert blocks(kind=KIND_U16) == GS_ERR_UNSUPPORTED
    for big in (dict(nqr=1 << 24), dict(ncr=1 << 24, ld=1 << 24), dict(nql=1 << 24), dict(ncl=1 << 24), dict(sq=1 << 32), dict(sc=(1 << 64) - 4), dict(sq=1 << 31)):
        assert blocks(**big) == GS_ERR_UNSUPPORTED, big
    assert (out16 == 0xFFFF).all()
    for empty in (dict(n=0), dict(n=0, Q=None, Cm=None, it=None, qlist=None, clist=None, o=None, nql=0, ncl=0)):
        parts.value = 77
        assert blocks(**empty) == 0 and parts.value == 1 and (out16 == 0xFFFF).all(), empty
    assert blocks() == 0 and parts.value == 1
    want = _canary((3, 3), np.uint16)
    want[np.ix_(ql, cl)] = HC.counts(q[ql], c[cl], 4)
    assert np.array_equal(out16, want)
