"""gs_index_search_merge_dev, its host twin gs_index_search_merge and gs_topk_reset_dev (gs_split.hip, SPEC 17 item 17) against tests/pyref_split.py on
every word of the running lists.

Three pieces of 256-slot signatures: 90 points, 3 points (fewer than most knbn: short counts, +inf padding) and 70 points of which 30 are copies of
points of the first piece (equal distances in both lists: the order falls to the id). The third piece carries DESCENDING caller ids, so that the
search's own tie order (node number) is not the id order the merge asks for. The id offsets are 0, 2^32 + 5 and 2^33. The answers a piece gives to
the listed rows are taken from Hnsw.search_arrays on those rows (held to the oracle by tests/test_gpu_parity.py); what is under test is everything
after them."""
import numpy as np
import pytest

import helpers as H
import pyref_split as RS

pytestmark = pytest.mark.gpu

M, NBNG, EFC = 256, 8, 32
OFFSETS = (0, (1 << 32) + 5, 1 << 33)
KNBNS = (1, 2, 50, 63, 64, 65, 1024)
NQS = (1, 65, 300)
ROWS = ("none", "empty", "one", "every_other", "all")


def _rows(kind, nq):
    return {"none": None, "empty": np.zeros(0, np.uint32), "one": np.array([nq // 2], np.uint32), "every_other": np.arange(0, nq, 2, dtype=np.uint32),
            "all": np.arange(nq, dtype=np.uint32)}[kind]


def _ef(knbn):
    return max(knbn, 64)


class Dev:
    """device copies of running lists (and whatever else a case uploads), freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.alloc(max(a.nbytes, 8))
        self.bufs.append(p)
        if a.nbytes:
            self.ctx.upload(p, a)
        return p

    def free(self):
        while self.bufs:
            self.ctx.free(self.bufs.pop())


@pytest.fixture(scope="module")
def world(gpu_ctx):
    import gsearch_amd as G

    class W:
        pass
    w = W()
    base = H.synth_sig_db(1, 90, M, 5)                                            # 90 points of one family: lists that fill
    other = H.synth_sig_db(1, 40, M, 6)
    sigs = [base, H.synth_sig_db(1, 3, M, 7), np.concatenate([other, base[10:40]])]
    ids = [None, None, np.arange(len(sigs[2]), dtype=np.uint64)[::-1].copy()]
    w.pieces = []
    for s, i in zip(sigs, ids):
        hn = G.Hnsw.new(NBNG, 1000, 16, EFC, G.DistHamming(), seed=3)
        hn.parallel_insert(s, ids=i)
        w.pieces.append(hn)
    w.queries = H.queries_from(np.concatenate(sigs), max(NQS), 11)
    w.ctx, w.cache = gpu_ctx, {}

    def answers(p, knbn, nq, kind):
        """what piece p answers to the listed rows of the first nq queries"""
        key = (p, knbn, nq, kind)
        if key not in w.cache:
            rows = _rows(kind, nq)
            q = w.queries[:nq] if rows is None else w.queries[:nq][rows.astype(np.int64)]
            w.cache[key] = w.pieces[p].search_arrays(q, knbn, _ef(knbn)) if len(q) else (np.zeros((0, knbn), np.uint64), np.zeros((0, knbn), np.float32),
                                                                                            np.zeros(0, np.uint32), np.zeros(0, np.uint64))
        return w.cache[key]
    w.answers = answers
    yield w
    for hn in w.pieces:
        hn.close()


def _same(got, want):
    return all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(x).view(np.uint8)) for g, x in zip(got, want)) and len(got) == len(want)


def _fold_dev(w, knbn, nq, kind, ctx=None, poke=None):
    """reset, then the three pieces in turn through the device form -> the four arrays"""
    import gsearch_amd as G
    ctx = ctx or w.ctx
    dev = Dev(ctx)
    try:
        d_q = dev.up(w.queries[:nq])
        garbage = (np.full((nq, knbn), 123, np.uint64), np.full((nq, knbn), 0.5, np.float32), np.full(nq, 77, np.uint32), np.full(nq, 99, np.uint64))
        d_run = [dev.up(a) for a in garbage]
        G.topk_reset_dev(ctx, nq, knbn, *d_run)
        rows = _rows(kind, nq)
        d_rows = None if rows is None else dev.up(rows)
        for p, hn in enumerate(w.pieces):
            if poke:
                poke(hn)
            hn.search_merge_dev(d_q, nq, knbn, _ef(knbn), *d_run, d_rows=d_rows, nr=0 if rows is None else len(rows), id_offset=OFFSETS[p])
        return (ctx.download(d_run[0], (nq, knbn), np.uint64), ctx.download(d_run[1], (nq, knbn), np.float32), ctx.download(d_run[2], (nq,), np.uint32),
                ctx.download(d_run[3], (nq,), np.uint64))
    finally:
        dev.free()


def _fold_ref(w, knbn, nq, kind):
    run = RS.empty_lists(nq, knbn)
    for p in range(len(w.pieces)):
        run = RS.merge_rows(run, w.answers(p, knbn, nq, kind), _rows(kind, nq), OFFSETS[p])
    return run


@pytest.mark.parametrize("kind", ROWS)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("knbn", KNBNS)
def test_three_pieces_folded_in_turn_equal_the_restatement(world, knbn, nq, kind):
    w = world
    want = _fold_ref(w, knbn, nq, kind)
    got = _fold_dev(w, knbn, nq, kind)
    assert _same(got, want)
    run = RS.empty_lists(nq, knbn)
    for p, hn in enumerate(w.pieces):
        hn.search_merge(w.queries[:nq], knbn, _ef(knbn), *run, rows=_rows(kind, nq), id_offset=OFFSETS[p])
    assert _same(run, want)
    if kind == "all" and nq == 300:                                                # the case is what it claims
        ids, dist, cnt, _ = want
        assert (cnt == min(knbn, 163)).any() or knbn > 65                         # lists that fill, and cut the merge at knbn
        assert int(ids[ids != RS.NOID].max()) >= 1 << 33 and np.isinf(dist[cnt < knbn][:, -1]).all()
        if knbn >= 50:
            real = [(int(dist[q, j].view(np.uint32)), int(ids[q, j])) for q in range(nq) for j in range(int(cnt[q]))]
            across = sum(1 for a, b in zip(real, real[1:]) if a[0] == b[0] and a[1] < (1 << 32) <= b[1])
            assert across > 0                                                       # equal distances met across two pieces' lists


def test_the_third_piece_ties_inside_one_answer_are_not_in_id_order(world):
    """why the kernel puts a piece's answers in (distance, id) order first: with descending caller ids, equal distances come out of the search
    in node order, the larger id first"""
    ids, dist, cnt, _ = world.answers(2, 50, 300, "all")
    assert any(dist[q, j] == dist[q, j + 1] and ids[q, j] > ids[q, j + 1] for q in range(300) for j in range(int(cnt[q]) - 1))


def test_unlisted_rows_of_filled_lists_stay_byte_identical(world):
    w, knbn, nq = world, 50, 65
    before = RS.merge_rows(RS.empty_lists(nq, knbn), w.answers(0, knbn, nq, "all"), None, OFFSETS[0])
    rows = _rows("every_other", nq)
    want = RS.merge_rows(before, w.answers(1, knbn, nq, "every_other"), rows, OFFSETS[1])
    dev = Dev(w.ctx)
    try:
        d_q, d_rows = dev.up(w.queries[:nq]), dev.up(rows)
        d_run = [dev.up(a) for a in before]
        w.pieces[1].search_merge_dev(d_q, nq, knbn, _ef(knbn), *d_run, d_rows=d_rows, nr=len(rows), id_offset=OFFSETS[1])
        got = (w.ctx.download(d_run[0], (nq, knbn), np.uint64), w.ctx.download(d_run[1], (nq, knbn), np.float32), w.ctx.download(d_run[2], (nq,), np.uint32),
               w.ctx.download(d_run[3], (nq,), np.uint64))
    finally:
        dev.free()
    assert _same(got, want)
    odd = np.arange(1, nq, 2)
    assert all(np.array_equal(g[odd], b[odd]) for g, b in zip(got, before)) and not np.array_equal(got[0][rows.astype(np.int64)], before[0][rows.astype(np.int64)])
    host = [np.array(a, copy=True) for a in before]
    w.pieces[1].search_merge(w.queries[:nq], knbn, _ef(knbn), *host, rows=rows, id_offset=OFFSETS[1])
    assert _same(host, want)


def test_search_dev_equals_search_arrays(world):
    w, knbn, nq = world, 5, 65
    dev = Dev(w.ctx)
    try:
        d_q = dev.up(w.queries[:nq])
        d = [dev.up(np.zeros((nq, knbn), np.uint64)), dev.up(np.zeros((nq, knbn), np.float32)), dev.up(np.zeros(nq, np.uint32)), dev.up(np.zeros(nq, np.uint64))]
        w.pieces[0].search_dev(d_q, nq, knbn, 64, *d)
        got = (w.ctx.download(d[0], (nq, knbn), np.uint64), w.ctx.download(d[1], (nq, knbn), np.float32), w.ctx.download(d[2], (nq,), np.uint32),
               w.ctx.download(d[3], (nq,), np.uint64))
    finally:
        dev.free()
    assert _same(got, w.pieces[0].search_arrays(w.queries[:nq], knbn, 64))


def test_rows_of_a_length_that_is_no_multiple_of_16_bytes(gpu_ctx):
    """uint16 signatures of 100 slots are rows of 200 bytes: the gather of the listed rows cannot go by 16-byte words"""
    import gsearch_amd as G
    m, knbn, nq = 100, 4, 9
    db = H.synth_sig_db(3, 8, m, 21, dtype=np.uint16)
    hn = G.Hnsw.new(NBNG, 1000, 16, EFC, G.DistHamming(), dtype=np.uint16, seed=3)
    dev = Dev(gpu_ctx)
    try:
        hn.parallel_insert(db)
        q = H.queries_from(db, nq, 4)
        rows = np.array([1, 4, 8], np.uint32)
        want = RS.merge_rows(RS.empty_lists(nq, knbn), hn.search_arrays(q[rows.astype(np.int64)], knbn, 64), rows, 7)
        d_run = [dev.up(a) for a in RS.empty_lists(nq, knbn)]
        hn.search_merge_dev(dev.up(q), nq, knbn, 64, *d_run, d_rows=dev.up(rows), nr=3, id_offset=7)
        got = (gpu_ctx.download(d_run[0], (nq, knbn), np.uint64), gpu_ctx.download(d_run[1], (nq, knbn), np.float32), gpu_ctx.download(d_run[2], (nq,), np.uint32),
               gpu_ctx.download(d_run[3], (nq,), np.uint64))
        assert _same(got, want) and int(want[2][1]) == knbn
    finally:
        dev.free()
        hn.close()


def test_on_poisoned_scratch(world):
    """as tests/test_gpu_stale_scratch.py: every new device allocation and newly taken scratch slot filled with 0xA5, the pieces' per-call buffers
    before every call, on a context of its own"""
    import gsearch_amd as G
    w, knbn, nq = world, 64, 65
    want = _fold_ref(w, knbn, nq, "every_other")
    ctx = G.Context(0)
    pieces = []
    try:
        G.debug_mem_fill(0xA5)
        for hn in w.pieces:                                                        # the same pieces on the poisoned context
            cp = G.Hnsw.new(NBNG, 1000, 16, EFC, seed=3, ctx=ctx)
            cp.import_graph(hn.get_data(), hn.export_graph())
            cp.set_ids(hn.get_ids())
            pieces.append(cp)

        class P:
            pass
        pw = P()
        pw.pieces, pw.queries, pw.ctx = pieces, w.queries, ctx
        got = _fold_dev(pw, knbn, nq, "every_other", ctx=ctx, poke=lambda hn: hn.debug_fill_scratch(0xA5))
        run = RS.empty_lists(nq, knbn)
        for p, hn in enumerate(pieces):
            hn.debug_fill_scratch(0xA5)
            hn.search_merge(w.queries[:nq], knbn, _ef(knbn), *run, rows=_rows("every_other", nq), id_offset=OFFSETS[p])
    finally:
        G.debug_mem_fill(None)
        for cp in pieces:
            cp.close()
        ctx.close()
    assert _same(got, want) and _same(run, want)


def test_the_three_refusals(world):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_UNSUPPORTED
    w, knbn, nq = world, 5, 65
    before = RS.merge_rows(RS.empty_lists(nq, knbn), w.answers(0, knbn, nq, "all"), None, 0)
    dev = Dev(w.ctx)
    try:
        d_q = dev.up(w.queries[:nq])
        d_run = [dev.up(a) for a in before]
        for rows, code in (([3, 3, 9], GS_ERR_INVALID), ([9, 3], GS_ERR_INVALID), ([3, 65], GS_ERR_INVALID), ([0, 0xFFFFFFFF], GS_ERR_INVALID)):
            rows = np.array(rows, np.uint32)
            with pytest.raises(G.GsError) as e:
                w.pieces[1].search_merge_dev(d_q, nq, knbn, 64, *d_run, d_rows=dev.up(rows), nr=len(rows), id_offset=1000)
            assert e.value.code == code
            host = [np.array(a, copy=True) for a in before]
            with pytest.raises(G.GsError) as e:
                w.pieces[1].search_merge(w.queries[:nq], knbn, 64, *host, rows=rows, id_offset=1000)
            assert e.value.code == code and _same(host, before)
        with pytest.raises(G.GsError) as e:                                        # more rows than queries: refused before the list is read
            w.pieces[1].search_merge_dev(d_q, nq, knbn, 64, *d_run, d_rows=dev.up(np.arange(66, dtype=np.uint32)), nr=66, id_offset=1000)
        assert e.value.code == GS_ERR_INVALID
        got = (w.ctx.download(d_run[0], (nq, knbn), np.uint64), w.ctx.download(d_run[1], (nq, knbn), np.float32), w.ctx.download(d_run[2], (nq,), np.uint32),
               w.ctx.download(d_run[3], (nq,), np.uint64))
        assert _same(got, before)                                                  # a refused call wrote nothing
        big = Dev(w.ctx)
        try:
            d_big = [big.up(a) for a in RS.empty_lists(nq, 1025)]
            with pytest.raises(G.GsError) as e:
                w.pieces[0].search_merge_dev(d_q, nq, 1025, 1025, *d_big, id_offset=0)
            assert e.value.code == GS_ERR_UNSUPPORTED
            host = list(RS.empty_lists(nq, 1025))
            with pytest.raises(G.GsError) as e:
                w.pieces[0].search_merge(w.queries[:nq], 1025, 1025, *host)
            assert e.value.code == GS_ERR_UNSUPPORTED
        finally:
            big.free()
    finally:
        dev.free()
