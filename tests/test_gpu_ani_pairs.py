"""The superani pair stages on the device (gs_ani.hip: k_ani_anchors, k_ani_seg_count, k_ani_seg_write, k_ani_chain, k_ani_ends, k_ani_mark, k_ani_sides and
the block loop of ani_pairs_impl) on the constructed seed lists of tests/ani_pair_cases.py against the numpy restatement of SPEC 12 (tests/pyref_ani.py).
Every comparison is `==` on integers. The restatement of every case is computed once and shared."""
import numpy as np
import pytest

import ani_pair_cases as AC
import pyref_ani as PR
from test_gpu_ani import _chain_dev

pytestmark = pytest.mark.gpu
GS_OK = 0
GUARD = 4096
CANARY8 = np.uint64(0xC5C5C5C5C5C5C5C5)


class Table:
    def __init__(self, n_cu):
        self.n_cu = n_cu
        self.n_runs = max(AC.N_RUNS, (32 * n_cu + 3) // 3 * 3)          # more segments than the wavefronts of one launch
        self.cases = AC.all_cases(self.n_runs)
        self.names = list(self.cases)
        self.anchors, self.chain, self.want = {}, {}, {}
        for name, (qs, rs) in self.cases.items():
            a = PR.anchors(qs, rs)
            f, pred, root = PR.chain(a)
            ch = PR.kept_chains(f, pred, root)
            self.anchors[name], self.chain[name] = a, (f, pred, root)
            self.want[name] = [len(f), len(ch), *PR.side(qs, a["qidx"], ch, AC.K), *PR.side(rs, a["ridx"], ch, AC.K)]


@pytest.fixture(scope="module")
def table(gpu_ctx):
    t = Table(gpu_ctx.device_info()["n_cu"])
    a = t.anchors["many_segments"]
    heads = 1 + int((np.diff(a["rpos"]) > AC.G).sum())
    assert heads == t.n_runs > 32 * t.n_cu, "many_segments must have more segments than k_ani_chain and k_ani_mark have wavefronts"
    print("n_cu %d, 32 * n_cu = %d, segments of many_segments %d" % (t.n_cu, 32 * t.n_cu, heads))
    if t.n_runs == AC.N_RUNS:
        for name, row in AC.LITERAL.items():
            assert t.want[name] == row, name
    return t


def _one_call(t):
    """every case as a pair of one call, in a shuffled order, with empty lists and pairs of unrelated lists among them -> (Q, R, pairs, what, want)"""
    Q = [t.cases[n][0] for n in t.names] + [np.zeros((0, 4), np.uint32)]
    R = [t.cases[n][1] for n in t.names] + [np.zeros((0, 4), np.uint32)]
    at = {n: i for i, n in enumerate(t.names)}
    empty = len(t.names)
    pairs = [(i, i) for i in range(len(t.names))]
    what = list(t.names)
    cross = [("fork", "band(63)"), ("braid(64,4)", "braid(64,3)"), ("braid(64,3)", "braid(65,4)"), ("random(63)", "random(64)"), ("side_n(129)", "side_n(64)"),
             ("occ_grid_tandem", "occ_grid"), ("slice_occ4(2049)", "slice_diag(2049)"), ("range_values_occ5", "range_values")]
    want = [t.want[n] for n in t.names]
    for a, b in cross:                                       # the cases count their values from 1, so unrelated lists share many
        pairs.append((at[a], at[b]))
        what.append(a + " x " + b)
        want.append(PR.pair_counts(t.cases[a][0], t.cases[b][1]))
    for q, r in ((empty, at["fork"]), (at["fork"], empty), (empty, empty), (at["many_segments"], empty)):
        pairs.append((q, r))
        what.append("empty %d x %d" % (q, r))
        want.append([0] * 8)
    order = np.random.default_rng(5).permutation(len(pairs))
    return Q, R, [pairs[i] for i in order], [what[i] for i in order], np.array([want[i] for i in order], np.uint64)


def _same(got, want, what, note):
    """every pair that differs is named, not the first alone"""
    bad = [(name, g, w) for g, w, name in zip(np.asarray(got).tolist(), np.asarray(want).tolist(), what) if g != w]
    assert not bad, "%s: %d pairs differ: %s\n%s" % (note, len(bad), ", ".join(b[0] for b in bad),
                                                   "\n".join("%s: device %s, restatement %s" % b for b in bad[:12]))


def test_every_case_in_one_call_and_in_blocks(gpu_ctx, table):
    import gsearch_amd as G
    Q, R, pairs, what, want = _one_call(table)
    assert sum(1 for x in want if x[0] > 0) >= 50 and any(" x " in w and x[1] > 0 for w, x in zip(what, want.tolist()))
    got = G.ani_pairs(Q, R, pairs, ctx=gpu_ctx)
    _same(got, want, what, "one block")
    total = int(want[:, 0].sum())
    _same(G.ani_pairs(Q, R, pairs, max_block_anchors=total // 5, ctx=gpu_ctx), want, what, "a fifth of the anchors a block")
    _same(G.ani_pairs(Q, R, pairs, max_block_anchors=1, ctx=gpu_ctx), want, what, "every pair a block")


def test_device_form_leaves_guards_alone(gpu_ctx, table):
    ctx = gpu_ctx
    names = ["fork", "fork_mirror", "braid(64,4)", "side_n(0)", "side_n(1)", "side_n(63)", "side_n(64)", "side_n(65)", "side_n(128)", "side_n(129)",
             "side_intervals_q", "side_intervals_r", "side_contig_change(64)", "side_contig_change(65)", "random(2049)"]
    qs, rs = [table.cases[n][0] for n in names], [table.cases[n][1] for n in names]
    off = lambda ls: np.cumsum([0] + [len(x) for x in ls]).astype(np.uint64)                  # noqa: E731
    q, r = np.concatenate(qs), np.concatenate(rs)
    n = len(names)
    pairs = np.arange(n, dtype=np.uint32)[::-1].copy()
    arrs = [q, off(qs), r, off(rs), pairs, pairs]
    guarded = (0, 2)                                                                           # the seed arrays: exact size and a guard behind
    ptrs = [ctx.alloc(a.nbytes + (GUARD if i in guarded else 0)) for i, a in enumerate(arrs)]
    d_out = ctx.alloc(8 * (8 * n + GUARD))
    try:
        for i, (p, a) in enumerate(zip(ptrs, arrs)):
            if i in guarded:
                ctx.memset(p, 0xC5, a.nbytes + GUARD)
            ctx.upload(p, a)
        for mba in (0, 300):
            ctx.memset(d_out, 0xC5, 8 * (8 * n + GUARD))
            rc = ctx.L.gs_ani_pairs_dev(ctx.h, 16, ptrs[0], ptrs[1], n, ptrs[2], ptrs[3], n, ptrs[4], ptrs[5], n, d_out, mba)
            ctx.sync()
            assert rc == GS_OK
            out = ctx.download(d_out, (8 * n + GUARD,), np.uint64)
            _same(out[:8 * n].reshape(n, 8), [table.want[names[p]] for p in pairs.tolist()], [names[p] for p in pairs.tolist()], "max_block_anchors %d" % mba)
            assert (out[8 * n:] == CANARY8).all(), "written behind the last pair's row"
            for i in guarded:
                whole = ctx.download(ptrs[i], (arrs[i].nbytes + GUARD,), np.uint8)
                assert np.array_equal(whole[:arrs[i].nbytes], arrs[i].view(np.uint8).ravel()) and (whole[arrs[i].nbytes:] == 0xC5).all(), "seed array %d" % i
    finally:
        for p in ptrs + [d_out]:
            ctx.free(p)


def test_chain_alone_on_many_segments_and_whole_tiles(gpu_ctx, table):
    """f, pred and root of every anchor: the only place where what the second trip of k_ani_chain's grid-stride loop wrote is seen anchor by anchor"""
    names = ["many_segments", "singles(%d)" % AC.AN_TILE, "singles(%d)" % (AC.AN_TILE + 1), "singles(%d)" % (2 * AC.AN_TILE), "long_diagonal"]
    got = _chain_dev(gpu_ctx, [table.anchors[n] for n in names])
    for name, (f, pred, root) in zip(names, got):
        wf, wp, wr = table.chain[name]
        assert np.array_equal(f, wf), ("f", name)
        assert np.array_equal(pred, wp), ("pred", name)
        assert np.array_equal(root, wr), ("root", name)
    # the same pairs one by one: n a multiple of the tile closes the segment list in the last tile's last store
    for name in names[1:4]:
        (f, pred, root), = _chain_dev(gpu_ctx, [table.anchors[name]])
        assert (f == PR.W).all() and (pred == PR.NONE).all() and np.array_equal(root, np.arange(len(f))), name


def test_pairs_on_poisoned_scratch(table):
    """many_segments and braid(64, 4) need best, matched, diff and nchain cleared for every block"""
    import gsearch_amd as G
    names = ["many_segments", "braid(64,4)", "many_segments", "fork_mirror", "braid(64,4)"]
    Q, R = [table.cases[n][0] for n in names], [table.cases[n][1] for n in names]
    want = np.array([table.want[n] for n in names], np.uint64)
    ctx = G.Context(0)
    try:
        G.debug_mem_fill(0xFF)
        for mba in (1, 0):
            got = G.ani_pairs(Q, R, [(i, i) for i in range(len(names))], max_block_anchors=mba, ctx=ctx)
            _same(got, want, names, "fill 0xFF, max_block_anchors %d" % mba)
    finally:
        G.debug_mem_fill(None)
        ctx.close()
