"""superani on the device (gs_ani.hip) against the numpy restatement of SPEC 12 (tests/pyref_ani.py): seeds in position order (host and device
form), the chaining program alone on constructed anchors (gs_ani_chain_dev), pairs end to end at one and at several blocks, on poisoned scratch,
and superani() on files. Every comparison is `==` on integers (the output file: on bytes)."""
import gzip

import numpy as np
import pytest

import pyref_ani as PR
from test_ani_cpu import HAND, HAND_F, HAND_PRED, HAND_ROOT

pytestmark = pytest.mark.gpu
GS_OK, GS_ERR_INVALID = 0, -1
GUARD = 4096
CANARY4 = np.uint32(0xC5C5C5C5)
G_, W_ = PR.G, PR.W


# ---- seeds -------------------------------------------------------------------------------------------------------------------------------------
def _seed_genomes(k):
    rng = np.random.default_rng(40 + k)
    R = lambda n: PR.random_genome(rng, n)                                                  # noqa: E731
    noisy = R(3000).lower()[:1500] + b"NNNNNNNNNN" + R(700) + b"nRYK-" + R(40).lower() + b"N" * 40 + R(k) + b"N" + R(k - 1)
    return [[],                                                                             # a genome without records
            [R(k - 1)],
            [R(k)],
            [R(5000)],
            [R(4000), R(3), R(900), R(k - 1), R(2500), b"", R(k), R(1200)][:7],              # seven contigs, short ones between long ones
            [R(300_000)],                                                                    # several tiles and workgroups
            [noisy, b"NNNN", R(200)]]


class _Packed:
    """genomes on the device as gs_ani_sketch_batch_dev takes them"""

    def __init__(self, ctx, genomes):
        import gsearch_amd as G
        recs = [r for g in genomes for r in g]
        seq, rs, rl = G.pack_dna_records(recs)
        go = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
        self.ctx, self.ng, self.n_rec, self.n_bytes = ctx, len(genomes), len(recs), len(seq)
        nb = (len(seq) + 7) // 8 * 8 + 64
        self.ptrs = [ctx.alloc(nb), ctx.alloc(8 * max(len(recs), 1)), ctx.alloc(8 * max(len(recs), 1)), ctx.alloc(8 * len(go))]
        ctx.memset(self.ptrs[0], 0, nb)
        for p, a in zip(self.ptrs, (seq, rs, rl, go)):
            if a.size:
                ctx.upload(p, a)

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)

    def run(self, k, c, cap):
        ctx = self.ctx
        n_out, n_cnt = 4 * self.ng * cap + GUARD, self.ng + 64
        d_out, d_cnt = ctx.alloc(4 * n_out), ctx.alloc(4 * n_cnt)
        try:
            ctx.memset(d_out, 0xC5, 4 * n_out); ctx.memset(d_cnt, 0xC5, 4 * n_cnt)
            d_seq, d_rs, d_rl, d_go = self.ptrs
            rc = ctx.L.gs_ani_sketch_batch_dev(ctx.h, k, c, d_seq, self.n_bytes, d_rs, d_rl, self.n_rec, d_go, self.ng, cap, d_out, d_cnt)
            ctx.sync()
            return rc, ctx.download(d_cnt, (n_cnt,), np.uint32), ctx.download(d_out, (n_out,), np.uint32)
        finally:
            ctx.free(d_out); ctx.free(d_cnt)


def _verify_rows(rc, cnt, out, want, cap, what):
    ng = len(want)
    assert [int(x) for x in cnt[:ng]] == [len(w) for w in want], (what, "counts")
    assert (cnt[ng:] == CANARY4).all(), (what, "a count was written past the last genome")
    untouched = np.ones(len(out), bool)
    for g, w in enumerate(want):
        n = min(len(w), cap)
        assert np.array_equal(out[4 * g * cap:4 * (g * cap + n)], w[:n].ravel()), (what, "genome %d: the first %d of %d seeds" % (g, n, len(w)))
        untouched[4 * g * cap:4 * (g * cap + n)] = False
    bad = np.flatnonzero(out[untouched] != CANARY4)
    assert len(bad) == 0, (what, "%d words outside the rows' seeds were written, the first at word %d (cap %d)" % (len(bad), int(np.flatnonzero(untouched)[bad[0]]), cap))
    assert rc == (GS_OK if max([len(w) for w in want] + [0]) <= cap else GS_ERR_INVALID), (what, rc)


@pytest.mark.parametrize("c", [1, 30])
@pytest.mark.parametrize("k", [11, 16])
def test_seeds_host_and_device_form(gpu_ctx, k, c):
    import gsearch_amd as G
    genomes = _seed_genomes(k)
    want = [PR.seeds(g, k, c) for g in genomes]
    assert len(want[2]) == (1 if c == 1 else len(want[2])) and len(want[1]) == 0 and (c > 1 or len(want[5]) == 300_000 - k + 1)
    sk = G.AniSketcher(k, c, gpu_ctx)
    assert sk.sketch_genomes([]) == []                                                       # no genome at all
    got = sk.sketch_genomes(genomes)
    for g, (a, w) in enumerate(zip(got, want)):
        assert a.seeds.shape == w.shape and np.array_equal(a.seeds, w), (k, c, "genome %d" % g)
        assert a.bases == PR.bases(genomes[g])
    b = _Packed(gpu_ctx, genomes)
    try:
        longest = max(len(w) for w in want)
        _verify_rows(*b.run(k, c, longest), want, longest, (k, c, "cap = longest"))
        _verify_rows(*b.run(k, c, longest - 1), want, longest - 1, (k, c, "cap = longest - 1"))
    finally:
        b.free()
    e = _Packed(gpu_ctx, [])
    try:
        rc, cnt, out = e.run(k, c, 8)
        assert rc == GS_OK and (cnt == CANARY4).all() and (out == CANARY4).all()
    finally:
        e.free()


def test_seed_parameters_are_checked(gpu_ctx):
    import gsearch_amd as G
    for k, c in ((7, 30), (17, 30), (16, 0)):
        with pytest.raises(G.GsError):
            G.AniSketcher(k, c, gpu_ctx).sketch_genomes([[b"ACGT" * 20]])


# ---- the chaining program alone --------------------------------------------------------------------------------------------------------------
def _mk(rows):
    """rows of (rcontig, rpos, qcontig, qpos, strand) -> anchors of one pair"""
    a = np.array(rows, np.int64).reshape(-1, 5)
    return {"rcontig": a[:, 0], "rpos": a[:, 1], "qcontig": a[:, 2], "qpos": a[:, 3], "strand": a[:, 4]}


def _diag(n, r0, q0, step=10, qc=0, s=0, rc=0):
    return [(rc, r0 + step * i, qc, q0 + step * i if s == 0 else q0 - step * i, s) for i in range(n)]


def _back(between):
    """anchor 0, `between` anchors on another q contig that chain with nobody on q contig 0, then an anchor whose only candidate is anchor 0"""
    mid = [(0, 101 + i, 1, 5000 - i, 0) for i in range(between)]                              # q runs backwards: they do not chain with one another either
    return _mk([(0, 100, 0, 100, 0)] + mid + [(0, 400, 0, 400, 0)])


def _random_pair(rng, n):
    rc = np.sort(rng.integers(0, 3, n))
    rp = rng.integers(0, 30 * n + 10, n)
    order = np.lexsort((rp, rc))
    rc, rp = rc[order], rp[order]
    s = rng.integers(0, 2, n)
    qc = rng.integers(0, 2, n)
    noise = rng.integers(-40, 41, n) * (rng.random(n) < 0.5)
    qp = np.where(s == 0, rp + 1000 + noise, 10_000_000 - rp + noise)
    return {"rcontig": rc, "rpos": rp, "qcontig": qc, "qpos": qp, "strand": s}


def _chain_dev(ctx, pairs, expect=GS_OK):
    off = np.cumsum([0] + [len(p["rpos"]) for p in pairs]).astype(np.uint64)
    n = int(off[-1])
    cols = [np.concatenate([np.asarray(p[x], np.int64) for p in pairs]).astype(np.uint32) if pairs else np.zeros(0, np.uint32)
            for x in ("rcontig", "rpos", "qcontig", "qpos", "strand")]
    d_in = [ctx.alloc(4 * max(n, 1)) for _ in cols]
    d_off = ctx.alloc(8 * len(off))
    d_out = [ctx.alloc(4 * (n + GUARD)) for _ in range(3)]
    try:
        for d, a in zip(d_in, cols):
            if n:
                ctx.upload(d, a)
        ctx.upload(d_off, off)
        for d in d_out:
            ctx.memset(d, 0xC5, 4 * (n + GUARD))
        rc = ctx.L.gs_ani_chain_dev(ctx.h, *d_in, d_off, len(pairs), *d_out)
        ctx.sync()
        assert rc == expect
        f, pred, root = (ctx.download(d, (n + GUARD,), np.uint32) for d in d_out)
        for a in (f, pred, root):
            assert (a[n:] == CANARY4).all(), "written past the last anchor"
        return [(f[int(off[i]):int(off[i + 1])].view(np.int32), pred[int(off[i]):int(off[i + 1])], root[int(off[i]):int(off[i + 1])]) for i in range(len(pairs))]
    finally:
        for d in d_in + d_out + [d_off]:
            ctx.free(d)


def _check_chain(ctx, pairs):
    got = _chain_dev(ctx, pairs)
    for i, (p, (f, pred, root)) in enumerate(zip(pairs, got)):
        wf, wp, wr = PR.chain(p)
        assert f.tolist() == wf.tolist(), ("f", i)
        assert pred.tolist() == wp.tolist(), ("pred", i)
        assert root.tolist() == wr.tolist(), ("root", i)
    return got


def test_chain_hand_worked_and_window_edges(gpu_ctx):
    hand = _mk([(0, r, qc, q, s) for r, q, qc, s in HAND])
    # dq = G after a long diagonal (f = 20 * 130 pays for the 2490 of difference), and dq = G + 1
    long_ = _diag(130, 0, 0)
    dq_g = _mk(long_ + [(0, 1300, 0, 1290 + G_, 0)])
    dq_g1 = _mk(long_ + [(0, 1300, 0, 1290 + G_ + 1, 0)])
    pairs = [hand, _back(63), _back(64),
             _mk([(0, 0, 0, 0, 0), (0, G_, 0, G_, 0)]), _mk([(0, 0, 0, 0, 0), (0, G_ + 1, 0, G_ + 1, 0)]), dq_g, dq_g1,
             _mk(_diag(5, 1000, 9000, s=1) + _diag(5, 2000, 8000, s=1, qc=1)),               # strand 1 runs towards smaller q
             _mk([(0, 10, 0, 500, 0), (0, 20, 0, 490, 0), (0, 30, 0, 480, 0)])]               # q runs backwards on strand 0: nothing chains
    got = _check_chain(gpu_ctx, pairs)
    assert got[0][0].tolist() == HAND_F and got[0][1].tolist() == HAND_PRED and got[0][2].tolist() == HAND_ROOT
    assert int(got[1][1][64]) == 0 and int(got[1][0][64]) == 2 * W_                            # exactly 64 back: taken
    assert int(got[2][1][65]) == PR.NONE and int(got[2][0][65]) == W_                          # 65 back: out of the band
    assert int(got[3][1][1]) == 0 and int(got[4][1][1]) == PR.NONE                            # dr = G, dr = G + 1
    assert int(got[5][1][130]) == 129 and int(got[6][1][130]) == PR.NONE                      # dq = G, dq = G + 1
    assert got[7][0].tolist() == [20, 40, 60, 80, 100] * 2 and got[8][0].tolist() == [20, 20, 20]


def test_chain_mixed_counts_in_one_call(gpu_ctx):
    rng = np.random.default_rng(77)
    pairs = []
    for n in (0, 1, 63, 64, 65, 129, 5000):
        pairs += [_random_pair(rng, n), _random_pair(rng, 0)]
    got = _check_chain(gpu_ctx, pairs)
    assert sum(int((p != PR.NONE).sum()) for _, p, _ in got) > 1000                            # the random anchors do chain
    assert _chain_dev(gpu_ctx, []) == []


def test_chain_segment_boundaries_at_ring_positions(gpu_ctx):
    """runs of anchors separated by r gaps > G: each gap starts a segment; run lengths 64, 65 and 63 put the following boundary at ring positions 0, 1 and
    63, and a run of 200 keeps a segment going through three chunks of the ring"""
    rows, r0 = [], 0
    for n in (64, 65, 63, 1, 2, 200, 128, 127, 5):
        rows += _diag(n, r0, r0 + 7)
        r0 = rows[-1][1] + G_ + 1
    rows += _diag(70, 0, 0, rc=1)                                                             # another r contig also starts a segment
    _check_chain(gpu_ctx, [_mk(rows), _mk(rows[:64]), _mk(rows[64:129])])


def test_chain_refuses_anchors_out_of_order(gpu_ctx):
    _chain_dev(gpu_ctx, [_mk([(0, 100, 0, 100, 0), (0, 50, 0, 150, 0)])], expect=GS_ERR_INVALID)
    _chain_dev(gpu_ctx, [_mk(_diag(70, 0, 0)), _mk([(1, 5, 0, 5, 0), (0, 6, 0, 6, 0)])], expect=GS_ERR_INVALID)


# ---- pairs end to end --------------------------------------------------------------------------------------------------------------------------
def _pair_genomes():
    rng = np.random.default_rng(2024)
    base = PR.random_genome(rng, 60_000)
    sub = lambda p: PR.substitute(rng, base, p)                                              # noqa: E731
    rep = PR.random_genome(rng, 2000)
    m = sub(0.02)
    out = [[base], [sub(0.01)], [sub(0.05)], [sub(0.15)], [PR.indels(rng, sub(0.01), 0.002)],
           [m[:20_000] + PR.revcomp(m[20_000:30_000]) + m[30_000:]],                         # a 10 kbp inversion
           [m[:5000] + m[40_000:52_000] + m[5000:40_000] + m[52_000:]],                      # a translocated block
           [m[:17_000], m[17_000:45_001], m[45_001:]],                                       # three contigs
           [base[:10_000] + rep + base[10_000:30_000] + rep + base[30_000:50_000] + rep + base[50_000:]],      # 3 copies: below MAX_OCC
           [base[:8000] + b"".join(rep + base[8000 + 7000 * i:15_000 + 7000 * i] for i in range(6)) + base[50_000:]],      # 6 copies: above
           [PR.random_genome(rng, 60_000)], []]
    return out


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    """the genomes, their seeds from the device (== the restatement), and the restatement's eight integers of every (query, reference) pair"""
    import gsearch_amd as G
    genomes = _pair_genomes()
    sk = G.AniSketcher(16, 30, gpu_ctx).sketch_genomes(genomes)
    ref_seeds = [PR.seeds(g) for g in genomes]
    for a, w in zip(sk, ref_seeds):
        assert np.array_equal(a.seeds, w)
    n = len(genomes)
    table = np.array([[PR.pair_counts(ref_seeds[q], ref_seeds[r]) for q in range(n)] for r in range(n)], np.uint64)     # [reference][query]
    return genomes, sk, table


def test_pairs_every_pair_at_one_and_at_several_blocks(gpu_ctx, batch):
    import gsearch_amd as G
    genomes, sk, table = batch
    n = len(genomes)
    got = G.ani_pairs(sk, sk, None, ctx=gpu_ctx)
    assert np.array_equal(got.reshape(n, n, 8), table)
    assert table[0, 1, 1] >= 1 and table[10, 0, 1] == 0 and table[5, 0, 1] >= 3 and table[7, 0, 1] >= 3 and (table[11] == 0).all()
    assert table[8, 8, 0] > len(sk[8].seeds) + 300 and table[9, 9, 0] < len(sk[9].seeds) - 300     # a 3-copy repeat gives 9 anchors a seed, a 6-copy one none
    total = int(table[:, :, 0].sum())
    small = G.ani_pairs(sk, sk, None, max_block_anchors=total // 5, ctx=gpu_ctx)              # at least 5 blocks
    assert np.array_equal(small, got)
    one = G.ani_pairs(sk, sk, None, max_block_anchors=1, ctx=gpu_ctx)                         # every pair a block of its own
    assert np.array_equal(one, got)
    # a pair listed twice, pairs in another order, no pair at all
    pairs = [(1, 0), (3, 2), (1, 0), (0, 11), (11, 0), (4, 4)]
    got = G.ani_pairs(sk, sk, pairs, ctx=gpu_ctx)
    assert np.array_equal(got, np.array([table[r, q] for q, r in pairs]))
    assert G.ani_pairs(sk, sk, [], ctx=gpu_ctx).shape == (0, 8)
    with pytest.raises(G.GsError):
        G.ani_pairs(sk, sk, [(0, n)], ctx=gpu_ctx)


def test_pairs_estimates_follow_the_planted_rates(gpu_ctx, batch):
    import gsearch_amd as G
    genomes, sk, table = batch
    est = G.ani_estimate(table[0, 1:4], [sk[q].bases for q in (1, 2, 3)], sk[0].bases)
    for (ani, afq, afr), p, row, q in zip(est, (0.01, 0.05, 0.15), table[0, 1:4], (1, 2, 3)):
        assert [float(ani), float(afq), float(afr)] == [float(x) for x in PR.estimate(row, sk[q].bases, sk[0].bases)]
        f = int(row[2]) / int(row[3])
        sigma = float(ani) * np.sqrt(f * (1 - f) / int(row[3])) / (16 * f)
        assert abs(float(ani) - (1 - p)) <= 6 * sigma


def test_pairs_on_poisoned_scratch_twice(batch):
    import gsearch_amd as G
    genomes, sk, table = batch
    n = len(genomes)
    ctx = G.Context(0)
    try:
        for fill in (0xFF, 0x01, 0x00):
            G.debug_mem_fill(fill)
            for _ in range(2):
                again = G.AniSketcher(16, 30, ctx).sketch_genomes(genomes[:4] + genomes[10:])
                for a, w in zip(again, sk[:4] + sk[10:]):
                    assert np.array_equal(a.seeds, w.seeds), "seeds, fill 0x%02X" % fill
                got = G.ani_pairs(sk, sk, None, max_block_anchors=int(table[:, :, 0].sum()) // 3, ctx=ctx)
                assert np.array_equal(got.reshape(n, n, 8), table), "fill 0x%02X" % fill
            G.debug_mem_fill(None)
    finally:
        G.debug_mem_fill(None)
        ctx.close()


def test_large_pair_device_form_equals_host_form(gpu_ctx):
    """2 Mbp at p = 0.03: about 67 k seeds a side and 40 k anchors, so the scans, the slices and the segment list cross several workgroups"""
    import gsearch_amd as G
    rng = np.random.default_rng(31)
    base = PR.random_genome(rng, 2_000_000)
    mut = PR.substitute(rng, base, 0.03)
    genomes = [[base], [mut[:700_000], mut[700_000:]]]
    sk = G.AniSketcher(16, 30, gpu_ctx).sketch_genomes(genomes)
    ref = [PR.seeds(g) for g in genomes]
    for a, w in zip(sk, ref):
        assert np.array_equal(a.seeds, w)
    want = np.array([PR.pair_counts(ref[1], ref[0])], np.uint64)
    assert want[0, 0] > 30_000 and want[0, 1] >= 2
    host = G.ani_pairs([sk[1]], [sk[0]], None, ctx=gpu_ctx)
    assert np.array_equal(host, want)
    ctx = gpu_ctx
    q, r = np.ascontiguousarray(sk[1].seeds), np.ascontiguousarray(sk[0].seeds)
    arrs = [q, np.array([0, len(q)], np.uint64), r, np.array([0, len(r)], np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint32)]
    ptrs = [ctx.alloc(a.nbytes) for a in arrs]
    d_out = ctx.alloc(8 * (8 + GUARD))
    try:
        for p, a in zip(ptrs, arrs):
            ctx.upload(p, a)
        ctx.memset(d_out, 0xC5, 8 * (8 + GUARD))
        rc = ctx.L.gs_ani_pairs_dev(ctx.h, 16, ptrs[0], ptrs[1], 1, ptrs[2], ptrs[3], 1, ptrs[4], ptrs[5], 1, d_out, 0)
        ctx.sync()
        assert rc == GS_OK
        out = ctx.download(d_out, (8 + GUARD,), np.uint64)
        assert np.array_equal(out[:8], want[0]) and (out[8:] == np.uint64(0xC5C5C5C5C5C5C5C5)).all()
    finally:
        for p in ptrs + [d_out]:
            ctx.free(p)


# ---- superani() --------------------------------------------------------------------------------------------------------------------------------
def _fasta(genome, name):
    out = bytearray()
    for i, rec in enumerate(genome):
        out += b">%s_%d some text\n" % (name.encode(), i)
        out += b"\n".join(rec[j:j + 70] for j in range(0, len(rec), 70)) + b"\n"
    return bytes(out)


def test_superani_on_files(gpu_ctx, batch, tmp_path):
    import gsearch_amd as G
    genomes, sk, table = batch
    paths = {}
    for g in (0, 1, 5, 7, 10):
        p = tmp_path / ("g%d.fa%s" % (g, ".gz" if g in (1, 7) else ""))
        text = _fasta(genomes[g], "g%d" % g)
        p.write_bytes(gzip.compress(text) if g in (1, 7) else text)
        paths[g] = str(p)
    ql, rl = [1, 7, 10, 1], [0, 5, 0]                                                         # a query and a reference listed twice
    (tmp_path / "q.txt").write_text("".join(paths[g] + "\n" for g in ql))
    (tmp_path / "r.txt").write_text("\n".join(paths[g] for g in rl))                          # no newline at the end
    est = G.superani(tmp_path / "q.txt", tmp_path / "r.txt", tmp_path / "out.tsv", ctx=gpu_ctx)
    want = [[PR.estimate(table[r, q], PR.bases(genomes[q]), PR.bases(genomes[r])) for q in ql] for r in rl]
    assert est.shape == (3, 4, 3) and np.array_equal(est, np.array(want, np.float32))
    text = (tmp_path / "out.tsv").read_bytes()
    assert text == PR.superani_text([paths[g] for g in ql], [paths[g] for g in rl], want)
    lines = text.decode().splitlines()
    assert len(lines) == 12 and [x.split("\t")[1] for x in lines] == [paths[g] for g in rl for _ in ql]        # reference-major
    assert lines[0] == lines[3] and 0.98 < float(lines[0].split("\t")[2]) < 1 and lines[2].split("\t")[2:] == ["0", "0", "0"]
