"""superaai's device-resident entry points (gs_frac.hip): gs_frac_sketch_batch_dev (fixed row pitch `cap`, the cut at cap, one gather per
sketching round into the caller's buffer) and gs_frac_similarity_qxc_dev (reads the offsets back to choose between the LDS and the
global-memory query), against the numpy reference of SPEC 9 (tests/pyref_aai.py) and the host forms."""
import numpy as np
import pytest

import pyref_aai as PR
from test_gpu_aai import AA, CASES, _family, _genome, _protein

pytestmark = pytest.mark.gpu
GS_OK, GS_ERR_INVALID = 0, -1
GUARD = 4096                                            # words behind the last row that the test owns and the call must leave alone
CANARY8, CANARY4 = np.uint64(0xC5C5C5C5C5C5C5C5), np.uint32(0xC5C5C5C5)


class _Batch:
    """genomes (lists of records) on the device as gs_frac_sketch_batch_dev takes them: residues without line breaks end to end, record
    starts and lengths, genome record offsets"""

    def __init__(self, ctx, genomes):
        recs = [PR.clean(r) for g in genomes for r in g]
        rl = np.array([len(r) for r in recs], np.uint64)
        rs = (np.cumsum(rl, dtype=np.uint64) - rl).astype(np.uint64)
        go = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
        seq = np.frombuffer(b"".join(recs), np.uint8)
        self.ctx, self.ng, self.n_rec, self.n_bytes = ctx, len(genomes), len(recs), len(seq)
        self.ptrs = [ctx.alloc(len(seq) + 64), ctx.alloc(8 * max(len(recs), 1)), ctx.alloc(8 * max(len(recs), 1)), ctx.alloc(8 * len(go))]
        ctx.memset(self.ptrs[0], 0, len(seq) + 64)
        for p, a in zip(self.ptrs, (seq, rs, rl, go)):
            if a.size:
                ctx.upload(p, a)

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)

    def run(self, k, scaled, num, cap, null_out=False):
        """-> (return code, the count buffer with its guard, the whole output buffer with its guard): both filled with a canary first"""
        ctx = self.ctx
        n_out, n_cnt = self.ng * cap + GUARD, self.ng + 64
        d_out, d_cnt = ctx.alloc(8 * n_out), ctx.alloc(4 * n_cnt)
        try:
            ctx.memset(d_out, 0xC5, 8 * n_out); ctx.memset(d_cnt, 0xC5, 4 * n_cnt)
            d_seq, d_rs, d_rl, d_go = self.ptrs
            rc = ctx.L.gs_frac_sketch_batch_dev(ctx.h, k, scaled, num, d_seq, self.n_bytes, d_rs, d_rl, self.n_rec, d_go, self.ng, cap,
                                                None if null_out else d_out, d_cnt)
            ctx.sync()
            return rc, ctx.download(d_cnt, (n_cnt,), np.uint32), ctx.download(d_out, (n_out,), np.uint64)
        finally:
            ctx.free(d_out); ctx.free(d_cnt)


def _verify(rc, cnt, out, want, cap, what):
    ng = len(want)
    assert [int(x) for x in cnt[:ng]] == [len(w) for w in want], (what, "counts")
    assert (cnt[ng:] == CANARY4).all(), (what, "a count was written past the last genome")
    untouched = np.ones(len(out), bool)
    for g, w in enumerate(want):
        n = min(len(w), cap)
        assert np.array_equal(out[g * cap:g * cap + n], w[:n]), (what, "genome %d: the first %d of %d values" % (g, n, len(w)))
        untouched[g * cap:g * cap + n] = False
    bad = np.flatnonzero(out[untouched] != CANARY8)
    assert len(bad) == 0, (what, "%d words outside the rows' values were written, the first at word %d (cap %d)" % (
        len(bad), int(np.flatnonzero(untouched)[bad[0]]), cap))
    assert rc == (GS_OK if max([len(w) for w in want] + [0]) <= cap else GS_ERR_INVALID), (what, rc)


@pytest.mark.parametrize("k", [1, 2, 7, 17, 32])
def test_sketch_batch_dev_bit_exact(gpu_ctx, k):
    """The genomes and (scaled, num) cases of test_sketch_bit_exact_every_k through the device form, with two short genomes that finish in
    the first sketching round around the long ones. At k = 1 and 2 a long genome has a few hundred distinct windows at most: with num = 5120
    its speculative threshold fails and is widened over several rounds, and its candidates overflow their slots, so the genomes of the batch
    are gathered into the caller's rows in different rounds. The (1, 0) case keeps every hash: 300 000 candidates of one genome go through
    the radix path. Each case at cap = the longest sketch (success) and one less (GS_ERR_INVALID, true counts, rows cut at cap); every word
    of the output outside the rows' values, a guard region behind the last row included, keeps its canary."""
    rng = np.random.default_rng(300 + k)
    genomes = [_genome(rng, k, n) for n in (0, k, 500, 40_000, 300_000)] + [[]] + [[b""]] + [_genome(rng, k, 700)]
    genomes.insert(3, [_protein(rng, 900)])                       # ... 500, 900, 40 000, 300 000, none, empty, 700
    b = _Batch(gpu_ctx, genomes)
    try:
        for scaled, num in CASES + [(1, 0)]:
            want = [PR.sketch(g, k, scaled, num) for g in genomes]
            longest = max(len(w) for w in want)
            what = (k, scaled, num)
            _verify(*b.run(k, scaled, num, longest), want, longest, what + ("cap = longest",))
            if longest:
                _verify(*b.run(k, scaled, num, longest - 1), want, longest - 1, what + ("cap = longest - 1",))
            # cap = 0 and no output buffer: the counts alone
            rc, cnt, _ = b.run(k, scaled, num, 0, null_out=True)
            assert [int(x) for x in cnt[:len(want)]] == [len(w) for w in want] and (cnt[len(want):] == CANARY4).all(), what
            assert rc == (GS_ERR_INVALID if longest else GS_OK), what
    finally:
        b.free()


def test_sketch_batch_dev_empty_inputs(gpu_ctx):
    """an empty batch, a batch of genomes without records, and one whose records are all shorter than k"""
    k = 7
    b = _Batch(gpu_ctx, [])
    try:
        rc, cnt, out = b.run(k, 100, 5120, 16)
        assert rc == GS_OK and (cnt == CANARY4).all() and (out == CANARY8).all()
    finally:
        b.free()
    for genomes in ([[], [], []], [[b"MKV", b""], [AA[:k - 1]], [b"\r\n"]]):
        b = _Batch(gpu_ctx, genomes)
        try:
            for cap in (0, 5):
                _verify(*b.run(k, 100, 5120, cap), [np.zeros(0, np.uint64)] * len(genomes), cap, (genomes, cap))
        finally:
            b.free()


def _csr(sketches):
    off = np.zeros(len(sketches) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in sketches])
    flat = np.concatenate([np.asarray(x, np.uint64) for x in sketches] + [np.zeros(1, np.uint64)])
    return flat, off


def _sim_dev(ctx, G, Q, R, num, counts=True):
    """gs_frac_similarity_qxc_dev on uploaded CSR sketches -> (sim, common, union) (the last two None without counts)"""
    (q, qo), (r, ro) = _csr(Q), _csr(R)
    nq, nr = len(Q), len(R)
    ptrs = [ctx.alloc(a.nbytes) for a in (q, qo, r, ro)] + [ctx.alloc(8 * nq * nr), ctx.alloc(4 * nq * nr), ctx.alloc(4 * nq * nr)]
    try:
        for p, a in zip(ptrs, (q, qo, r, ro)):
            ctx.upload(p, a)
        for p, w in zip(ptrs[4:], (8, 4, 4)):
            ctx.memset(p, 0xC5, w * nq * nr)
        G.frac_similarity_qxc_dev(ctx, num, ptrs[0], ptrs[1], nq, ptrs[2], ptrs[3], nr, ptrs[4], ptrs[5] if counts else None, ptrs[6] if counts else None)
        ctx.sync()
        sim = ctx.download(ptrs[4], (nq, nr), np.float64)
        com, uni = ctx.download(ptrs[5], (nq, nr), np.uint32), ctx.download(ptrs[6], (nq, nr), np.uint32)
    finally:
        for p in ptrs:
            ctx.free(p)
    if not counts:
        assert (com == CANARY4).all() and (uni == CANARY4).all()             # (the call had no pointer to them)
        return sim, None, None
    return sim, com, uni


def _same_as_host(ctx, G, Q, R, num):
    hs, hc, hu = G.frac_similarity_qxc(Q, R, num, return_counts=True)
    ds, dc, du = _sim_dev(ctx, G, Q, R, num)
    assert np.array_equal(ds.view(np.uint64), hs.view(np.uint64)) and np.array_equal(dc, hc) and np.array_equal(du, hu)
    return hs, hc, hu


def _same_as_reference(Q, R, num, sim, com, uni):
    for i, a in enumerate(Q):
        for j, b in enumerate(R):
            c, u = PR.similarity_counts(a, b, num)
            assert com[i, j] == c and uni[i, j] == u and sim[i, j] == float(c) / float(max(1, u)), (i, j)


@pytest.mark.parametrize("nq,nr", [(1, 1), (3, 257), (130, 70)])
def test_similarity_dev_equals_host(gpu_ctx, nq, nr):
    """the shapes and sketches of test_similarity_counts_exact; (3, 257) also with both optional outputs null"""
    import gsearch_amd as G
    rng = np.random.default_rng(nq * 1000 + nr)
    num = 64
    Q = _family(rng, nq, 80, num, 0.4)
    R = _family(rng, nr, 80, num, 0.4)
    Q[0] = np.zeros(0, np.uint64)
    if nq > 2:
        Q[1] = R[0].copy()
        Q[2] = R[min(2, nr - 1)][:num].copy()
    hs, _, _ = _same_as_host(gpu_ctx, G, Q, R, num)
    if nq == 3:
        ds, _, _ = _sim_dev(gpu_ctx, G, Q, R, num, counts=False)
        assert np.array_equal(ds.view(np.uint64), hs.view(np.uint64))


def test_similarity_dev_long_and_mixed_queries(gpu_ctx):
    """the sketches of test_similarity_long_sketches, and a batch whose longest query is above the 8192 values that fit in LDS beside short
    and empty ones: the launch then reads some queries from LDS and others from global memory"""
    import gsearch_amd as G
    rng = np.random.default_rng(77)
    Q = _family(rng, 5, 12_000, 0, 0.5) + [np.zeros(0, np.uint64)]
    R = _family(rng, 9, 12_000, 0, 0.5)
    Q[0] = np.unique(np.concatenate([Q[0], rng.integers(0, 2 ** 64, 20_000, dtype=np.uint64)]))
    _same_as_host(gpu_ctx, G, Q, R, 0)
    Q2 = [x[:5120] for x in Q] + [np.sort(rng.choice(R[0], min(len(R[0]), 3000), replace=False))]
    R2 = [x[:5120] for x in R]
    _same_as_host(gpu_ctx, G, Q2, R2, 5120)
    _same_as_host(gpu_ctx, G, Q2, R2, 100)
    mixed = [Q2[1], Q[0], Q[-1], Q2[-1], Q[1][:8192], Q[1][:8193], Q[2][:40]]
    assert max(len(x) for x in mixed) > 8192 and sorted(len(x) for x in mixed)[:2] == [0, 40]
    for num in (0, 5120):
        s, c, u = _same_as_host(gpu_ctx, G, mixed, R, num)
        _same_as_reference(mixed, R[:3], num, s, c, u)


def test_similarity_extreme_hash_values(gpu_ctx):
    """sketches that hold 0 and 2^64 - 1, the ends of the hash range, through the host and the device form"""
    import gsearch_amd as G
    top = 2 ** 64 - 1
    A, B = np.array([0, 5, top], np.uint64), np.array([0, 7, top], np.uint64)
    assert PR.similarity_counts(A, B, 0) == (2, 4) and PR.similarity_counts(A, B, 2) == (1, 2)
    rng = np.random.default_rng(9)
    Q = [A, B, np.array([0], np.uint64), np.array([top], np.uint64), np.zeros(0, np.uint64)]
    R = [B, A, np.array([top], np.uint64), np.array([0, top], np.uint64)]
    for x in _family(rng, 6, 80, 0, 0.4):
        Q.append(np.unique(np.concatenate([x, np.array([0, top], np.uint64)])))
        R.append(np.unique(np.concatenate([x[::2], np.array([top], np.uint64)])))
    assert all(x.dtype == np.uint64 for x in Q + R) and sum(int(x[-1]) == top for x in Q if len(x)) >= 8 and sum(int(x[0]) == 0 for x in Q if len(x)) >= 8
    for num in (0, 2, 64):
        s, c, u = _same_as_host(gpu_ctx, G, Q, R, num)
        _same_as_reference(Q, R, num, s, c, u)
    s, c, u = G.frac_similarity_qxc([A], [B], 0, return_counts=True)
    assert (int(c[0, 0]), int(u[0, 0]), float(s[0, 0])) == (2, 4, 0.5)
