"""hypermash similarity at a shape that makes the host loops of hmh_similarity_dev (gs_hmh.hip) go round more than once: several query
passes (the C | N matrix of a pass stays under 1 GB) and several P-vector blocks of small sketches on either side, the last pass and the
last blocks partial. The kernels themselves are covered at small shapes by test_gpu_hmh.py; here the offsets that exist only with more than
one pass or block are under test (the window over the sorted small rows, row numbers relative to the pass, cq + qa, sim + qa * nr, dlr + b0,
the reuse of the C | N and P-vector buffers)."""
import numpy as np
import pytest

import helpers as H
import pyref_hmh as PR

pytestmark = pytest.mark.gpu

M = 16384
CT = 128                # tile edge of k_hmh_cn
PB = 2048               # small sketches per P-vector block
NR = 20_000
TAIL = 77               # rows of the last pass


def qpass_of(nr):
    """query rows per pass, the formula of hmh_similarity_dev"""
    return max(CT, (1 << 28) // max(nr, 1) // CT * CT)


def _small_rows(rng, bases, n):
    """n distinct rows of cardinality <= 2^19: a base sketch of a 60-200 kbp genome with a random 2-90 % of its registers emptied; every
    tenth row keeps 0.5-3 % only, so that pairs of such rows from different bases have no register in common (C == 0)"""
    out = np.empty((n, M), np.uint16)
    for i in range(n):
        x = bases[i % len(bases)].copy()
        x[rng.random(M) < (rng.uniform(0.97, 0.995) if i % 10 == 0 else rng.uniform(0.02, 0.9))] = 0
        out[i] = x
    return out


def _large_rows(rng, bases, n):
    """n distinct rows of cardinality > 2^19: a base sketch of a 3-6 Mbp genome with a random 2-30 % of its registers redrawn among the
    values such genomes produce (7-13 leading zeros: smaller counts would pull the estimate under the limit)"""
    out = np.empty((n, M), np.uint16)
    for i in range(n):
        x = bases[i % len(bases)].copy()
        f = rng.random(M) < rng.uniform(0.02, 0.3)
        k = int(f.sum())
        x[f] = (rng.integers(7, 14, k) << 10 | rng.integers(0, 1024, k)).astype(np.uint16)
        out[i] = x
    return out


def _place(rng, n, small_at, n_small, small, large, empty_at, one_at, one):
    """n rows: `small` rows at the positions small_at, `large` rows elsewhere, the empty and the one-k-mer sketch at their own positions"""
    S = np.empty((n, M), np.uint16)
    is_small = np.zeros(n, bool)
    is_small[small_at] = True
    assert int(is_small.sum()) == n_small == len(small) and n - n_small == len(large)
    S[is_small] = small
    S[~is_small] = large
    S[empty_at] = 0
    S[one_at] = one
    return S


def _distinct(S):
    w = np.random.default_rng(1).integers(1, 1 << 62, M).astype(np.uint64)
    h = np.concatenate([(S[i:i + 2048].astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64) for i in range(0, len(S), 2048)])
    return len(np.unique(h)) == len(S)


def _blocks(rows_small_sorted, qa, qb):
    """sizes of the P-vector blocks the small rows of [qa, qb) are cut into"""
    n = int(((rows_small_sorted >= qa) & (rows_small_sorted < qb)).sum())
    return [min(PB, n - a) for a in range(0, n, PB)]


def test_similarity_across_passes_and_blocks(gpu_ctx):
    """13 389 x 20 000 sketches (2.7e8 pairs): two query passes (13 312 rows, then 77: not a tile multiple; 20 000 columns are not one
    either), the 2441 small query rows of the first pass in two P-vector blocks (2048 + 393), the 31 of the second pass in one, the 2500
    small reference rows in two blocks (2048 + 452); the test prints these figures as it computes them from the library's formulas.
    Checked (1) against the numpy reference on a sample that holds cells on both sides of every pass and block boundary, the corners, the
    last row and column and random cells of every class, (2) bit for bit against calls small enough to be one pass and one block per side,
    (3) bit for bit against the device-resident form.
    Peak host memory about 4 GB: the sketches (1.1 GB, twice while they are put together), the result (2.1 GB) and one slice of a second
    result at a time. About 9 s on an MI355X machine, most of it the host side (rows, reference cardinalities, the reference sample)."""
    import gsearch_amd as G
    ctx = gpu_ctx
    rng = np.random.default_rng(2024)
    nr = NR
    qpass = qpass_of(nr)
    nq = qpass + TAIL
    assert nq > qpass and (nq - qpass) % CT and nr % CT, "the shape no longer gives a partial second pass: qpass = %d" % qpass

    # ---- rows
    sb = [PR.sketch([H.dna_ascii(H.rand_dna(rng, n))], 21) for n in (60_000, 100_000, 200_000)]
    lb = [PR.sketch([H.dna_ascii(H.rand_dna(rng, n))], 21) for n in (3_000_000, 6_000_000)]
    one = PR.sketch([b"ACGTACGTACGTACGTACGTA"], 21)
    # small query rows: on both sides of the pass boundary, the boundary rows themselves, and some in the second pass only
    q_small = np.unique(np.concatenate([rng.choice(np.arange(qpass - 1), 2440, replace=False), [qpass - 1, qpass],
                                        qpass + 1 + rng.choice(np.arange(TAIL - 2), 30, replace=False)]))
    r_small = np.sort(rng.choice(np.arange(nr - 1), 2500, replace=False))
    q_empty, q_one, r_empty, r_one = 5, nq - 3, 100, 12_345
    q_small = q_small[(q_small != q_empty) & (q_small != q_one)]
    r_small = r_small[(r_small != r_empty) & (r_small != r_one)]
    Q = _place(rng, nq, q_small, len(q_small), _small_rows(rng, sb, len(q_small)), _large_rows(rng, lb, nq - len(q_small)), q_empty, q_one, one)
    R = _place(rng, nr, r_small, len(r_small), _small_rows(rng, sb, len(r_small)), _large_rows(rng, lb, nr - len(r_small)), r_empty, r_one, one)
    assert _distinct(Q) and _distinct(R), "two rows of one side are equal: a misplaced write between them could not be seen"

    # ---- classes, by the reference cardinality of every row (the device computes the same numbers: checked)
    cq = np.array([PR.cardinality(x) for x in Q], np.uint64)
    cr = np.array([PR.cardinality(x) for x in R], np.uint64)
    assert np.array_equal(G.hmh_cardinality(Q), cq) and np.array_equal(G.hmh_cardinality(R), cr)
    sq = np.flatnonzero((cq >= 1) & (cq <= PR.SMALL))
    sr = np.flatnonzero((cr >= 1) & (cr <= PR.SMALL))
    lq = np.flatnonzero(cq > PR.SMALL)
    lr = np.flatnonzero(cr > PR.SMALL)
    # (the one-k-mer sketch has reference cardinality 0, like the empty one: neither small nor large)
    assert np.array_equal(sq, q_small) and np.array_equal(sr, r_small)
    assert sorted(np.flatnonzero(cq == 0)) == sorted([q_empty, q_one]) and sorted(np.flatnonzero(cr == 0)) == sorted([r_empty, r_one])
    assert len(lq) == nq - len(sq) - 2 and len(lr) == nr - len(sr) - 2
    # the loops of hmh_similarity_dev at this shape
    passes = [(qa, min(qa + qpass, nq)) for qa in range(0, nq, qpass)]
    qblocks = [_blocks(sq, a, b) for a, b in passes]
    rblocks = _blocks(sr, 0, nr)
    print("passes %s, small query blocks per pass %s, small reference blocks %s" % ([b - a for a, b in passes], qblocks, rblocks))
    assert len(passes) >= 2 and (passes[-1][1] - passes[-1][0]) % CT
    assert len(qblocks[0]) >= 2 and qblocks[0][-1] < PB and len(qblocks[-1]) >= 1
    assert len(rblocks) >= 2 and rblocks[-1] < PB
    assert (qpass - 1) in sq and qpass in sq and (sq > qpass).any()

    # ---- the call under test
    sim = G.hmh_similarity_qxc(Q, R)
    assert sim.shape == (nq, nr)

    # ---- (1) the numpy reference on a sample
    def pick(a, n):
        return rng.choice(a, min(n, len(a)), replace=False)

    sample = {}
    for name, pos in (("pass", qpass),) + tuple(("qblock%d" % b, int(sq[b])) for b in range(PB, len(sq), PB) if sq[b] < qpass):
        # rows on both sides of the boundary against columns of both classes (a block boundary lies between consecutive SMALL rows)
        before = pos - 1 if name == "pass" else int(sq[np.searchsorted(sq, pos) - 1])
        cols = np.concatenate([pick(sr, 12), pick(lr, 12), [sr[PB - 1], sr[PB], 0, nr - 1]])
        sample[name] = [(q, int(r)) for q in (before, pos) for r in cols]
    for b in range(PB, len(sr), PB):
        rows = np.concatenate([pick(sq[sq < qpass], 12), pick(sq[sq >= qpass], 6), pick(lq, 8), [sq[PB - 1], sq[PB], qpass - 1, qpass]])
        sample["rblock%d" % b] = [(int(q), int(r)) for q in rows for r in (sr[b - 1], sr[b])]
    sample["corners"] = [(0, 0), (0, nr - 1), (nq - 1, 0), (nq - 1, nr - 1)]
    sample["last_row"] = [(nq - 1, r) for r in range(nr)]
    sample["last_col"] = [(q, nr - 1) for q in range(nq)]
    for nm, rows, cols in (("small_small", sq, sr), ("small_large", sq, lr), ("large_small", lq, sr), ("large_large", lq, lr)):
        sample[nm] = list(zip(pick(rows, 150).tolist() + pick(rows[rows >= qpass], 150).tolist(), rng.choice(cols, 300).tolist()))
    # C == 0 between sketches that are not empty: sparse small rows of different bases (chosen by the reference's count, not the result)
    sparse_q, sparse_r = sq[(Q[sq] != 0).sum(axis=1) < 600], sr[(R[sr] != 0).sum(axis=1) < 600]
    cand = zip(rng.choice(sparse_q, 600).tolist(), rng.choice(sparse_r, 600).tolist())
    sample["c_zero"] = [(q, r) for q, r in cand if PR.counts(Q[q], R[r])[0] == 0]
    sample["empty"] = [(q_empty, int(r)) for r in pick(np.arange(nr), 100)] + [(int(q), r_empty) for q in pick(np.arange(nq), 100)]
    sample["one_kmer"] = [(q_one, int(r)) for r in pick(np.arange(nr), 150)] + [(int(q), r_one) for q in pick(np.arange(nq), 150)]
    # every listed kind is there, on the side of the boundary it is named for
    assert {"pass", "qblock%d" % PB, "rblock%d" % PB, "corners", "last_row", "last_col", "small_small", "small_large", "large_small", "large_large",
            "c_zero", "empty", "one_kmer"} <= set(sample) and all(len(v) for v in sample.values())
    assert {q for q, _ in sample["pass"]} == {qpass - 1, qpass}
    assert {q for q, _ in sample["qblock%d" % PB]} == {int(sq[PB - 1]), int(sq[PB])}
    assert {r for _, r in sample["rblock%d" % PB]} == {int(sr[PB - 1]), int(sr[PB])}
    assert any(q >= qpass for q, _ in sample["small_small"]) and any(q < qpass for q, _ in sample["small_small"])
    seen, n_small_cells = set(), 0
    for name, cells in sample.items():
        for q, r in cells:
            if (q, r) in seen:
                continue
            seen.add((q, r))
            a, b = int(cq[q]), int(cr[r])
            ref = PR.similarity(Q[q], R[r], a, b)
            small = max(a, b) <= PR.SMALL
            n_small_cells += small
            assert abs(sim[q, r] - ref) <= (1e-9 if small else 1e-12), (name, q, r, a, b, sim[q, r], ref)
    assert len(sample["c_zero"]) >= 100 and n_small_cells >= 500
    assert all(sim[q, r] == 0.0 for name in ("c_zero", "empty", "one_kmer") for q, r in sample[name])
    # both branches produce non-zero similarities in the second pass and in the second blocks: the cells are not trivially equal
    assert (sim[qpass:][:, sr[PB:]] > 0).any() and (sim[sq[PB:PB + 50]][:, sr[PB:]] > 0).any() and (sim[qpass:][:, lr] > 0).any()

    # ---- (2) bit for bit against calls of one pass and one block per side
    q_step, r_cuts = 3000, [0, nr // 2, nr]
    for c0, c1 in zip(r_cuts[:-1], r_cuts[1:]):
        assert int(((sr >= c0) & (sr < c1)).sum()) <= PB and q_step <= qpass_of(c1 - c0) and q_step * (c1 - c0) < 1 << 28
        Rp = np.ascontiguousarray(R[c0:c1])
        for a in range(0, nq, q_step):
            b = min(a + q_step, nq)
            assert int(((sq >= a) & (sq < b)).sum()) <= PB
            part = G.hmh_similarity_qxc(Q[a:b], Rp)
            bad = np.argwhere(part != sim[a:b, c0:c1])
            assert len(bad) == 0, "%d cells differ from the single-pass call, the first at row %d, column %d: %r vs %r" % (
                len(bad), a + bad[0][0], c0 + bad[0][1], sim[a + bad[0][0], c0 + bad[0][1]], part[bad[0][0], bad[0][1]])
            del part

    # ---- (3) the device-resident form at the same shape, compared pass-sized chunk by chunk
    dq, dr, ds = ctx.alloc(Q.nbytes), ctx.alloc(R.nbytes), ctx.alloc(8 * nq * nr)
    try:
        ctx.upload(dq, Q); ctx.upload(dr, R)
        ctx.memset(ds, 0xFF, 8 * nq * nr)                   # (a cell the call leaves alone reads as NaN and compares unequal)
        G.hmh_similarity_qxc_dev(ctx, dq, nq, dr, nr, ds)
        ctx.sync()
        for a in range(0, nq, 2000):
            b = min(a + 2000, nq)
            assert np.array_equal(ctx.download(ds + 8 * a * nr, (b - a, nr), np.float64), sim[a:b]), "rows %d..%d of the _dev form differ" % (a, b)
    finally:
        for p in (dq, dr, ds):
            ctx.free(p)
        ctx.release_scratch()
