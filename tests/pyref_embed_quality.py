"""numpy restatement of SPEC.md section 8.1 (ann: the quality of an embedding by neighbourhood conservation), written from the SPEC text alone; it shares
no code with the library. The per-node arrays have two definitions here, which tests/test_embed_quality_cpu.py holds to each other:

  * arrays_sort  : every row's distances to the other nodes sorted; rad2 is element kq_eff - 1, rank the position of e2 from the left;
  * arrays_count : rank counts d2 < e2; rad2 is the one value x with #{d2 < x} < kq_eff <= #{d2 <= x}, found by halving the range of bit patterns.

The summary (f64) and the text report follow from the arrays."""
import numpy as np

import pyref_embed as R8

F = np.float32
QUANTILES = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
DIM_MAX = 4
UNUSED = np.uint32(0xFFFFFFFF)
BLOCK = 256


def refusals(ids, dist, cnt, pos, kq):
    """the broken input rules (empty: valid)"""
    n = ids.shape[0]
    bad = list(R8.validate(ids, dist, cnt)) if n else []
    pos = np.asarray(pos)
    if n < 2:
        bad.append("n")
    if kq < 1:
        bad.append("kq")
    if pos.ndim != 2 or not 1 <= pos.shape[1] <= DIM_MAX:
        bad.append("dim")
    elif not np.isfinite(pos).all():
        bad.append("coordinate")
    return bad


def d2_rows(y, rows):
    """d2(i, j) for i in rows and every j: the sum over t in order, from +0, of (y_i[t] - y_j[t])^2, every operation in f32"""
    y = np.asarray(y, F)
    out = np.zeros((len(rows), len(y)), F)
    with np.errstate(over="ignore"):
        for t in range(y.shape[1]):
            df = y[rows, t][:, None] - y[None, :, t]
            out = out + df * df
    assert out.dtype == F and not np.isnan(out).any() and not np.signbit(out).any()
    return out


def _blocks(n):
    return [np.arange(b, min(n, b + BLOCK)) for b in range(0, n, BLOCK)]


def _edges(D, rows, ids, cnt, e2):
    for r, i in enumerate(rows):
        c = int(cnt[i])
        e2[i, :c] = D[r, ids[i, :c].astype(np.int64)]


def arrays_sort(ids, cnt, pos, kq):
    n, knbn = ids.shape
    kq_eff = min(int(kq), n - 1)
    rank, e2, rad2 = np.full((n, knbn), UNUSED), np.zeros((n, knbn), F), np.zeros(n, F)
    for rows in _blocks(n):
        D = d2_rows(pos, rows)
        _edges(D, rows, ids, cnt, e2)
        for r, i in enumerate(rows):
            others = np.sort(np.delete(D[r], i))
            rad2[i] = others[kq_eff - 1]
            c = int(cnt[i])
            rank[i, :c] = np.searchsorted(others, e2[i, :c], side="left")
    return rank, e2, rad2


def arrays_count(ids, cnt, pos, kq):
    n, knbn = ids.shape
    kq_eff = min(int(kq), n - 1)
    rank, e2, rad2 = np.full((n, knbn), UNUSED), np.zeros((n, knbn), F), np.zeros(n, F)
    for rows in _blocks(n):
        D = d2_rows(pos, rows)
        _edges(D, rows, ids, cnt, e2)
        other = np.ones(D.shape, bool)
        other[np.arange(len(rows)), rows] = False
        for r, i in enumerate(rows):
            for t in range(int(cnt[i])):
                rank[i, t] = int(((D[r] < e2[i, t]) & other[r]).sum())
        bits = D.view(np.uint32).astype(np.int64)
        lo, hi = np.zeros(len(rows), np.int64), np.full(len(rows), 0x7F800000, np.int64)     # +0 .. +inf
        while (lo < hi).any():
            mid = (lo + hi) // 2
            enough = ((bits <= mid[:, None]) & other).sum(axis=1) >= kq_eff
            hi = np.where(enough, mid, hi)
            lo = np.where(enough, lo, mid + 1)
        x = lo.astype(np.uint32).view(F)
        assert ((((D < x[:, None]) & other).sum(axis=1) < kq_eff) & (((D <= x[:, None]) & other).sum(axis=1) >= kq_eff)).all()
        rad2[rows] = x
    return rank, e2, rad2


def _quantiles(v):
    v = np.sort(np.asarray(v, np.float64))
    N = len(v)
    return np.array([v[int(np.floor(q * (N - 1)))] if N else np.nan for q in QUANTILES], np.float64)


def summary(cnt, rank, e2, rad2, kq):
    n, knbn = rank.shape
    cnt = np.asarray(cnt, np.int64)
    kq_eff = min(int(kq), n - 1)
    used = np.arange(knbn)[None, :] < cnt[:, None]
    has = cnt >= 1
    c = ((rank < kq_eff) & used).sum(axis=1)
    n_rows, n_edges, n_conserved = int(has.sum()), int(cnt.sum()), int(c.sum())
    n_nomatch = int((has & (c == 0)).sum())
    emax2 = np.where(used, e2, F(0)).max(axis=1)[has].astype(np.float64)
    r2 = np.asarray(rad2, F)[has].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.sqrt(emax2 / r2)
    ratio[(emax2 == 0) & (r2 == 0)] = 1.0
    ratio[(emax2 != 0) & (r2 == 0)] = np.inf
    ratio[np.isinf(emax2) & np.isinf(r2)] = 1.0
    return dict(n=n, knbn=knbn, kq=int(kq), kq_eff=kq_eff, n_rows=n_rows, n_edges=n_edges, n_conserved=n_conserved, n_nomatch=n_nomatch,
                mean_conserved=n_conserved / (n_rows - n_nomatch) if n_rows > n_nomatch else 0.0,
                frac_conserved=n_conserved / n_edges if n_edges else float("nan"),
                hist_conserved=np.bincount(c[has], minlength=knbn + 1).astype(np.uint64), quantiles=list(QUANTILES),
                q_edge=_quantiles(np.sqrt(emax2)), q_radius=_quantiles(np.sqrt(r2)), q_ratio=_quantiles(ratio))


def quality(ids, dist, cnt, pos, kq=200, arrays=arrays_sort):
    assert not refusals(ids, dist, cnt, pos, kq)
    rank, e2, rad2 = arrays(ids, cnt, np.asarray(pos, F), kq)
    s = summary(cnt, rank, e2, rad2, kq)
    s["rank"], s["e2"], s["rad2"] = rank, e2, rad2
    return s


def text(s):
    """the report of SPEC 8.1: seven fixed lines, numbers as C's %g (the quantile levels) and %.6g"""
    def row(name, v):
        return "%s quantiles: %s\n" % (name, " ".join("%g:%.6g" % (q, x) for q, x in zip(QUANTILES, v)))
    return ("embedding quality of %d nodes, knbn %d: %d rows with neighbours, %d edges, kq %d\n" % (s["n"], s["knbn"], s["n_rows"], s["n_edges"], s["kq_eff"])
            + "neighbourhoods without a match: %d\n" % s["n_nomatch"]
            + "neighbours conserved per matched row: mean %.6g\n" % s["mean_conserved"]
            + "edges conserved: %d, fraction %.6g\n" % (s["n_conserved"], s["frac_conserved"])
            + row("embedded edge length", s["q_edge"]) + row("embedded radius", s["q_radius"]) + row("edge / radius", s["q_ratio"]))
