"""Independent numpy restatement of SPEC.md section 8 (ann: k-NN graph statistics and the UMAP-like embedding) and of SPEC 2's EXP.

Vectorised over nodes. Every sum keeps the order the SPEC pins: ragged sums walk the slots in order and add only where a node has that slot
(np.where / index subsets), never a padded zero, so that -0.0 stays -0.0. All epoch arithmetic is float32 (+ - * / and compares), the
calibration float64; numpy rounds every operation once and contracts nothing, as the device build does (-ffp-contract=off)."""
import numpy as np

U64 = np.uint64
GAMMA = U64(0x9E3779B97F4A7C15)
TAG_INIT, TAG_NEG = U64(0x696E6974), U64(0x6E6567)
LN2_HI, LN2_LO, INV_LN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00

# SPEC 8 constants (gs_spec.hpp)
DIM, EPOCHS, NEG, NEG_RATE, LR, SEED = 2, 300, 8, 1.0, 0.25, 0x5EED
LIGHT, CLAMP, EPS = 64, np.float32(4.0), np.float32(0.001)
BISECT, TOL, MIN_SCALE = 64, 1e-5, 1e-3
HIST_BINS, HUBS = 64, 16
QUANTILES = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
F = np.float32


def defaults(**kw):
    p = dict(dim=DIM, epochs=EPOCHS, neg_samples=NEG, neg_rate=NEG_RATE, lr=LR, seed=SEED)
    p.update(kw)
    return p


# ---- SPEC 2 ------------------------------------------------------------------------------------------------------------------------------
def spec_ln(x):
    x = np.asarray(x, np.float64)
    bits = x.view(np.uint64)
    e = ((bits >> U64(52)) & U64(0x7FF)).astype(np.int64) - 1023
    t = ((bits & U64(0x000FFFFFFFFFFFFF)) | U64(0x3FF0000000000000)).view(np.float64)
    big = t > 1.4142135623730951
    t = np.where(big, t * 0.5, t)
    e = e + big
    s = (t - 1.0) / (t + 1.0)
    z = s * s
    p = np.full_like(s, 1.0 / 23.0)
    for d in (21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    return e.astype(np.float64) * 0.6931471805599453 + 2.0 * s * p


def _pow2(k):
    return ((k + 1023).astype(np.uint64) << U64(52)).view(np.float64)


def spec_exp(x):
    """SPEC 2 EXP: Cody-Waite by ln 2, degree-13 Horner, exact power-of-two scale (two factors below 2^-1022)"""
    x = np.asarray(x, np.float64)
    scalar = x.ndim == 0
    x = np.atleast_1d(x)
    lo, hi, nan = x < -745.2, x > 709.7, np.isnan(x)
    xs = np.where(lo | hi | nan, 0.0, x)
    k = np.trunc(xs * INV_LN2 + np.where(xs < 0.0, -0.5, 0.5)).astype(np.int64)
    kf = k.astype(np.float64)
    r = (xs - kf * LN2_HI) - kf * LN2_LO
    p = np.full_like(r, 1.0 / 6227020800.0)
    for f in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / f
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    sub = k < -1022
    out = np.where(sub, (p * _pow2(np.where(sub, k + 1000, 0))) * _pow2(np.full_like(k, -1000)), p * _pow2(np.where(sub, 0, k)))
    out = np.where(lo, 0.0, np.where(hi, np.inf, np.where(nan, x, out)))
    return out[0] if scalar else out


def mix(z):
    """SplitMix64 output function (uint64 arrays, wrapping)"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def mulhi(a, b):
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    m32 = U64(0xFFFFFFFF)
    al, ah, bl, bh = a & m32, a >> U64(32), b & m32, b >> U64(32)
    with np.errstate(over="ignore"):
        ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
        mid = (ll >> U64(32)) + (lh & m32) + (hl & m32)
        return hh + (lh >> U64(32)) + (hl >> U64(32)) + (mid >> U64(32))


def init_positions(n, dim, seed):
    """seeded initial positions in [-10, 10): 24 bits of mix(mix(seed ^ "init") + GAMMA (i dim + t + 1)), exact in f32"""
    s = np.arange(n * dim, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix(mix(U64(seed) ^ TAG_INIT) + GAMMA * (s + U64(1)))
    u = (h >> U64(40)).astype(np.float32) * F(2.0 ** -24)
    return (u * F(20.0) - F(10.0)).reshape(n, dim)


def epoch_key(seed, e):
    with np.errstate(over="ignore"):
        return mix(U64(seed) ^ TAG_NEG) + GAMMA * U64(e + 1)


def neg_samples(seed, e, n, S):
    """(n, S) negative samples of epoch e: mulhi(mix(mix(ekey) + GAMMA (i S + s + 1)), n)"""
    c = np.arange(n * S, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix(mix(epoch_key(seed, e)) + GAMMA * (c + U64(1)))
    return mulhi(h, U64(n)).reshape(n, S)


# ---- input rules, calibration, union, adjacency -------------------------------------------------------------------------------------------
def validate(ids, dist, cnt):
    """the SPEC 8 input rules; returns a list of the broken ones (empty: valid)"""
    n, knbn = ids.shape
    bad = []
    if (cnt > knbn).any():
        return ["count"]
    for i in range(n):
        c = int(cnt[i])
        r, d = ids[i, :c], dist[i, :c]
        if (r >= n).any():
            bad.append("id")
        if (r == i).any():
            bad.append("self")
        if len(np.unique(r)) != c:
            bad.append("repeat")
        if not (d >= 0).all() or (c > 1 and (d[1:] < d[:-1]).any()):
            bad.append("dist")
    return sorted(set(bad))


def calibrate(dist, cnt):
    """memberships p (n, knbn) f32: rho = smallest distance > 0, sigma by bisection to sum = log2(count), floored at 1e-3 x mean"""
    dist = np.asarray(dist, np.float32)
    n, knbn = dist.shape
    cnt = np.asarray(cnt, np.int64)
    p = np.zeros((n, knbn), np.float32)
    p[cnt == 1, 0] = 1.0
    rows = np.nonzero(cnt >= 2)[0]
    if len(rows) == 0:
        return p
    d = dist[rows].astype(np.float64)
    c = cnt[rows]
    slot = np.arange(knbn)[None, :] < c[:, None]
    posd = slot & (dist[rows] > 0)
    first = np.argmax(posd, axis=1)
    rho = np.where(posd.any(axis=1), d[np.arange(len(rows)), first], 0.0)
    target = spec_ln(c.astype(np.float64)) / spec_ln(2.0)
    lo, hi, mid = np.zeros(len(rows)), np.zeros(len(rows)), np.ones(len(rows))
    hi_inf, active = np.ones(len(rows), bool), np.ones(len(rows), bool)
    dd = d - rho[:, None]

    def psum(sig):
        ps = np.zeros(len(rows))
        for t in range(knbn):
            x = dd[:, t]
            v = np.where(x > 0.0, spec_exp(-(x / sig)), 1.0)
            ps = np.where(slot[:, t], ps + v, ps)
        return ps
    for _ in range(BISECT):
        ps = psum(mid)
        active = active & ~(np.abs(ps - target) < TOL)
        up = active & (ps > target)
        dn = active & ~(ps > target)
        hi = np.where(up, mid, hi)
        hi_inf = np.where(up, False, hi_inf)
        lo = np.where(dn, mid, lo)
        mid = np.where(up, (lo + hi) / 2.0, np.where(dn, np.where(hi_inf, mid * 2.0, (lo + hi) / 2.0), mid))
        if not active.any():
            break
    mean = np.zeros(len(rows))
    for t in range(knbn):
        mean = np.where(slot[:, t], mean + d[:, t], mean)
    mean = mean / c.astype(np.float64)
    mid = np.where(mid < MIN_SCALE * mean, MIN_SCALE * mean, mid)
    for t in range(knbn):
        x = dd[:, t]
        v = np.where(x > 0.0, spec_exp(-(x / mid)), 1.0).astype(np.float32)
        p[rows, t] = np.where(slot[:, t], v, 0.0)
    return p


def adjacency(ids, cnt, memb):
    """CSR (off, adj u32, w f32) and W (n,) f32: node i's own row in row order, then the nodes j whose row holds i and i's row does not,
    ascending by j; w = (p_ij + p_ji) - p_ij p_ji; W_i summed in adjacency order"""
    n, knbn = ids.shape
    cnt = np.asarray(cnt, np.int64)
    slot = np.arange(knbn)[None, :] < cnt[:, None]
    src = np.repeat(np.arange(n, dtype=np.int64), knbn).reshape(n, knbn)[slot]
    dst = ids[slot].astype(np.int64)
    pe = memb[slot].astype(np.float32)
    tt = np.tile(np.arange(knbn), n).reshape(n, knbn)[slot]
    key = src * n + dst
    order = np.argsort(key)
    skey, sp = key[order], pe[order]

    def lookup(k):
        pos = np.searchsorted(skey, k)
        pos = np.minimum(pos, len(skey) - 1)
        hit = skey[pos] == k if len(skey) else np.zeros(len(k), bool)
        return hit, np.where(hit, sp[pos] if len(skey) else 0, 0).astype(np.float32)
    hit_r, p_r = lookup(dst * n + src)          # does dst's row hold src, and with which p
    w_fwd = (pe + p_r) - pe * p_r
    rev = ~hit_r                               # dst gets src as a reverse-only entry
    zero = np.zeros(rev.sum(), np.float32)
    w_rev = (zero + pe[rev]) - zero * pe[rev]
    node = np.concatenate([src, dst[rev]])
    nbr = np.concatenate([dst, src[rev]])
    grp = np.concatenate([np.zeros(len(src), np.int64), np.ones(rev.sum(), np.int64)])
    sub = np.concatenate([tt, src[rev]])
    w = np.concatenate([w_fwd, w_rev]).astype(np.float32)
    o = np.lexsort((sub, grp, node))
    node, adj, w = node[o], nbr[o].astype(np.uint32), w[o]
    deg = np.bincount(node, minlength=n).astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(deg)
    W = np.zeros(n, np.float32)
    for k in range(int(deg.max()) if n else 0):
        a = np.nonzero(deg > k)[0]
        W[a] = W[a] + w[off[a] + k]
    return off, adj, w, W


# ---- epochs ---------------------------------------------------------------------------------------------------------------------------
def _clamp(x):
    return np.where(x > CLAMP, CLAMP, np.where(x < -CLAMP, -CLAMP, x))


def _terms(yi, yj, c_of_d2):
    diff = yi - yj
    d2 = diff[:, 0] * diff[:, 0]
    for t in range(1, diff.shape[1]):
        d2 = d2 + diff[:, t] * diff[:, t]
    c = c_of_d2(d2)
    return _clamp(c[:, None] * diff)


def _seq_terms(y, nodes, ks, off, deg, adj, w, g2, negs, S):
    """terms of entries ks (one per node in `nodes`) of the attraction-then-negative sequences; valid: where the entry contributes"""
    D = y.shape[1]
    out = np.zeros((len(nodes), D), np.float32)
    valid = np.zeros(len(nodes), bool)
    att = ks < deg[nodes]
    if att.any():
        a = nodes[att]
        e = off[a] + ks[att]
        j = adj[e].astype(np.int64)
        wk = w[e]
        out[att] = _terms(y[a], y[j], lambda d2: (F(-2.0) * wk) / (F(1.0) + d2))
        valid[att] = True
    neg = ~att & (ks < deg[nodes] + S)
    if neg.any():
        a = nodes[neg]
        j = negs[a, ks[neg] - deg[a]].astype(np.int64)
        keep = j != a
        a, j = a[keep], j[keep]
        idx = np.nonzero(neg)[0][keep]
        g = g2[a]
        out[idx] = _terms(y[a], y[j], lambda d2: g / ((EPS + d2) * (F(1.0) + d2)))
        valid[idx] = True
    return out, valid


def epoch(y, e, off, adj, w, W, p):
    n, D = y.shape
    E, S = p["epochs"], p["neg_samples"]
    deg = (off[1:] - off[:-1]).astype(np.int64)
    negs = neg_samples(p["seed"], e, n, S)
    g2 = F(2.0) * ((F(p["neg_rate"]) * W) / F(S))
    acc = np.zeros((n, D), np.float32)
    light = np.nonzero(deg <= LIGHT)[0]
    L = deg[light] + S
    for k in range(int(L.max()) if len(light) else 0):
        a = light[L > k]
        t, v = _seq_terms(y, a, np.full(len(a), k), off, deg, adj, w, g2, negs, S)
        acc[a[v]] = acc[a[v]] + t[v]
    heavy = np.nonzero(deg > LIGHT)[0]
    if len(heavy):
        Lh = deg[heavy] + S
        part = np.zeros((len(heavy), 64, D), np.float32)
        for r in range(int((Lh.max() + 63) // 64)):
            hs = np.nonzero(Lh > r * 64)[0]
            ks = r * 64 + np.arange(64)
            hh, ll = np.repeat(hs, 64), np.tile(np.arange(64), len(hs))
            kk = np.tile(ks, len(hs))
            inside = kk < Lh[hh]
            hh, ll, kk = hh[inside], ll[inside], kk[inside]
            t, v = _seq_terms(y, heavy[hh], kk, off, deg, adj, w, g2, negs, S)
            part[hh[v], ll[v]] = part[hh[v], ll[v]] + t[v]
        o = 32
        while o >= 1:
            part[:, :o] = part[:, :o] + part[:, o:2 * o]
            o //= 2
        acc[heavy] = part[:, 0]
    lr_e = F(p["lr"]) * (F(E - e) / F(E))
    return y + lr_e * acc


def embed(ids, dist, cnt, params=None, init=None, return_memb=False):
    """positions (n, dim) f32 after E epochs (SPEC 8)"""
    p = params or defaults()
    ids = np.asarray(ids, np.uint64)
    n = ids.shape[0]
    memb = calibrate(dist, cnt)
    off, adj, w, W = adjacency(ids, cnt, memb)
    y = init_positions(n, p["dim"], p["seed"]) if init is None else np.array(init, np.float32)
    for e in range(p["epochs"]):
        y = epoch(y, e, off, adj, w, W, p)
    return (y, memb) if return_memb else y


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def stats(ids, dist, cnt):
    n, knbn = ids.shape
    cnt = np.asarray(cnt, np.int64)
    slot = np.arange(knbn)[None, :] < cnt[:, None]
    occ = np.bincount(ids[slot].astype(np.int64), minlength=n).astype(np.uint32)
    n_edges = int(cnt.sum())
    mean = n_edges / n
    dv = occ.astype(np.float64) - mean
    m2 = float(np.cumsum(dv * dv)[-1])
    m3 = float(np.cumsum((dv * dv) * dv)[-1])
    std = float(np.sqrt(m2 / n))
    skew = (m3 / n) / (std * std * std) if std > 0 else 0.0
    hist = np.bincount(np.minimum(occ, HIST_BINS).astype(np.int64), minlength=HIST_BINS + 1).astype(np.uint64)
    order = np.lexsort((np.arange(n), -occ.astype(np.int64)))[:HUBS]
    rows = cnt >= 1
    first = np.sort(dist[rows, 0].astype(np.float32))
    last = np.sort(dist[np.nonzero(rows)[0], cnt[rows] - 1].astype(np.float32))
    N = len(first)
    qi = [int(np.floor(q * (N - 1))) for q in QUANTILES]
    return dict(n=n, knbn=knbn, n_edges=n_edges, n_empty=int((cnt == 0).sum()), max_occ=int(occ.max()), occ_mean=mean, occ_std=std, occ_skew=skew,
                hubs=[(int(i), int(occ[i])) for i in order], q_first=np.array([first[k] for k in qi] if N else [np.nan] * 7, np.float32),
                q_last=np.array([last[k] for k in qi] if N else [np.nan] * 7, np.float32), occ=occ, hist=hist)


# ---- quality ------------------------------------------------------------------------------------------------------------------------
def family_purity(xy, fam, k=10):
    """mean over points of the fraction of their k nearest 2-D neighbours (f64 Euclidean, ties by index) in the same family"""
    xy = np.asarray(xy, np.float64)
    d = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((fam[nn] == fam[:, None]).mean())
