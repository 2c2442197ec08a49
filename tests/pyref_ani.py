"""numpy restatement of SPEC 12 (superani: FracMinHash seeds, anchors, colinear chaining, per-side counts, closed form, writer).
It takes nothing from the library: the device tests compare integers with `==` against what is computed here."""
import math

import numpy as np

W, B, G, MAX_OCC, MIN_ANCHORS = 20, 64, 2500, 4, 3
NONE = 0xFFFFFFFF
MIN_AF = 0.10
M64 = (1 << 64) - 1
_CODE = np.full(256, 255, np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch + 32] = _i


def clean(rec):
    """bytes -> base codes 0..3 of the kept bases (everything but ACGT / acgt dropped)"""
    c = _CODE[np.frombuffer(bytes(rec), np.uint8)]
    return c[c != 255]


def mix(v):
    """output function of SplitMix64 (SPEC 2) applied to x = v, elementwise on uint64"""
    z = np.asarray(v, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def bases(genome):
    return int(sum(len(clean(r)) for r in genome))


def seeds(genome, k=16, c=30):
    """genome: list of records (bytes) -> (n, 4) uint32 {value, contig, pos, fwd} in position order"""
    assert 8 <= k <= 16 and c >= 1
    thr = np.uint64(M64 // c)
    out = []
    for ci, rec in enumerate(genome):
        code = clean(rec).astype(np.uint64)
        nw = len(code) - k + 1
        if nw <= 0:
            continue
        fwd = np.zeros(nw, np.uint64)
        rc = np.zeros(nw, np.uint64)
        for t in range(k):
            fwd = fwd * np.uint64(4) + code[t:t + nw]
            rc = rc + ((np.uint64(3) - code[t:t + nw]) << np.uint64(2 * t))
        v = np.minimum(fwd, rc)
        keep = np.nonzero(mix(v) <= thr)[0]
        s = np.zeros((len(keep), 4), np.uint32)
        s[:, 0] = v[keep]
        s[:, 1] = ci
        s[:, 2] = keep
        s[:, 3] = v[keep] == fwd[keep]
        out.append(s)
    return np.concatenate(out) if out else np.zeros((0, 4), np.uint32)


def anchors(qs, rs):
    """-> dict of int64 arrays rcontig, rpos, qcontig, qpos, strand, ridx, qidx, ordered by r seed index, then q seed index"""
    qv, rv = qs[:, 0].astype(np.int64), rs[:, 0].astype(np.int64)
    order = np.argsort(qv, kind="stable")
    qsorted = qv[order]
    left, right = np.searchsorted(qsorted, rv, "left"), np.searchsorted(qsorted, rv, "right")
    occ_q = right - left
    _, inv, cnt = np.unique(rv, return_inverse=True, return_counts=True)
    occ_r = cnt[inv] if len(rv) else np.zeros(0, np.int64)
    n = np.where((occ_q <= MAX_OCC) & (occ_r <= MAX_OCC), occ_q, 0)
    ridx = np.repeat(np.arange(len(rv)), n)
    within = np.arange(len(ridx)) - np.repeat(np.cumsum(n) - n, n)
    qidx = order[np.repeat(left, n) + within] if len(ridx) else np.zeros(0, np.int64)
    q, r = qs[qidx].astype(np.int64), rs[ridx].astype(np.int64)
    return {"rcontig": r[:, 1], "rpos": r[:, 2], "qcontig": q[:, 1], "qpos": q[:, 2], "strand": r[:, 3] ^ q[:, 3], "ridx": ridx.astype(np.int64),
            "qidx": np.asarray(qidx, np.int64)}


def chain(a):
    """the dynamic program of SPEC 12 over one pair's anchors -> (f int64, pred, root); pred = NONE where an anchor starts a chain"""
    rc, rp, qc, qp, s = (np.asarray(a[x], np.int64) for x in ("rcontig", "rpos", "qcontig", "qpos", "strand"))
    n = len(rp)
    f = np.full(n, W, np.int64)
    pred = np.full(n, NONE, np.int64)
    root = np.arange(n, dtype=np.int64)
    for i in range(n):
        lo = max(0, i - B)
        if lo == i:
            continue
        j = slice(lo, i)
        dr = rp[i] - rp[j]
        dq = qp[i] - qp[j] if s[i] == 0 else qp[j] - qp[i]
        ok = (rc[j] == rc[i]) & (qc[j] == qc[i]) & (s[j] == s[i]) & (dr >= 1) & (dr <= G) & (dq >= 1) & (dq <= G)
        if not ok.any():
            continue
        cand = np.where(ok, f[j] + W - np.abs(dr - dq), -(1 << 62))
        m = int(cand.max())
        if m > W:
            jj = lo + len(cand) - 1 - int(np.argmax(cand[::-1] == m))        # the largest j among the best
            f[i], pred[i], root[i] = m, jj, root[jj]
    return f, pred, root


def kept_chains(f, pred, root):
    """-> list of chains (anchor indices from the end back to the root) with at least MIN_ANCHORS anchors"""
    best = {}
    for i in range(len(f)):
        r = int(root[i])
        if r not in best or f[i] > f[best[r]]:
            best[r] = i                                              # ties: the smallest index stays
    out = []
    for r in sorted(best):
        path, x = [], best[r]
        while True:
            path.append(x)
            if pred[x] == NONE:
                break
            x = int(pred[x])
        if len(path) >= MIN_ANCHORS:
            out.append(path)
    return out


def side(sd, idx, chains, k):
    """seeds of one side, the seed index of every anchor on that side, the kept chains -> (M, C, A)"""
    n = len(sd)
    matched = np.zeros(n, bool)
    diff = np.zeros(n + 1, np.int64)
    for path in chains:
        ii = idx[path]
        matched[ii] = True
        diff[ii.min()] += 1
        diff[ii.max() + 1] -= 1
    cov = np.cumsum(diff[:n]) > 0
    ctg, pos = sd[:, 1].astype(np.int64), sd[:, 2].astype(np.int64)
    joined = np.zeros(n, bool)                                       # seed i continues the run of seed i - 1
    if n > 1:
        joined[1:] = cov[1:] & cov[:-1] & (ctg[1:] == ctg[:-1])
    start = cov & ~joined
    end = cov & ~np.append(joined[1:], False)
    return int((matched & cov).sum()), int(cov.sum()), int((pos[end] + k).sum() - pos[start].sum())


def pair_counts(qs, rs, k=16):
    """-> [n_anchors, n_chains_kept, M_q, C_q, A_q, M_r, C_r, A_r]"""
    a = anchors(qs, rs)
    f, pred, root = chain(a)
    ch = kept_chains(f, pred, root)
    return [len(f), len(ch), *side(qs, a["qidx"], ch, k), *side(rs, a["ridx"], ch, k)]


def estimate(counts, bases_q, bases_r, k=16):
    """the closed form: -> (ani, af_q, af_r) as float32"""
    _, _, mq, cq, aq, _, _, ar = (int(x) for x in counts)
    ani = math.pow(mq / cq, 1.0 / k) if cq else 0.0
    afq = aq / bases_q if bases_q else 0.0
    afr = ar / bases_r if bases_r else 0.0
    if max(afq, afr) < MIN_AF:
        ani = 0.0
    return np.float32(ani), np.float32(afq), np.float32(afr)


def fmt_f32(x):
    """Rust's `{}` of an f32: the fewest significant digits that read back to the same f32, positional, no trailing `.0`"""
    x = np.float32(x)
    if x == 0:
        return "0"
    for p in range(0, 9):
        s = "%.*e" % (p, float(x))
        if np.float32(float(s)) == x:
            break
    mant, exp = s.split("e")
    sign = "-" if mant.startswith("-") else ""
    digits, e = mant.lstrip("-").replace(".", ""), int(exp)
    if e >= len(digits) - 1:
        return sign + digits + "0" * (e - len(digits) + 1)
    if e >= 0:
        return sign + digits[:e + 1] + "." + digits[e + 1:]
    return sign + "0." + "0" * (-e - 1) + digits


def superani_text(query_paths, ref_paths, est):
    """est[j][i] = (ani, af_q, af_r) of reference j and query i -> the bytes of the output file: reference-major, then query"""
    out = []
    for j, r in enumerate(ref_paths):
        for i, q in enumerate(query_paths):
            out.append("%s\t%s\t%s\t%s\t%s\n" % (q, r, fmt_f32(est[j][i][0]), fmt_f32(est[j][i][1]), fmt_f32(est[j][i][2])))
    return "".join(out).encode("utf-8")


# ---- test genomes (shared by the host and the device tests) -------------------------------------------------------------------------------
def random_genome(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def substitute(rng, g, p):
    a = np.frombuffer(g, np.uint8).copy()
    hit = np.nonzero(rng.random(len(a)) < p)[0]
    code = _CODE[a[hit]]
    a[hit] = np.frombuffer(b"ACGT", np.uint8)[(code + rng.integers(1, 4, len(hit))) % 4]
    return bytes(a)


def indels(rng, g, p):
    out, i = bytearray(), 0
    for at in np.nonzero(rng.random(len(g)) < p)[0]:
        out += g[i:at]
        if rng.random() < 0.5:
            out += random_genome(rng, 1)
            i = at
        else:
            i = at + 1
    return bytes(out + g[i:])


def revcomp(g):
    return bytes(g[::-1]).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))
