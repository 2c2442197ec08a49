"""SPEC 13.1 (hmmsearch: Forward scores behind a Viterbi floor) restated in numpy, plus a cell-by-cell f64 Forward that is the restatement's own
yardstick. The scored path is integers only (int64 arrays that hold int32 values); the table of lse is computed here in f64, on its own. The model,
the tables, the specials, NEG and STAR are those of SPEC 13 (pyref_hmm.py). Nothing here calls the library."""
import math

import numpy as np

import pyref_hmm as R

NEG, STAR, NO_SCORE = R.NEG, R.STAR, R.NO_SCORE
LSE_N = 5903                                       # entries of T that are not 0
FWD_MAX_L = 65536
CLASS_G = (1, 2, 3, 4, 6, 8, 12, 16, 20)           # nodes per group; a profile takes the smallest G with 64 G >= M
FLOOR_ALL = -(1 << 31) + 1                         # the floor of a profile without STATS LOCAL VITERBI: every pair that has a Viterbi score


def logsum_table():
    """T[j] = floor(1024 log2(1 + 2^(-2 j / 1024)) + 1/2), j = 0 .. 5902, and T[5903] = 0 -> int64 [5904]"""
    t = [int(math.floor(1024.0 * math.log2(1.0 + 2.0 ** (-2.0 * j / 1024.0)) + 0.5)) for j in range(LSE_N)]
    return np.array(t + [0], np.int64)


T = logsum_table()


def lse(a, b):
    """hi + T[min((hi - lo + 1) >> 1, 5903)] on integers (scalars or arrays)"""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    return hi + T[np.minimum((hi - lo + 1) >> 1, LSE_N)]


def group_size(M):
    return next(g for g in CLASS_G if 64 * g >= M)


def stats_lines(text):
    """per model of a HMMER3 text: ([msv mu, lambda, viterbi mu, lambda, forward tau, lambda], has) with has bit 0 / 1 / 2 = the line was there"""
    if isinstance(text, bytes):
        text = text.decode("ascii", "replace")
    out, cur = [], None
    for ln in text.split("\n"):
        f = ln.split()
        if not f:
            continue
        if ln.startswith("HMMER3/"):
            cur = [[0.0] * 6, 0]
            out.append(cur)
        elif cur is not None and f[0] == "STATS" and len(f) > 4 and f[1] == "LOCAL" and f[2] in ("MSV", "VITERBI", "FORWARD"):
            w = ("MSV", "VITERBI", "FORWARD").index(f[2])
            cur[0][2 * w], cur[0][2 * w + 1] = float(f[3]), float(f[4])
            cur[1] |= 1 << w
        elif f[0] == "HMM":
            cur = None
    return [(v, h) for v, h in out]


def viterbi_floor(mu, lam, p=1e-3):
    """the Viterbi score (units) whose Gumbel tail mass is p: threshold_units(mu - ln(-ln(1 - p)) / lambda)"""
    x = R.threshold_units(mu - math.log(-math.log1p(-p)) / lam)
    return max(FLOOR_ALL, min(x, (1 << 31) - 1))


def floors(models, p=1e-3):
    return np.array([viterbi_floor(m["mu"], m["lam"], p) if m["mu"] is not None else FLOOR_ALL for m in models], np.int32)


def forward_pvalue(b, tau, lam):
    return 1.0 if b < tau else math.exp(-lam * (b - tau))


def _padded(tab):
    """the device's table of a profile: [28][64 G], word j of a row = node j + 1, padding STAR, row 27 = PDD (sum of tDD in front of j inside its group)"""
    M = tab.shape[1] - 1
    G = group_size(M)
    t = np.full((28, 64 * G), STAR, np.int64)
    t[:27, :M] = tab[:, 1:]
    dd = t[R.ROW_DD].reshape(64, G)
    t[27] = (np.cumsum(dd, axis=1) - dd).reshape(-1)
    return t, G


def blocked_batch(tab, records, scan_steps=6, join=lse, cells=None):
    """the blocked row step of SPEC 13.1 over many records against one profile -> int32 [n_rec]; a record of no residues: NO_SCORE. Every record runs
    its own length model and takes no more steps once its last row is done: the records are walked longest first, so the live ones are a prefix of
    the arrays. The defaults are the Forward score. join: what joins alternatives, lse or np.maximum (with np.maximum and all six scan steps this is
    the Viterbi score of SPEC 13 in the device's order). scan_steps < 6: the lane scan cut off after that many steps - what a kernel computes whose
    later steps do nothing; only to measure which expected scores travel through which step. cells: a dict that gets the largest M or C cell."""
    n, M = len(records), tab.shape[1] - 1
    Ls = np.array([len(r) for r in records], np.int64)
    out = np.full(n, NO_SCORE, np.int64)
    live = np.flatnonzero(Ls > 0)
    if len(live) == 0:
        return out.astype(np.int32)
    live = live[np.argsort(-Ls[live], kind="stable")]
    assert Ls.max() <= FWD_MAX_L
    Lv = Ls[live]
    x = np.zeros((len(live), int(Lv.max())), np.int64)
    for j, r in enumerate(live):
        x[j, :Lv[j]] = R.encode(records[r])
    sp = np.array([R.specials(int(L), M) for L in Lv], np.int64)
    tloop, tmove, null, tbm = sp[:, 0], sp[:, 1], sp[:, 2], int(sp[0, 3])
    t, G = _padded(tab)
    nl = len(live)
    g3 = lambda row: t[row].reshape(64, G)                                       # noqa: E731
    tMM, tMI, tMD, tIM, tII, tDM, tDD, PDD = (g3(r) for r in (R.ROW_MM, R.ROW_MI, R.ROW_MD, R.ROW_IM, R.ROW_II, R.ROW_DM, R.ROW_DD, 27))
    gsum = tDD.sum(axis=1)
    cs = np.concatenate([[0], np.cumsum(gsum)])
    A = [cs[1:] - cs[np.maximum(np.arange(64) + 1 - (1 << s), 0)] for s in range(6)]          # A_l(s), meaningful for l >= 2^s
    valid = (np.arange(64 * G) < M).reshape(64, G)
    msc_of = t[:20].reshape(20, 64, G)
    Mv = np.full((nl, 64, G), NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    Jall = np.full(nl, NEG, np.int64); Call = Jall.copy(); Ball = tmove.copy()
    tloop_all = tloop
    top = -(1 << 62)
    for i in range(1, int(Lv.max()) + 1):
        nl = int(np.count_nonzero(Lv >= i))                                                   # the records still running: the first nl
        Mv, Iv, Dv = Mv[:nl], Iv[:nl], Dv[:nl]
        J, C, B, tloop = Jall[:nl], Call[:nl], Ball[:nl], tloop_all[:nl]
        negcol = np.full((nl, 1), NEG, np.int64)
        msc = msc_of[x[:nl, i - 1]]
        give = join(join(Mv + tMM, Iv + tIM), Dv + tDM).reshape(nl, 64 * G)
        prev = np.concatenate([negcol, give[:, :-1]], axis=1).reshape(nl, 64, G)              # give[k - 1], give[0] = NEG
        In = np.maximum(join(Mv + tMI, Iv + tII), NEG)
        Mn = np.maximum(msc + join(prev, (B + tbm)[:, None, None]), NEG)
        Dn = np.empty_like(Mn)
        dl = np.full(nl * 64, NEG, np.int64).reshape(nl, 64)
        Dn[:, :, 0] = dl
        for q in range(1, G):
            dl = np.maximum(join(dl + tDD[:, q - 1], Mn[:, :, q - 1] + tMD[:, q - 1]), NEG)
            Dn[:, :, q] = dl
        b = np.maximum(join(dl + tDD[:, G - 1], Mn[:, :, G - 1] + tMD[:, G - 1]), NEG)
        for s in range(scan_steps):
            d = 1 << s
            nb = b.copy()
            nb[:, d:] = np.maximum(join(b[:, d:], b[:, :-d] + A[s][d:]), NEG)                  # groups below 2^s keep their b
            b = nb
        c_in = np.concatenate([negcol, b[:, :-1]], axis=1)
        Dn = np.maximum(join(Dn, c_in[:, :, None] + PDD), NEG)
        e = np.full((nl, 64), NEG, np.int64)
        for q in range(G):
            e = np.where(valid[:, q], join(join(e, Mn[:, :, q]), Dn[:, :, q]), e)
        while e.shape[1] > 1:
            e = join(e[:, 0::2], e[:, 1::2])
        E = e[:, 0]
        Jn = np.maximum(join(J + tloop, E + R.T_EJ), NEG)
        Cn = np.maximum(join(C + tloop, E + R.T_EC), NEG)
        Bn = join(i * tloop, Jn) + tmove[:nl]
        Jall[:nl], Call[:nl], Ball[:nl] = Jn, Cn, Bn
        Mv, Iv, Dv = Mn, In, Dn
        top = max(top, int(Mn.max()), int(Cn.max()))
        assert top < (1 << 31) - (1 << 20)
    if cells is not None:
        cells["max_cell"] = max(top, cells.get("max_cell", top))
    raw = Call + tmove - null
    assert (np.abs(raw) < (1 << 31)).all()
    out[live] = raw
    return out.astype(np.int32)


def forward_batch(tab, records):
    """raw Forward score (units) of many records against one profile, in the blocked order of SPEC 13.1 -> int32 [n_rec]"""
    return blocked_batch(tab, records)


def forward(tab, rec):
    return int(forward_batch(tab, [rec])[0])


def search_forward(models, records, floor=None, vit=None):
    """(vit, fwd), int32 [n_rec, n_prof]: Forward for the pairs with vit != NO_SCORE and vit >= floor[p] (floor None: every pair with a Viterbi
    score), NO_SCORE for the others"""
    if vit is None:
        vit = R.search(models, records)
    fwd = np.full(vit.shape, NO_SCORE, np.int32)
    for p, m in enumerate(models):
        fl = FLOOR_ALL if floor is None else int(floor[p])
        sel = np.flatnonzero((vit[:, p] != NO_SCORE) & (vit[:, p].astype(np.int64) >= fl))
        if len(sel):
            fwd[sel, p] = forward_batch(m["tables"], [records[r] for r in sel])
    return vit, fwd


def forward_f64(tab, rec):
    """the Forward score in units as a float: the recurrences of SPEC 13 with log2-sum-exp2 in f64 in place of every max that joins alternatives,
    cell by cell along k for D, on the same integer tables and specials. The yardstick of forward_batch(); small shapes only."""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    assert L >= 1
    t = tab.astype(np.float64) / 1024.0
    t[t <= STAR / 1024.0] = -np.inf
    tloop, tmove, null, tbm, _, _ = (v / 1024.0 for v in R.specials(L, M))
    la = np.logaddexp2
    ninf = -np.inf
    Mv = np.full(M + 1, ninf); Iv = Mv.copy(); Dv = Mv.copy()
    J = C = ninf
    B = tmove
    with np.errstate(invalid="ignore"):
        for i in range(1, L + 1):
            msc = t[x[i - 1]]
            give = la(la(Mv + t[R.ROW_MM], Iv + t[R.ROW_IM]), Dv + t[R.ROW_DM])
            Mn = np.full(M + 1, ninf)
            Mn[1:] = msc[1:] + la(give[:-1], B + tbm)
            In = la(Mv + t[R.ROW_MI], Iv + t[R.ROW_II])
            In[0] = ninf; In[M] = ninf
            Dn = np.full(M + 1, ninf)
            d = ninf
            for k in range(2, M + 1):
                d = la(d + t[R.ROW_DD][k - 1], Mn[k - 1] + t[R.ROW_MD][k - 1])
                Dn[k] = d
            E = ninf
            for k in range(1, M + 1):
                E = la(la(E, Mn[k]), Dn[k])
            J = la(J + tloop, E + R.T_EJ / 1024.0)
            C = la(C + tloop, E + R.T_EC / 1024.0)
            B = la(i * tloop, J) + tmove
            Mv, Iv, Dv = Mn, In, Dn
    return float(C + tmove - null) * 1024.0


def table_bytes(models, stats, ids, fwd):
    """the text gsearch_amd.hmmsearch(score="forward") writes: a row per (record, profile) with a Forward raw >= 0, sorted by (profile, -raw, record);
    E from STATS LOCAL FORWARD (`-` without the line), pass_ga by the Forward raw. stats: stats_lines() of the models, in order"""
    Z = len(ids)
    rows = []
    for p in range(len(models)):
        for r in range(Z):
            s = int(fwd[r, p])
            if s != NO_SCORE and s >= 0:
                rows.append((p, -s, r))
    out = [b"target\tprofile\tacc\tbits\tevalue\tpass_ga\n"]
    for p, ns, r in sorted(rows):
        m, (st, has) = models[p], stats[p]
        b = R.bits(-ns)
        ev = "%.3E" % (Z * forward_pvalue(b, st[4], st[5])) if has & 4 else "-"
        ga = "-" if m["ga_units"] is None else ("1" if -ns >= m["ga_units"] else "0")
        out.append(("%s\t%s\t%s\t%.2f\t%s\t%s\n" % (ids[r], m["name"], m["acc"] or "-", b, ev, ga)).encode())
    return b"".join(out)
