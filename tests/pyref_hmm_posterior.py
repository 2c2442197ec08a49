"""SPEC 13.4 (hmmsearch: Backward scores and posterior envelopes) restated in numpy, plus a cell-by-cell f64 Forward / Backward that is the
restatement's own yardstick. The scored path is integers only (int64 arrays that hold int32 values); lse, its table, the padded tables and the groups
are those of SPEC 13.1 (pyref_hmm_forward.py), the model and the specials those of SPEC 13 (pyref_hmm.py). Nothing here calls the library."""
import numpy as np

import pyref_hmm as R
import pyref_hmm_forward as F

NEG, STAR, NO_SCORE, NO_HIT = R.NEG, R.STAR, R.NO_SCORE, R.NO_HIT
lse = F.lse
ENV_WORDS = 4
LO, HI = -156, -425                                # round(1024 log2(1 - 0.10)), round(1024 log2(1 - 0.25))
assert (LO, HI) == (round(1024 * np.log2(0.90)), round(1024 * np.log2(0.75)))


def _groups(tab):
    """the padded table of SPEC 13.1 as [64, G] arrays per row, and what both passes need of it"""
    M = tab.shape[1] - 1
    t, G = F._padded(tab)
    g = {"M": M, "G": G, "valid": (np.arange(64 * G) < M).reshape(64, G), "msc": t[:20].reshape(20, 64, G)}
    for name, row in (("MM", R.ROW_MM), ("MI", R.ROW_MI), ("MD", R.ROW_MD), ("IM", R.ROW_IM), ("II", R.ROW_II), ("DM", R.ROW_DM), ("DD", R.ROW_DD), ("PDD", 27)):
        g[name] = t[row].reshape(64, G)
    g["gsum"] = g["DD"].sum(axis=1)
    cs = np.concatenate([[0], np.cumsum(g["gsum"])])
    lanes = np.arange(64)
    g["A_up"] = [cs[1:] - cs[np.maximum(lanes + 1 - (1 << s), 0)] for s in range(6)]           # A_l(s) of 13.1, meaningful for l >= 2^s
    g["A_dn"] = [cs[np.minimum(lanes + (1 << s), 64)] - cs[:-1] for s in range(6)]             # groups l .. l + 2^s - 1, meaningful for l <= 63 - 2^s
    g["SDD"] = g["gsum"][:, None] - g["PDD"]                                                    # tDD from a node to its group's end
    return g


def _tree(e):
    while len(e) > 1:
        e = lse(e[0::2], e[1::2])
    return int(e[0])


def forward_rows(tab, x, Lsp=None, g=None):
    """the blocked Forward of SPEC 13.1 over the residues x (indices) under the length model of Lsp residues (None: len(x)) ->
    (E, J, C as int64 [L + 1] with row 0 = NEG, raw = C[L] + tmove - null(Lsp))"""
    g = g or _groups(tab)
    L, M, G = len(x), g["M"], g["G"]
    tloop, tmove, null, tbm, _, _ = R.specials(L if Lsp is None else Lsp, M)
    Mv = np.full((64, G), NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    E = np.full(L + 1, NEG, np.int64); J = E.copy(); C = E.copy()
    B = tmove
    for i in range(1, L + 1):
        msc = g["msc"][x[i - 1]]
        give = lse(lse(Mv + g["MM"], Iv + g["IM"]), Dv + g["DM"]).reshape(-1)
        prev = np.concatenate([[NEG], give[:-1]]).reshape(64, G)
        In = np.maximum(lse(Mv + g["MI"], Iv + g["II"]), NEG)
        Mn = np.maximum(msc + lse(prev, B + tbm), NEG)
        Dn = np.empty_like(Mn)
        dl = np.full(64, NEG, np.int64)
        Dn[:, 0] = dl
        for q in range(1, G):
            dl = np.maximum(lse(dl + g["DD"][:, q - 1], Mn[:, q - 1] + g["MD"][:, q - 1]), NEG)
            Dn[:, q] = dl
        b = np.maximum(lse(dl + g["DD"][:, G - 1], Mn[:, G - 1] + g["MD"][:, G - 1]), NEG)
        for s in range(6):
            d = 1 << s
            nb = b.copy()
            nb[d:] = np.maximum(lse(b[d:], b[:-d] + g["A_up"][s][d:]), NEG)
            b = nb
        c_in = np.concatenate([[NEG], b[:-1]])
        Dn = np.maximum(lse(Dn, c_in[:, None] + g["PDD"]), NEG)
        e = np.full(64, NEG, np.int64)
        for q in range(G):
            e = np.where(g["valid"][:, q], lse(lse(e, Mn[:, q]), Dn[:, q]), e)
        E[i] = _tree(e)
        J[i] = max(int(lse(J[i - 1] + tloop, E[i] + R.T_EJ)), NEG)
        C[i] = max(int(lse(C[i - 1] + tloop, E[i] + R.T_EC)), NEG)
        B = int(lse(i * tloop, J[i])) + tmove
        Mv, Iv, Dv = Mn, In, Dn
    return E, J, C, int(C[L]) + tmove - null


def backward_rows(tab, x, g=None):
    """the blocked Backward of SPEC 13.4 -> (bN, bJ as int64 [L + 1], raw = bN[0] - null)"""
    g = g or _groups(tab)
    L, M, G = len(x), g["M"], g["G"]
    tloop, tmove, null, tbm, _, _ = R.specials(L, M)
    valid = g["valid"]
    Mv = np.full((64, G), NEG, np.int64); Iv = Mv.copy()
    bN = np.full(L + 1, NEG, np.int64); bJ = bN.copy()
    n = j = NEG
    for s in range(L + 1):
        i = L - s
        if s:
            take = np.where(valid, g["msc"][x[i]] + Mv, NEG)
        else:
            take = np.full((64, G), NEG, np.int64)                                            # row L has no row below
        e = np.full(64, NEG, np.int64)
        if s:
            for q in range(G):
                e = np.where(valid[:, q], lse(e, take[:, q]), e)
        bB = _tree(e) + tbm
        bC = s * tloop + tmove
        if s:
            j = max(int(lse(j + tloop, bB + tmove)), NEG)
            n = max(int(lse(n + tloop, bB + tmove)), NEG)
        bE = int(lse(j + R.T_EJ, bC + R.T_EC))
        bN[i], bJ[i] = n, j
        tk = np.concatenate([take.reshape(-1)[1:], [NEG]]).reshape(64, G)                     # take of node k + 1
        c = lse(bE, tk + g["DM"])
        Dv = np.empty((64, G), np.int64)
        dl = None
        for q in range(G - 1, -1, -1):
            dl = c[:, q] if q == G - 1 else np.maximum(lse(c[:, q], dl + g["DD"][:, q]), NEG)
            dl = np.where(valid[:, q], dl, NEG)                                               # a padding node holds NEG
            Dv[:, q] = dl
        b = dl
        for st in range(6):
            d = 1 << st
            nb = b.copy()
            nb[:64 - d] = np.maximum(lse(b[:64 - d], b[d:] + g["A_dn"][st][:64 - d]), NEG)    # groups above 63 - 2^s keep their b
            b = nb
        c_in = np.concatenate([b[1:], [NEG]])                                                 # bD of the first node of the group above
        Dv = np.maximum(lse(Dv, c_in[:, None] + g["SDD"]), NEG)
        dnext = np.concatenate([Dv[:, 1:], c_in[:, None]], axis=1)
        Mn = np.maximum(lse(lse(lse(bE, tk + g["MM"]), Iv + g["MI"]), dnext + g["MD"]), NEG)
        Iv = np.maximum(lse(tk + g["IM"], Iv + g["II"]), NEG)
        Mv = Mn
    return bN, bJ, int(bN[0]) - null


def occupancy(E, J, C, bN, bJ, L, M):
    """(out, cont, exit) as int64 [L + 1] (row 0 unused, 0) and total_f, all in units"""
    tloop, tmove, _, _, _, _ = R.specials(L, M)
    total = int(C[L]) + tmove
    i = np.arange(1, L + 1)
    bC = (L - i) * tloop + tmove
    out = np.zeros(L + 1, np.int64); cont = out.copy(); ex = out.copy()
    out[1:] = lse(lse(i * tloop + bN[1:], J[:-1] + tloop + bJ[1:]), C[:-1] + tloop + bC) - total
    ex[1:] = E[1:] + lse(bJ[1:] + R.T_EJ, bC + R.T_EC) - total
    cont[1:] = lse(out[1:], ex[1:])
    return out, cont, ex, total


def runs(out, cont, lo=LO, hi=HI, use_cont=True):
    """the envelopes (a, b, peak) of the run rule; out / cont indexed 1 .. L (ints or floats)"""
    L = len(out) - 1
    res, i = [], 1
    while i <= L:
        if out[i] <= lo:
            a = i
            while i < L and out[i + 1] <= lo and (cont[i] <= lo or not use_cont):
                i += 1
            peak = min(out[a:i + 1])
            if peak <= hi:
                res.append((a, i, peak))
        i += 1
    return res


def posterior(tab, rec, rows=False):
    """everything of one pair: dict with fwd, bck (raw), env = [(i_from, i_to, env_raw, peak)], and with rows the int64 out / cont [L + 1]"""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    assert 1 <= L <= F.FWD_MAX_L
    g = _groups(tab)
    E, J, C, fwd = forward_rows(tab, x, g=g)
    bN, bJ, bck = backward_rows(tab, x, g=g)
    out, cont, _, _ = occupancy(E, J, C, bN, bJ, L, M)
    tloop = R.specials(L, M)[0]
    env = []
    for a, b, peak in runs(out, cont):
        Ld = b - a + 1
        seg = fwd if Ld == L else forward_rows(tab, x[a - 1:b], Lsp=L, g=g)[3]
        env.append((a, b, seg + (L - Ld) * tloop, int(peak)))
    r = {"fwd": fwd, "bck": bck, "env": env, "bN": bN, "bJ": bJ}
    if rows:
        r["out"], r["cont"] = out, cont
    return r


def envelope_pairs(models, records, pair_rec, pair_prof, max_env, rows=False):
    """what gs_hmm_envelopes writes: (int32 fwd [n], int32 bck [n], uint32 n_env [n], int32 env [n, max_env, 4]) and, with rows, the lists of the
    pairs' int32 out[1..L] and cont[1..L] (None for a pair that gets none); a record with a byte that is no residue is an empty pair"""
    n = len(pair_rec)
    fwd = np.full(n, NO_SCORE, np.int32); bck = fwd.copy()
    ne = np.zeros(n, np.uint32)
    env = np.zeros((n, max_env, ENV_WORDS), np.int32)
    outs, conts = [None] * n, [None] * n
    memo = {}
    for j, (r, p) in enumerate(zip(pair_rec, pair_prof)):
        r, p = int(r), int(p)
        if r == NO_HIT or len(records[r]) == 0 or (R._LUT[np.frombuffer(bytes(records[r]), np.uint8)] >= 20).any():
            continue
        if (r, p) not in memo:
            memo[r, p] = posterior(models[p]["tables"], records[r], rows=True)
        m = memo[r, p]
        fwd[j], bck[j], ne[j] = m["fwd"], m["bck"], len(m["env"])
        for d, e in enumerate(m["env"][:max_env]):
            env[j, d] = e
        outs[j], conts[j] = m["out"][1:].astype(np.int32), m["cont"][1:].astype(np.int32)
    return (fwd, bck, ne, env, outs, conts) if rows else (fwd, bck, ne, env)


# ---- the yardstick: f64, cell by cell --------------------------------------------------------------------------------------------------------------
def posterior_f64(tab, rec):
    """Forward and Backward of SPEC 13.4 in f64 (logaddexp2 for every join, along k one cell after the other for D and bD) on the same integer tables
    and specials, everything in units as floats -> dict: total_f, total_b, bN, bJ [L + 1], out, cont [L + 1] (row 0 unused)"""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    t = tab.astype(np.float64)
    t[tab <= STAR] = -np.inf
    tloop, tmove, _, tbm, _, _ = (float(v) for v in R.specials(L, M))
    tE = float(R.T_EJ)
    la, ninf = np.logaddexp2, -np.inf
    u = 1024.0                                                                                # logaddexp2 works in bits
    lau = lambda a, b: u * la(a / u, b / u)                                                   # noqa: E731
    tr = {n: t[r] for n, r in (("MM", R.ROW_MM), ("MI", R.ROW_MI), ("MD", R.ROW_MD), ("IM", R.ROW_IM), ("II", R.ROW_II), ("DM", R.ROW_DM), ("DD", R.ROW_DD))}
    fE = np.full(L + 1, ninf); fJ = fE.copy(); fC = fE.copy()
    Mv = np.full(M + 1, ninf); Iv = Mv.copy(); Dv = Mv.copy()
    B = tmove
    with np.errstate(invalid="ignore"):
        for i in range(1, L + 1):
            give = lau(lau(Mv + tr["MM"], Iv + tr["IM"]), Dv + tr["DM"])
            Mn = np.full(M + 1, ninf)
            Mn[1:] = t[x[i - 1]][1:] + lau(give[:-1], B + tbm)
            In = lau(Mv + tr["MI"], Iv + tr["II"])
            In[0] = In[M] = ninf
            Dn = np.full(M + 1, ninf)
            for k in range(2, M + 1):
                Dn[k] = lau(Dn[k - 1] + tr["DD"][k - 1], Mn[k - 1] + tr["MD"][k - 1])
            fE[i] = u * la.reduce(np.concatenate([Mn[1:], Dn[1:]]) / u)
            fJ[i] = lau(fJ[i - 1] + tloop, fE[i] + tE)
            fC[i] = lau(fC[i - 1] + tloop, fE[i] + tE)
            B = lau(i * tloop, fJ[i]) + tmove
            Mv, Iv, Dv = Mn, In, Dn
        total_f = fC[L] + tmove
        bN = np.full(L + 1, ninf); bJ = bN.copy()
        bC = (L - np.arange(L + 1)) * tloop + tmove
        bM = np.full(M + 2, ninf); bI = bM.copy()                                             # of the row below; index M + 1 stays -inf
        for i in range(L, -1, -1):
            take = np.full(M + 2, ninf)
            if i < L:
                take[1:M + 1] = t[x[i]][1:] + bM[1:M + 1]
                bB = tbm + u * la.reduce(take[1:M + 1] / u)
                bJ[i] = lau(bJ[i + 1] + tloop, bB + tmove)
                bN[i] = lau(bN[i + 1] + tloop, bB + tmove)
            bE = lau(bJ[i] + tE, bC[i] + tE)
            nD = np.full(M + 2, ninf); nM = nD.copy(); nI = nD.copy()
            for k in range(M, 0, -1):
                if k == M:
                    nD[k] = nM[k] = bE
                else:
                    nD[k] = lau(lau(bE, take[k + 1] + tr["DM"][k]), nD[k + 1] + tr["DD"][k])
                    nI[k] = lau(take[k + 1] + tr["IM"][k], bI[k] + tr["II"][k])
                    nM[k] = lau(lau(lau(bE, take[k + 1] + tr["MM"][k]), bI[k] + tr["MI"][k]), nD[k + 1] + tr["MD"][k])
            bM, bI = nM, nI
        i = np.arange(1, L + 1)
        out = np.zeros(L + 1); cont = out.copy()
        out[1:] = lau(lau(i * tloop + bN[1:], fJ[:-1] + tloop + bJ[1:]), fC[:-1] + tloop + bC[1:]) - total_f
        cont[1:] = lau(out[1:], fE[1:] + lau(bJ[1:] + tE, bC[1:] + tE) - total_f)
    return {"total_f": float(total_f), "total_b": float(bN[0]), "bN": bN, "bJ": bJ, "out": out, "cont": cont}


# ---- the table of hmmsearch(envelopes=) -------------------------------------------------------------------------------------------------------------
def listed_pairs(models, fwd_or_vit):
    """the (record, profile) pairs of the score table of hmmsearch(), in its order: raw >= 0, by (profile, -raw, record)"""
    rows = []
    for p in range(len(models)):
        for r in range(fwd_or_vit.shape[0]):
            s = int(fwd_or_vit[r, p])
            if s != NO_SCORE and s >= 0:
                rows.append((p, -s, r))
    return [(r, p) for p, _, r in sorted(rows)]


def envelope_table_bytes(models, ids, listed, n_env, env):
    """the text hmmsearch(envelopes=) writes for the listed pairs: a row per envelope, sorted like the score table and then by env (from 1)"""
    out = [b"target\tprofile\tacc\tenv\tn_env\ti_from\ti_to\tenv_bits\tpeak_occ\n"]
    for j, (r, p) in enumerate(listed):
        m = models[p]
        for d in range(int(n_env[j])):
            a, b, raw, peak = (int(v) for v in env[j][d])
            out.append(("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%.2f\t%.3f\n" % (ids[r], m["name"], m["acc"] or "-", d + 1, int(n_env[j]), a, b, raw / 1024.0,
                                                                      1.0 - 2.0 ** (peak / 1024.0))).encode())
    return b"".join(out)
