"""SPEC 13.5 (hmmsearch: the null2 bias correction of envelope and sequence scores) restated in numpy, plus a cell-by-cell f64 Forward / Backward with
full matrices that is the restatement's own yardstick. The scored path is integers only (int64 arrays that hold int32 values); lse, the padded tables
and the groups are those of SPEC 13.1 / 13.4 (pyref_hmm_forward.py, pyref_hmm_posterior.py), the model and the specials those of SPEC 13
(pyref_hmm.py). Nothing here calls the library."""
import numpy as np

import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_posterior as P

NEG, STAR, NO_SCORE, NO_HIT = R.NEG, R.STAR, R.NO_SCORE, R.NO_HIT
lse = F.lse
N2_WORDS = 4                                       # corr, dom_bias, seg_raw, mass
OMEGA = -8192                                      # 1024 log2(1 / 256): the prior of the null2 model
CORR_MAX = 1 << 30                                 # |corr| and |the sum of corr| are clamped here: OMEGA + corr stays an int32
assert OMEGA == round(1024 * np.log2(1 / 256))


def lg(n):
    """log2(n) to the nearest unit, in integers"""
    return (R.lgq(n) + 512) >> 10


def _clamp(v):
    return max(-CORR_MAX, min(int(v), CORR_MAX))


def _fold_tree(vals, valid):
    """per group the fold over its valid nodes in node order from NEG, then the balanced tree of SPEC 13.1 over the 64 groups"""
    e = np.full(64, NEG, np.int64)
    for q in range(vals.shape[1]):
        e = np.where(valid[:, q], lse(e, vals[:, q]), e)
    return P._tree(e)


def forward_kept(g, x, L):
    """Forward of SPEC 13.1 over the residues x under the length model of L residues, exactly P.forward_rows, and M and I of every row ->
    (fM, fI as int64 [Ld + 1, 64, G] (row 0 unused), E, J, C as int64 [Ld + 1])"""
    Ld, M, G = len(x), g["M"], g["G"]
    tloop, tmove, _, tbm, _, _ = R.specials(L, M)
    Mv = np.full((64, G), NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    fM = np.full((Ld + 1, 64, G), NEG, np.int64); fI = fM.copy()
    E = np.full(Ld + 1, NEG, np.int64); J = E.copy(); C = E.copy()
    B = tmove
    for i in range(1, Ld + 1):
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
        E[i] = P._tree(e)
        J[i] = max(int(lse(J[i - 1] + tloop, E[i] + R.T_EJ)), NEG)
        C[i] = max(int(lse(C[i - 1] + tloop, E[i] + R.T_EC)), NEG)
        B = int(lse(i * tloop, J[i])) + tmove
        Mv, Iv, Dv = Mn, In, Dn
        fM[i], fI[i] = Mn, In
    return fM, fI, E, J, C


def segment(tab, x, L, g=None):
    """everything of one segment x (residue indices, Ld of them) of a record of L residues -> dict: corr, dom_bias, seg_raw, mass (ints), n2 (int64
    [20]), occM, occI (int64 [M], nodes 1 .. M; occI of node M is NEG), occX"""
    g = g or P._groups(tab)
    Ld, M, G = len(x), g["M"], g["G"]
    assert 1 <= Ld <= L <= F.FWD_MAX_L
    tloop, tmove, null, tbm, _, _ = R.specials(L, M)
    valid = g["valid"]
    valid_i = (np.arange(64 * G) < M - 1).reshape(64, G)                                      # I of node M and of padding nodes holds mass that no path carries
    fM, fI, E, J, C = forward_kept(g, x, L)
    total = int(C[Ld]) + tmove
    # Backward of SPEC 13.4 over the segment's rows, bC from the segment's rows, and the accumulators beside the row
    Mv = np.full((64, G), NEG, np.int64); Iv = Mv.copy()
    oM = Mv.copy(); oI = Mv.copy()
    oX = NEG
    n = j = NEG
    for s in range(Ld + 1):
        i = Ld - s
        if s:
            take = np.where(valid, g["msc"][x[i]] + Mv, NEG)
        else:
            take = np.full((64, G), NEG, np.int64)
        e = np.full(64, NEG, np.int64)
        if s:
            for q in range(G):
                e = np.where(valid[:, q], lse(e, take[:, q]), e)
        bB = P._tree(e) + tbm
        bC = s * tloop + tmove
        if s:
            j = max(int(lse(j + tloop, bB + tmove)), NEG)
            n = max(int(lse(n + tloop, bB + tmove)), NEG)
        bE = int(lse(j + R.T_EJ, bC + R.T_EC))
        tk = np.concatenate([take.reshape(-1)[1:], [NEG]]).reshape(64, G)
        c = lse(bE, tk + g["DM"])
        Dv = np.empty((64, G), np.int64)
        dl = None
        for q in range(G - 1, -1, -1):
            dl = c[:, q] if q == G - 1 else np.maximum(lse(c[:, q], dl + g["DD"][:, q]), NEG)
            dl = np.where(valid[:, q], dl, NEG)
            Dv[:, q] = dl
        b = dl
        for st in range(6):
            d = 1 << st
            nb = b.copy()
            nb[:64 - d] = np.maximum(lse(b[:64 - d], b[d:] + g["A_dn"][st][:64 - d]), NEG)
            b = nb
        c_in = np.concatenate([b[1:], [NEG]])
        Dv = np.maximum(lse(Dv, c_in[:, None] + g["SDD"]), NEG)
        dnext = np.concatenate([Dv[:, 1:], c_in[:, None]], axis=1)
        Mn = np.maximum(lse(lse(lse(bE, tk + g["MM"]), Iv + g["MI"]), dnext + g["MD"]), NEG)
        Iv = np.maximum(lse(tk + g["IM"], Iv + g["II"]), NEG)
        Mv = Mn
        if i >= 1:                                                                            # the fold of 13.5, rows Ld .. 1
            oM = lse(oM, fM[i] + Mv)
            oI = lse(oI, fI[i] + Iv)
            xn = int(lse(lse(i * tloop + n, J[i - 1] + tloop + j), C[i - 1] + tloop + bC))
            oX = int(lse(oX, xn))
            assert -(1 << 31) < min(int((fM[i] + Mv).min()), int((fI[i] + Iv).min())) and max(int(oM.max()), int(oI.max()), oX) < (1 << 31)
    occM = np.maximum(oM - total, NEG)
    occI = np.maximum(oI - total, NEG)
    occX = max(oX - total, NEG)
    lgd = lg(Ld)
    ii = _fold_tree(occI, valid_i)
    n2 = np.array([int(lse(lse(_fold_tree(occM + g["msc"][a], valid), ii), occX)) - lgd for a in range(20)], np.int64)
    mass = int(lse(lse(_fold_tree(occM, valid), ii), occX)) - lgd
    corr = _clamp(int(n2[np.asarray(x, np.int64)].sum()))
    occI_row = np.where(valid_i, occI, NEG).reshape(-1)[:M]
    return {"corr": corr, "dom_bias": int(lse(0, OMEGA + corr)), "seg_raw": total + (L - Ld) * tloop - null, "mass": mass, "n2": n2,
            "occM": occM.reshape(-1)[:M].copy(), "occI": occI_row, "occX": occX}


def seq_bias(corrs):
    """the sequence bias of a pair from the corr of its listed envelopes"""
    return int(lse(0, OMEGA + _clamp(sum(int(c) for c in corrs))))


def null2_pairs(models, records, pair_rec, pair_prof, n_env, env, max_env):
    """what gs_hmm_null2 writes: (int32 slots [n, max_env, 4], int32 seq_bias [n], int32 n2 [n, max_env, 20], and per pair the lists of the listed
    slots' int32 occM and occI rows). A pair without a record, with an empty one or with a byte that is no residue: zeros and no rows"""
    n = len(pair_rec)
    slots = np.zeros((n, max_env, N2_WORDS), np.int32)
    sb = np.zeros(n, np.int32)
    n2 = np.zeros((n, max_env, 20), np.int32)
    occM, occI = [[] for _ in range(n)], [[] for _ in range(n)]
    memo, groups = {}, {}
    for j, (r, p) in enumerate(zip(pair_rec, pair_prof)):
        r, p = int(r), int(p)
        if r == NO_HIT or len(records[r]) == 0 or (R._LUT[np.frombuffer(bytes(records[r]), np.uint8)] >= 20).any():
            continue
        x = R.encode(records[r])
        if p not in groups:
            groups[p] = P._groups(models[p]["tables"])
        corrs = []
        for d in range(min(int(n_env[j]), max_env)):
            a, b = int(env[j, d, 0]), int(env[j, d, 1])
            if (r, p, a, b) not in memo:
                memo[r, p, a, b] = segment(models[p]["tables"], x[a - 1:b], len(x), g=groups[p])
            m = memo[r, p, a, b]
            slots[j, d] = (m["corr"], m["dom_bias"], m["seg_raw"], m["mass"])
            n2[j, d] = m["n2"]
            occM[j].append(m["occM"].astype(np.int32)); occI[j].append(m["occI"].astype(np.int32))
            corrs.append(m["corr"])
        sb[j] = seq_bias(corrs)
    return slots, sb, n2, occM, occI


def pair(tab, rec, whole_if_none=False):
    """envelopes (SPEC 13.4) and null2 of one pair -> dict: fwd, env [(a, b, env_raw, peak)], seg [segment() per envelope], seq_bias, whole (True: the
    record had no envelope and, with whole_if_none, the whole record stands for one)"""
    x = R.encode(rec)
    post = P.posterior(tab, rec)
    env, whole = post["env"], False
    if not env and whole_if_none:
        env, whole = [(1, len(x), post["fwd"], 0)], True
    g = P._groups(tab)
    seg = [segment(tab, x[a - 1:b], len(x), g=g) for a, b, _, _ in env]
    return {"fwd": post["fwd"], "env": env, "seg": seg, "seq_bias": seq_bias([s["corr"] for s in seg]), "whole": whole}


# ---- the yardstick: f64, cell by cell, full matrices ------------------------------------------------------------------------------------------------
def segment_f64(tab, x, L):
    """Forward and Backward over the segment in f64 on the same integer tables and specials, every cell kept; the expected usage of every emitting
    state from their products -> dict in units as floats: n2 [20], corr, mass (log2 of the summed usage over Ld), total_f, total_b"""
    Ld, M = len(x), tab.shape[1] - 1
    t = tab.astype(np.float64)
    t[tab <= STAR] = -np.inf
    tloop, tmove, _, tbm, _, _ = (float(v) for v in R.specials(L, M))
    tE = float(R.T_EJ)
    la, ninf, u = np.logaddexp2, -np.inf, 1024.0
    lau = lambda a, b: u * la(a / u, b / u)                                                   # noqa: E731
    tr = {n: t[r] for n, r in (("MM", R.ROW_MM), ("MI", R.ROW_MI), ("MD", R.ROW_MD), ("IM", R.ROW_IM), ("II", R.ROW_II), ("DM", R.ROW_DM), ("DD", R.ROW_DD))}
    fM = np.full((Ld + 1, M + 1), ninf); fI = fM.copy()
    fE = np.full(Ld + 1, ninf); fJ = fE.copy(); fC = fE.copy()
    Dv = np.full(M + 1, ninf)
    B = tmove
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(1, Ld + 1):
            Mv, Iv = fM[i - 1], fI[i - 1]
            give = lau(lau(Mv + tr["MM"], Iv + tr["IM"]), Dv + tr["DM"])
            fM[i, 1:] = t[x[i - 1]][1:] + lau(give[:-1], B + tbm)
            In = lau(Mv + tr["MI"], Iv + tr["II"])
            In[0] = In[M] = ninf
            fI[i] = In
            Dn = np.full(M + 1, ninf)
            for k in range(2, M + 1):
                Dn[k] = lau(Dn[k - 1] + tr["DD"][k - 1], fM[i, k - 1] + tr["MD"][k - 1])
            fE[i] = u * la.reduce(np.concatenate([fM[i, 1:], Dn[1:]]) / u)
            fJ[i] = lau(fJ[i - 1] + tloop, fE[i] + tE)
            fC[i] = lau(fC[i - 1] + tloop, fE[i] + tE)
            B = lau(i * tloop, fJ[i]) + tmove
            Dv = Dn
        total_f = fC[Ld] + tmove
        bN = np.full(Ld + 1, ninf); bJ = bN.copy()
        bC = (Ld - np.arange(Ld + 1)) * tloop + tmove
        bM = np.full((Ld + 2, M + 2), ninf); bI = bM.copy()                                   # row Ld + 1 and column M + 1 stay -inf
        for i in range(Ld, -1, -1):
            take = np.full(M + 2, ninf)
            if i < Ld:
                take[1:M + 1] = t[x[i]][1:] + bM[i + 1, 1:M + 1]
                bB = tbm + u * la.reduce(take[1:M + 1] / u)
                bJ[i] = lau(bJ[i + 1] + tloop, bB + tmove)
                bN[i] = lau(bN[i + 1] + tloop, bB + tmove)
            bE = lau(bJ[i] + tE, bC[i] + tE)
            nD = np.full(M + 2, ninf)
            for k in range(M, 0, -1):
                if k == M:
                    nD[k] = bM[i, k] = bE
                else:
                    nD[k] = lau(lau(bE, take[k + 1] + tr["DM"][k]), nD[k + 1] + tr["DD"][k])
                    bI[i, k] = lau(take[k + 1] + tr["IM"][k], bI[i + 1, k] + tr["II"][k])
                    bM[i, k] = lau(lau(lau(bE, take[k + 1] + tr["MM"][k]), bI[i + 1, k] + tr["MI"][k]), nD[k + 1] + tr["MD"][k])
        i = np.arange(1, Ld + 1)
        pM = np.exp2((fM[1:, 1:] + bM[1:Ld + 1, 1:M + 1] - total_f) / u).sum(axis=0)           # expected number of residues M_k emits, k = 1 .. M
        pI = np.exp2((fI[1:, 1:M] + bI[1:Ld + 1, 1:M] - total_f) / u).sum(axis=0)              # I_k, k = 1 .. M - 1
        xn = lau(lau(i * tloop + bN[1:], fJ[:-1] + tloop + bJ[1:]), fC[:-1] + tloop + bC[1:])
        pX = float(np.exp2((xn - total_f) / u).sum())
        emit = np.exp2(t[:20, 1:] / u)                                                        # odds of residue a at node k
        n2 = u * np.log2(((emit * pM).sum(axis=1) + pI.sum() + pX) / Ld)
        mass = u * np.log2((pM.sum() + pI.sum() + pX) / Ld)
    return {"n2": n2, "corr": float(n2[np.asarray(x, np.int64)].sum()), "mass": float(mass), "total_f": float(total_f), "total_b": float(bN[0])}


def bias_f64(corrs):
    """the bias in units, f64, from the corr values (units) of the envelopes it covers"""
    return 1024.0 * float(np.logaddexp2(0.0, (OMEGA + sum(corrs)) / 1024.0))


# ---- the tables of hmmsearch(score="forward", bias=True) --------------------------------------------------------------------------------------------
def table_bytes(models, stats, ids, fwd, sbias):
    """the text hmmsearch(score="forward", bias=True) writes: a row per (record, profile) with an uncorrected Forward raw >= 0 - the pairs null2 ran
    for -, sorted by (profile, corrected raw descending, record); bits, evalue and pass_ga of the corrected raw fwd - seq_bias, then bias %.2f bits.
    sbias: int [n_rec, n_prof], read where a row exists"""
    Z = len(ids)
    rows = []
    for p in range(len(models)):
        for r in range(Z):
            s = int(fwd[r, p])
            if s != NO_SCORE and s >= 0:
                rows.append((p, -(s - int(sbias[r, p])), r))
    out = [b"target\tprofile\tacc\tbits\tevalue\tpass_ga\tbias\n"]
    for p, ns, r in sorted(rows):
        m, (st, has) = models[p], stats[p]
        b = R.bits(-ns)
        ev = "%.3E" % (Z * F.forward_pvalue(b, st[4], st[5])) if has & 4 else "-"
        ga = "-" if m["ga_units"] is None else ("1" if -ns >= m["ga_units"] else "0")
        out.append(("%s\t%s\t%s\t%.2f\t%s\t%s\t%.2f\n" % (ids[r], m["name"], m["acc"] or "-", b, ev, ga, int(sbias[r, p]) / 1024.0)).encode())
    return b"".join(out)


def listed_pairs(models, fwd, sbias):
    """the (record, profile) pairs of table_bytes(), in its order"""
    rows = []
    for p in range(len(models)):
        for r in range(fwd.shape[0]):
            s = int(fwd[r, p])
            if s != NO_SCORE and s >= 0:
                rows.append((p, -(s - int(sbias[r, p])), r))
    return [(r, p) for p, _, r in sorted(rows)]


def envelope_table_bytes(models, ids, listed, n_env, env, slots):
    """the text hmmsearch(envelopes=, bias=True) writes: the envelope table of SPEC 13.4 with env_bits of the corrected score env_raw - dom_bias and a
    column env_bias (%.2f bits) behind it"""
    out = [b"target\tprofile\tacc\tenv\tn_env\ti_from\ti_to\tenv_bits\tpeak_occ\tenv_bias\n"]
    for j, (r, p) in enumerate(listed):
        m = models[p]
        for d in range(int(n_env[j])):
            a, b, raw, peak = (int(v) for v in env[j][d])
            bias = int(slots[j][d][1])
            out.append(("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%.2f\t%.3f\t%.2f\n" % (ids[r], m["name"], m["acc"] or "-", d + 1, int(n_env[j]), a, b, (raw - bias) / 1024.0,
                                                                            1.0 - 2.0 ** (peak / 1024.0), bias / 1024.0)).encode())
    return b"".join(out)
