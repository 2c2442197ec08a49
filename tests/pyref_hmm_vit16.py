"""SPEC 13.7 (the packed int16 Viterbi filter) restated in numpy a row at a time, plus a naive cell-by-cell loop that is the restatement's own yardstick,
and the staged search on top of the other restatements. Integers only: int64 arrays holding int16 cells, no float. Nothing here calls the library.

The definition of D is the recurrence as written, every step saturating: D[k] = max(sat(M[k-1] + tMD16[k-1]), sat(D[k-1] + tDD16[k-1])). With tDD16 <= 0
and every sat(M + tMD16) at least NEG16 that chain equals max(NEG16, b[j] + the WIDE sum of tDD16 between j and k) over j < k (SPEC 13.7), which is the
closed form vit16_batch() uses (d_form="wide") and what a lane scan with int32 group sums computes. d_form="sat_groups" is the other scan: 64 groups
of `group` nodes and six doubling steps whose sums of tDD16 over 2^s groups are kept in int16, saturated. Its D cells can be larger, its scores are not."""
import numpy as np

import pyref_hmm as R

NEG16, MAX16 = -32768, 32767
VF_OVER = (1 << 31) - 1


def h(x):
    """half units: the ceiling of x / 2, clamped below"""
    return np.maximum(NEG16, (np.asarray(x, np.int64) + 1) >> 1)


def sat(a):
    return np.clip(a, NEG16, MAX16)


def tables16(tab):
    """int16 [27][M + 1]: h of every word of a profile's table"""
    t = h(tab)
    assert t.max() <= MAX16
    return t.astype(np.int16)


def vit16_naive(tab, rec, cells=False):
    """vf by the recurrences of SPEC 13.7 as written, cell by cell (the yardstick; small shapes only). cells=True: (vf, M16, I16, D16, E16) with the
    rows computed so far"""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    if L == 0:
        return R.NO_SCORE
    t = [[int(v) for v in row] for row in tables16(tab)]
    s = lambda a: max(NEG16, min(MAX16, a))       # noqa: E731
    tloop, tmove, null, tbm, _, _ = R.specials(L, M)
    Mm = [[NEG16] * (M + 1) for _ in range(L + 1)]
    Im = [[NEG16] * (M + 1) for _ in range(L + 1)]
    Dm = [[NEG16] * (M + 1) for _ in range(L + 1)]
    E16 = [NEG16] * (L + 1)
    B, J, C = tmove, R.NEG, R.NEG
    vf = None
    for i in range(1, L + 1):
        ent = s(int(h(B + tbm)))
        for k in range(1, M + 1):
            best = max(s(Mm[i - 1][k - 1] + t[R.ROW_MM][k - 1]), s(Im[i - 1][k - 1] + t[R.ROW_IM][k - 1]), s(Dm[i - 1][k - 1] + t[R.ROW_DM][k - 1]), ent)
            Mm[i][k] = s(t[x[i - 1]][k] + best)
            if k < M:
                Im[i][k] = max(s(Mm[i - 1][k] + t[R.ROW_MI][k]), s(Im[i - 1][k] + t[R.ROW_II][k]))
            if k >= 2:
                Dm[i][k] = max(s(Mm[i][k - 1] + t[R.ROW_MD][k - 1]), s(Dm[i][k - 1] + t[R.ROW_DD][k - 1]))
        E16[i] = max(Mm[i][1:])
        if E16[i] == MAX16:
            vf = VF_OVER
            break
        E = 2 * E16[i]
        J = max(J + tloop, E + R.T_EJ, R.NEG)
        C = max(C + tloop, E + R.T_EC, R.NEG)
        B = max(i * tloop, J) + tmove
    if vf is None:
        vf = C + tmove - null
    return (vf, Mm, Im, Dm, E16) if cells else vf


def _d_sat_groups(Mn, t, group):
    """D of a row [n, M + 1] by the lane scan of SPEC 13.1 with everything kept in int16: 64 groups of `group` nodes (64 * group >= M, padding NEG16), Dloc
    from NEG16 inside a group, six doubling steps b_l = max(b_l, sat(b_(l - 2^s) + A_l(s))) whose sums A_l(s) of tDD16 over 2^s groups SATURATE, then
    D[q] = max(Dloc[q], sat(c_in + PDD[q])) with saturated prefix sums"""
    n, M = Mn.shape[0], Mn.shape[1] - 1
    G, W = group, 64 * group
    assert W >= M
    pad = lambda v: np.concatenate([v[..., 1:], np.full(v.shape[:-1] + (W - M,), NEG16, np.int64)], axis=-1).reshape(v.shape[:-1] + (64, G))      # noqa: E731
    m, tdd, tmd = pad(Mn), pad(t[R.ROW_DD]), pad(t[R.ROW_MD])
    dloc = np.full((n, 64, G), NEG16, np.int64)
    pdd = np.zeros((64, G), np.int64)
    for q in range(1, G):
        dloc[:, :, q] = np.maximum(sat(dloc[:, :, q - 1] + tdd[:, q - 1]), sat(m[:, :, q - 1] + tmd[:, q - 1]))
        pdd[:, q] = sat(pdd[:, q - 1] + tdd[:, q - 1])
    b = np.maximum(sat(dloc[:, :, G - 1] + tdd[:, G - 1]), sat(m[:, :, G - 1] + tmd[:, G - 1]))
    a = tdd.sum(axis=1)                                                         # wide sum of a group
    csum = np.concatenate([[0], np.cumsum(a)])
    for s in range(6):
        d = 1 << s
        A = sat(csum[d + 1:65] - csum[1:65 - d])                                # groups l - d + 1 .. l for l = d .. 63, saturated
        nb = b.copy()
        nb[:, d:] = np.maximum(b[:, d:], sat(b[:, :-d] + A))
        b = nb
    c_in = np.concatenate([np.full((n, 1), NEG16, np.int64), b[:, :-1]], axis=1)
    D = np.maximum(dloc, sat(c_in[:, :, None] + pdd[None]))
    Dn = np.full_like(Mn, NEG16)
    Dn[:, 1:] = D.reshape(n, W)[:, :M]
    Dn[:, 1] = NEG16
    return Dn


def vit16_batch(tab, records, d_form="wide", group=None, keep=None):
    """vf of many records against one profile at once -> int32 [n_rec]; NO_SCORE for an empty record or one with a byte that is no residue, VF_OVER
    from the first row with E16 == 32767. keep: a list that receives (M16, I16, D16, E16) of every row, [n_rec, M + 1] each (small shapes only)"""
    n, M = len(records), tab.shape[1] - 1
    Ls = np.array([len(r) for r in records], np.int64)
    out = np.full(n, R.NO_SCORE, np.int64)
    ok = np.array([len(r) > 0 and bool((R._LUT[np.frombuffer(bytes(r), np.uint8)] < 20).all()) for r in records], bool)
    live = np.flatnonzero(ok)
    if len(live) == 0:
        return out.astype(np.int32)
    assert Ls.max() <= R.MAX_L
    Lv = Ls[live]
    x = np.zeros((len(live), int(Lv.max())), np.int64)
    for j, r in enumerate(live):
        x[j, :Lv[j]] = R.encode(records[r])
    sp = np.array([R.specials(int(L), M) for L in Lv], np.int64)
    tloop, tmove, null, tbm = sp[:, 0], sp[:, 1], sp[:, 2], int(sp[0, 3])
    t = tables16(tab).astype(np.int64)
    msc_of = t[:20].copy()
    Mv = np.full((len(live), M + 1), NEG16, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    P = np.zeros(M + 1, np.int64)
    P[2:] = np.cumsum(t[R.ROW_DD, 1:M])                                         # wide
    J = np.full(len(live), R.NEG, np.int64); C = J.copy(); B = tmove.copy()
    over = np.zeros(len(live), bool)
    for i in range(1, int(Lv.max()) + 1):
        on = (Lv >= i) & ~over
        if not on.any():
            break
        ent = sat(h(B + tbm))
        msc = msc_of[x[:, i - 1]]
        inn = np.maximum(np.maximum(sat(Mv + t[R.ROW_MM]), sat(Iv + t[R.ROW_IM])), sat(Dv + t[R.ROW_DM]))
        Mn = np.full_like(Mv, NEG16)
        Mn[:, 1:] = sat(msc[:, 1:] + np.maximum(inn[:, :-1], ent[:, None]))
        In = np.maximum(sat(Mv + t[R.ROW_MI]), sat(Iv + t[R.ROW_II]))
        In[:, 0] = NEG16; In[:, M] = NEG16
        if d_form == "wide":
            Dn = np.full_like(Mv, NEG16)
            if M >= 2:
                b = sat(Mn[:, 1:M] + t[R.ROW_MD, 1:M])
                Dn[:, 2:] = np.maximum(P[2:] + np.maximum.accumulate(b - P[2:], axis=1), NEG16)
        else:
            assert d_form == "sat_groups" and group
            Dn = _d_sat_groups(Mn, t, group)
        E16 = Mn[:, 1:].max(axis=1)
        if keep is not None:
            keep.append((Mn.copy(), In.copy(), Dn.copy(), E16.copy()))
        over |= on & (E16 == MAX16)
        on &= ~over
        E = 2 * E16
        Jn = np.maximum(np.maximum(J + tloop, E + R.T_EJ), R.NEG)
        Cn = np.maximum(np.maximum(C + tloop, E + R.T_EC), R.NEG)
        Bn = np.maximum(i * tloop, Jn) + tmove
        J, C, B = np.where(on, Jn, J), np.where(on, Cn, C), np.where(on, Bn, B)
        Mv, Iv, Dv = Mn, In, Dn
    raw = np.where(over, VF_OVER, C + tmove - null)
    assert (np.abs(raw) < (1 << 31)).all()
    out[live] = raw
    return out.astype(np.int32)


def vit16(tab, rec, **kw):
    return int(vit16_batch(tab, [rec], **kw)[0])


def search(models, records):
    """int32 [n_rec, n_prof] of vf"""
    out = np.zeros((len(records), len(models)), np.int32)
    for p, m in enumerate(models):
        out[:, p] = vit16_batch(m["tables"], records)
    return out


def passes(score, floor):
    """bool [n_rec, n_prof]: the pair has the score and it reaches the profile's floor (None: every pair that has the score); VF_OVER passes every floor"""
    score = np.asarray(score)
    ok = score != R.NO_SCORE
    return ok if floor is None else ok & (score.astype(np.int64) >= np.asarray(floor, np.int64)[None, :])


def _behind(models, records, sel, batch):
    out = np.full(sel.shape, R.NO_SCORE, np.int32)
    for p, m in enumerate(models):
        rows = np.flatnonzero(sel[:, p])
        if len(rows):
            out[rows, p] = batch(m["tables"], [records[r] for r in rows])
    return out


def search_staged(models, records, vf_floor, use_msv=False, msv_floor=None, forward=False, vit_floor=None, msv=None):
    """what gs_hmm_search_staged writes -> (msv or None, vf, vit, fwd or None), int32 [n_rec, n_prof]: MSV of every pair (use_msv), vf of every pair
    or of the pairs that pass msv_floor, the Viterbi score of pyref_hmm for the pairs whose vf passes vf_floor, Forward behind that matrix and vit_floor
    as pyref_hmm_forward.search_forward() runs it; NO_SCORE wherever a stage did not run"""
    import pyref_hmm_forward as F
    import pyref_hmm_msv as V
    if use_msv and msv is None:
        msv = V.search(models, records)
    ran = V.passes(msv, msv_floor) if use_msv else np.ones((len(records), len(models)), bool)
    vf = _behind(models, records, ran, vit16_batch)
    vit = _behind(models, records, passes(vf, vf_floor), R.viterbi_batch)
    fwd = F.search_forward(models, records, floor=vit_floor, vit=vit)[1] if forward else None
    return (msv if use_msv else None), vf, vit, fwd
