"""SPEC 13.3 (hmmsearch: the MSV prefilter in front of Viterbi) restated in numpy, plus a naive loop that is the restatement's own yardstick. MSV is
the local multihit model of SPEC 13 without insert and delete states and with tMM = 0: ungapped diagonals, any number of them. Integers only in the
scored path. Built on pyref_hmm (units, tables, specials, Viterbi) and pyref_hmm_forward (STATS lines, the floor arithmetic, Forward); nothing here
calls the library."""
import numpy as np

import pyref_hmm as R
import pyref_hmm_forward as F

NEG, NO_SCORE, T_EJ, T_EC = R.NEG, R.NO_SCORE, R.T_EJ, R.T_EC
FLOOR_ALL = F.FLOOR_ALL
MSV_P = 0.02                                        # HMMER's F1


def _encode(rec):
    """residue indices 0..19 of a record, or None when a byte is no residue (either case is a residue, as the device reads them)"""
    x = R._LUT[np.frombuffer(bytes(rec).upper(), np.uint8)]
    return None if (x >= 20).any() else x


def msv(tab, rec):
    """raw MSV score (units) of one record against one profile, a row at a time"""
    x = _encode(rec)
    if x is None or len(x) == 0:
        return NO_SCORE
    L, M = len(x), tab.shape[1] - 1
    assert L <= R.MAX_L
    t = tab.astype(np.int64)
    tloop, tmove, null, tbm, _, _ = R.specials(L, M)
    Mv = np.full(M + 1, NEG, np.int64)                                          # index k = 0..M, column 0 stays NEG
    J = C = NEG
    B = tmove
    for i in range(1, L + 1):
        Mn = np.full(M + 1, NEG, np.int64)
        Mn[1:] = np.maximum(t[x[i - 1], 1:] + np.maximum(Mv[:-1], B + tbm), NEG)
        E = int(Mn[1:].max())
        J = max(J + tloop, E + T_EJ, NEG)
        C = max(C + tloop, E + T_EC, NEG)
        B = max(i * tloop, J) + tmove
        Mv = Mn
    raw = C + tmove - null
    assert -(1 << 31) < raw < (1 << 31)
    return int(raw)


def msv_naive(tab, rec):
    """the same score by the recurrences as SPEC 13.3 writes them, cell by cell (the yardstick of msv(); small shapes only)"""
    x = _encode(rec)
    if x is None or len(x) == 0:
        return NO_SCORE
    L, M = len(x), tab.shape[1] - 1
    t = [[int(v) for v in row] for row in tab]
    tloop, tmove, null, tbm, _, _ = R.specials(L, M)
    Mm = [[NEG] * (M + 1) for _ in range(L + 1)]
    B = [tmove] + [0] * L
    J = [NEG] * (L + 1)
    C = [NEG] * (L + 1)
    for i in range(1, L + 1):
        E = NEG
        for k in range(1, M + 1):
            Mm[i][k] = max(NEG, t[x[i - 1]][k] + max(Mm[i - 1][k - 1], B[i - 1] + tbm))
            E = max(E, Mm[i][k])
        J[i] = max(NEG, J[i - 1] + tloop, E + T_EJ)
        C[i] = max(NEG, C[i - 1] + tloop, E + T_EC)
        B[i] = max(i * tloop, J[i]) + tmove
    return C[L] + tmove - null


def msv_batch(tab, records):
    """msv() of many records against one profile at once: the same row step on [n_rec, M + 1] arrays, every record with its own length model; a record
    takes no more steps once its last row is done -> int32 [n_rec]"""
    n, M = len(records), tab.shape[1] - 1
    enc = [_encode(r) for r in records]
    out = np.full(n, NO_SCORE, np.int64)
    live = np.array([j for j, x in enumerate(enc) if x is not None and len(x) > 0], np.int64)
    if len(live) == 0:
        return out.astype(np.int32)
    Lv = np.array([len(enc[j]) for j in live], np.int64)
    assert Lv.max() <= R.MAX_L
    x = np.zeros((len(live), int(Lv.max())), np.int64)
    for j, r in enumerate(live):
        x[j, :Lv[j]] = enc[r]
    sp = np.array([R.specials(int(L), M) for L in Lv], np.int64)
    tloop, tmove, null, tbm = sp[:, 0], sp[:, 1], sp[:, 2], int(sp[0, 3])
    msc_of = tab[:20].astype(np.int64)                                          # [20, M + 1]
    Mv = np.full((len(live), M + 1), NEG, np.int64)
    J = np.full(len(live), NEG, np.int64); C = J.copy(); B = tmove.copy()
    for i in range(1, int(Lv.max()) + 1):
        on = Lv >= i
        msc = msc_of[x[:, i - 1]]
        Mn = np.full_like(Mv, NEG)
        Mn[:, 1:] = np.maximum(msc[:, 1:] + np.maximum(Mv[:, :-1], (B + tbm)[:, None]), NEG)
        E = Mn[:, 1:].max(axis=1)
        Jn = np.maximum(np.maximum(J + tloop, E + T_EJ), NEG)
        Cn = np.maximum(np.maximum(C + tloop, E + T_EC), NEG)
        Bn = np.maximum(i * tloop, Jn) + tmove
        J, C, B = np.where(on, Jn, J), np.where(on, Cn, C), np.where(on, Bn, B)
        Mv = Mn
    raw = C + tmove - null
    assert (np.abs(raw) < (1 << 31)).all()
    out[live] = raw
    return out.astype(np.int32)


def search(models, records):
    """int32 [n_rec, n_prof] MSV raw scores"""
    out = np.zeros((len(records), len(models)), np.int32)
    for p, m in enumerate(models):
        out[:, p] = msv_batch(m["tables"], records)
    return out


def msv_floor(mu, lam, p=MSV_P):
    """the MSV score (units) whose Gumbel tail mass under STATS LOCAL MSV is p: the arithmetic of the Viterbi floor (SPEC 13.1)"""
    return F.viterbi_floor(mu, lam, p)


def floors(stats, p=MSV_P):
    """int32 [n_prof] from the (values, has) pairs of pyref_hmm_forward.stats_lines(): FLOOR_ALL for a profile without the MSV line"""
    return np.array([msv_floor(v[0], v[1], p) if has & 1 else FLOOR_ALL for v, has in stats], np.int32)


def passes(score, floor):
    """bool [n_rec, n_prof]: the pair has the score and it reaches the profile's floor (floor None: every pair that has the score)"""
    s = np.asarray(score).astype(np.int64)
    fl = np.full(s.shape[1], FLOOR_ALL, np.int64) if floor is None else np.asarray(floor).astype(np.int64)
    return (s != NO_SCORE) & (s >= fl[None, :])


def search_filtered(models, records, floor=None, forward=False, vit_floor=None, msv=None):
    """(msv, vit) or (msv, vit, fwd), int32 [n_rec, n_prof]: MSV of every pair, the Viterbi score of pyref_hmm for the pairs that pass `floor`
    (NO_SCORE for the others), and Forward behind that matrix and vit_floor as pyref_hmm_forward.search_forward() runs it"""
    if msv is None:
        msv = search(models, records)
    sel = passes(msv, floor)
    vit = np.full(msv.shape, NO_SCORE, np.int32)
    for p, m in enumerate(models):
        rows = np.flatnonzero(sel[:, p])
        if len(rows):
            vit[rows, p] = R.viterbi_batch(m["tables"], [records[r] for r in rows])
    if not forward:
        return msv, vit
    return msv, vit, F.search_forward(models, records, floor=vit_floor, vit=vit)[1]
