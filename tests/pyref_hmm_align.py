"""SPEC 13.6 (hmmsearch: the optimal-accuracy alignment of an envelope) restated in numpy on int64, a row at a time with pointer bytes; a second
definition of the same section, cell by cell on full matrices with an explicit arg-max walk; an f64 yardstick (posteriors from a cell-by-cell f64
Forward / Backward, then the program in floats); and the text hmmsearch(alignments=) writes. Forward and its kept cells are pyref_hmm_null2's, Backward
is that file's loop with the posteriors stored where it folds. lse, the padded tables and the groups are those of SPEC 13.1 / 13.4, the model and the
specials those of SPEC 13. Nothing here calls the library."""
import numpy as np

import pyref_hmm as R
import pyref_hmm_forward as F
import pyref_hmm_null2 as N2
import pyref_hmm_posterior as P

NEG, STAR, NO_SCORE, NO_HIT = R.NEG, R.STAR, R.NO_SCORE, R.NO_HIT
lse = F.lse
ALI_WORDS = 8                                      # i_from, i_to, k_from, k_to, oa, n_match, n_ins, n_del
ALI_MAX_LD = 8192
OFF = -(1 << 30)
PTR_B = 3                                          # M pointer: 0 M, 1 I, 2 D of node k - 1 in row i - 1, 3 B[i-1]; bit 2: I from I; bit 3: D from D
TRANS = (("MM", R.ROW_MM), ("MI", R.ROW_MI), ("MD", R.ROW_MD), ("IM", R.ROW_IM), ("II", R.ROW_II), ("DM", R.ROW_DM), ("DD", R.ROW_DD))


def exp2_unrounded():
    """65536 * 2^(-f / 1024) for f = 0 .. 1023, before rounding"""
    return 65536.0 * np.exp2(-np.arange(1024) / 1024.0)


EXP2 = np.floor(exp2_unrounded() + 0.5).astype(np.int64)


def w(u):
    """the Q16 weight of a posterior of u units, u <= 0: EXP2[-u & 1023] >> (-u >> 10), 0 from 17 * 1024 units down"""
    n = -np.asarray(u, np.int64)
    return EXP2[n & 1023] >> np.minimum(n >> 10, 31)


def posterior(g, x, L):
    """pM, pI (int64 [Ld + 1, 64 G], word k - 1 = node k, row 0 unused; NEG for padding nodes and for I of node M) and pX (int64 [Ld + 1]) of the
    segment x (residue indices) of a record of L residues: Forward is N2.forward_kept, Backward is N2.segment's loop, word for word"""
    Ld, M, G = len(x), g["M"], g["G"]
    assert 1 <= Ld <= L <= F.FWD_MAX_L
    tloop, tmove, _, tbm, _, _ = R.specials(L, M)
    valid = g["valid"]
    valid_i = (np.arange(64 * G) < M - 1).reshape(64, G)
    fM, fI, E, J, C = N2.forward_kept(g, x, L)
    total = int(C[Ld]) + tmove
    pM = np.full((Ld + 1, 64 * G), NEG, np.int64); pI = pM.copy()
    pX = np.full(Ld + 1, NEG, np.int64)
    Mv = np.full((64, G), NEG, np.int64); Iv = Mv.copy()
    n = j = NEG
    for s in range(Ld + 1):
        i = Ld - s
        take = np.where(valid, g["msc"][x[i]] + Mv, NEG) if s else np.full((64, G), NEG, np.int64)
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
        if i >= 1:
            pM[i] = np.where(valid, np.minimum(0, np.maximum(NEG, fM[i] + Mv - total)), NEG).reshape(-1)
            pI[i] = np.where(valid_i, np.minimum(0, np.maximum(NEG, fI[i] + Iv - total)), NEG).reshape(-1)
            xn = int(lse(lse(i * tloop + n, J[i - 1] + tloop + j), C[i - 1] + tloop + bC))
            pX[i] = min(0, max(NEG, xn - total))
    return pM, pI, pX


def masks(tab):
    """per transition the int64 [M + 1] words [t]: 0 where the table word of node k is > STAR, else OFF"""
    return {name: np.where(tab[row].astype(np.int64) > STAR, 0, OFF) for name, row in TRANS}


def _walk(Ld, M, ptr, kE, c_from_e, oa, a, pM, pI):
    """the walk of 13.6 over pointer bytes -> (slot words, columns int64 [n, 4] of (state, k, record row, p))"""
    i = Ld
    while not c_from_e[i]:
        i -= 1
        assert i >= 1
    i_to, k_to = i, int(kE[i])
    k, st, cols = k_to, 0, []
    while True:
        assert 1 <= i <= Ld and 1 <= k <= M
        p = int(ptr[i, k])
        if st == 0:
            cols.append((0, k, a + i - 1, int(pM[i, k - 1])))
            if p & 3 == PTR_B:
                break
            st, i, k = p & 3, i - 1, k - 1
        elif st == 1:
            cols.append((1, k, a + i - 1, int(pI[i, k - 1])))
            st, i = (1 if p & 4 else 0), i - 1
        else:
            cols.append((2, k, a + i - 1, 0))
            st, k = (2 if p & 8 else 0), k - 1
    cols.reverse()
    cols = np.array(cols, np.int64).reshape(-1, 4)
    nm, ni, nd = (int((cols[:, 0] == s).sum()) for s in range(3))
    return (a + i - 1, a + i_to - 1, k, k_to, int(oa), nm, ni, nd), cols


def program_rows(tab, pM, pI, pX, a=1, use_masks=True):
    """the program of 13.6 a row at a time with a pointer byte per cell, then the walk -> (slot words, columns). a: the record row of the segment's
    first row. use_masks=False drops the rule of allowed transitions (every [t] = 0): what the mask test shows to be wrong"""
    Ld, M = len(pX) - 1, tab.shape[1] - 1
    assert Ld <= ALI_MAX_LD
    m = masks(tab)
    if not use_masks:
        m = {k: np.zeros_like(v) for k, v in m.items()}
    AM = np.full(M + 1, OFF, np.int64); AI = AM.copy(); AD = AM.copy()
    ptr = np.zeros((Ld + 1, M + 1), np.uint8)
    kE = np.zeros(Ld + 1, np.int64)
    c_from_e = np.zeros(Ld + 1, bool)
    # the D links: node j hands D on to node j + 1 iff [tDD[j]] = 0; sid numbers the stretches of nodes between broken links
    sid = np.zeros(M + 1, np.int64)
    sid[1:] = np.cumsum(m["DD"][1:] != 0)
    big = sid[1:M] << 32
    Nn, C = 0, OFF
    for i in range(1, Ld + 1):
        wM = np.concatenate([[0], w(pM[i, :M])]); wI = np.concatenate([[0], w(pI[i, :M])]); wX = int(w(pX[i]))
        ca, cb, cc = AM + m["MM"], AI + m["IM"], AD + m["DM"]
        s = np.maximum(np.maximum(np.maximum(ca, cb), cc)[:-1], Nn)
        Mn = np.full(M + 1, OFF, np.int64)
        Mn[1:] = wM[1:] + s
        code = np.where(ca[:-1] == s, 0, np.where(cb[:-1] == s, 1, np.where(cc[:-1] == s, 2, PTR_B)))
        from_m = AM + m["MI"]
        v = np.maximum(from_m, AI + m["II"])
        ibit = from_m != v
        In = np.maximum(wI + v, OFF)
        In[0] = OFF
        Dn = np.full(M + 1, OFF, np.int64)
        dbit = np.ones(M + 1, bool)
        if M >= 2:
            bb = Mn[1:M] + m["MD"][1:M]
            bb = np.where(bb >= 0, bb, OFF)                                                     # an unreachable word is OFF here: only reachable words are read
            Dn[2:] = np.maximum.accumulate(big + (bb - OFF)) - big + OFF
            dbit[2:] = bb != Dn[2:]
        ptr[i, 1:] = code
        ptr[i] |= (ibit.astype(np.uint8) << 2) | (dbit.astype(np.uint8) << 3)
        e = int(Mn[1:].max())
        kE[i] = 1 + int(np.argmax(Mn[1:] == e))
        Nn += wX
        C = max(C + wX, e)
        c_from_e[i] = C == e
        AM, AI, AD = Mn, In, Dn
    assert 0 <= C < (1 << 29)
    return _walk(Ld, M, ptr, kE, c_from_e, C, a, pM, pI)


def program_cells(tab, pM, pI, pX, a=1):
    """the same section cell by cell as it is written: full matrices of Python integers (None = unreachable), every alternative spelled out, and a walk
    that decides each step by comparing the values of the alternatives in the listed order (the twin of program_rows; small shapes only)"""
    Ld, M = len(pX) - 1, tab.shape[1] - 1
    ok = {name: [bool(v > STAR) for v in tab[row]] for name, row in TRANS}
    wm = [[0] * (M + 1)] + [[0] + [int(v) for v in w(pM[i, :M])] for i in range(1, Ld + 1)]
    wi = [[0] * (M + 1)] + [[0] + [int(v) for v in w(pI[i, :M])] for i in range(1, Ld + 1)]
    wx = [0] + [int(w(pX[i])) for i in range(1, Ld + 1)]
    via = lambda v, t, k: v if v is not None and ok[t][k] else None                           # noqa: E731
    best = lambda alts: max((v for v in alts if v is not None), default=None)                 # noqa: E731
    AM = [[None] * (M + 1) for _ in range(Ld + 1)]; AI = [[None] * (M + 1) for _ in range(Ld + 1)]; AD = [[None] * (M + 1) for _ in range(Ld + 1)]
    AN = [0] * (Ld + 1); AE = [None] * (Ld + 1); AC = [None] * (Ld + 1)
    m_alts = lambda i, k: [via(AM[i - 1][k - 1], "MM", k - 1), via(AI[i - 1][k - 1], "IM", k - 1), via(AD[i - 1][k - 1], "DM", k - 1), AN[i - 1]]      # noqa: E731
    i_alts = lambda i, k: [via(AM[i - 1][k], "MI", k), via(AI[i - 1][k], "II", k)]             # noqa: E731
    d_alts = lambda i, k: [via(AM[i][k - 1], "MD", k - 1), via(AD[i][k - 1], "DD", k - 1)]     # noqa: E731
    for i in range(1, Ld + 1):
        AN[i] = AN[i - 1] + wx[i]
        for k in range(1, M + 1):
            AM[i][k] = wm[i][k] + best(m_alts(i, k))
            if k < M:
                v = best(i_alts(i, k))
                AI[i][k] = None if v is None else wi[i][k] + v
            AD[i][k] = best(d_alts(i, k)) if k >= 2 else None
        AE[i] = max(AM[i][1:])
        AC[i] = best([None if AC[i - 1] is None else AC[i - 1] + wx[i], AE[i]])
    first = lambda alts, v: next(n for n, x in enumerate(alts) if x == v)                      # noqa: E731
    i = Ld
    while AC[i] != AE[i]:
        i -= 1
    i_to = i
    k_to = k = 1 + AM[i][1:].index(AE[i])
    st, cols = 0, []
    while True:
        if st == 0:
            cols.append((0, k, a + i - 1, int(pM[i, k - 1])))
            src = first(m_alts(i, k), AM[i][k] - wm[i][k])
            if src == 3:
                break
            st, i, k = src, i - 1, k - 1
        elif st == 1:
            cols.append((1, k, a + i - 1, int(pI[i, k - 1])))
            st, i = first(i_alts(i, k), AI[i][k] - wi[i][k]), i - 1
        else:
            cols.append((2, k, a + i - 1, 0))
            st, k = (0, 2)[first(d_alts(i, k), AD[i][k])], k - 1
    cols.reverse()
    cols = np.array(cols, np.int64).reshape(-1, 4)
    nm, ni, nd = (int((cols[:, 0] == s).sum()) for s in range(3))
    return (a + i - 1, a + i_to - 1, k, k_to, AC[Ld], nm, ni, nd), cols


def segment(tab, x, L, a=1, g=None, use_masks=True):
    """the alignment of the segment x (residue indices) of a record of L residues whose first row is record row a -> (slot words, columns [n, 4])"""
    g = g or P._groups(tab)
    pM, pI, pX = posterior(g, x, L)
    return program_rows(tab, pM, pI, pX, a, use_masks)


def align_pairs(models, records, pair_rec, pair_prof, n_env, env, max_env, use_masks=True):
    """what gs_hmm_align writes: (int32 slots [n, max_env, 8], per pair the list of its listed slots' columns as int64 [n_cols, 4] of (state, k, i, pp)).
    A pair without a record, with an empty one or with a byte that is no residue: zeros and no columns. use_masks=False: what a program that forgot
    the rule of allowed transitions would write (program_rows)"""
    n = len(pair_rec)
    slots = np.zeros((n, max_env, ALI_WORDS), np.int32)
    cols = [[] for _ in range(n)]
    memo, groups = {}, {}
    for j, (r, p) in enumerate(zip(pair_rec, pair_prof)):
        r, p = int(r), int(p)
        if r == NO_HIT or len(records[r]) == 0 or (R._LUT[np.frombuffer(bytes(records[r]), np.uint8)] >= 20).any():
            continue
        x = R.encode(records[r])
        if p not in groups:
            groups[p] = P._groups(models[p]["tables"])
        for d in range(min(int(n_env[j]), max_env)):
            a, b = int(env[j, d, 0]), int(env[j, d, 1])
            if (r, p, a, b) not in memo:
                memo[r, p, a, b] = segment(models[p]["tables"], x[a - 1:b], len(x), a, g=groups[p], use_masks=use_masks)
            slots[j, d], c = memo[r, p, a, b]
            cols[j].append(c)
    return slots, cols


def column_words(c):
    """the two int32 words per column of gs_hmm_align's col_out from columns (state, k, i, pp)"""
    out = np.zeros((len(c), 2), np.int64)
    out[:, 0] = (c[:, 0] << 28) | (c[:, 1] << 16) | (c[:, 2] - 1)
    out[:, 1] = c[:, 3]
    return out.astype(np.int32)


def path_value(tab, cols, pX, a, use=w):
    """the value of a path under the weights: `use` of every M and I cell's posterior plus `use`(pX) of the segment's rows outside the path's rows"""
    emit = cols[cols[:, 0] != 2]
    rows = np.ones(len(pX), bool)
    rows[0] = False
    rows[emit[:, 2] - a + 1] = False
    return int(use(emit[:, 3]).sum() + use(pX[rows]).sum())


def cigar(cols):
    """run lengths of the columns' states as text, e.g. 30M40D51M"""
    out, st = [], cols[:, 0]
    i = 0
    while i < len(st):
        j = i
        while j < len(st) and st[j] == st[i]:
            j += 1
        out.append("%d%s" % (j - i, "MID"[int(st[i])]))
        i = j
    return "".join(out)


STEP_ROW = {(0, 0): R.ROW_MM, (0, 1): R.ROW_MI, (0, 2): R.ROW_MD, (1, 0): R.ROW_IM, (1, 1): R.ROW_II, (2, 0): R.ROW_DM, (2, 2): R.ROW_DD}


def steps_allowed(tab, cols):
    """every step between two columns is a transition of the model whose table word is > STAR, and moves as that transition moves"""
    for (s0, k0, i0, _), (s1, k1, i1, _) in zip(cols[:-1].tolist(), cols[1:].tolist()):
        if (s0, s1) not in STEP_ROW or tab[STEP_ROW[s0, s1], k0] <= STAR:
            return False
        if (k1 - k0, i1 - i0) != ((1, 1), (0, 1), (1, 0))[s1]:
            return False
    return bool(len(cols)) and cols[0, 0] == 0 and cols[-1, 0] == 0


def viterbi_columns(tab, rec):
    """the domains of the Viterbi path of SPEC 13.2 with their cells: pyref_hmm_trace.trace's row step and walk (the same lines, its assertions left to
    it), every visited cell kept -> a list per domain, in sequence order, of int64 [n, 3] columns (state, k, i)"""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    t = tab.astype(np.int64)
    tloop, tmove, _, tbm = R.specials(L, M)[:4]
    Mv = np.full(M + 1, NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    Pd = np.zeros(M + 1, np.int64)
    Pd[2:] = np.cumsum(t[R.ROW_DD, 1:M])
    ptr = np.zeros((L + 1, M + 1), np.uint8)
    kE = np.zeros(L + 1, np.int64)
    c_from_e = np.zeros(L + 1, bool); j_from_e = np.zeros(L + 1, bool); b_from_n = np.zeros(L + 1, bool)
    J = C = NEG
    B, b_from_n[0] = tmove, True
    for i in range(1, L + 1):
        msc = t[x[i - 1]]
        a, b, c = Mv + t[R.ROW_MM], Iv + t[R.ROW_IM], Dv + t[R.ROW_DM]
        s = np.maximum(np.maximum(np.maximum(a, b), c)[:-1], B + tbm)
        Mn = np.full(M + 1, NEG, np.int64)
        Mn[1:] = np.maximum(msc[1:] + s, NEG)
        code = np.where(a[:-1] == s, 0, np.where(b[:-1] == s, 1, np.where(c[:-1] == s, 2, PTR_B)))
        from_m = Mv + t[R.ROW_MI]
        In = np.maximum(np.maximum(from_m, Iv + t[R.ROW_II]), NEG)
        ibit = from_m != In
        In[0] = NEG; In[M] = NEG
        Dn = np.full(M + 1, NEG, np.int64)
        dbit = np.ones(M + 1, bool)
        if M >= 2:
            bb = np.maximum(Mn[1:M] + t[R.ROW_MD, 1:M], NEG)
            Dn[2:] = Pd[2:] + np.maximum.accumulate(bb - Pd[2:])
            dbit[2:] = Mn[1:M] + t[R.ROW_MD, 1:M] != Dn[2:]
        ptr[i, 1:] = code
        ptr[i] |= (ibit.astype(np.uint8) << 2) | (dbit.astype(np.uint8) << 3)
        e = int(Mn[1:].max())
        kE[i] = 1 + int(np.argmax(Mn[1:] == e))
        Jn, Cn = max(J + tloop, e + R.T_EJ, NEG), max(C + tloop, e + R.T_EC, NEG)
        c_from_e[i], j_from_e[i] = e + R.T_EC == Cn, e + R.T_EJ == Jn
        b_from_n[i] = i * tloop >= Jn
        J, C = Jn, Cn
        B = max(i * tloop, J) + tmove
        Mv, Iv, Dv = Mn, In, Dn
    doms = []
    i, first = L, True
    while True:
        while not (c_from_e[i] if first else j_from_e[i]):
            i -= 1
        first = False
        k, st, cells = int(kE[i]), 0, []
        while True:
            p = int(ptr[i, k])
            cells.append((st, k, i))
            if st == 0:
                if p & 3 == PTR_B:
                    break
                st, i, k = p & 3, i - 1, k - 1
            elif st == 1:
                st, i = (1 if p & 4 else 0), i - 1
            else:
                st, k = (2 if p & 8 else 0), k - 1
        doms.append(np.array(cells[::-1], np.int64))
        i -= 1
        if b_from_n[i]:
            break
    return doms[::-1]


# ---- the yardstick: f64, cell by cell, full matrices ------------------------------------------------------------------------------------------------
def posterior_f64(tab, x, L):
    """N2.segment_f64's Forward and Backward (the same lines) with every cell kept -> (PM, PI float [Ld + 1, M + 1] and PX float [Ld + 1]: the
    posterior probabilities of M_k / I_k emitting x_i and of x_i being emitted outside the core)"""
    Ld, M = len(x), tab.shape[1] - 1
    t = tab.astype(np.float64)
    t[tab <= STAR] = -np.inf
    tloop, tmove, _, tbm, _, _ = (float(v) for v in R.specials(L, M))
    tE = float(R.T_EJ)
    la, ninf, u = np.logaddexp2, -np.inf, 1024.0
    lau = lambda p, q: u * la(p / u, q / u)                                                   # noqa: E731
    tr = {n: t[r] for n, r in TRANS}
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
        bM = np.full((Ld + 2, M + 2), ninf); bI = bM.copy()
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
        PM = np.zeros((Ld + 1, M + 1)); PI = PM.copy(); PX = np.zeros(Ld + 1)
        PM[1:, 1:] = np.exp2((fM[1:, 1:] + bM[1:Ld + 1, 1:M + 1] - total_f) / u)
        PI[1:, 1:M] = np.exp2((fI[1:, 1:M] + bI[1:Ld + 1, 1:M] - total_f) / u)
        xn = lau(lau(i * tloop + bN[1:], fJ[:-1] + tloop + bJ[1:]), fC[:-1] + tloop + bC[1:])
        PX[1:] = np.exp2((xn - total_f) / u)
    return np.minimum(PM, 1.0), np.minimum(PI, 1.0), np.minimum(PX, 1.0)


def program_f64(tab, PM, PI, PX):
    """the program of 13.6 in floats over f64 posteriors (-inf = unreachable) -> oa as a float: the expected number of correctly placed residues"""
    Ld, M = len(PX) - 1, tab.shape[1] - 1
    ninf = -np.inf
    m = {name: np.where(tab[row] > STAR, 0.0, ninf) for name, row in TRANS}
    AM = np.full(M + 1, ninf); AI = AM.copy(); AD = AM.copy()
    Nn, C = 0.0, ninf
    for i in range(1, Ld + 1):
        s = np.maximum(np.maximum(np.maximum(AM + m["MM"], AI + m["IM"]), AD + m["DM"])[:-1], Nn)
        Mn = np.full(M + 1, ninf)
        Mn[1:] = PM[i, 1:] + s
        In = PI[i] + np.maximum(AM + m["MI"], AI + m["II"])
        In[0] = In[M] = ninf
        Dn = np.full(M + 1, ninf)
        for k in range(2, M + 1):
            Dn[k] = max(Mn[k - 1] + m["MD"][k - 1], Dn[k - 1] + m["DD"][k - 1])
        e = float(Mn[1:].max())
        Nn += PX[i]
        C = max(C + PX[i], e)
        AM, AI, AD = Mn, In, Dn
    return C


# ---- the text of hmmsearch(alignments=) ---------------------------------------------------------------------------------------------------------------
ALIGN_HEADER = b"# == target\tprofile\tacc\tenv\tn_env\tali_from\tali_to\thmm_from\thmm_to\tM\tacc\tn_match\tn_ins\tn_del\n"


def alignment_block(tab, rec, cols):
    """the four text lines of one alignment: model, match, target, PP"""
    cons = R.consensus(tab).decode().lower()
    model, match, target, pp = [], [], [], []
    for st, k, i, p in (tuple(int(v) for v in c) for c in cols):
        res = chr(bytes(rec)[i - 1]).upper()
        if st == 0:
            c = cons[k - 1]
            model.append(c); target.append(res)
            match.append(c if c.upper() == res else ("+" if int(tab[R.AA.index(res), k]) > 0 else " "))
        elif st == 1:
            model.append("."); match.append(" "); target.append(res.lower())
        else:
            model.append(cons[k - 1]); match.append(" "); target.append("-")
        if st == 2:
            pp.append(".")
        else:
            d = (10 * int(w(p)) + 32768) >> 16
            pp.append("*" if d >= 10 else str(d))
    return "".join("  %-6s %s\n" % (lab, "".join(s)) for lab, s in (("model", model), ("match", match), ("target", target), ("PP", pp))).encode()


def alignment_bytes(models, ids, records, listed, n_env, env, slots, cols):
    """the text hmmsearch(alignments=) writes: per pair of `listed`, in its order (the envelope table's), per listed envelope a header line and the four
    lines of alignment_block(). slots, cols as align_pairs() returns them"""
    out = [ALIGN_HEADER]
    for j, (r, p) in enumerate(listed):
        m = models[p]
        for d in range(len(cols[j])):
            s = [int(v) for v in slots[j][d]]
            Ld = int(env[j][d][1]) - int(env[j][d][0]) + 1
            out.append(("==\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\t%d\t%d\t%d\n" % (ids[r], m["name"], m["acc"] or "-", d + 1, int(n_env[j]), s[0], s[1], s[2], s[3],
                                                                                          m["tables"].shape[1] - 1, s[4] / (65536.0 * Ld), s[5], s[6], s[7])).encode())
            out.append(alignment_block(m["tables"], records[r], cols[j][d]))
    return b"".join(out)
