"""SPEC 13.2 (hmmsearch: the domains of the Viterbi path) restated in numpy, plus a cell-by-cell walk over full matrices that is the restatement's own
yardstick, and the writer of the domain table. Integers only. Nothing here calls the library."""
import numpy as np

import pyref_hmm as R

DOM_WORDS = 8
TRACE_MAX_L = 65536
CLAMP = -(1 << 19)                                  # every traced cell lies above it, far from NEG (SPEC 13.2)
PTR_B = 3                                           # M pointer: 0 M, 1 I, 2 D of node k - 1 in row i - 1, 3 B[i-1]
DOMAIN_HEADER = b"target\tprofile\tacc\tdom\tn_dom\ti_from\ti_to\tk_from\tk_to\tM\tseg_bits\tn_match\tn_ins\tn_del\n"


def _check(tab, rec, raw, doms, L, sp):
    """the two identities of SPEC 13.2, the order of the domains and the score of SPEC 13"""
    tloop, tmove, null = sp[0], sp[1], sp[2]
    for (i_from, i_to, k_from, k_to, seg, nm, ni, nd) in doms:
        assert nm + ni == i_to - i_from + 1 and nm + nd == k_to - k_from + 1, (i_from, i_to, k_from, k_to, nm, ni, nd)
    assert all(a[1] < b[0] for a, b in zip(doms, doms[1:]))
    n, a = len(doms), sum(d[1] - d[0] + 1 for d in doms)
    assert n >= 1
    assert raw == sum(d[4] for d in doms) + n * tmove + (n - 1) * R.T_EJ + R.T_EC + (L - a) * tloop + tmove - null
    assert raw == R.viterbi(tab, rec)


def trace(tab, rec):
    """(raw, domains) of one record against one profile: the row step of pyref_hmm.viterbi, which also leaves a byte of pointers per cell (bits 0-1 the
    M pointer, bit 2: I from I, bit 3: D from D) and E, B, the lowest node of E and the three decisions per row; then the walk of SPEC 13.2 over them.
    domains: a list of 8-tuples (i_from, i_to, k_from, k_to, seg, n_match, n_ins, n_del) in sequence order; an empty record: (NO_SCORE, [])"""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    if L == 0:
        return R.NO_SCORE, []
    assert L <= TRACE_MAX_L
    NEG = R.NEG
    t = tab.astype(np.int64)
    sp = R.specials(L, M)
    tloop, tmove, null, tbm = sp[:4]
    Mv = np.full(M + 1, NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    P = np.zeros(M + 1, np.int64)
    P[2:] = np.cumsum(t[R.ROW_DD, 1:M])
    ptr = np.zeros((L + 1, M + 1), np.uint8)
    Mm = np.full((L + 1, M + 1), NEG, np.int32); Im = Mm.copy(); Dm = Mm.copy()
    E = np.full(L + 1, NEG, np.int64); Bs = np.zeros(L + 1, np.int64); kE = np.zeros(L + 1, np.int64)
    c_from_e = np.zeros(L + 1, bool); j_from_e = np.zeros(L + 1, bool); b_from_n = np.zeros(L + 1, bool)
    J = C = NEG
    Bs[0], b_from_n[0] = tmove, True
    for i in range(1, L + 1):
        B = int(Bs[i - 1])
        msc = t[x[i - 1]]
        a, b, c = Mv + t[R.ROW_MM], Iv + t[R.ROW_IM], Dv + t[R.ROW_DM]
        inn = np.maximum(np.maximum(a, b), c)
        s = np.maximum(inn[:-1], B + tbm)
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
            Dn[2:] = P[2:] + np.maximum.accumulate(bb - P[2:])
            dbit[2:] = Mn[1:M] + t[R.ROW_MD, 1:M] != Dn[2:]
        ptr[i, 1:] = code
        ptr[i] |= (ibit.astype(np.uint8) << 2) | (dbit.astype(np.uint8) << 3)
        e = int(Mn[1:].max())
        assert e >= int(Dn[1:].max()) and int(Mn[1:].min()) > CLAMP             # E = max_k M: no path leaves through D; no M cell is near the clamp
        E[i], kE[i] = e, 1 + int(np.argmax(Mn[1:] == e))
        Jn, Cn = max(J + tloop, e + R.T_EJ, NEG), max(C + tloop, e + R.T_EC, NEG)
        c_from_e[i], j_from_e[i] = e + R.T_EC == Cn, e + R.T_EJ == Jn
        b_from_n[i] = i * tloop >= Jn
        J, C = Jn, Cn
        Bs[i] = max(i * tloop, J) + tmove
        Mv, Iv, Dv = Mn, In, Dn
        Mm[i], Im[i], Dm[i] = Mn, In, Dn
    raw = int(C + tmove - null)
    doms = []
    i, first = L, True
    while True:
        while not (c_from_e[i] if first else j_from_e[i]):
            i -= 1
            assert i >= 1
        first = False
        i_to, k_to = i, int(kE[i])
        k, st, nm, ni, nd = k_to, 0, 0, 0, 0
        while True:
            assert 1 <= i <= L and 1 <= k <= M
            p = int(ptr[i, k])
            if st == 0:
                assert Mm[i, k] > CLAMP
                nm += 1
                if p & 3 == PTR_B:
                    break
                st, i, k = p & 3, i - 1, k - 1
            elif st == 1:
                assert Im[i, k] > CLAMP
                ni += 1
                st, i = (1 if p & 4 else 0), i - 1
            else:
                assert Dm[i, k] > CLAMP
                nd += 1
                st, k = (2 if p & 8 else 0), k - 1
        doms.append((i, i_to, k, k_to, int(E[i_to] - Bs[i - 1]), nm, ni, nd))
        i -= 1
        if b_from_n[i]:
            break
    doms.reverse()
    _check(tab, rec, raw, doms, L, sp)
    return raw, doms


def trace_naive(tab, rec):
    """the same by the rules as SPEC 13.2 writes them: full matrices cell by cell, then every step of the walk decided by comparing values
    (the yardstick of trace(); small shapes only)"""
    x = R.encode(rec)
    L, M = len(x), tab.shape[1] - 1
    if L == 0:
        return R.NO_SCORE, []
    NEG = R.NEG
    t = [[int(v) for v in row] for row in tab]
    sp = R.specials(L, M)
    tloop, tmove, null, tbm = sp[:4]
    Mm = [[NEG] * (M + 1) for _ in range(L + 1)]
    Im = [[NEG] * (M + 1) for _ in range(L + 1)]
    Dm = [[NEG] * (M + 1) for _ in range(L + 1)]
    B = [tmove] + [0] * L
    J = [NEG] * (L + 1)
    C = [NEG] * (L + 1)
    E = [NEG] * (L + 1)
    for i in range(1, L + 1):
        for k in range(1, M + 1):
            best = B[i - 1] + tbm
            for prev, row in ((Mm, R.ROW_MM), (Im, R.ROW_IM), (Dm, R.ROW_DM)):
                best = max(best, prev[i - 1][k - 1] + t[row][k - 1])
            Mm[i][k] = max(t[x[i - 1]][k] + best, NEG)
            if k < M:
                Im[i][k] = max(Mm[i - 1][k] + t[R.ROW_MI][k], Im[i - 1][k] + t[R.ROW_II][k], NEG)
            if k >= 2:
                Dm[i][k] = max(Mm[i][k - 1] + t[R.ROW_MD][k - 1], Dm[i][k - 1] + t[R.ROW_DD][k - 1], NEG)
            E[i] = max(E[i], Mm[i][k])
        assert E[i] >= max(Dm[i][1:])
        J[i] = max(J[i - 1] + tloop, E[i] + R.T_EJ, NEG)
        C[i] = max(C[i - 1] + tloop, E[i] + R.T_EC, NEG)
        B[i] = max(i * tloop, J[i]) + tmove
    raw = C[L] + tmove - null
    doms = []
    i = L
    while C[i] != E[i] + R.T_EC:                                                  # C[i]: from E[i] if equal, else from C[i-1]
        assert C[i] == C[i - 1] + tloop
        i -= 1
    while True:
        i_to = i
        k = k_to = min(k for k in range(1, M + 1) if Mm[i][k] == E[i])             # E[i]: the lowest k
        st, nm, ni, nd = "M", 0, 0, 0
        while True:
            if st == "M":
                assert Mm[i][k] > CLAMP
                nm += 1
                s = Mm[i][k] - t[x[i - 1]][k]
                if k > 1 and Mm[i - 1][k - 1] + t[R.ROW_MM][k - 1] == s:
                    st = "M"
                elif k > 1 and Im[i - 1][k - 1] + t[R.ROW_IM][k - 1] == s:
                    st = "I"
                elif k > 1 and Dm[i - 1][k - 1] + t[R.ROW_DM][k - 1] == s:
                    st = "D"
                else:
                    assert B[i - 1] + tbm == s
                    break
                i, k = i - 1, k - 1
            elif st == "I":
                assert Im[i][k] > CLAMP
                ni += 1
                if Mm[i - 1][k] + t[R.ROW_MI][k] == Im[i][k]:
                    st = "M"
                else:
                    assert Im[i - 1][k] + t[R.ROW_II][k] == Im[i][k]
                i -= 1
            else:
                assert Dm[i][k] > CLAMP
                nd += 1
                if Mm[i][k - 1] + t[R.ROW_MD][k - 1] == Dm[i][k]:
                    st = "M"
                else:
                    assert Dm[i][k - 1] + t[R.ROW_DD][k - 1] == Dm[i][k]
                k -= 1
        doms.append((i, i_to, k, k_to, Mm[i_to][k_to] - B[i - 1], nm, ni, nd))
        i -= 1
        if B[i] == i * tloop + tmove:                                              # B[i]: from N if equal, and the trace is complete
            break
        assert B[i] == J[i] + tmove
        while J[i] != E[i] + R.T_EJ:                                              # J[i]: from E[i] if equal, else from J[i-1]
            assert J[i] == J[i - 1] + tloop
            i -= 1
    doms.reverse()
    _check(tab, rec, raw, doms, L, sp)
    return raw, doms


def trace_pairs(models, records, pair_rec, pair_prof, max_dom):
    """what gs_hmm_trace writes: (int32 raw [n], uint32 n_dom [n], int32 dom [n, max_dom, 8]); a record with a byte that is no residue is an empty pair"""
    n = len(pair_rec)
    raw, nd, dom = np.full(n, R.NO_SCORE, np.int32), np.zeros(n, np.uint32), np.zeros((n, max_dom, DOM_WORDS), np.int32)
    memo = {}
    for j, (r, p) in enumerate(zip(pair_rec, pair_prof)):
        r, p = int(r), int(p)
        if r == R.NO_HIT or len(records[r]) == 0 or (R._LUT[np.frombuffer(bytes(records[r]), np.uint8)] >= 20).any():
            continue
        if (r, p) not in memo:
            memo[r, p] = trace(models[p]["tables"], records[r])
        raw[j], doms = memo[r, p]
        nd[j] = len(doms)
        for d, words in enumerate(doms[:max_dom]):
            dom[j, d] = words
    return raw, nd, dom


def domain_table_bytes(models, ids, scores, raw, n_dom, dom, pair_rec, pair_prof):
    """the text gsearch_amd.hmmsearch(domains=) writes from a trace of the pairs the score table lists: a header line, then a row per domain,
    sorted like the score table (profile, -score, record) and then by the domain's number"""
    at = {(int(r), int(p)): j for j, (r, p) in enumerate(zip(pair_rec, pair_prof))}
    rows = []
    for p in range(len(models)):
        for r in range(len(ids)):
            s = int(scores[r, p])
            if s != R.NO_SCORE and s >= 0:
                rows.append((p, -s, r))
    out = [DOMAIN_HEADER]
    for p, _, r in sorted(rows):
        m, j = models[p], at[r, p]
        assert n_dom[j] <= dom.shape[1]
        for d in range(int(n_dom[j])):
            w = [int(v) for v in dom[j, d]]
            out.append(("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%d\t%d\t%d\n" % (ids[r], m["name"], m["acc"] or "-", d + 1, int(n_dom[j]), w[0], w[1], w[2], w[3],
                                                                                     m["M"], w[4] / 1024.0, w[5], w[6], w[7])).encode())
    return b"".join(out)
