"""SPEC 13 (hmmsearch: profile-HMM Viterbi scores, best hits) restated in numpy, plus a naive loop that is the restatement's own yardstick.
Integers only in the scored path: Python ints and int64 arrays, no float, no math.log. Nothing here calls the library."""
import functools
import math

import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY"
UNIT_C, UNIT_S = 1015206383, 36                     # units of 2^-10 bit per 10^-5 nat = 1024 / (10^5 ln 2) = UNIT_C / 2^UNIT_S
BG = [-3754, -6189, -4325, -3997, -4766, -3939, -5578, -4181, -4170, -3456, -5524, -4703, -4477, -4772, -4309, -3964, -4310, -3986, -6608, -5160]
NEG = -(1 << 29)
STAR = -(1 << 18)
MAX_FILE_VALUE = 9999999                            # a file value is below 100 nats
MAX_M = 1280
MAX_L = 1 << 18
NO_SCORE = -(1 << 31)
NO_HIT = 0xFFFFFFFF
T_EJ = T_EC = -1024
ROW_MM, ROW_MI, ROW_MD, ROW_IM, ROW_II, ROW_DM, ROW_DD = 20, 21, 22, 23, 24, 25, 26      # rows of a table after the 20 match rows (the file's order)


class HmmError(ValueError):
    pass


@functools.lru_cache(maxsize=None)
def lgq(n):
    """log2(n) in units of 2^-20, 1 <= n < 2^32: the exponent, then 20 fraction bits by repeated squaring of a 32-bit mantissa on 64-bit words"""
    assert 1 <= n < (1 << 32)
    e = n.bit_length() - 1
    x = n << (31 - e)
    r = e << 20
    for j in range(19, -1, -1):
        x = (x * x) >> 31
        if x >= (1 << 32):
            x >>= 1
            r |= 1 << j
    return r


def units_log(num, den):
    """units(ln(num / den)), rounded to the nearest unit (floor of x + 1/2)"""
    return (lgq(num) - lgq(den) + 512) >> 10


def specials(L, M):
    """(tloop, tmove, null, tBM, nloop, nmove) of a target of L residues and a profile of M nodes"""
    nloop, nmove = units_log(L, L + 1), units_log(1, L + 1)
    return units_log(L, L + 3), units_log(3, L + 3), L * nloop + nmove, units_log(2, M * (M + 1)), nloop, nmove


def file_units(tok):
    """one number of a profile file -> score in units; `*` = probability 0"""
    if tok == "*":
        return STAR
    ip, dot, fr = tok.partition(".")
    if not ip.isdigit() or (dot and not fr.isdigit()) or len(ip) > 4:
        raise HmmError("not a number: %r" % tok)
    if len(fr) > 5:
        raise HmmError("more than 5 decimals: %r" % tok)
    d = int(ip) * 100000 + int((fr + "00000")[:5])
    if d > MAX_FILE_VALUE:
        raise HmmError("value of 100 nats or more: %r" % tok)
    return -((d * UNIT_C + (1 << (UNIT_S - 1))) >> UNIT_S)


def bits_units(tok):
    """a cutoff in bits as the file writes it (sign, at most 5 decimals) -> units, rounded half up"""
    neg = tok.startswith("-")
    ip, dot, fr = tok.lstrip("+-").partition(".")
    if not ip.isdigit() or (dot and fr and not fr.isdigit()) or len(fr) > 5 or len(ip) > 6:
        raise HmmError("not a cutoff: %r" % tok)
    den = 10 ** len(fr)
    d = int(ip) * den + (int(fr) if fr else 0)
    d = -d if neg else d
    return (2 * d * 1024 + den) // (2 * den)


def header_number(tok):
    """a number of a header line (GA / TC / NC, STATS LOCAL): sign, digits, then optionally a point and digits -> float; anything else is malformed"""
    ip, _, fr = (tok[1:] if tok[:1] in ("+", "-") else tok).partition(".")
    if not ip.isdigit() or (fr and not fr.isdigit()):
        raise HmmError("not a number: %r" % tok)
    return float(tok)


def threshold_units(bits):
    """a caller's cutoff in bits (a float) -> units: floor(bits * 1024 + 1/2)"""
    return int(math.floor(float(bits) * 1024.0 + 0.5))


def _fields(ln):
    """a line split at blanks: space, tab and carriage return, nothing else (a vertical tab or a form feed is part of a field)"""
    return [t for t in ln.replace("\t", " ").replace("\r", " ").split(" ") if t]


def parse_hmm(text):
    """HMMER3 ASCII (bytes or str), one or more models -> list of dicts: name, acc, M, ga/tc/nc (pairs of floats or None), ga_units (or None), mu, lam
    (or None), tables = int32 [27][M + 1] (rows 0..19 match scores of residue a at node k, column 0 zero; rows 20..26 the transitions of node k = 0..M)"""
    if isinstance(text, bytes):
        text = text.decode("ascii", "replace")
    lines = text.split("\n")
    pos, models = 0, []

    def nxt():
        nonlocal pos
        while pos < len(lines):
            ln = lines[pos]
            pos += 1
            if _fields(ln):
                return ln
        raise HmmError("truncated file")

    while True:
        while pos < len(lines) and not _fields(lines[pos]):
            pos += 1
        if pos >= len(lines):
            break
        if not nxt().startswith("HMMER3/"):
            raise HmmError("not a HMMER3 profile")
        m = {"name": None, "acc": "", "M": 0, "ga": None, "tc": None, "nc": None, "ga_units": None, "mu": None, "lam": None}
        alph = None
        while True:
            f = _fields(nxt())
            if f[0] == "HMM":
                break
            if f[0] == "NAME" and len(f) > 1:
                m["name"] = f[1]
            elif f[0] == "ACC" and len(f) > 1:
                m["acc"] = f[1]
            elif f[0] == "LENG" and len(f) > 1:
                if not f[1].isdigit():
                    raise HmmError("LENG")
                m["M"] = int(f[1])
            elif f[0] == "ALPH" and len(f) > 1:
                alph = f[1].lower()
            elif f[0] in ("GA", "TC", "NC") and len(f) > 2:
                a, b = f[1].rstrip(";"), f[2].rstrip(";")
                m[f[0].lower()] = (header_number(a), header_number(b))
                if f[0] == "GA":
                    m["ga_units"] = bits_units(a)
            elif f[0] == "STATS" and len(f) > 4 and f[1] == "LOCAL" and f[2] in ("MSV", "VITERBI", "FORWARD"):
                mu, lam = header_number(f[3]), header_number(f[4])
                if f[2] == "VITERBI":
                    m["mu"], m["lam"] = mu, lam
        if m["name"] is None or alph is None or m["M"] < 1:
            raise HmmError("NAME, LENG or ALPH missing")
        if alph != "amino":
            raise HmmError("ALPH %s" % alph)
        if m["M"] > MAX_M:
            raise HmmError("unsupported: M > %d" % MAX_M)
        M = m["M"]
        nxt()                                            # the line that names the transitions
        tab = np.zeros((27, M + 1), np.int32)
        f = _fields(nxt())
        if f[0] == "COMPO":
            f = _fields(nxt())
        if len(f) != 20:
            raise HmmError("insert emissions of node 0")
        [file_units(t) for t in f]
        for k in range(0, M + 1):
            if k > 0:
                f = _fields(nxt())
                if len(f) < 21 or f[0] != str(k):
                    raise HmmError("node %d expected" % k)
                for a in range(20):
                    tab[a, k] = file_units(f[1 + a]) - BG[a]
                f = _fields(nxt())
                if len(f) != 20:
                    raise HmmError("insert emissions of node %d" % k)
                [file_units(t) for t in f]
            f = _fields(nxt())
            if len(f) != 7:
                raise HmmError("transitions of node %d" % k)
            for t in range(7):
                tab[20 + t, k] = file_units(f[t])
        if _fields(nxt()) != ["//"]:
            raise HmmError("no // after node %d" % M)
        m["tables"] = tab
        models.append(m)
    if not models:
        raise HmmError("no model")
    return models


_LUT = np.full(256, 255, np.uint8)
_LUT[np.frombuffer(AA.encode(), np.uint8)] = np.arange(20, dtype=np.uint8)


def encode(rec):
    """residues (bytes of the 20 upper-case letters) -> indices 0..19"""
    x = _LUT[np.frombuffer(bytes(rec), np.uint8)]
    assert (x < 20).all()
    return x


def viterbi(tab, rec):
    """raw score (units) of one record against one profile: the recurrences of SPEC 13, a row at a time, D through its closed form
    D[k] = P[k] + max_{j <= k}(b[j] - P[j]) with P the prefix sums of tDD and b[j] = max(M[i][j-1] + tMD[j-1], NEG) - the floor of every cell is
    the source term NEG of every node, so the closed form is the clamped recurrence exactly"""
    x = encode(rec)
    L, M = len(x), tab.shape[1] - 1
    if L == 0:
        return NO_SCORE
    assert L <= MAX_L
    t = tab.astype(np.int64)
    tloop, tmove, null, tbm, _, _ = specials(L, M)
    Mv = np.full(M + 1, NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()        # index k = 0..M, column 0 stays NEG
    P = np.zeros(M + 1, np.int64)
    P[2:] = np.cumsum(t[ROW_DD, 1:M])                                          # P[k] = tDD[1] + .. + tDD[k-1]
    J = C = NEG
    B = tmove
    for i in range(1, L + 1):
        msc = t[x[i - 1]]
        inn = np.maximum(np.maximum(Mv + t[ROW_MM], Iv + t[ROW_IM]), Dv + t[ROW_DM])      # value handed from node k to node k + 1
        Mn = np.full(M + 1, NEG, np.int64)
        Mn[1:] = np.maximum(msc[1:] + np.maximum(inn[:-1], B + tbm), NEG)
        In = np.maximum(np.maximum(Mv + t[ROW_MI], Iv + t[ROW_II]), NEG)
        In[0] = NEG; In[M] = NEG
        Dn = np.full(M + 1, NEG, np.int64)
        if M >= 2:
            b = np.maximum(Mn[1:M] + t[ROW_MD, 1:M], NEG)                       # b of node k = 2..M
            Dn[2:] = P[2:] + np.maximum.accumulate(b - P[2:])
        E = int(max(Mn[1:].max(), Dn[1:].max()))
        J = max(J + tloop, E + T_EJ, NEG)
        C = max(C + tloop, E + T_EC, NEG)
        B = max(i * tloop, J) + tmove
        Mv, Iv, Dv = Mn, In, Dn
    raw = C + tmove - null
    assert -(1 << 31) < raw < (1 << 31)
    return int(raw)


def viterbi_naive(tab, rec):
    """the same score by the recurrences as written, cell by cell (the yardstick of viterbi(); small shapes only)"""
    x = encode(rec)
    L, M = len(x), tab.shape[1] - 1
    if L == 0:
        return NO_SCORE
    t = [[int(v) for v in row] for row in tab]
    tloop, tmove, null, tbm, _, _ = specials(L, M)
    Mm = [[NEG] * (M + 1) for _ in range(L + 1)]
    Im = [[NEG] * (M + 1) for _ in range(L + 1)]
    Dm = [[NEG] * (M + 1) for _ in range(L + 1)]
    B = [tmove] + [0] * L
    J = [NEG] * (L + 1)
    C = [NEG] * (L + 1)
    for i in range(1, L + 1):
        E = NEG
        for k in range(1, M + 1):
            best = B[i - 1] + tbm
            for prev, row in ((Mm, ROW_MM), (Im, ROW_IM), (Dm, ROW_DM)):
                best = max(best, prev[i - 1][k - 1] + t[row][k - 1])
            Mm[i][k] = max(t[x[i - 1]][k] + best, NEG)
            if k < M:
                Im[i][k] = max(Mm[i - 1][k] + t[ROW_MI][k], Im[i - 1][k] + t[ROW_II][k], NEG)
            if k >= 2:
                Dm[i][k] = max(Mm[i][k - 1] + t[ROW_MD][k - 1], Dm[i][k - 1] + t[ROW_DD][k - 1], NEG)
            E = max(E, Mm[i][k], Dm[i][k])
        J[i] = max(J[i - 1] + tloop, E + T_EJ, NEG)
        C[i] = max(C[i - 1] + tloop, E + T_EC, NEG)
        B[i] = max(i * tloop, J[i]) + tmove
    return C[L] + tmove - null


def viterbi_batch(tab, records):
    """viterbi() of many records against one profile at once: the same row step on [n_rec, M + 1] arrays, every record with its own length model;
    a record takes no more steps once its last row is done -> int32 [n_rec]"""
    n, M = len(records), tab.shape[1] - 1
    Ls = np.array([len(r) for r in records], np.int64)
    out = np.full(n, NO_SCORE, np.int64)
    live = np.flatnonzero(Ls > 0)
    if len(live) == 0:
        return out.astype(np.int32)
    assert Ls.max() <= MAX_L
    Lv = Ls[live]
    x = np.zeros((len(live), int(Lv.max())), np.int64)
    for j, r in enumerate(live):
        x[j, :Lv[j]] = encode(records[r])
    sp = np.array([specials(int(L), M) for L in Lv], np.int64)
    tloop, tmove, null, tbm = sp[:, 0], sp[:, 1], sp[:, 2], int(sp[0, 3])
    t = tab.astype(np.int64)
    msc_of = t[:20].copy()                                                      # [20, M + 1]
    Mv = np.full((len(live), M + 1), NEG, np.int64); Iv = Mv.copy(); Dv = Mv.copy()
    P = np.zeros(M + 1, np.int64)
    P[2:] = np.cumsum(t[ROW_DD, 1:M])
    J = np.full(len(live), NEG, np.int64); C = J.copy(); B = tmove.copy()
    for i in range(1, int(Lv.max()) + 1):
        on = Lv >= i
        msc = msc_of[x[:, i - 1]]
        inn = np.maximum(np.maximum(Mv + t[ROW_MM], Iv + t[ROW_IM]), Dv + t[ROW_DM])
        Mn = np.full_like(Mv, NEG)
        Mn[:, 1:] = np.maximum(msc[:, 1:] + np.maximum(inn[:, :-1], (B + tbm)[:, None]), NEG)
        In = np.maximum(np.maximum(Mv + t[ROW_MI], Iv + t[ROW_II]), NEG)
        In[:, 0] = NEG; In[:, M] = NEG
        Dn = np.full_like(Mv, NEG)
        if M >= 2:
            b = np.maximum(Mn[:, 1:M] + t[ROW_MD, 1:M], NEG)
            Dn[:, 2:] = P[2:] + np.maximum.accumulate(b - P[2:], axis=1)
        E = np.maximum(Mn[:, 1:].max(axis=1), Dn[:, 1:].max(axis=1))
        Jn = np.maximum(np.maximum(J + tloop, E + T_EJ), NEG)
        Cn = np.maximum(np.maximum(C + tloop, E + T_EC), NEG)
        Bn = np.maximum(i * tloop, Jn) + tmove
        J, C, B = np.where(on, Jn, J), np.where(on, Cn, C), np.where(on, Bn, B)
        Mv, Iv, Dv = Mn, In, Dn
    raw = C + tmove - null
    assert (np.abs(raw) < (1 << 31)).all()
    out[live] = raw
    return out.astype(np.int32)


def search(models, records):
    """int32 [n_rec, n_prof]"""
    out = np.zeros((len(records), len(models)), np.int32)
    for p, m in enumerate(models):
        out[:, p] = viterbi_batch(m["tables"], records)
    return out


def best_hits(scores, genome_rec_off, thr):
    """per genome and profile: (record, raw) of the largest raw >= thr[p], ties to the lowest record; no hit: (NO_HIT, NO_SCORE)"""
    scores = np.asarray(scores, np.int64)
    ng, npf = len(genome_rec_off) - 1, scores.shape[1]
    rec = np.full((ng, npf), NO_HIT, np.uint32)
    sc = np.full((ng, npf), NO_SCORE, np.int32)
    for g in range(ng):
        for p in range(npf):
            for r in range(int(genome_rec_off[g]), int(genome_rec_off[g + 1])):
                s = int(scores[r, p])
                if s != NO_SCORE and s >= int(thr[p]) and s > int(sc[g, p]):
                    rec[g, p], sc[g, p] = r, s
    return rec, sc


def consensus(tab):
    """the most probable residue of every node's match emission (score + background; ties: the first in alphabet order)"""
    return bytes(ord(AA[int(a)]) for a in np.argmax(tab[:20, 1:].astype(np.int64) + np.array(BG, np.int64)[:, None], axis=0))


def bits(raw):
    return raw / 1024.0


def pvalue(b, mu, lam):
    return -math.expm1(-math.exp(-lam * (b - mu)))


def table_bytes(models, ids, scores):
    """the text gsearch_amd.hmmsearch() writes: a row per (record, profile) with raw >= 0, sorted by (profile, -raw, record)"""
    Z = len(ids)
    rows = []
    for p, m in enumerate(models):
        for r in range(Z):
            s = int(scores[r, p])
            if s != NO_SCORE and s >= 0:
                rows.append((p, -s, r))
    out = [b"target\tprofile\tacc\tbits\tevalue\tpass_ga\n"]
    for p, ns, r in sorted(rows):
        m = models[p]
        b = bits(-ns)
        ev = "%.3E" % (Z * pvalue(b, m["mu"], m["lam"])) if m["mu"] is not None else "-"
        ga = "-" if m["ga_units"] is None else ("1" if -ns >= m["ga_units"] else "0")
        out.append(("%s\t%s\t%s\t%.2f\t%s\t%s\n" % (ids[r], m["name"], m["acc"] or "-", b, ev, ga)).encode())
    return b"".join(out)


# ---- synthetic models -------------------------------------------------------------------------------------------------------------------
def _nats(p):
    return "%.5f" % abs(math.log(min(p, 1.0))) if p > 0 else "*"


def synth_model(rng, M, name=None, conserved=0.6, ga=25.0):
    """a random model as probabilities: every node prefers one residue; transitions favour match -> match"""
    mat = np.zeros((M + 1, 20))
    for k in range(1, M + 1):
        p = rng.dirichlet(np.full(20, 0.5)) * (1 - conserved)
        p[rng.integers(20)] += conserved
        mat[k] = p / p.sum()
    ins = np.tile(np.exp(-np.array([2.68618, 4.42225, 2.77519, 2.73123, 3.46354, 2.40513, 3.72494, 3.29354, 2.67741, 2.69355, 4.24690, 2.90347, 2.73739,
                                    3.18146, 2.89801, 2.37887, 2.77519, 2.98518, 4.58477, 3.61503])), (M + 1, 1))
    tr = np.zeros((M + 1, 7))
    for k in range(M + 1):
        mi, md = rng.uniform(0.005, 0.05, 2)
        ii, dd = rng.uniform(0.3, 0.6, 2)
        tr[k] = [1 - mi - md, mi, md, 1 - ii, ii, 1 - dd, dd]
    tr[0, 5:] = [1.0, 0.0]
    tr[M, 0], tr[M, 2], tr[M, 5], tr[M, 6] = 1 - tr[M, 1], 0.0, 1.0, 0.0
    return {"name": name or "SYN%d" % M, "acc": "SYN%05d.1" % M, "M": M, "mat": mat, "ins": ins, "tr": tr, "ga": ga, "mu": -8.5 - math.log(M) / 2, "lam": 0.7}


def write_hmm(s, dialect="f", compo=True):
    """the text of a synthetic model in either dialect of the reference's sets (3/f: trailer MAP CONS RF MM CS; 3/b: MAP RF CS, `;` after cutoffs)"""
    M = s["M"]
    semi = ";" if dialect == "b" else ""
    out = ["HMMER3/f [3.3 | Nov 2019]" if dialect == "f" else "HMMER3/b [3.0 | March 2010]", "NAME  %s" % s["name"]]
    if s.get("acc"):
        out.append("ACC   %s" % s["acc"])
    out += ["DESC  synthetic", "LENG  %d" % M, "ALPH  %s" % s.get("alph", "amino"), "RF    no"]
    if dialect == "f":
        out += ["MM    no", "CONS  yes"]
    out += ["CS    no", "MAP   yes", "NSEQ  10", "EFFN  1.000000", "CKSUM 1"]
    if s.get("ga") is not None:
        out += ["GA    %.2f %.2f%s" % (s["ga"], s["ga"], semi), "TC    %.2f %.2f%s" % (s["ga"] + 0.5, s["ga"], semi), "NC    %.2f %.2f%s" % (s["ga"] - 0.5, s["ga"], semi)]
    out += ["STATS LOCAL MSV      %9.4f  %.5f" % (s["mu"] + 0.5, s["lam"]), "STATS LOCAL VITERBI  %9.4f  %.5f" % (s["mu"], s["lam"]),
            "STATS LOCAL FORWARD  %9.4f  %.5f" % (s["mu"] + 4, s["lam"])]
    out.append("HMM     " + "".join("     %s   " % c for c in AA))
    out.append("            m->m     m->i     m->d     i->m     i->i     d->m     d->d")
    row = lambda v: "".join("  %7s" % _nats(p) for p in v)
    if compo:
        out.append("  COMPO " + row(s["mat"][1:].mean(axis=0)))
    for k in range(M + 1):
        if k:
            cons = AA[int(np.argmax(s["mat"][k]))].lower()
            out.append("%7d " % k + row(s["mat"][k]) + ("%7d %s - - -" % (k, cons) if dialect == "f" else "%7d - -" % k))
        out.append("        " + row(s["ins"][k]))
        out.append("        " + row(s["tr"][k]))
    out.append("//")
    return ("\n".join(out) + "\n").encode()


def background(rng, n):
    """n iid residues of the SPEC's background composition"""
    f = np.array([.0787945, .0151600, .0535222, .0668298, .0397062, .0695071, .0229198, .0590092, .0594422, .0963728, .0237718, .0414386, .0482904,
                  .0395639, .0540978, .0683364, .0540687, .0673417, .0114135, .0304133])
    return bytes(ord(AA[i]) for i in rng.choice(20, size=n, p=f / f.sum()))
