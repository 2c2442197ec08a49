"""Independent numpy reference of SPEC.md section 7 (HyperMinHash of hypermash): registers, cardinality, similarity and distance.
Written from SPEC alone; imports nothing from gsearch_amd. Used by the hypermash tests and tools/hmh_rate.py."""
import numpy as np

P, Q, R = 14, 6, 10
M = 1 << P
SMALL = float(1 << (P + 5))
GAMMA = np.uint64(0x9E3779B97F4A7C15)
M64 = (1 << 64) - 1
_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def canonical_kmers(record, k):
    """SPEC 1.1: non-ACGT bytes dropped, case folded; min(fwd, rc) & mask of every window -> uint64 array"""
    c = _CODE[np.frombuffer(bytes(record), np.uint8)]
    c = c[c != 255].astype(np.uint64)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    fwd = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    two = np.uint64(2)
    for t in range(k):
        fwd = (fwd << two) | c[t:t + n]
        rc = (rc << two) | (np.uint64(3) - c[k - 1 - t:k - 1 - t + n])
    mask = np.uint64(M64 if k == 32 else (1 << (2 * k)) - 1)
    return np.minimum(fwd, rc) & mask


def register_updates(v):
    """SPEC 7 register update of each value: (index, register) uint64 arrays"""
    v = np.asarray(v, np.uint64)
    x = v * np.uint64(0x517CC1B727220A95)
    h1 = _mix(x + GAMMA)
    h2 = _mix(x + GAMMA + GAMMA)
    idx = h1 >> np.uint64(64 - P)
    low = (h1 & np.uint64((1 << 50) - 1)).astype(np.float64)                # < 2^50: exact
    bitlen = np.frexp(low)[1].astype(np.int64)                               # 0 for 0
    lz = (51 - bitlen).astype(np.uint64)
    reg = (lz << np.uint64(R)) | (h2 & np.uint64((1 << R) - 1))
    return idx, reg


def sketch(records, k):
    """one genome (list of ASCII records) -> 16384 uint16 registers"""
    regs = np.zeros(M, np.uint64)
    for rec in records:
        v = canonical_kmers(rec, k)
        if len(v):
            idx, reg = register_updates(v)
            np.maximum.at(regs, idx.astype(np.int64), reg)
    return regs.astype(np.uint16)


def register_update_scalar(v):
    """the same rule with Python integers (a second, scalar path for the known-answer tests)"""
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    x = (v * 0x517CC1B727220A95) & M64
    h1, h2 = mix((x + 0x9E3779B97F4A7C15) & M64), mix((x + 2 * 0x9E3779B97F4A7C15) & M64)
    y = ((h1 << 14) & M64) ^ 0x3FFF
    lz = 64 - y.bit_length() + 1
    return h1 >> 50, (lz << 10) | (h2 & 0x3FF)


def spec_ln(x):
    """SPEC 2 LN, the same f64 operation sequence"""
    x = float(x)
    m, e = np.frexp(x)                      # x = m 2^e, m in [0.5, 1)
    t, e = float(m) * 2.0, int(e) - 1
    if t > 1.4142135623730951:
        t = t * 0.5
        e += 1
    s = (t - 1.0) / (t + 1.0)
    z = s * s
    p = 1.0 / 23.0
    for d in (21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    return float(e) * 0.6931471805599453 + 2.0 * s * p


def cardinality(regs):
    regs = np.asarray(regs, np.uint16)
    lz = (regs >> 10).astype(np.int64)
    ez = int((lz == 0).sum())
    units = sum(int(c) << (51 - int(l)) for l, c in zip(*np.unique(lz, return_counts=True)))
    s = float(units) * 2.0 ** -51
    ezf = float(ez)
    zl = spec_ln(ezf + 1.0)
    z = [zl]
    for _ in range(6):
        z.append(z[-1] * zl)
    beta = -0.370393911 * ezf
    beta = beta + 0.070471823 * z[0]
    beta = beta + 0.17393686 * z[1]
    beta = beta + 0.16339839 * z[2]
    beta = beta - 0.09237745 * z[3]
    beta = beta + 0.03738027 * z[4]
    beta = beta - 0.005384159 * z[5]
    beta = beta + 0.00042419 * z[6]
    m = float(M)
    alpha = 0.7213 / (1.0 + 1.079 / m)
    return int(((alpha * m) * (m - ezf)) / (beta + s))


_B1 = _B2 = None


def _bs():
    global _B1, _B2
    if _B1 is None:
        i = np.repeat(np.arange(1, 65), 1024).astype(np.float64)
        j = np.tile(np.arange(1, 1025), 64).astype(np.float64)
        den = 2.0 ** (P + R + i)
        b1, b2 = (1024 + j) / den, (1025 + j) / den
        last = i == 64
        b1[last], b2[last] = j[last] / 2.0 ** 87, (j[last] + 1) / 2.0 ** 87
        _B1, _B2 = b1, b2
    return _B1, _B2


def pvec(card):
    b1, b2 = _bs()
    c = float(card)
    return np.power(1.0 - b2, c) - np.power(1.0 - b1, c)


def counts(a, b):
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    C = int(((a == b) & (a != 0)).sum())
    N = int(((a != 0) | (b != 0)).sum())
    return C, N


def similarity(a, b, ca=None, cb=None):
    C, N = counts(a, b)
    ca = cardinality(a) if ca is None else ca
    cb = cardinality(b) if cb is None else cb
    if C == 0 or ca == 0 or cb == 0:
        return 0.0
    n, mn = float(max(ca, cb)), float(min(ca, cb))
    if n > SMALL:
        t = (1.0 + n) / mn
        d = (4.0 * n / mn) / (t * t)
        ec = 0.169919487159739093975315012348 * 16.0 * d + 0.5
    else:
        ec = float(np.dot(pvec(n), pvec(mn))) + 0.5 / P
    return 0.0 if C < ec else (C - ec) / N


def distance(sim, k):
    return 1.0 - (2.0 * sim / (1.0 + sim)) ** (1.0 / k)
