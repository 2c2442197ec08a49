"""Independent numpy restatement of SPEC 9 (superaai: FracMinHash sketches, similarity, AAI, output). Written from SPEC.md alone; it
imports nothing from gsearch_amd. The sourmash restatement at the end (add_hash / merge / intersection_size) is used only by a test that
checks SPEC 9's order-independence argument."""
import math

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
C1, C2 = np.uint64(0x87c37b91114253d5), np.uint64(0x4cf5ad432745937f)
SEED = 42


def _rotl(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _fmix(k):
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> np.uint64(33))


def murmur3_x64_128(keys, seed):
    """MurmurHash3_x64_128 of each row of `keys` (an (n, L) uint8 array, every row L bytes) -> (h1, h2) uint64 arrays"""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    n, L = keys.shape
    with np.errstate(over="ignore"):
        h1 = np.full(n, seed, dtype=np.uint64)
        h2 = np.full(n, seed, dtype=np.uint64)
        pad = np.zeros((n, (L + 15) // 16 * 16 + 16), dtype=np.uint8)
        pad[:, :L] = keys
        words = pad.view("<u8")
        nb = L // 16
        for i in range(nb):
            k1, k2 = words[:, 2 * i].copy(), words[:, 2 * i + 1].copy()
            k1 = _rotl(k1 * C1, 31) * C2
            h1 ^= k1
            h1 = _rotl(h1, 27) + h2
            h1 = h1 * np.uint64(5) + np.uint64(0x52dce729)
            k2 = _rotl(k2 * C2, 33) * C1
            h2 ^= k2
            h2 = _rotl(h2, 31) + h1
            h2 = h2 * np.uint64(5) + np.uint64(0x38495ab5)
        rem = L & 15
        t1, t2 = words[:, 2 * nb].copy(), words[:, 2 * nb + 1].copy()
        if rem > 8:
            h2 ^= _rotl(t2 * C2, 33) * C1
        if rem > 0:
            h1 ^= _rotl(t1 * C1, 31) * C2
        h1 ^= np.uint64(L)
        h2 ^= np.uint64(L)
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = _fmix(h1), _fmix(h2)
        h1 = h1 + h2
        h2 = h2 + h1
    return h1, h2


def smhasher_verification():
    """SMHasher's VerificationTest for MurmurHash3_x64_128: keys {}, {0}, {0,1}, ... (length i, seed 256 - i), the 256 x 16 output bytes
    hashed with seed 0, the first 4 bytes little-endian"""
    out = bytearray()
    for i in range(256):
        key = np.arange(i, dtype=np.uint8).reshape(1, i)
        h1, h2 = murmur3_x64_128(key, 256 - i)
        out += int(h1[0]).to_bytes(8, "little") + int(h2[0]).to_bytes(8, "little")
    h1, _ = murmur3_x64_128(np.frombuffer(bytes(out), np.uint8).reshape(1, -1), 0)
    return int(h1[0]) & 0xFFFFFFFF


def max_hash(scaled):
    if scaled == 0:
        return 0
    if scaled == 1:
        return 2 ** 64 - 1
    return int(float(2 ** 64 - 1) / float(scaled))


def clean(record):
    """a record's sequence: its bytes with '\n' and '\r' removed, nothing else changed"""
    return bytes(record).replace(b"\n", b"").replace(b"\r", b"")


def window_hashes(seq, k):
    a = np.frombuffer(seq, dtype=np.uint8)
    if len(a) < k:
        return np.zeros(0, np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(a, k)
    return murmur3_x64_128(win, SEED)[0]


def sketch(records, k, scaled, num):
    """SPEC 9: the num smallest distinct window hashes <= max_hash (all when num == 0), ascending"""
    mh = max_hash(scaled)
    if num == 0 and mh == 0:
        return np.zeros(0, np.uint64)
    parts = [window_hashes(clean(r), k) for r in records]
    h = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)
    if mh:
        h = h[h <= np.uint64(mh)]
    return h[:num] if num else h


def similarity_counts(A, B, num):
    """(common, |U|): U = the num smallest of A u B (all when num == 0), common = |A n B n U|"""
    U = np.union1d(A, B)
    if num:
        U = U[:num]
    common = len(np.intersect1d(np.intersect1d(A, B), U))
    return common, len(U)


def similarity(A, B, num):
    c, u = similarity_counts(A, B, num)
    return float(c) / float(max(1, u))


def aai(s, k):
    return 1.0 + math.log((2.0 * s) / (1.0 + s)) / float(k) if s > 0 else float("-inf")


def display(x):
    """Rust's `{}` for f64: shortest round-trip digits, positional, no exponent, no trailing '.0'"""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    r = repr(float(x))
    neg = r.startswith("-")
    r = r.lstrip("-")
    mant, _, exp = r.partition("e")
    ip, _, fp = mant.partition(".")
    digits, point = ip + fp, len(ip) + (int(exp) if exp else 0)
    if point <= 0:
        s = "0." + "0" * (-point) + digits
    elif point >= len(digits):
        s = digits + "0" * (point - len(digits))
    else:
        s = digits[:point] + "." + digits[point:]
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    s = s.lstrip("0") or "0"
    if s.startswith("."):
        s = "0" + s
    return ("-" if neg else "") + s


def read_list(data):
    """BufRead::lines().filter_map(Result::ok) over the bytes of a list file"""
    out, i = [], 0
    while i < len(data):
        j = data.find(b"\n", i)
        if j < 0:
            line, i = data[i:], len(data)
        else:
            line, i = data[i:j], j + 1
            if line.endswith(b"\r"):
                line = line[:-1]
        try:
            out.append(line.decode("utf-8"))
        except UnicodeDecodeError:
            pass
    return out


def output_text(qpaths, rpaths, sim, k):
    lines = []
    for i, q in enumerate(qpaths):
        for j, r in enumerate(rpaths):
            s = float(sim[i][j])
            lines.append("%s\t%s\t%s\t%s" % (q, r, display(s), display(aai(s, k))))
    return "\n".join(lines)


# ---- sourmash KmerMinHash, restated from memory (used only to test SPEC 9's order-independence argument) ----
class SourmashMinHash:
    def __init__(self, num, scaled):
        self.num, self.max_hash, self.mins = num, max_hash(scaled), []

    def add_hash(self, h):
        import bisect
        current_max = self.mins[-1] if self.mins else 2 ** 64 - 1
        if h > self.max_hash and self.max_hash != 0:
            return
        if self.num == 0 and self.max_hash == 0:
            return
        if h <= self.max_hash or h <= current_max or len(self.mins) < self.num:
            pos = bisect.bisect_left(self.mins, h)
            if pos < len(self.mins) and self.mins[pos] == h:
                return
            if pos == len(self.mins):
                self.mins.append(h)                  # at the end: pushed without truncation
            else:
                self.mins.insert(pos, h)
                if self.num != 0 and len(self.mins) > self.num:
                    self.mins.pop()

    def merged(self, other):
        m = sorted(set(self.mins) | set(other.mins))
        return m[:self.num] if self.num else m

    def intersection_size(self, other):
        combined = self.merged(other)
        i1 = set(self.mins) & set(other.mins)
        return len(i1 & set(combined)), len(combined)

    def jaccard(self, other):
        c, u = self.intersection_size(other)
        return float(c) / float(max(1, u))
