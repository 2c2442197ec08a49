"""A restatement of the .gsbx file (versions 1 and 2), written from the layout comment above gs_bigsi_save (gsearch_amd/csrc/gs_bigsi.hip) and from
SPEC.md 16.2 / 16.3 - none of it goes through the library.

A model is a dict: version (1 plain, 2 minimizer index), k, num_hash, data_t, m (0 in version 1), bloom_size, names (accession bytes per colour),
t, q (t_c and nk_c per colour, u64), rows ((bloom_size, ceil(n / 64)) u64). write(model) -> bytes; verify(bytes) -> (code, model or None), check by
check in the order of SPEC 16.2; describe(bytes) -> (code, header fields)."""
import struct

import numpy as np

OK, INVALID, UNSUPPORTED, IO = 0, -1, -3, -5
MAGIC = b"GSBIGSI1"
KMAX, HMAX, BMAX = 32, 16, 1 << 40
DATA_DNA, DATA_DNA_FWD = 0, 2


def words(n):
    return (n + 63) // 64


def make_model(version, k, num_hash, data_t, m, bloom_size, names, t, q, rows):
    n = len(names)
    return dict(version=version, k=k, num_hash=num_hash, data_t=data_t, m=m, bloom_size=bloom_size, names=[bytes(x) for x in names],
                t=np.ascontiguousarray(t, np.uint64).reshape(n), q=np.ascontiguousarray(q, np.uint64).reshape(n),
                rows=np.ascontiguousarray(rows, np.uint64).reshape(bloom_size, words(n)))


def same_model(a, b):
    return (all(a[k] == b[k] for k in ("version", "k", "num_hash", "data_t", "m", "bloom_size", "names"))
            and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in ("t", "q", "rows")))


def header(mo, n=None):
    n = len(mo["names"]) if n is None else n
    h = MAGIC + struct.pack("<IIII", mo["version"], mo["k"], mo["num_hash"], mo["data_t"])
    if mo["version"] == 2:
        h += struct.pack("<I", mo["m"])
    return h + struct.pack("<QQ", mo["bloom_size"], n)


def write(mo, layout=False):
    off = dict(magic=0, version=8, k=12, num_hash=16, data_t=20)
    at = 24
    if mo["version"] == 2:
        off["m"] = at
        at += 4
    off["bloom_size"], off["n"], off["header_end"] = at, at + 8, at + 16
    b = bytearray(header(mo))
    for i, nm in enumerate(mo["names"]):
        off["len%d" % i], off["name%d" % i] = len(b), len(b) + 4
        b += struct.pack("<I", len(nm)) + nm
    off["t"] = len(b)
    b += mo["t"].tobytes()
    off["q"] = len(b)
    b += mo["q"].tobytes()
    off["rows"] = len(b)
    b += mo["rows"].tobytes()
    return (bytes(b), off) if layout else bytes(b)


def _header(b):
    """SPEC 16.2 step 2 -> (code, fields, offset behind the header)"""
    if len(b) < 24 or b[:8] != MAGIC:
        return IO, None, 0
    version, k, num_hash, data_t = struct.unpack_from("<IIII", b, 8)
    if version not in (1, 2):
        return IO, None, 0
    at, m = 24, 0
    if version == 2:
        if len(b) < 28:
            return IO, None, 0
        m, = struct.unpack_from("<I", b, 24)
        at = 28
    if len(b) < at + 16:
        return IO, None, 0
    B, n = struct.unpack_from("<QQ", b, at)
    return OK, dict(version=version, k=k, num_hash=num_hash, data_t=data_t, minimizer_len=m, bloom_size=B, n_colours=n, row_words=words(n)), at + 16


def describe(b):
    code, d, _ = _header(b)
    return code, d


def verify(b):
    code, h, at = _header(b)
    if code:
        return code, None
    n, B, W = h["n_colours"], h["bloom_size"], h["row_words"]
    # step 3
    if (h["version"] == 2 and not 1 <= h["minimizer_len"] < h["k"]) or n >= 1 << 32:
        return IO, None
    # step 4
    if len(b) < at + 20 * n + B * W * 8:
        return IO, None
    # step 5
    names = []
    for _ in range(n):
        if at + 4 > len(b):
            return IO, None
        ln, = struct.unpack_from("<I", b, at)
        if ln > 1 << 20 or at + 4 + ln > len(b):
            return IO, None
        names.append(b[at + 4:at + 4 + ln])
        at += 4 + ln
    # step 6
    if len(b) != at + 16 * n + B * W * 8:
        return IO, None
    # step 7
    if not 1 <= h["k"] <= KMAX or not 1 <= h["num_hash"] <= HMAX or not 1 <= B < BMAX or h["data_t"] not in (DATA_DNA, DATA_DNA_FWD):
        return INVALID, None
    t, q = np.frombuffer(b, np.uint64, n, at), np.frombuffer(b, np.uint64, n, at + 8 * n)
    rows = np.frombuffer(b, np.uint64, B * W, at + 16 * n)
    return OK, make_model(h["version"], h["k"], h["num_hash"], h["data_t"], h["minimizer_len"], B, names, t, q, rows)


def fnv1a(data, h=0xCBF29CE484222325):
    for x in data:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def digest(b):
    """SPEC 16.3: every byte behind the fixed header"""
    _, _, at = _header(b)
    return fnv1a(b[at:])
