"""Hand-built .gsbx files (SPEC.md 16.2), in the style of deflate_cases.py: every case has a name that promises a property and a check of that promise on the
restatement (pyref_bigsi_file). VALID: name -> (model, promise(model)); REFUSED: name -> (bytes, code, promise()); sweep_files(): every proper prefix and
every byte replaced by 0xFF and by itself ^ 1, of a small valid version-2 file, each with the restatement's verdict."""
import struct

import numpy as np

import pyref_bigsi_file as R

OK, INVALID, UNSUPPORTED, IO = R.OK, R.INVALID, R.UNSUPPORTED, R.IO


def generated(seed, n, bloom_size, version=1, k=31, num_hash=3, data_t=R.DATA_DNA, m=0, accessions=True):
    """random bits in the n colours of every row (the bits beyond n stay 0), t_c = the bits of the column, nk_c = something larger"""
    rng = np.random.default_rng(seed)
    W = R.words(n)
    bits = rng.integers(0, 2, (bloom_size, W * 64), dtype=np.uint8)
    bits[:, n:] = 0
    rows = np.packbits(bits.reshape(bloom_size, W, 64), axis=2, bitorder="little").reshape(bloom_size, W * 8).copy().view(np.uint64) if W else np.zeros((bloom_size, 0), np.uint64)
    t = bits[:, :n].sum(axis=0).astype(np.uint64)
    names = [b"ACC_%03d.%d" % (i, i % 3) if accessions else b"" for i in range(n)]
    return R.make_model(version, k, num_hash, data_t, m, bloom_size, names, t, t * np.uint64(7) + np.uint64(1), rows)


def _valid():
    V = {}
    for n in (0, 1, 64, 65, 130):
        V["colours_%d" % n] = (generated(40 + n, n, 37), lambda mo, n=n: len(mo["names"]) == n and mo["rows"].shape == (37, (n + 63) // 64))
    V["without_accessions"] = (generated(50, 5, 20, accessions=False), lambda mo: not any(mo["names"]) and len(mo["names"]) == 5)
    V["with_accessions"] = (generated(51, 5, 20), lambda mo: all(mo["names"]))
    V["version_2_m_1"] = (generated(52, 3, 16, version=2, k=21, m=1), lambda mo: mo["version"] == 2 and mo["m"] == 1)
    V["version_2_m_k_minus_1"] = (generated(53, 3, 16, version=2, k=21, m=20), lambda mo: mo["version"] == 2 and mo["m"] == mo["k"] - 1)
    V["bloom_size_1"] = (generated(54, 70, 1), lambda mo: mo["bloom_size"] == 1 and mo["rows"].shape == (1, 2))
    V["bloom_size_a_few_hundred_forward_kmers"] = (generated(55, 9, 300, data_t=R.DATA_DNA_FWD, k=1, num_hash=16), lambda mo: mo["bloom_size"] == 300 and mo["data_t"] == 2)
    return V


VALID = _valid()


def base():
    """version 2, two colours with accessions, three rows"""
    return generated(60, 2, 3, version=2, k=21, m=11)


def _patch(b, off, fmt, *v):
    raw = struct.pack("<" + fmt, *v)
    return b[:off] + raw + b[off + len(raw):]


def _refused():
    Rf = {}
    bm = base()
    b0, off = R.write(bm, layout=True)
    assert R.verify(b0)[0] == OK

    def field(name, code, where, fmt, *v):
        o, size = off[where], struct.calcsize("<" + fmt)
        b = _patch(b0, o, fmt, *v)
        Rf[name] = (b, code, lambda: len(b) == len(b0) and b != b0 and b[:o] == b0[:o] and b[o + size:] == b0[o + size:])

    field("magic_wrong", IO, "magic", "8s", b"GSBIGSI2")
    field("version_3", IO, "version", "I", 3)
    field("version_2_m_0", IO, "m", "I", 0)
    field("version_2_m_equal_k", IO, "m", "I", bm["k"])
    field("n_2p32", IO, "n", "Q", 1 << 32)
    field("accession_length_2p20_plus_1", IO, "len0", "I", (1 << 20) + 1)
    for sec, cut in (("header", off["bloom_size"] + 3), ("accessions", off["name1"] + 2), ("t_c", off["t"] + 9), ("nk_c", off["q"] + 1), ("rows", off["rows"] + 8)):
        Rf["cut_inside_" + sec] = (b0[:cut], IO, lambda cut=cut: 0 < cut < len(b0))
    Rf["one_row_short"] = (b0[:-8], IO, lambda: R.words(2) == 1 and len(b0) - 8 >= off["rows"])
    Rf["one_byte_long"] = (b0 + b"\0", IO, lambda: True)
    hostile = R.header(dict(version=1, k=31, num_hash=3, data_t=0, m=0, bloom_size=1 << 40), n=1)
    hostile += bytes(100 - len(hostile))
    Rf["bloom_size_2p40_in_100_bytes"] = (hostile, IO, lambda: len(hostile) == 100 and R.describe(hostile)[1]["bloom_size"] == 1 << 40)
    # with no colour the rows are empty and the file is whole: only the parameter check is left to refuse it
    for name, B in (("bloom_size_2p40_no_colours", 1 << 40), ("bloom_size_0_no_colours", 0)):
        b = R.header(dict(version=1, k=31, num_hash=3, data_t=0, m=0, bloom_size=B), n=0)
        Rf[name] = (b, INVALID, lambda b=b: len(b) == 40)
    field("version_2_k_0_is_not_above_m", IO, "k", "I", 0)          # version 2 asks m < k first (step 3)
    field("k_33", INVALID, "k", "I", 33)
    field("num_hash_0", INVALID, "num_hash", "I", 0)
    field("num_hash_17", INVALID, "num_hash", "I", 17)
    field("data_t_amino_acids", INVALID, "data_t", "I", 1)
    v1 = R.write(generated(61, 2, 3))
    Rf["version_1_k_0"] = (_patch(v1, 12, "I", 0), INVALID, lambda: R.verify(v1)[0] == OK)
    return Rf


REFUSED = _refused()
_SWEEP = None


def sweep_files():
    """[(tag, bytes, code, model or None)] over base()"""
    global _SWEEP
    if _SWEEP is None:
        b0 = R.write(base())
        muts = [("p%d" % i, b0[:i]) for i in range(len(b0))]
        muts += [("f%d" % i, b0[:i] + b"\xff" + b0[i + 1:]) for i in range(len(b0)) if b0[i] != 0xFF]
        muts += [("x%d" % i, b0[:i] + bytes([b0[i] ^ 1]) + b0[i + 1:]) for i in range(len(b0))]
        _SWEEP = [(tag, b) + R.verify(b) for tag, b in muts]
    return _SWEEP
