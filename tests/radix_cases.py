"""Inputs of the tests of gs_radix.hip's three primitives: the stable radix sort of 64-bit keys, the run lengths of a sorted array, the one-workgroup
prefix sum. Every case is built from a fixed seed and most promise a property in their `props` (the edge of the kernel they are there for);
test_radix_cases_cpu.py checks each property without a device, so the GPU test that runs the same tables (test_gpu_radix.py) cannot pass on inputs
that miss their edge. The constants restate the geometry of the kernels: a wavefront owns a tile of TILE consecutive keys and walks it STEP keys at a
time; a pass sorts on one 8-bit digit; the scan gives each of its SCAN_LANES lanes a stretch of whole groups of four."""
import zlib

import numpy as np

import pyref_radix as R

TILE = 16384
STEP = 64
SCAN_LANES = 1024
U64 = np.uint64
ENDBITS = (8, 24, 32, 40, 64)                       # 1, 3, 4, 5 and 8 passes: the result ends in the second buffer after the odd ones
ODD_ENDBITS = (13, 33, 42, 62)                      # no multiple of 8: the consumers that sort on such a width keep the bits above it zero
SORT_SIZES = (0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE + 17)
STABLE_SIZES = (TILE + 1, 3 * TILE + 17)
STABLE_VALUES = {32: (0, 1, 0xFF, 0x100, 0x80000000, 0xDEADBEEF, 0xFFFFFFFF), 8: (0, 1, 2, 0x7F, 0x80, 0xFE, 0xFF)}
RLE_SIZES = (1, 2, 64, 65, TILE, TILE + 1, 4 * TILE + 1)
SCAN_SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 4100, 256 * 18)
SCAN_THROUGH_SORT = (17 * TILE + 5, 16)             # (n, endbit): 18 tiles, a histogram of 4608 counts


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def digit(keys, p):
    """the 8-bit digit pass p sorts on"""
    return ((np.asarray(keys, np.uint64) >> U64(8 * p)) & U64(255)).astype(np.int64)


def _with_digit(keys, p, d):
    """keys with the digit of pass p replaced by d (an array or a number)"""
    d = np.asarray(d, np.uint64)
    return (keys & ~(U64(255) << U64(8 * p))) | (d << U64(8 * p))


def tiles(n):
    return (n + TILE - 1) // TILE


def scan_stretch(cnt):
    """elements per lane of the one-workgroup scan: whole groups of four"""
    return ((cnt + SCAN_LANES - 1) // SCAN_LANES + 3) // 4 * 4


# ---- sort ---------------------------------------------------------------------------------------------------------------------------------------------
def sort_cases():
    """[{name, keys, endbit, props}]. Keys outside the bits a case sorts on are payload: they must travel with their key, in input order among equals."""
    out = []

    def add(name, keys, endbit, **props):
        keys = np.ascontiguousarray(keys, np.uint64)
        out.append(dict(name="%s_e%d" % (name, endbit), keys=keys, endbit=endbit, props=props))

    for e in ENDBITS:
        P, mask = R.passes(e), R.sort_mask(e)
        top = P - 1
        for n in SORT_SIZES:
            add("size_%d" % n, _u64(_rng("size %d %d" % (n, e)), n) & mask, e)
        n = 2 * TILE + 77
        rng = _rng("one digit %d" % e)
        add("all_equal", np.full(n, 0x0123456789ABCDEF, np.uint64), e, one_digit_passes=list(range(P)))
        add("same_digit_pass0", _with_digit(_u64(rng, n), 0, 0xA7), e, one_digit_passes=[0])
        if top:
            add("same_digit_top_pass", _with_digit(_u64(rng, n), top, 0x5C), e, one_digit_passes=[top])
        # 64 different digits in every step, the last step ragged (37 lanes)
        n = TILE + STEP + 37
        rng = _rng("64 digits %d" % e)
        add("step_of_64_digits_pass0", _with_digit(_u64(rng, n), 0, np.arange(n) % 64), e, distinct_step_pass=0)
        if top:
            # the digits below the top one are one constant, so the passes before it leave the order alone and the top pass meets the keys as given
            low = U64((1 << (8 * top)) - 1)
            add("step_of_64_digits_top_pass", _with_digit((_u64(rng, n) & ~low) | (U64(0x5A5A5A5A5A5A5A5A) & low), top, (np.arange(n) * 37 + 11) % 64), e,
                distinct_step_pass=top, constant_below=top)
        # two digits: 0 and 255 in every pass, lane by lane in the first
        n = TILE + 3 * STEP + 1
        rng = _rng("two digits %d" % e)
        k = _u64(rng, n)
        for p in range(P):
            k = _with_digit(k, p, 255 * (np.arange(n) % 2 if p == 0 else rng.integers(0, 2, n)))
        add("two_digits_alternating", k, e, two_digits=True)
        # orderings
        n = 2 * TILE + 5
        rng = _rng("orderings %d" % e)
        asc = np.sort(_u64(rng, n) & mask)
        add("already_sorted", asc, e, ascending=True)
        add("reverse_sorted", asc[::-1].copy(), e, descending=True)
        k = _u64(rng, n) & mask
        k[rng.choice(n, 300, replace=False)] = np.where(rng.integers(0, 2, 300) == 1, mask, U64(0))
        add("extremes_among_others", k, e, extremes=(0, int(mask)))
    # stability: index << endbit | value on the low endbit bits, seven values
    for e in (32, 8):
        for n in STABLE_SIZES:
            rng = _rng("stability %d %d" % (e, n))
            v = np.array(STABLE_VALUES[e], np.uint64)[rng.integers(0, 7, n)]
            add("stability_%d" % n, (np.arange(n, dtype=np.uint64) << U64(e)) | v, e, index_shift=e)
    for e in ODD_ENDBITS:
        n = 2 * TILE + 17
        add("endbit_no_multiple_of_8", _u64(_rng("odd endbit %d" % e), n) >> U64(64 - e), e, zero_from_endbit=True)
    n, e = SCAN_THROUGH_SORT
    add("scan_of_18_tiles", _u64(_rng("scan through sort"), n), e, hist_stretch=8)
    return out


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------------------------
def _from_lengths(rng, lengths, n=None):
    """a sorted array whose runs have the given lengths (cut to n), the run keys distinct and ascending"""
    lengths = np.asarray(lengths, np.int64)
    keys = np.unique(_u64(rng, 2 * len(lengths) + 8))[:len(lengths)]
    assert len(keys) == len(lengths)
    a = np.repeat(keys, lengths)
    return a if n is None else a[:n]


def rle_cases():
    """[{name, a, props}]: a is sorted ascending"""
    out = []

    def add(name, a, **props):
        out.append(dict(name=name, a=np.ascontiguousarray(a, np.uint64), props=props))

    for n in RLE_SIZES:
        rng = _rng("rle size %d" % n)
        add("size_%d" % n, _from_lengths(rng, rng.integers(1, 6, n), n))
    n = 4 * TILE + 1
    rng = _rng("rle shapes")
    add("all_distinct", _from_lengths(rng, np.ones(n, np.int64)), all_distinct=True)
    add("all_equal", np.full(n, 0xFEDCBA9876543210, np.uint64), all_equal=True)
    lens = np.ones(600, np.int64)
    lens[1::2] = rng.integers(2, 300, 300)
    add("single_keys_between_long_runs", _from_lengths(rng, lens), alternating=True)
    add("run_ends_at_the_tile_edge", _from_lengths(rng, [TILE - 100, 100, 200, 1, 77]), ends_at_edge=True)
    add("run_straddles_the_tile_edge", _from_lengths(rng, [TILE - 100, 200, 1, 77]), straddles_edge=True)
    add("run_straddles_every_step_edge", _from_lengths(rng, [STEP // 2] + [STEP] * (TILE // STEP), TILE), straddles_steps=True)
    add("run_longer_than_a_tile", _from_lengths(rng, [100, 10000, 30000, 50, 9850]), long_run=True)
    # keys that differ above bit 31 only: a comparison of the low words alone sees one run
    a = _from_lengths(rng, rng.integers(1, 200, 400))
    add("keys_differ_above_bit_31_only", (a & ~U64(0xFFFFFFFF)) | U64(0x12345678), high_bits_only=True)
    return out


# ---- scan -----------------------------------------------------------------------------------------------------------------------------------------------
def scan_cases():
    """[{name, v}]: counts below 2^20, so that every total stays below 2^32"""
    out = [dict(name="size_%d" % n, v=_rng("scan %d" % n).integers(0, 1 << 20, n).astype(np.uint32)) for n in SCAN_SIZES]
    out.append(dict(name="all_zeros", v=np.zeros(4100, np.uint32)))
    out.append(dict(name="all_ones", v=np.ones(256 * 18, np.uint32)))
    return out
