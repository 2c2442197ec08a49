"""The constructed cases of the orfs tests (SPEC 14): name, records as base codes, parameters. tests/test_gpu_orf.py runs them on the device against the
restatement; tests/test_orf_cpu.py checks without a device that each case has the shape its name promises. TILE is GS_ORF_TILE: the bases one
wavefront takes at a time."""
import numpy as np

import pyref_orf as P

TILE = 192
BG = b"ACG"                        # no stop in any of the six frames: ACG CGA GAC forward, CGT TCG GTC reverse


def bg(n):
    return P.codes((BG * (n // 3 + 1))[:n])


def with_codon(n, at, codon):
    b = bg(n).copy()
    b[at:at + 3] = P.codes(codon)
    return b


def framed(n_codons):
    """a stop, n codons without one, a stop - all in class 0 of the forward strand"""
    return P.codes(b"TAA" + b"GCT" * n_codons + b"TAA")


def small_cases():
    rng = np.random.default_rng(14)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)                                       # noqa: E731
    cs = []
    cs.append(("lengths 0..5", [rnd(n) for n in range(6)] + [P.codes(b"TAA"), P.codes(b"GCT"), P.codes(b"TTA")], {"min_aa": 1}))
    cs.append(("3 min_aa + {-1, 0, 1, 2} bases without a stop", [bg(3 * 30 + d) for d in (-1, 0, 1, 2)], {}))
    cs.append(("ORFs of min_aa - 1, min_aa, max_aa, max_aa + 1 codons", [framed(n) for n in (9, 10, 40, 41)], {"min_aa": 10, "max_aa": 40}))
    cs.append(("stops only", [P.codes(b"TTATCACTA" * 30 + b"TAATAGTGA" * 30), P.codes(b"TAA" * 100)], {"min_aa": 1}))
    cs.append(("no stop: six ORFs at the virtual ends", [bg(500), bg(501), bg(502)], {"min_aa": 1}))
    cs.append(("records of T - 1, T, T + 1, 2 T + 1 bases", [rnd(n) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)], {"min_aa": 1}))
    cs.append(("the same without a stop", [bg(n) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)], {"min_aa": 1}))
    straddle = [with_codon(2 * TILE + 40, at, cod) for cod in (b"TAA", b"TTA", b"TGA", b"TCA") for at in (TILE - 3, TILE - 2, TILE - 1, TILE)]
    cs.append(("a stop on each strand at the positions around a tile boundary", straddle, {"min_aa": 1}))
    thru = with_codon(3 * TILE + 50, 10, b"TAG")
    thru[2 * TILE + 30:2 * TILE + 33] = P.codes(b"TAG")
    thru2 = with_codon(4 * TILE + 7, 11, b"CTA")                                                 # the reverse strand's stop, carried through three tiles
    cs.append(("an ORF through a whole tile: the carry crosses two boundaries", [thru, thru2], {"min_aa": 1}))
    cs.append(("min_aa larger than T / 3", [thru, thru2, rnd(2 * TILE + 1)], {"min_aa": 70}))
    cs.append(("min_aa larger than T / 3, long ones dropped", [thru, thru2, bg(3000)], {"min_aa": 70, "max_aa": 140}))
    cs.append(("empty records between full ones", [rnd(300), rnd(0), rnd(0), rnd(250), rnd(0), rnd(2), rnd(700), rnd(0)], {"min_aa": 5}))
    tga = rnd(3000)
    for at in rng.integers(0, 2990, 200):
        tga[at:at + 3] = P.codes(b"TGA")
    cs.append(("table 11 on a sequence rich in TGA", [tga], {"min_aa": 5, "table": 11}))
    cs.append(("table 4 on a sequence rich in TGA", [tga], {"min_aa": 5, "table": 4}))
    return cs


SMALL = small_cases()
