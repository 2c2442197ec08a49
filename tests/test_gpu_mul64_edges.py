"""The device forms the 64 x 64-bit multiplies of fx64 and SplitMix64 from 32-bit multiply-adds (gs_spec.hpp: mulc64), with
the cross terms and the offset gamma added in their own steps. Push k-mer values at the edges of those carries through every sketcher that hashes
with them - all-ones (poly-T, forward strand), zero (poly-A), values with the top bit set, runs that flip between them, random - and compare
with the oracle (optdens, revoptdens, super, super2, hll, prob) or the numpy reference of SPEC 7 (hmh), bit for bit."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

M = 256


@functools.lru_cache(maxsize=1)
def _genomes():
    rng = np.random.default_rng(6401)
    n = 20_003                                           # >= 64 k-mers per slot at M = 256: the filtered emitter takes the interior words
    rnd = lambda L: H.dna_ascii(H.rand_dna(rng, L))
    runs = b"".join(b"T" * int(a) + rnd(int(b)) for a, b in zip(rng.integers(20, 70, 400), rng.integers(1, 20, 400)))
    return [
        [b"T" * n],                                      # forward k-mer all ones: x_hi = x_lo = 2^32 - 1 at k = 32
        [b"A" * n],                                      # zero
        [(b"TG" * n)[:n]],                               # 0b1110 repeated: top bit set, both halves near 2^32
        [(b"GT" * n)[:n], b"C" * 4_000],                 # 0b1011 repeated, a second record of poly-C
        [runs[:n]],                                      # runs of T long and short against random bases: the carries switch on and off
        [rnd(n)],
        [rnd(7_001), rnd(13_037)],
        [(b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTA" * 700)[:n]],  # one A every 32 bases: the all-ones value and its neighbours in every word position
    ]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# prob hashes with SplitMix64 only after its own table of distinct k-mer values, whose empty mark is (most likely) the all-ones value: poly-T read forward at
# k = 32 IS that value (NOTES.md, "ProbMinHash3a and the all-ones k-mer"): prob runs up to k = 21 here
CASES = [(a, k) for a in ("optdens", "revoptdens", "super", "super2", "hll", "prob") for k in (16, 17, 21, 32) if not (a == "prob" and k == 32)]


@pytest.mark.parametrize("algo,k", CASES)
def test_carry_edges_match_oracle(gpu_ctx, algo, k):
    import gsearch_amd as G
    genomes = _genomes()
    recs = [r for g in genomes for r in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    seq, rs, rl = O.pack_dna(recs)
    for data in ("dna", "dna_fwd"):
        ref = O.sketch_batch(O.params(k, M, algo, data), seq, rs, rl, goff)
        got = G.sketcher_for(G.SeqSketcherParams(k, M, algo, data)).sketch_packed(seq, rs, rl, goff)
        assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref)), (algo, k, data)


@pytest.mark.parametrize("k", [16, 21, 32])
def test_carry_edges_hmh_match_reference(gpu_ctx, k):
    import gsearch_amd as G
    import pyref_hmh as PR
    genomes = _genomes()
    sig = G.HyperMinHashSketch.for_k(k).sketch_genomes(genomes)
    for i, g in enumerate(genomes):
        assert np.array_equal(sig[i], PR.sketch(g, k)), (k, i)
