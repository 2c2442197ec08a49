"""The filtered slot-min emitter (MinEmitF, gsearch_amd/csrc/gs_sketch.hip) drops a k-mer on the high words of s0 and s3 alone (gs_hiword.hpp): it
passes every k-mer whose key is below the bound and 0.39 % of the others, whose exact key decides in the flush. A k-mer dropped wrongly would be a slot
minimum lost, so every case is held against the oracle bit for bit - for the three key forms (23-bit keys: optdens, revoptdens; u32 keys: super2 at
k = 16; u64 keys: super2 at k = 21, 32) and for every way the bound moves: fixed at the speculative cap, falling through many values under the
running bound alone, a second walk after a cap that was too low, and across the switch from the direct form to the filtered one.

Shapes, genomes and references are those of tests/test_gpu_sketch_pairs.py (m = 256, one-record genomes of 20 011 to 60 000 bases and three genomes
of 10 or 11 records at every base offset, alone and tiled to >= 520 genomes so that the cap is live)."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
import test_gpu_sketch_pairs as P

pytestmark = pytest.mark.gpu

ALGOS = ("optdens", "revoptdens", "super2")
KS = (16, 21, 32)


def _key_dtype(algo, k):
    if algo != "super2":
        return np.float32
    return np.uint32 if k == 16 else np.uint64            # 32-bit k-mer values at k = 16: u32 keys


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("algo", ALGOS)
def test_signatures_equal_the_oracle(gpu_ctx, algo, k):
    """alone (several workgroups per genome: no cap, the running bound from the first refresh on) and tiled (under the cap); the batch holds the
    multi-record genomes"""
    assert P._check(k, algo).dtype == _key_dtype(algo, k)


@pytest.mark.parametrize("algo,k", [("optdens", 21), ("revoptdens", 16), ("super2", 16), ("super2", 32)])
@pytest.mark.parametrize("cap", ["0", "-3"])
def test_moving_bounds(gpu_ctx, monkeypatch, cap, algo, k):
    """GS_SKETCH_CAP=0: no cap, the bound is the running maximum of the table and falls through a new value - a new scalar limit - at every refresh;
    -3: a cap that nearly every genome misses, so the workgroup walks again under the running bound, with the limit rebuilt for the second walk"""
    monkeypatch.setenv("GS_SKETCH_CAP", cap)
    assert P._check(k, algo).dtype == _key_dtype(algo, k)


M_SWITCH = 2048


@functools.lru_cache(maxsize=None)
def _switch_batch():
    """m = 2 048 over genomes of 131 100 to 170 003 bases (>= 64 k-mers per slot: the launch is filtered), one workgroup each, no cap: a trip of the
    workgroup brings 16 384 k-mers, 8 per slot, so after the refreshes at words 1 and 2 some of the 2 048 minima are still above a quarter of the
    key range (0.75^16 = 1 %: ~20 slots) and the emitter stays on its direct form; by word 8 (0.75^64) the bound is below direct_above and the
    filtered form takes over, 2 to 4 trips before the genome ends"""
    rng = np.random.default_rng(2055)
    recs = [H.dna_ascii(H.rand_dna(rng, n)) for n in (131_100, 150_001, 170_003)]
    seq, rs, rl = O.pack_dna(recs)
    pad = (-len(seq)) % 8
    if pad:
        seq = np.concatenate([seq, np.zeros(pad, np.uint8)])
    packed = (seq, rs, rl, np.arange(len(recs) + 1, dtype=np.uint64))
    return packed, P._tiled(packed)


@pytest.mark.parametrize("algo,k", [("optdens", 21), ("super2", 16), ("super2", 21)])
def test_switch_from_the_direct_to_the_filtered_form(gpu_ctx, monkeypatch, algo, k):
    import gsearch_amd as G
    monkeypatch.setenv("GS_SKETCH_CAP", "0")
    packed, (tiled, reps) = _switch_batch()
    ref = O.sketch_batch(O.params(k, M_SWITCH, algo), *packed)
    sk = G.sketcher_for(G.SeqSketcherParams(k, M_SWITCH, algo))
    big = sk.sketch_packed(*tiled)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["table_in_lds"] and info["workgroups_per_genome"] == 1, info
    assert big.dtype == ref.dtype == _key_dtype(algo, k)
    assert np.array_equal(big.view(np.uint32), np.tile(ref.view(np.uint32), (reps, 1)))
