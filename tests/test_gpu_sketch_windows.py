"""The interior-word walk of the sketcher builds its k-mer windows by funnel shifts of the previous and the current packed word
and the filtered emitter works on h + gamma. Every k from 1 to 32 the
parameter check accepts, both strand rules, on genomes long enough that whole waves take the
interior, filtered path, must give the oracle's bits."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

M = 256


def _genomes():
    rng = np.random.default_rng(2032)
    fam = H.family(rng, 70_000, [0.002, 0.03])
    genomes = [[H.dna_ascii(g)] for g in fam]
    # records that are not multiples of 32 bases, so words of one record start at every offset of the packed stream
    genomes.append([H.dna_ascii(H.rand_dna(rng, n)) for n in (20_011, 9_999, 31, 17_005, 24_003)])
    genomes.append([b"A" * 70_003])                  # poly-A: one k-mer, its reverse complement poly-T
    genomes.append([b"N" * 70_000])                  # no k-mer at all
    genomes.append([H.dna_ascii(H.rand_dna(rng, 40_000)) + b"N" * 33 + H.dna_ascii(H.rand_dna(rng, 30_001))])
    return genomes


@functools.lru_cache(maxsize=1)
def _packed():
    """the genomes packed once, and the same packed buffer repeated until the batch has >= 520 genomes (2 x the CUs of an MI355X): then
    min_geom gives every genome ONE workgroup, the form the bench runs, and only that form sets the speculative cap of the filtered emitter"""
    genomes = _genomes()
    recs = [r for g in genomes for r in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    seq, rs, rl = O.pack_dna(recs)
    reps = -(-520 // len(genomes))
    seq_r = np.tile(seq, reps)
    rs_r = np.concatenate([rs + np.uint64(r * len(seq) * 4) for r in range(reps)])
    rl_r = np.tile(rl, reps)
    goff_r = np.concatenate([goff[:-1] + np.uint64(r * len(rs)) for r in range(reps)] + [np.array([reps * len(rs)], np.uint64)])
    return (seq, rs, rl, goff), (seq_r, rs_r, rl_r, goff_r), reps


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(k, algo, data):
    """the genomes alone (each split over several workgroups) and tiled (one workgroup per genome, speculative cap), both filtered, == oracle"""
    import gsearch_amd as G
    one, tiled, reps = _packed()
    ref = O.sketch_batch(O.params(k, M, algo, data), *one)
    sk = G.sketcher_for(G.SeqSketcherParams(k, M, algo, data))
    got = sk.sketch_packed(*one)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["workgroups_per_genome"] > 1, info
    assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref))
    big = sk.sketch_packed(*tiled)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["table_in_lds"] and info["workgroups_per_genome"] == 1, info
    assert np.array_equal(_bits(big), np.tile(_bits(ref), (reps, 1)))


@pytest.mark.parametrize("data", ["dna", "dna_fwd"])
@pytest.mark.parametrize("k", [k for k in range(1, 33) if k != 15])          # k = 15 is rejected by the parameter check (as in gsearch)
def test_sketch_windows_match_oracle_for_every_k(gpu_ctx, k, data):
    _check(k, "optdens", data)


@pytest.mark.parametrize("k", [1, 2, 9, 14, 16, 17, 18, 21, 31, 32])
def test_sketch_windows_revoptdens_match_oracle(gpu_ctx, k):
    for data in ("dna", "dna_fwd"):
        _check(k, "revoptdens", data)


@pytest.mark.parametrize("k", [5, 16, 17, 21, 32])
def test_sketch_windows_second_walk_match_oracle(gpu_ctx, monkeypatch, k):
    """GS_SKETCH_CAP=-3: the speculative bound of the one-workgroup form is (m / N)(ln m - 3), about 0.9 % of the key range for these genomes;
    the minima of ~8 % of the slots of a 70 kb genome lie above it, and the poly-A genome fills at most two slots under any bound: their checks fail and
    the workgroups walk their genomes a second time under the running bound alone"""
    monkeypatch.setenv("GS_SKETCH_CAP", "-3")
    _check(k, "optdens", "dna")
