"""The filtered slot-min emitter (MinEmitF, gsearch_amd/csrc/gs_sketch.hip) takes the k-mers of an interior word two at a time - one queue push for the
lanes where either survives, a second one for the lanes where both do, a flush test behind each. Every case is held against the oracle bit for bit.

Where the pair path is live: under the speculative cap (one workgroup per genome: the batch is tiled to >= 520 genomes). At m = 256 a genome of N = 20 000
to 60 000 bases has the cap (m / N)(ln m + 7) at 5 to 16 % of the key range - with the 20 000-base genomes about a sixth of the k-mers survive, so of a
wave's 64 lanes about ten pass per k-mer, nearly every pair has a lane where both pass (64 x 0.16^2 = 1.6 expected: the second push) and 64 survivors
are pending - a flush, with the rest moved to the front - every three or four pairs, after the first push of a pair as often as after the second. The
benchmark's 7 % survivors (a quarter of the pairs with a second push: 64 x 0.07^2 = 0.3) lie between that and the long genomes below."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

M = 256
KS = (11, 16, 17, 21, 31, 32)          # both funnel forms (k <= 16, k > 16); segments of even (odd k) and odd (even k) length
# a one-workgroup genome is walked 512 words a trip, wave w taking words 64 w .. 64 w + 63 of each: 129 + 512 (n - 1) + 40 words give wave 1 exactly n
# interior words (word 0 is the record's first: wave 0 starts on the rolling path) and leave wave 2 a partial wave (41 lanes) in its last trip.
# 63, 64, 65: on both sides of the bound refresh, which comes every 64th word under a cap
TRIPS = (1, 2, 63, 64, 65)


def _bits(a):
    return a.view(np.uint32)


def _pack_at(records, offsets):
    """records packed so that record i starts at base offset offsets[i] of a 32-base word (O.pack_dna only starts records on 4-base boundaries)"""
    total = sum(len(r) for r in records) + 64 * len(records) + 64
    packed = np.zeros(total // 4 + 16, dtype=np.uint8)
    starts, lens, off = [], [], 0
    for r, o in zip(records, offsets):
        off = (off + 31) // 32 * 32 + o
        a = np.frombuffer(r, dtype=np.uint8)
        n = O.lib().go_pack_dna(O._p(a), len(a), O._p(packed), off)
        starts.append(off)
        lens.append(n)
        off += n
    return packed[:(off + 31) // 32 * 8 + 8], np.array(starts, np.uint64), np.array(lens, np.uint64)


def _tiled(packed, n_min=520):
    """the packed buffer repeated until the batch has >= 520 genomes (2 x the CUs of an MI355X): every genome gets ONE workgroup, and only that form sets
    the speculative cap of the filtered emitter"""
    seq, rs, rl, goff = packed
    assert len(seq) % 8 == 0
    reps = -(-n_min // (len(goff) - 1))
    seq_r = np.tile(seq, reps)
    rs_r = np.concatenate([rs + np.uint64(r * len(seq) * 4) for r in range(reps)])
    goff_r = np.concatenate([goff[:-1] + np.uint64(r * len(rs)) for r in range(reps)] + [np.array([reps * len(rs)], np.uint64)])
    return (seq_r, rs_r, np.tile(rl, reps), goff_r), reps


def _genomes(long):
    """-> (records, base offset of each record's start, records per genome)"""
    rng = np.random.default_rng(2051)
    recs, offs, per = [], [], []
    for n in (20_011, 33_333, 60_000):                                  # one record each
        recs.append(H.dna_ascii(H.rand_dna(rng, n))); offs.append(0); per.append(1)
    # three genomes of 11, 11 and 10 records of ~4 500 bases (~140 words: whole waves inside a record between the rolling paths at its edges),
    # the 32 records starting at the base offsets 0..31
    for lo, hi in ((0, 11), (11, 22), (22, 32)):
        for o in range(lo, hi):
            recs.append(H.dna_ascii(H.rand_dna(rng, 4_300 + 37 * o))); offs.append(o)
        per.append(hi - lo)
    if long:
        for i, n in enumerate(TRIPS):
            recs.append(H.dna_ascii(H.rand_dna(rng, 32 * (129 + 512 * (n - 1) + 40) + (0, 1, 17, 31, 5)[i]))); offs.append(0); per.append(1)
    return recs, offs, per


@functools.lru_cache(maxsize=None)
def _packed(long):
    recs, offs, per = _genomes(long)
    seq, rs, rl = _pack_at(recs, offs)
    assert [int(s) % 32 for s in rs] == offs
    packed = (seq, rs, rl, np.cumsum([0] + per).astype(np.uint64))
    return packed, _tiled(packed)


@functools.lru_cache(maxsize=None)
def _ref(long, k, algo):
    return O.sketch_batch(O.params(k, M, algo), *_packed(long)[0])


def _check(k, algo="optdens", long=False):
    """the genomes alone (several workgroups each: no cap, the filter starts on its direct form and warms up) and tiled (one workgroup per genome,
    under the speculative cap) == oracle"""
    import gsearch_amd as G
    packed, (tiled, reps) = _packed(long)
    ref = _ref(long, k, algo)
    sk = G.sketcher_for(G.SeqSketcherParams(k, M, algo))
    got = sk.sketch_packed(*packed)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["workgroups_per_genome"] > 1, info
    assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref))
    big = sk.sketch_packed(*tiled)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["table_in_lds"] and info["workgroups_per_genome"] == 1, info
    assert np.array_equal(_bits(big), np.tile(_bits(ref), (reps, 1)))
    return got


@pytest.mark.parametrize("k", KS)
def test_pairs_under_the_cap_optdens(gpu_ctx, k):
    _check(k)


@pytest.mark.parametrize("k", [16, 21])
def test_pairs_under_the_cap_revoptdens(gpu_ctx, k):
    _check(k, "revoptdens")


@pytest.mark.parametrize("k", [21, 32])
def test_pairs_under_the_cap_super2_u64_keys(gpu_ctx, k):
    assert _check(k, "super2").dtype == np.uint64


@pytest.mark.parametrize("k", [21, 32])
def test_interior_words_per_wave_and_a_mixed_batch(gpu_ctx, k):
    """one call with everything: the one-record genomes, the records at every base offset, and genomes that give a wave 1, 2, 63, 64 and 65 interior
    words before a partial last wave"""
    _check(k, long=True)


@pytest.mark.parametrize("k", [21, 32])
def test_cap_fallback_walks_again(gpu_ctx, monkeypatch, k):
    """GS_SKETCH_CAP=-3: under the cap (m / N)(ln m - 3) a slot expects ln m - 3 = 2.5 k-mers, so it stays empty with probability e^-2.5 = 8 % and
    every genome has some of its 256 slots at or above the cap: each workgroup walks its genome again under the running bound alone, and the queue
    starts empty a second time"""
    monkeypatch.setenv("GS_SKETCH_CAP", "-3")
    _check(k)


def test_direct_regime_through_the_generic_pair_hook(gpu_ctx):
    """m = 2048 over 30 000 bases: fewer than 64 k-mers per slot, so the launch takes the unfiltered emitter, which sees the pairs of the funnel walk
    through the generic hook (two single emits)"""
    import gsearch_amd as G
    rng = np.random.default_rng(2052)
    seq, rs, rl = O.pack_dna([H.dna_ascii(H.rand_dna(rng, 30_000 + i)) for i in range(3)])
    goff = np.arange(4, dtype=np.uint64)
    for k in (16, 21):
        ref = O.sketch_batch(O.params(k, 2048, "optdens"), seq, rs, rl, goff)
        sk = G.sketcher_for(G.SeqSketcherParams(k, 2048, "optdens"))
        got = sk.sketch_packed(seq, rs, rl, goff)
        info = sk.ctx.last_sketch_info()
        assert not info["filtered"] and info["table_in_lds"], info
        assert np.array_equal(_bits(got), _bits(ref))
