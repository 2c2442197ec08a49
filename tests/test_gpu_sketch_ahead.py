"""walk_genome's two-stage DNA loop (gsearch_amd/csrc/gs_walk.hpp): a lane loads the words of its next trip before it walks the word of this one, and finds
its record again only when it leaves the record's span of units. Held against the oracle bit for bit where that can go wrong: genomes whose length puts
the last trip of a lane, a wave or a workgroup on either side of a trip's edge; a genome whose records make consecutive trips of a lane land in the same
record, the next one, one several further on and one behind a run of records shorter than k; a genome at base 0 and a genome that ends in the last 8-byte
word of the buffer; the second walk of the filtered sketcher; and the other sketchers that stream through the same walker."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

M = 256
TRIP_N = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537)        # words: one lane, a wave, a workgroup's trip (512), two and three trips, each +- 1
TRIP_R = (0, 1, 31)
HOP_LENS = (16384 * 3 + 7, 16389, 20, 20, 20, 16389, 2000, 2000, 2000, 2000, 33, 64, 95, 31, 16389, 16384 * 3 + 7, 20, 31, 20, 31, 16384 * 3 + 7, 16389, 16389,
            2000, 95, 64, 33, 2000, 20, 16384 * 3 + 7, 31, 16389, 2000, 2000, 2000, 2000, 2000, 2000, 16389, 16384 * 3 + 7)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pack(genomes):
    recs = [r for g in genomes for r in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    seq, rs, rl = O.pack_dna(recs)
    return seq, rs, rl, goff


def _tiled(packed, n_min=520):
    """the packed buffer repeated until the batch has >= 520 genomes (2 x the CUs of an MI355X): every genome gets ONE workgroup, and only that form sets
    the speculative cap of the filtered emitter (test_gpu_sketch_windows.py)"""
    seq, rs, rl, goff = packed
    reps = -(-n_min // (len(goff) - 1))
    seq_r = np.tile(seq, reps)
    rs_r = np.concatenate([rs + np.uint64(r * len(seq) * 4) for r in range(reps)])
    rl_r = np.tile(rl, reps)
    goff_r = np.concatenate([goff[:-1] + np.uint64(r * len(rs)) for r in range(reps)] + [np.array([reps * len(rs)], np.uint64)])
    return (seq_r, rs_r, rl_r, goff_r), reps


@functools.lru_cache(maxsize=1)
def _trip_edges():
    rng = np.random.default_rng(2041)
    packed = _pack([[H.dna_ascii(H.rand_dna(rng, 32 * n + r))] for n in TRIP_N for r in TRIP_R])
    return packed, _tiled(packed)


@functools.lru_cache(maxsize=1)
def _hopping():
    """one genome of 40 records: a workgroup's trip is 512 words = 16 384 bases, so a lane's next trip lies in the same record (3 x 16 384 + 7), in the next
    (16 389), several further on (runs of 2 000, 95, 64, 33) or behind a run of records shorter than k (20 at k = 21; 20 and 31 at k = 32)"""
    rng = np.random.default_rng(2042)
    packed = _pack([[H.dna_ascii(H.rand_dna(rng, n)) for n in HOP_LENS]])
    return packed, _tiled(packed)


@functools.lru_cache(maxsize=None)
def _ref(which, k, algo, data="dna"):
    packed = {"trip": _trip_edges, "hop": _hopping}[which]()[0]
    return O.sketch_batch(O.params(k, M, algo, data), *packed)


def _check(which, k, algo="optdens", data="dna", alone_parts=None):
    """the genomes alone (split over several workgroups each) and tiled (one workgroup per genome, filtered, under the speculative cap) == oracle"""
    import gsearch_amd as G
    packed, (tiled, reps) = {"trip": _trip_edges, "hop": _hopping}[which]()
    ref = _ref(which, k, algo, data)
    sk = G.sketcher_for(G.SeqSketcherParams(k, M, algo, data))
    got = sk.sketch_packed(*packed)
    if algo in ("optdens", "revoptdens"):
        info = sk.ctx.last_sketch_info()
        assert info["filtered"] and info["workgroups_per_genome"] > 1, info
    assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref))
    big = sk.sketch_packed(*tiled)
    if algo in ("optdens", "revoptdens"):
        info = sk.ctx.last_sketch_info()
        assert info["filtered"] and info["table_in_lds"] and info["workgroups_per_genome"] == 1, info
    assert np.array_equal(_bits(big), np.tile(_bits(ref), (reps, 1)))


@pytest.mark.parametrize("k", [21, 32])
def test_trip_edges(gpu_ctx, k):
    """genomes of 32 n + r bases, n on both sides of a lane's, a wave's and a workgroup's trip: the last loads ahead, and the first trip that has none"""
    _check("trip", k)


@pytest.mark.parametrize("k", [21, 32])
def test_record_hopping(gpu_ctx, k):
    _check("hop", k)


def test_second_walk_starts_the_pipeline_afresh(gpu_ctx, monkeypatch):
    """GS_SKETCH_CAP=-3: the speculative bound fails for most of these genomes and their workgroups walk them a second time under the running bound alone"""
    monkeypatch.setenv("GS_SKETCH_CAP", "-3")
    _check("trip", 21)


@pytest.mark.parametrize("r", TRIP_R)
def test_buffer_edges(gpu_ctx, r):
    """the first genome's record starts at base 0 of the buffer, and the buffer ends with the 8-byte word the last genome's last base lies in: no padding
    behind it for a load ahead to fall into"""
    import gsearch_amd as G
    rng = np.random.default_rng(2043 + r)
    seq, rs, rl, goff = _pack([[H.dna_ascii(H.rand_dna(rng, n))] for n in (32 * 600, 32 * 513 + 5, 32 * 700 + 31, 32 * 1024 + r)])
    assert rs[0] == 0
    end = int(rs[-1] + rl[-1])
    seq = np.ascontiguousarray(seq[:-(-end // 32) * 8])
    assert len(seq) % 8 == 0 and (end - 1) // 32 == len(seq) // 8 - 1
    ref = O.sketch_batch(O.params(21, M, "optdens"), seq, rs, rl, goff)
    sk = G.sketcher_for(G.SeqSketcherParams(21, M, "optdens"))
    got = sk.sketch_packed(seq, rs, rl, goff)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["workgroups_per_genome"] > 1, info
    assert np.array_equal(_bits(got), _bits(ref))
    # one workgroup per genome: the same four genomes 130 times over, the buffer still ending with the last genome's last word
    reps = 130
    stride = (len(seq) + 8) // 8 * 8                                              # whole words per copy; the last copy is cut where `seq` is
    seq_r = np.zeros(stride * reps, np.uint8)
    for i in range(reps):
        seq_r[i * stride: i * stride + len(seq)] = seq
    seq_r = np.ascontiguousarray(seq_r[:(reps - 1) * stride + len(seq)])
    rs_r = np.concatenate([rs + np.uint64(i * stride * 4) for i in range(reps)])
    goff_r = np.concatenate([goff[:-1] + np.uint64(i * len(rs)) for i in range(reps)] + [np.array([reps * len(rs)], np.uint64)])
    big = sk.sketch_packed(seq_r, rs_r, np.tile(rl, reps), goff_r)
    info = sk.ctx.last_sketch_info()
    assert info["filtered"] and info["workgroups_per_genome"] == 1, info
    assert np.array_equal(_bits(big), np.tile(_bits(ref), (reps, 1)))


@pytest.mark.parametrize("algo", ["revoptdens", "super2", "hll", "prob"])
def test_other_sketchers_on_the_same_walker(gpu_ctx, algo):
    _check("hop", 21, algo)


def test_super2_aa_many_short_records(gpu_ctx):
    """the AA path keeps its one-stage loop: a proteome of records of 5 to 400 residues, alone and one workgroup per proteome"""
    import gsearch_amd as G
    rng = np.random.default_rng(2044)
    prots = [[H.aa_ascii(rng.integers(0, 20, size=int(n))) for n in rng.integers(5, 401, size=150)] for _ in range(3)]
    recs = [r for g in prots for r in g]
    goff = np.cumsum([0] + [len(g) for g in prots]).astype(np.uint64)
    seq, rs, rl = O.filter_aa(recs)
    ref = O.sketch_batch(O.params(7, M, "super2", "aa"), seq, rs, rl, goff)
    sk = G.sketcher_for(G.SeqSketcherParams(7, M, "super2", "aa"))
    got = sk.sketch_packed(seq, rs, rl, goff)
    assert got.dtype == ref.dtype and np.array_equal(got, ref)
    reps = 174
    pad = (-len(seq)) % 32
    seq_p = np.concatenate([seq, np.zeros(pad, np.uint8)])
    big = sk.sketch_packed(np.tile(seq_p, reps), np.concatenate([rs + np.uint64(i * len(seq_p)) for i in range(reps)]), np.tile(rl, reps),
                           np.concatenate([goff[:-1] + np.uint64(i * len(rs)) for i in range(reps)] + [np.array([reps * len(rs)], np.uint64)]))
    assert np.array_equal(big, np.tile(ref, (reps, 1)))
