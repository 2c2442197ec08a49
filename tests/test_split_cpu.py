"""The host rules of split databases (SPEC 17 items 12-18) without a device: the restatement tests/pyref_split.py against sharding.merge_topk_shards,
against its own invariants and against the functions of gsearch_amd/split.py that tohnsw_split / request_split use; the split.json text."""
import numpy as np
import pytest

import pyref_split as RS

NOID = np.uint64(0xFFFFFFFFFFFFFFFF)


def _piece_answers(rng, nq, knbn, n_points, levels):
    """answers of one piece of n_points points: per query min(knbn, n_points) distinct local ids at distances drawn from a few levels (so that
    distances tie inside and across pieces), ascending by (distance, id), padded"""
    ids, dist, cnt = np.full((nq, knbn), NOID, np.uint64), np.full((nq, knbn), np.inf, np.float32), np.zeros(nq, np.uint32)
    for q in range(nq):
        k = min(knbn, n_points)
        loc = rng.choice(n_points, k, replace=False).astype(np.uint64)
        d = rng.choice(levels, k).astype(np.float32)
        o = np.lexsort((loc, d))
        ids[q, :k], dist[q, :k], cnt[q] = loc[o], d[o], k
    return ids, dist, cnt, rng.integers(1, 100, nq).astype(np.uint64)


@pytest.mark.parametrize("knbn,sizes", [(5, (12, 3, 9)), (8, (2, 1, 30)), (1, (4, 4)), (6, (2, 2))])
def test_merge_rows_folded_over_pieces_equals_the_merge_of_their_union(knbn, sizes):
    from gsearch_amd.sharding import merge_topk_shards
    rng = np.random.default_rng(knbn)
    nq, levels = 7, np.array([0.0, 0.25, 0.5, 0.5, 1.0], np.float32)
    pieces = [_piece_answers(rng, nq, knbn, n, levels) for n in sizes]
    off = RS.offsets(sizes)
    assert any(c.min() < knbn for _, _, c, _ in pieces) or min(sizes) >= knbn              # short lists where a piece is smaller than knbn
    run = RS.empty_lists(nq, knbn)
    for p, ans in enumerate(pieces):
        run = RS.merge_rows(run, ans, None, off[p])
    shard_ids = [np.where(ids == NOID, NOID, ids + np.uint64(off[p])) for p, (ids, _, _, _) in enumerate(pieces)]
    want_ids, want_dist = merge_topk_shards(shard_ids, [d for _, d, _, _ in pieces], knbn)
    assert np.array_equal(run[0], want_ids) and np.array_equal(run[1].view(np.uint32), want_dist.view(np.uint32))
    assert np.array_equal(run[2], np.minimum(knbn, sum(c.astype(np.int64) for _, _, c, _ in pieces)))
    assert np.array_equal(run[3], sum(e for _, _, _, e in pieces))
    # the case is what it claims: equal distances met across pieces, and the id decided
    tied = [(run[1][q, j] == run[1][q, j + 1]) for q in range(nq) for j in range(int(run[2][q]) - 1)]
    assert any(tied) or knbn == 1


def test_merge_rows_touches_listed_rows_only_and_puts_the_running_entry_first():
    run = (np.array([[5, 9], [7, NOID], [1, 2]], np.uint64), np.array([[0.5, 0.5], [0.25, np.inf], [0.0, 1.0]], np.float32), np.array([2, 1, 2], np.uint32),
           np.array([10, 20, 30], np.uint64))
    ans = (np.array([[3, 0], [7, 8]], np.uint64), np.array([[0.5, 0.75], [0.25, 0.25]], np.float32), np.array([2, 2], np.uint32), np.array([1, 2], np.uint64))
    ids, dist, cnt, ev = RS.merge_rows(run, ans, [0, 1], 0)
    assert ids.tolist() == [[3, 5], [7, 7], [1, 2]] and dist.tolist() == [[0.5, 0.5], [0.25, 0.25], [0.0, 1.0]]
    assert cnt.tolist() == [2, 2, 2] and ev.tolist() == [11, 22, 30]
    ids, _, cnt, _ = RS.merge_rows(run, ans, [1, 2], 1 << 32)
    assert ids.tolist() == [[5, 9], [7, (1 << 32) + 3], [1, (1 << 32) + 7]] and cnt.tolist() == [2, 2, 2]


@pytest.mark.parametrize("n,pieces,seed", [(24, 1, 0), (24, 2, 0), (24, 5, 3), (7, 7, 1), (1000, 13, 9)])
def test_random_assignment_is_a_partition_with_sizes_within_one(n, pieces, seed):
    from gsearch_amd.split import random_pieces
    parts = RS.random_assignment(n, pieces, seed)
    assert sorted(i for p in parts for i in p) == list(range(n)) and all(p == sorted(p) for p in parts)
    sizes = [len(p) for p in parts]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    assert random_pieces(n, pieces, seed) == parts
    if pieces == 1:
        assert parts == [list(range(n))]
    elif n >= 24:
        assert parts != RS.random_assignment(n, pieces, seed + 1) and parts[0] != list(range(sizes[0]))      # seeded, and no contiguous cut


def test_random_assignment_refuses_more_pieces_than_genomes():
    import gsearch_amd as G
    from gsearch_amd.split import random_pieces
    for pieces in (0, 4):
        with pytest.raises(G.GsError) as e:
            random_pieces(3, pieces, 0)
        assert e.value.code == G._lib.GS_ERR_INVALID


def test_cutting_at_max_piece():
    from gsearch_amd.split import medoid_pieces
    assign = [1, 0, 1, 1, 1, 1, 1, 3, 1, 1, 1, 0]                                    # medoid 1 holds 9 genomes, medoid 2 none
    assert RS.cut_pieces(assign, 4, 4) == [(0, [1, 11]), (1, [0, 2, 3]), (1, [4, 5, 6]), (1, [8, 9, 10]), (3, [7])]
    assert RS.cut_pieces(assign, 4, None) == [(0, [1, 11]), (1, [0, 2, 3, 4, 5, 6, 8, 9, 10]), (3, [7])]
    assert RS.cut_pieces(assign, 4, 9) == RS.cut_pieces(assign, 4, None) and [len(f) for _, f in RS.cut_pieces(assign, 4, 8)] == [2, 5, 4, 1]
    for max_piece in (None, 1, 2, 4, 8, 9, 100):
        got = medoid_pieces(assign, 4, max_piece)
        assert got == RS.cut_pieces(assign, 4, max_piece)
        assert max_piece is None or max(len(f) for _, f in got) <= max_piece


def test_medoid_argmin_takes_the_first_of_equal_counts():
    assert RS.medoid_argmin([[3, 1, 1], [0, 0, 5], [9, 8, 7]]).tolist() == [1, 0, 2]


def test_routing_and_offsets():
    from gsearch_amd.split import id_offsets, route_rows
    table, counts = np.array([[2, 0], [1, 2], [0, 1], [2, 1]]), np.array([2, 2, 1, 2])
    piece_medoid = [0, 1, 1, 2]
    want = RS.routing(table, counts, piece_medoid)
    assert want == [[0, 2], [1, 3], [1, 3], [0, 1, 3]]                              # row 2's second entry is beyond its count
    got = route_rows(table, counts, piece_medoid)
    assert [g.tolist() for g in got] == want and all(g.dtype == np.uint32 for g in got)
    assert [g.tolist() for g in route_rows(table, counts, [None, 2])] == [[0, 1, 2, 3], [0, 1, 3]]
    assert RS.offsets([3, 0, 5, 2]) == [0, 3, 3, 8] == id_offsets([3, 0, 5, 2])


SPLIT_JSON = """{
 "version": 1,
 "mode": "medoid",
 "seed": 7,
 "sketch": {
  "kmer_size": 21,
  "sketch_size": 512,
  "algo": "OPTDENS",
  "data_t": "DNA"
 },
 "block_flag": false,
 "router": "router",
 "medoids": [
  "db/a \\"quoted\\" name.fna",
  "db/sub/é.fa.gz"
 ],
 "pieces": [
  {
   "dir": "part_000",
   "medoid": 0
  },
  {
   "dir": "part_001",
   "medoid": 1
  },
  {
   "dir": "part_002",
   "medoid": 1
  }
 ]
}
"""


def test_split_json_text_is_the_literal():
    import json
    from gsearch_amd.split import split_json_text
    from gsearch_amd.state import HnswParams, ProcessingParams
    params = ProcessingParams(HnswParams(1_500_000, 400, 8, 1.0), 21, 512, "optdens", "dna", False)
    text = split_json_text("medoid", 7, params, [("part_000", 0), ("part_001", 1), ("part_002", 1)], ['db/a "quoted" name.fna', "db/sub/é.fa.gz"], "router")
    assert text == SPLIT_JSON
    text = split_json_text("random", 0, params, [("part_000", None)], [], None)
    o = json.loads(text)
    assert o["router"] is None and o["medoids"] == [] and o["pieces"] == [{"dir": "part_000", "medoid": None}] and list(o) == list(json.loads(SPLIT_JSON))
