"""The hnsw2knn neighbour-list text (upstream src/bin/hnsw2knn.rs, README section "hnsw2knn") written from Hnsw.knn_graph's arrays:
one line per node, `path:` then, per neighbour in ascending order, a tab, `path:` and the distance with six decimals. No GPU needed."""
import io

import numpy as np

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)

EXPECTED = (
    "db/g0.fna:\tdb/g2.fna:0.000000\tdb/g1.fna:0.333333\n"
    "db/g2.fna:\tdb/g0.fna:0.000000\tdb/g1.fna:0.999500\n"
    "db/g1.fna:\n"
    "db/g3.fna:\tdb/g0.fna:1.000000\n"
)


def test_writer_matches_fixture():
    import gsearch_amd as G
    seqdict = [("db/g0.fna", "g0 chromosome", 5000), ("db/g1.fna", "g1", 4000), ("db/g2.fna", "g2", 4500), ("db/g3.fna", "g3", 10)]
    node_ids = np.array([0, 2, 1, 3], np.uint64)
    ids = np.array([[2, 1], [0, 1], [U64MAX, U64MAX], [0, U64MAX]], np.uint64)
    dist = np.array([[0.0, 1.0 / 3.0], [0.0, 0.9995], [np.inf, np.inf], [1.0, np.inf]], np.float32)
    cnt = np.array([2, 2, 0, 1], np.uint32)
    out = io.StringIO()
    assert G.dump_knn_graph(seqdict, node_ids, ids, dist, cnt, out) == 4
    assert out.getvalue() == EXPECTED


def test_writer_uses_caller_ids():
    """rows and neighbours are looked up in seqdict by the caller's id, as ReqAnswer.dump does"""
    import gsearch_amd as G
    seqdict = {7: ("x.fa", "x", 1), 1000000000000: ("y.fa", "y", 2)}
    out = io.StringIO()
    G.dump_knn_graph(seqdict, np.array([1000000000000], np.uint64), np.array([[7]], np.uint64), np.array([[0.25]], np.float32),
                     np.array([1], np.uint32), out)
    assert out.getvalue() == "y.fa:\tx.fa:0.250000\n"
