"""tohnsw_split / request_split (gsearch_amd/split.py, SPEC 17 items 12-18) on planted families, with the K, S, NBNG and EFC of tests/test_gpu_commands.py.

Database folder: 24 genomes of 20 kbp in 4 families of 9, 5, 5 and 5 - each family its root and mutants of it at 0.2 to 6 %, one file per genome over
two sub-folders. Queries: one further mutant (2 %) of every root. The yardsticks are tohnsw / request themselves (held to the oracle by
tests/test_gpu_commands.py) on the same folders and on every piece, the restatement tests/pyref_split.py for everything the split adds, and
ReqAnswer.dump for the text."""
import hashlib
import io
import json
import os
import shutil

import numpy as np
import pytest

import helpers as H
import pyref_split as RS
from test_gpu_commands import EFC, K, NBNG, S, SEED, BATCH, _fasta, _write

pytestmark = pytest.mark.gpu

KNBN, EF_REQ, LEN, CAP = 5, 64, 20000, 4096
THR = float(np.float32(0.99))
FAMILIES = (9, 5, 5, 5)
MUS = (0.002, 0.005, 0.01, 0.02, 0.03, 0.04, 0.05, 0.06)
BUILD = dict(ef=EFC, algo="optdens", seed=SEED, insert_batch=BATCH, capacity=CAP)


def _name(f, i):
    return os.path.join("sub_%d" % (f % 2), "f%d_m%02d.fna" % (f, i))


class Corpus:
    def __init__(self, root):
        rng = np.random.default_rng(31)
        self.root = str(root)
        self.db, self.queries = os.path.join(self.root, "db"), os.path.join(self.root, "queries")
        self.roots, self.rel = [], []
        for f, size in enumerate(FAMILIES):
            root_g = H.rand_dna(rng, LEN)
            self.roots.append(root_g)
            for i in range(size):
                g = root_g if i == 0 else H.mutate(rng, root_g, MUS[i - 1])
                _write(os.path.join(self.db, _name(f, i)), _fasta([(b"g", H.dna_ascii(g))]))
                self.rel.append(_name(f, i))
            _write(os.path.join(self.queries, "q%d.fna" % f), _fasta([(b"q", H.dna_ascii(H.mutate(rng, root_g, 0.02)))]))
        _write(os.path.join(self.db, "sub_0", "only_n.fna"), _fasta([(b"n", b"N" * 2000)]))          # a file without a kept record
        self.root_paths = [os.path.join(self.db, _name(f, 0)) for f in range(len(FAMILIES))]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, gpu_ctx):
    return Corpus(tmp_path_factory.mktemp("split"))


def _request(tag, fn, db, corpus, **kw):
    out, mt = os.path.join(corpus.root, tag + ".neighbors.txt"), os.path.join(corpus.root, tag + ".matches")
    for p in (out, mt):
        if os.path.exists(p):
            os.remove(p)
    res = fn(db, corpus.queries, KNBN, out=out, matches=mt, ef=EF_REQ, **kw)
    return res, open(out, "rb").read(), open(mt, "rb").read()


def _digest(d, skip=("processing_state.json",)):
    return {n: hashlib.sha256(open(os.path.join(d, n), "rb").read()).hexdigest() for n in sorted(os.listdir(d)) if n not in skip}


def _dict(d):
    from gsearch_amd.state import SeqDict
    return SeqDict.reload_json(os.path.join(d, "seqdict.json")).items


def _text(items, seqdict, ids, dist, cnt):
    import gsearch_amd as G
    buf = io.StringIO()
    for i, item in enumerate(items):
        G.ReqAnswer(i, item, [G.Neighbour(int(ids[i, j]), float(dist[i, j])) for j in range(int(cnt[i]))]).dump(seqdict, THR, buf)
    return buf.getvalue().encode()


def _split_json(d):
    return json.load(open(os.path.join(d, "split.json"), encoding="utf-8"))


@pytest.fixture(scope="module")
def whole(corpus):
    import gsearch_amd as G

    class B:
        pass
    b = B()
    b.dir = os.path.join(corpus.root, "whole")
    b.report = G.tohnsw(corpus.db, b.dir, K, S, NBNG, **BUILD)
    b.res, b.neighbors, b.matches = _request("whole", G.request, b.dir, corpus)
    b.listed = [p for p, _, _ in _dict(b.dir)]
    assert [os.path.relpath(p, corpus.db) for p in b.listed] == sorted(corpus.rel) and b.report["nb_file"] == 25
    return b


def _build_split(corpus, tag, **kw):
    import gsearch_amd as G
    d = os.path.join(corpus.root, tag)
    args = dict(BUILD)
    args.update(kw)
    return d, G.tohnsw_split(corpus.db, d, K, S, NBNG, **args)


@pytest.fixture(scope="module")
def random_splits(corpus):
    return {n: _build_split(corpus, "random_%d" % n, pieces=n, files_per_round=7) for n in (2, 5)}


@pytest.fixture(scope="module")
def by_roots(corpus):
    return _build_split(corpus, "by_roots", mode="medoid", medoids=corpus.root_paths)


# ---- (a) one piece is tohnsw ---------------------------------------------------------------------------------------------------------------------------
def test_one_piece_is_byte_for_byte_what_tohnsw_and_request_write(corpus, whole):
    import gsearch_amd as G
    from gsearch_amd.state import ProcessingParams, ProcessingState
    d, rep = _build_split(corpus, "random_1", pieces=1, files_per_round=10)
    assert sorted(os.listdir(d)) == ["part_000", "split.json"]                                      # the spill file is gone
    assert _digest(os.path.join(d, "part_000")) == _digest(whole.dir) and len(_digest(whole.dir)) == 5
    a, b = ProcessingState.reload_json(os.path.join(d, "part_000")), ProcessingState.reload_json(whole.dir)
    assert (a.nb_seq, a.nb_file) == (b.nb_seq, b.nb_file) == (24, 25)
    assert [os.path.basename(p) for p in rep["skipped_files"]] == ["only_n.fna"] and rep["nb_point"] == 24 and rep["pieces"][0]["nb_point"] == 24
    o = _split_json(d)
    assert o["mode"] == "random" and o["router"] is None and o["pieces"] == [{"dir": "part_000", "medoid": None}]
    assert open(os.path.join(d, "split.json"), encoding="utf-8").read() == G.split_json_text("random", SEED, ProcessingParams.reload_json(whole.dir),
                                                                                              [("part_000", None)], [], None)
    res, neighbors, matches = _request("one", G.request_split, d, corpus)
    assert neighbors == whole.neighbors and matches == whole.matches
    assert np.array_equal(res["ids"], whole.res["ids"]) and np.array_equal(res["distances"].view(np.uint32), whole.res["distances"].view(np.uint32))
    assert np.array_equal(res["counts"], whole.res["counts"]) and np.array_equal(res["evals"], whole.res["evals"]) and res["items"] == whole.res["items"]
    assert set(whole.res) <= set(res) and res["pieces"][0]["rows"] == 4 and set(res["pieces"][0]["seconds"]) == {"load", "search_merge"}


# ---- (b), (c) random pieces ---------------------------------------------------------------------------------------------------------------------------
def _merge_of_requests(corpus, dirs, tag):
    """the restatement's merge of what `request` answers on every piece, with the offsets of the pieces' own dictionaries"""
    import gsearch_amd as G
    run, lengths, per_piece = RS.empty_lists(4, KNBN), [len(_dict(d)) for d in dirs], []
    for p, d in enumerate(dirs):
        res, _, _ = _request("%s_piece%d" % (tag, p), G.request, d, corpus)                          # every piece is a database request accepts
        per_piece.append(res)
        run = RS.merge_rows(run, (res["ids"], res["distances"], res["counts"], res["evals"]), None, RS.offsets(lengths)[p])
    return run, [it for d in dirs for it in _dict(d)], per_piece


@pytest.mark.parametrize("pieces", [2, 5])
def test_random_pieces_answer_as_the_merge_of_their_own_requests(corpus, whole, random_splits, pieces):
    import gsearch_amd as G
    d, rep = random_splits[pieces]
    o = _split_json(d)
    dirs = [os.path.join(d, p["dir"]) for p in o["pieces"]]
    assert [p["dir"] for p in o["pieces"]] == ["part_%03d" % i for i in range(pieces)] and len(rep["pieces"]) == pieces
    parts = RS.random_assignment(24, pieces, SEED)
    assert [[p for p, _, _ in _dict(x)] for x in dirs] == [[whole.listed[i] for i in part] for part in parts]       # a partition of the files, list order inside
    assert pieces != 5 or min(len(p) for p in parts) < KNBN                                          # pieces smaller than nbanswers
    (ids, dist, cnt, ev), seqdict, _ = _merge_of_requests(corpus, dirs, "random_%d" % pieces)
    res, neighbors, matches = _request("split_%d" % pieces, G.request_split, d, corpus)
    assert np.array_equal(res["ids"], ids) and np.array_equal(res["distances"].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(res["counts"], cnt) and np.array_equal(res["evals"], ev)
    assert neighbors == _text(res["items"], seqdict, ids, dist, cnt) and res["items"] == whole.res["items"]
    assert [r["rows"] for r in res["pieces"]] == [4] * pieces and [r["id_offset"] for r in res["pieces"]] == RS.offsets([len(p) for p in parts])
    assert all(r["loaded"] for r in res["pieces"]) and res["probe"] is None
    # (c) the same directories as a list of databases built separately
    res2, neighbors2, matches2 = _request("list_%d" % pieces, G.request_split, dirs, corpus)
    assert neighbors2 == neighbors and matches2 == matches and np.array_equal(res2["ids"], ids)
    with pytest.raises(G.GsError) as e:
        G.request_split(dirs, corpus.queries, KNBN, probe=1, out=os.path.join(corpus.root, "never.txt"))
    assert e.value.code == G._lib.GS_ERR_INVALID and not os.path.exists(os.path.join(corpus.root, "never.txt"))


# ---- (d) medoids given by the caller -------------------------------------------------------------------------------------------------------------------
def _family(path):
    return int(os.path.basename(path)[1])


def test_medoids_given_as_the_family_roots(corpus, whole, by_roots):
    import gsearch_amd as G
    d, rep = by_roots
    o = _split_json(d)
    assert o["mode"] == "medoid" and o["router"] == "router" and o["medoids"] == corpus.root_paths and [p["medoid"] for p in o["pieces"]] == [0, 1, 2, 3]
    for p in o["pieces"]:                                                                            # every genome lies in its root's piece
        fams = {_family(path) for path, _, _ in _dict(os.path.join(d, p["dir"]))}
        assert fams == {p["medoid"]}
    assert [len(_dict(os.path.join(d, p["dir"]))) for p in o["pieces"]] == list(FAMILIES)
    assert [p for p, _, _ in _dict(os.path.join(d, "router"))] == corpus.root_paths
    res, neighbors, _ = _request("router_as_db", G.request, os.path.join(d, "router"), corpus)       # the router is an ordinary database
    assert res["ids"][:, 0].tolist() == [0, 1, 2, 3]
    res, neighbors, matches = _request("probe1", G.request_split, d, corpus, probe=1)
    seqdict = [it for p in o["pieces"] for it in _dict(os.path.join(d, p["dir"]))]
    for q in range(4):                                                                               # every mutant's first answer is its parent
        assert seqdict[int(res["ids"][q, 0])][0] == corpus.root_paths[q]
    assert [r["rows"] for r in res["pieces"]] == [1, 1, 1, 1] and res["probe"] == 1
    only = os.path.join(corpus.root, "one_query")                                                    # one query: only its piece is loaded
    shutil.copytree(corpus.queries, only)
    for f in (0, 1, 3):
        os.remove(os.path.join(only, "q%d.fna" % f))
    out = os.path.join(corpus.root, "one_query.txt")
    res = G.request_split(d, only, KNBN, probe=1, out=out, matches=out + ".matches", ef=EF_REQ)
    assert [(r["rows"], r["loaded"]) for r in res["pieces"]] == [(0, False), (0, False), (1, True), (0, False)] and res["index_source"] == ["hnswdump.gsidx"]
    assert all(_family(seqdict[int(i)][0]) == 2 for i in res["ids"][0, :int(res["counts"][0])])
    full, n_full, m_full = _request("probe4", G.request_split, d, corpus, probe=4)
    plain, n_plain, m_plain = _request("probe_none", G.request_split, d, corpus)
    assert n_full == n_plain and m_full == m_plain and full["probe"] is None and [r["rows"] for r in full["pieces"]] == [4] * 4
    for bad in (0, 5):
        with pytest.raises(G.GsError) as e:
            G.request_split(d, corpus.queries, KNBN, probe=bad, out=os.path.join(corpus.root, "never.txt"))
        assert e.value.code == G._lib.GS_ERR_INVALID and not os.path.exists(os.path.join(corpus.root, "never.txt"))


# ---- (e) a family cut at max_piece ---------------------------------------------------------------------------------------------------------------------
def test_a_family_of_nine_cut_at_four_is_three_pieces_on_one_medoid(corpus, whole):
    import gsearch_amd as G
    d, rep = _build_split(corpus, "by_roots_cut", mode="medoid", medoids=corpus.root_paths, max_piece=4)
    o = _split_json(d)
    assert [p["medoid"] for p in o["pieces"]] == [0, 0, 0, 1, 1, 2, 2, 3, 3]
    sizes = [len(_dict(os.path.join(d, p["dir"]))) for p in o["pieces"]]
    assert sizes == [3, 3, 3, 3, 2, 3, 2, 3, 2]
    fam0 = [p for x in o["pieces"][:3] for p, _, _ in _dict(os.path.join(d, x["dir"]))]
    assert fam0 == [p for p in whole.listed if _family(p) == 0]                                       # list order, cut in runs
    res, neighbors, _ = _request("cut_probe1", G.request_split, d, corpus, probe=1)
    assert [r["rows"] for r in res["pieces"]] == [1] * 9 and all(r["loaded"] for r in res["pieces"])
    seqdict = [it for p in o["pieces"] for it in _dict(os.path.join(d, p["dir"]))]
    got = [seqdict[int(i)][0] for i in res["ids"][0, :int(res["counts"][0])]]
    assert len({p for p in got if _family(p) == 0}) == KNBN and len({fam0.index(p) // 3 for p in got}) > 1   # family 0's answers come from more than one of its pieces


# ---- (f) medoids found by clustering -------------------------------------------------------------------------------------------------------------------
def test_n_medoids_names_them_by_clustering_and_sends_every_genome_to_the_nearest(corpus, whole):
    import gsearch_amd as G
    k = 4
    d, rep = _build_split(corpus, "clustered", mode="medoid", n_medoids=k, files_per_round=10)
    o = _split_json(d)
    router = os.path.join(d, "router")
    assert len(o["medoids"]) == k and [p for p, _, _ in _dict(router)] == o["medoids"] and set(o["medoids"]) <= set(whole.listed)
    res, _, _ = _request("clustered_router", G.request, router, corpus)                              # a database of k points
    assert res["ids"].shape == (4, KNBN) and int(res["counts"].max()) <= k
    full = G.Hnsw.load(os.path.join(whole.dir, "hnswdump.gsidx"))
    rt = G.Hnsw.load(os.path.join(router, "hnswdump.gsidx"))
    try:
        assert rt.get_nb_point() == k
        assign = RS.medoid_argmin(rt.count_matrix(full.get_data()))
    finally:
        full.close()
        rt.close()
    want = RS.cut_pieces(assign, k, None)
    assert [p["medoid"] for p in o["pieces"]] == [j for j, _ in want]
    assert [[p for p, _, _ in _dict(os.path.join(d, x["dir"]))] for x in o["pieces"]] == [[whole.listed[i] for i in files] for _, files in want]
    res, neighbors, _ = _request("clustered_probe2", G.request_split, d, corpus, probe=2)
    assert res["probe"] == 2 and neighbors


# ---- (g) add to one piece ------------------------------------------------------------------------------------------------------------------------------
def test_add_to_one_piece_shifts_the_ids_of_the_pieces_behind_it(corpus, random_splits):
    import gsearch_amd as G
    src, _ = random_splits[2]
    d = os.path.join(corpus.root, "random_2_grown")
    shutil.copytree(src, d)
    new = os.path.join(corpus.root, "new_genomes")
    os.makedirs(new)
    shutil.copyfile(os.path.join(corpus.queries, "q1.fna"), os.path.join(new, "exactly_q1.fna"))
    rep = G.add(os.path.join(d, "part_000"), new)
    assert (rep["first_id"], rep["nb_point_total"]) == (12, 13)
    dirs = [os.path.join(d, "part_000"), os.path.join(d, "part_001")]
    (ids, dist, cnt, ev), seqdict, _ = _merge_of_requests(corpus, dirs, "grown")
    res, neighbors, _ = _request("grown", G.request_split, d, corpus)
    assert [r["id_offset"] for r in res["pieces"]] == [0, 13]
    assert int(res["ids"][1, 0]) == 12 and res["distances"][1, 0] == 0 and seqdict[12][0] == os.path.join(new, "exactly_q1.fna")
    assert np.array_equal(res["ids"], ids) and np.array_equal(res["counts"], cnt) and neighbors == _text(res["items"], seqdict, ids, dist, cnt)
    assert int(res["ids"].max()) >= 13 and b"exactly_q1.fna" in neighbors


# ---- (h), (i) refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_pieces_whose_parameters_disagree_are_refused_before_anything_is_written(corpus, random_splits):
    import gsearch_amd as G
    src, _ = random_splits[2]
    d = os.path.join(corpus.root, "random_2_edited")
    shutil.copytree(src, d)
    p = os.path.join(d, "part_001", "parameters.json")
    text = open(p).read()
    assert '"kmer_size":%d' % K in text
    open(p, "w").write(text.replace('"kmer_size":%d' % K, '"kmer_size":%d' % (K - 2)))
    out, mt = os.path.join(corpus.root, "refused.txt"), os.path.join(corpus.root, "refused.matches")
    for db in (d, [os.path.join(d, "part_000"), os.path.join(d, "part_001")]):
        with pytest.raises(G.GsError) as e:
            G.request_split(db, corpus.queries, KNBN, out=out, matches=mt, ef=EF_REQ)
        assert e.value.code == G._lib.GS_ERR_INVALID and not os.path.exists(out) and not os.path.exists(mt)


def test_universal_is_unsupported(corpus, random_splits):
    import gsearch_amd as G
    d, _ = random_splits[2]
    out = os.path.join(corpus.root, "universal_out")
    with pytest.raises(G.GsError) as e:
        G.tohnsw_split(corpus.db, out, K, S, NBNG, pieces=2, universal="profiles.hmm", **BUILD)
    assert e.value.code == G._lib.GS_ERR_UNSUPPORTED and not os.path.exists(out)
    with pytest.raises(G.GsError) as e:
        G.request_split(d, corpus.queries, KNBN, universal="profiles.hmm", out=os.path.join(corpus.root, "never.txt"))
    assert e.value.code == G._lib.GS_ERR_UNSUPPORTED and not os.path.exists(os.path.join(corpus.root, "never.txt"))
