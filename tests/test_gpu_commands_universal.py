"""tohnsw / add / request with `universal` (SPEC 17 item 11): a universal-gene database built on the device from a directory of nucleotide files. The expected
signatures are the host composition's - sketch_genomes(universal_genes(...)) -, the dictionary names the kept files with the residues sketched, the file
without a hit is skipped, universal.json holds the profile names, add continues the ids, a 1 % mutant of a database genome finds its parent first, and
the refusals of SPEC 17 item 11 carry their codes. Genomes: tests/universal_case.py, every planted gene the consensus with 15 % of its residues replaced, so
that the database genomes differ from one another."""
import json
import os

import numpy as np
import pytest

import pyref_hmm as RH
import universal_case as U

pytestmark = pytest.mark.gpu
K, S, NBNG, EFC = 5, 256, 8, 64


class _World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory, gpu_ctx):
    import gsearch_amd as G
    w = _World()
    w.root = str(tmp_path_factory.mktemp("commands_universal"))
    w.profiles = U.profile_paths()
    w.names = [m["name"] for m in U.models()]
    cons = [RH.consensus(m["tables"]) for m in U.models()]
    w.src, w.more, w.query = (os.path.join(w.root, n) for n in ("src", "more", "query"))
    for d in (w.src, w.more, w.query):
        os.makedirs(d)
    w.genomes = [U.genome(60 + g, cons, (0, 1), fraction=0.15) for g in range(7)]
    w.paths = []
    for g, (contigs, proteins, _) in enumerate(w.genomes):
        w.paths.append(U.write_genome(w.src if g < 5 else w.more, "a%d" % g, contigs, proteins, forms=("fna",))["fna"])
    contigs, proteins, _ = U.genome(70, cons, (), fraction=0.0)
    w.nohit = U.write_genome(w.src, "nohit", contigs, proteins, forms=("fna",))["fna"]
    w.mutant = U.write_genome(w.query, "mutant_of_a2", U.mutate(9, w.genomes[2][0], 0.01), [], forms=("fna",))["fna"]
    w.sk = G.sketcher_for(G.SeqSketcherParams(K, S, "optdens", "aa"), gpu_ctx)
    w.lists = G.universal_genes(w.paths + [w.nohit, w.mutant], w.profiles, ctx=gpu_ctx, translate="genes")[0]
    assert [len(g) for g in w.lists] == [2] * 7 + [0, 2]
    w.sig = w.sk.sketch_genomes(w.lists[:7] + w.lists[8:])                   # rows 0..6 the database genomes, row 7 the mutant
    w.residues = [sum(len(r) for r in g) for g in w.lists]
    w.db = os.path.join(w.root, "database")
    w.report = G.tohnsw(w.src, w.db, K, S, NBNG, ef=EFC, aa=True, seed=3, universal=w.profiles, translate="genes", ctx=gpu_ctx)
    return w


def _data(G, d):
    hn = G.Hnsw.load(os.path.join(d, "hnswdump.gsidx"))
    try:
        return hn.get_ids(), hn.get_data()
    finally:
        hn.close()


def _seqdict(d):
    from gsearch_amd.state import SeqDict
    return [(os.path.basename(p), f, n) for p, f, n in SeqDict.reload_json(os.path.join(d, "seqdict.json")).items]


def test_tohnsw_builds_the_universal_database(world):
    import gsearch_amd as G
    from gsearch_amd.state import ProcessingState
    rep = world.report
    assert (rep["nb_file"], rep["nb_point"], rep["nb_record"]) == (6, 5, 10) and [os.path.basename(p) for p in rep["skipped_files"]] == ["nohit.fna"]
    ids, data = _data(G, world.db)
    assert np.array_equal(ids, np.arange(5, dtype=np.uint64)) and np.array_equal(data.view(np.uint8), np.ascontiguousarray(world.sig[:5]).view(np.uint8))
    assert _seqdict(world.db) == [("a%d.fna" % g, "", world.residues[g]) for g in range(5)]
    side = json.load(open(os.path.join(world.db, "universal.json")))
    assert side["profiles"] == world.names and side["options"]["translate"] == "genes"
    st = ProcessingState.reload_json(world.db)
    assert (st.nb_seq, st.nb_file) == (10, 6)                                # nb_seq counts hits
    assert sorted(os.listdir(world.db)) == sorted(["parameters.json", "seqdict.json", "processing_state.json", "hnswdump.gsidx", "hnswdump.hnsw.graph",
                                                   "hnswdump.hnsw.data", "universal.json"])
    assert set(rep["sketch_stats"]["stage_s"]) == set(G.UNIVERSAL_STAGES)


def test_add_continues_the_ids_and_request_finds_the_parent(world, gpu_ctx):
    import shutil
    import gsearch_amd as G
    d = os.path.join(world.root, "database_added")
    shutil.copytree(world.db, d)
    rep = G.add(d, world.more, universal=G.HmmDb(world.profiles, gpu_ctx), translate="genes", ctx=gpu_ctx)
    assert (rep["first_id"], rep["nb_point"], rep["nb_point_total"]) == (5, 2, 7)
    ids, data = _data(G, d)
    assert np.array_equal(ids, np.arange(7, dtype=np.uint64)) and np.array_equal(data.view(np.uint8), np.ascontiguousarray(world.sig[:7]).view(np.uint8))
    assert _seqdict(d) == [("a%d.fna" % g, "", world.residues[g]) for g in range(7)]
    assert json.load(open(os.path.join(d, "universal.json")))["profiles"] == world.names
    out, matches = os.path.join(world.root, "neighbors.txt"), os.path.join(world.root, "matches.txt")
    res = G.request(d, world.query, 3, out=out, matches=matches, ef=64, universal=world.profiles, translate="genes", ctx=gpu_ctx)
    assert int(res["ids"][0, 0]) == 2 and res["distances"][0, 0] < res["distances"][0, 1], (res["ids"], res["distances"])
    assert [(os.path.basename(p), f, n) for p, f, n in res["items"]] == [("mutant_of_a2.fna", "", world.residues[8])] and "a2.fna" in open(out).read()


def test_refusals(world, gpu_ctx):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_UNSUPPORTED
    new = os.path.join(world.root, "refused")

    def code(call, *a, **kw):
        with pytest.raises(G.GsError) as e:
            call(*a, ctx=gpu_ctx, **kw)
        return e.value.code
    assert code(G.tohnsw, world.src, new, 16, S, NBNG, universal=world.profiles, translate="genes") == GS_ERR_INVALID             # no AA database
    assert code(G.tohnsw, world.src, new, K, S, NBNG, aa=True, block=True, universal=world.profiles, translate="genes") == GS_ERR_UNSUPPORTED
    assert code(G.tohnsw, world.src, new, K, S, NBNG, aa=True, translate=True) == GS_ERR_INVALID                                  # ORFs only feed universal
    assert code(G.tohnsw, world.src, new, K, S, NBNG, aa=True, universal=world.profiles, translate="genes", universal_opts={"ctx": None}) == GS_ERR_INVALID
    assert not os.path.exists(new)
    before = sorted((n, os.path.getsize(os.path.join(world.db, n))) for n in os.listdir(world.db))
    for call, arg in ((G.add, world.more), (G.request, world.query)):
        extra = {"nbanswers": 3, "out": os.path.join(world.root, "r.txt"), "matches": os.path.join(world.root, "m.txt")} if call is G.request else {}
        assert code(call, world.db, arg, translate="genes", **extra) == GS_ERR_INVALID                                           # a sidecar directory, no universal
        assert code(call, world.db, arg, translate="genes", universal=world.profiles[:1], **extra) == GS_ERR_INVALID             # other profiles
        assert code(call, world.db, arg, translate="genes", universal=world.profiles[::-1], **extra) == GS_ERR_INVALID           # another order
    assert sorted((n, os.path.getsize(os.path.join(world.db, n))) for n in os.listdir(world.db)) == before


def test_files_of_extracted_genes(world, gpu_ctx):
    """universal=False: the files hold the universal genes already and are sketched as plain protein FASTA - against a universal-gene database, and as
    the source of a database, which then has no sidecar"""
    import gsearch_amd as G
    faa, q = os.path.join(world.root, "extracted"), os.path.join(world.root, "extracted_query")
    os.makedirs(faa)
    os.makedirs(q)
    for g in range(5):
        U.write_fasta(os.path.join(faa, "a%d.faa" % g), ["u%d" % i for i in range(len(world.lists[g]))], world.lists[g])
    U.write_fasta(os.path.join(q, "mutant_of_a2.faa"), ["u0", "u1"], world.lists[8])
    out, matches = os.path.join(world.root, "n2.txt"), os.path.join(world.root, "m2.txt")
    res = G.request(world.db, q, 3, out=out, matches=matches, ef=64, universal=False, ctx=gpu_ctx)
    assert int(res["ids"][0, 0]) == 2 and res["items"][0][2] == world.residues[8]
    d = os.path.join(world.root, "database_extracted")
    rep = G.tohnsw(faa, d, K, S, NBNG, ef=EFC, aa=True, seed=3, universal=False, ctx=gpu_ctx)
    assert rep["nb_point"] == 5 and not os.path.exists(os.path.join(d, "universal.json"))
    assert np.array_equal(_data(G, d)[1].view(np.uint8), np.ascontiguousarray(world.sig[:5]).view(np.uint8))
    # such a database takes raw genomes through the profiles too: nothing forbids it, there is no sidecar to hold it to
    res = G.request(d, world.query, 3, out=out, matches=matches, ef=64, universal=world.profiles, translate="genes", ctx=gpu_ctx)
    assert int(res["ids"][0, 0]) == 2
