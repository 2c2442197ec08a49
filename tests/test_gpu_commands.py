"""tohnsw / add / request / reformat on directories of files (gsearch_amd/commands.py, SPEC 17) against the CPU oracle on the same files.

The yardstick is never the commands: the test parses the FASTA files itself, sketches the kept records with oracle_lib.sketch_batch, builds the graph with
oracle_lib.Index.parallel_insert and answers with its parallel_search; the expected texts come from ReqAnswer.dump (held to a literal by
test_answer_format.py) and from a restatement of matcher.rs in this file.

Database folder: 12 genomes = 3 random roots x 4 mutants, 20 kbp each in 2-3 records, written as .fna / .fa.gz / .fasta over two nested sub-folders; one
of them also holds a `capsid` record; next to them a file of N's only, a file of `capsid` records only, an empty .fna and a notes.txt. Query folder: one
further mutant of each root, one unrelated genome, one file of N's only (in the middle of the name order). k = 21, s = 512, optdens, nbng = 8, ef = 64."""
import gzip
import hashlib
import io
import json
import os
import shutil

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

K, S, NBNG, EFC, SEED, BATCH = 21, 512, 8, 64, 11, 64
KNBN, EF_REQ = 5, 64
THR = float(np.float32(0.99))
LEN = 20000
MUS = (0.002, 0.01, 0.03, 0.06)
SUFFIXES = (".fna", ".fa", ".fasta", ".fna.gz", ".fa.gz", ".fasta.gz")


# ---- files, written and parsed by the test ----------------------------------------------------------------------------------------------------------
def _fasta(records, width=70):
    out = []
    for name, s in records:
        out.append(b">" + name + b"\n")
        out += [s[o:o + width] + b"\n" for o in range(0, len(s), width)]
    return b"".join(out)


def _write(path, blob):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(gzip.compress(blob, 6) if str(path).endswith(".gz") else blob)


def _read(path):
    blob = open(path, "rb").read()
    return gzip.decompress(blob) if str(path).endswith(".gz") else blob


def _kept_records(text):
    """the records the reader keeps (dnafiles.rs:53-86): not `capsid` in the header line, a sequence that is not empty"""
    recs = []
    for chunk in text.split(b">")[1:]:
        head, _, body = chunk.partition(b"\n")
        seq = body.replace(b"\n", b"").replace(b"\r", b"")
        if b"capsid" not in head and len(seq):
            recs.append(seq)
    return recs


def _walk(root):
    """files of a folder in name order, then its sub-folders in name order (SPEC 17)"""
    names = sorted(os.listdir(root))
    out = [os.path.join(root, n) for n in names if os.path.isfile(os.path.join(root, n)) and n.endswith(SUFFIXES)]
    for n in names:
        if os.path.isdir(os.path.join(root, n)):
            out += _walk(os.path.join(root, n))
    return out


def _split(rng, s, parts):
    cuts = sorted(int(c) for c in rng.choice(np.arange(2000, len(s) - 2000), parts - 1, replace=False))
    return [s[a:b] for a, b in zip([0] + cuts, cuts + [len(s)])]


REL = ["g00.fna", "g01.fa.gz", "g02.fasta", "g03.fna",
       "sub_a/g10.fa.gz", "sub_a/g11.fasta", "sub_a/g12.fna", "sub_a/inner/g13.fa.gz",
       "sub_a/inner/g20.fasta", "sub_b/g21.fna", "sub_b/g22.fa.gz", "sub_b/g23.fasta"]
EXTRA = {"a_only_n.fna": _fasta([(b"nothing", b"N" * 3000)]), "sub_a/capsid_only.fna": _fasta([(b"c1 capsid protein", b"ACGT" * 200), (b"c2 major capsid", b"GGCA" * 100)]),
         "sub_b/empty.fna": b"", "notes.txt": b">not a genome\nACGT\n"}


class Corpus:
    def __init__(self, root):
        rng = np.random.default_rng(2024)
        self.root = str(root)
        self.db, self.queries = os.path.join(self.root, "db"), os.path.join(self.root, "queries")
        roots = [H.rand_dna(rng, LEN) for _ in range(3)]
        self.texts = {}
        for gi, rel in enumerate(REL):
            s = H.dna_ascii(H.mutate(rng, roots[gi // 4], MUS[gi % 4]))
            recs = _split(rng, s, 2 + gi % 2)
            if gi == 2:
                recs[0] = recs[0][:500] + b"NNNNNNnn" + recs[0][500:900].lower() + recs[0][900:]
            named = [(b"ctg%d of genome %d" % (i, gi), r) for i, r in enumerate(recs)]
            if gi == 5:
                named.insert(1, (b"phage capsid gene", H.dna_ascii(H.rand_dna(rng, 1500))))
            self.texts[rel] = _fasta(named, 60 + gi)
        self.texts.update(EXTRA)
        for rel, t in self.texts.items():
            _write(os.path.join(self.db, rel), t)
        q = {"q_a_root0.fna": roots[0], "q_c_root1.fa.gz": roots[1], "q_e_root2.fasta": roots[2]}
        self.qtexts = {n: _fasta([(b"q", H.dna_ascii(H.mutate(rng, r, 0.02))[:12000]), (b"q2", H.dna_ascii(H.mutate(rng, r, 0.02))[12000:])]) for n, r in q.items()}
        self.qtexts["q_d_unrelated.fna"] = _fasta([(b"u", H.dna_ascii(H.rand_dna(rng, LEN)))])
        self.qtexts["q_b_only_n.fna"] = _fasta([(b"n", b"n" * 500 + b"N" * 500)])
        for n, t in self.qtexts.items():
            _write(os.path.join(self.queries, n), t)

    def subset(self, name, rels):
        """the same files under another root, layout kept"""
        dst = os.path.join(self.root, name)
        for rel in rels:
            os.makedirs(os.path.dirname(os.path.join(dst, rel)), exist_ok=True)
            shutil.copyfile(os.path.join(self.db, rel), os.path.join(dst, rel))
        return dst


def _oracle_sigs(genomes, k=K, m=S, algo="optdens", data="dna"):
    recs = [r for g in genomes for r in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    seq, rs, rl = O.pack_dna(recs) if data == "dna" else O.filter_aa(recs)
    sig = O.sketch_batch(O.params(k, m, algo, data), seq, rs, rl, goff, nthreads=min(8, os.cpu_count() or 1))
    nsym = np.array([int(rl[goff[i]:goff[i + 1]].sum()) for i in range(len(genomes))], np.int64)
    return sig, nsym


class Folder:
    """what the oracle makes of a folder: the files in name order, those with a symbol to sketch, their signatures by sequence and with block"""

    def __init__(self, root):
        self.listed = _walk(root)
        recs = [_kept_records(_read(p)) for p in self.listed]
        sig, nsym = _oracle_sigs([r if r else [b""] for r in recs])
        self.keep = [i for i in range(len(self.listed)) if nsym[i] > 0]
        self.paths = [self.listed[i] for i in self.keep]
        self.recs = [recs[i] for i in self.keep]
        self.sig, self.nsym = sig[self.keep], nsym[self.keep]
        self.block_sig, block_nsym = _oracle_sigs([[b"".join(r)] for r in self.recs])
        assert np.array_equal(block_nsym, self.nsym)
        self.nb_seq = sum(len(r) for r in self.recs)

    def items(self, fasta_id=""):
        return [(p, fasta_id, int(n)) for p, n in zip(self.paths, self.nsym)]


def _oracle_index(parts, m=S, M=NBNG, efc=EFC, seed=SEED, batch=BATCH, dtype=np.float32):
    oix = O.Index(dtype, m, M, efc, max_layer=16, scale_modify=1.0, extend_candidates=True, keep_pruned=False, seed=seed)
    for p in parts:
        oix.parallel_insert(p, batch=batch)
    return oix


def _same_graph(g, og):
    """adjacency beyond a node's degree is unspecified: both sides are cut at the oracle's degrees"""
    def cut(a, deg):
        a = np.asarray(a)
        return np.where(np.arange(a.shape[-1]) < np.asarray(og[deg])[..., None], a, 0)
    assert g["entry"] == og["entry"] and g["n_upper"] == og["n_upper"]
    for key in ("levels", "upidx", "deg0"):
        assert np.array_equal(g[key], og[key]), key
    assert np.array_equal(cut(g["nbr0"], "deg0"), cut(og["nbr0"], "deg0")) and np.array_equal(cut(g["cnt0"], "deg0"), cut(og["cnt0"], "deg0"))
    if og["n_upper"]:
        assert np.array_equal(g["degU"], og["degU"]) and np.array_equal(cut(g["nbrU"], "degU"), cut(og["nbrU"], "degU"))


def _neighbors_text(items, seqdict, ids, dist, cnt):
    import gsearch_amd as G
    buf = io.StringIO()
    for i, item in enumerate(items):
        G.ReqAnswer(i, item, [G.Neighbour(int(ids[i, j]), float(dist[i, j])) for j in range(int(cnt[i]))]).dump(seqdict, THR, buf)
    return buf.getvalue()


def _matches_rule(items, seqdict, ids, dist, cnt):
    """matcher.rs:86-94,110-122,262-275 restated: targets by database path, merit = f64 product of the distances < 0.99 as f32, ascending, ties and request
    genomes in order of appearance (SPEC 17), five lines at the most, `{:.3E}` = %.3E without `+` and exponent padding"""
    out = ""
    for i, item in enumerate(items):
        merit, order = {}, []
        for j in range(int(cnt[i])):
            path = seqdict[int(ids[i, j])][0]
            if path not in merit:
                merit[path] = 1.0
                order.append(path)
            if np.float32(dist[i, j]) < np.float32(0.99):
                merit[path] *= float(np.float32(dist[i, j]))
        out += "\n\n request genome : %s" % item[0]
        for path in sorted(order, key=lambda p: float(np.float32(merit[p])))[:5]:
            mant, exp = ("%.3E" % float(np.float32(merit[path]))).split("E")
            out += "\n\t matched genome %s  merit : %sE%d" % (path, mant, int(exp))
    return out


def _dir_digest(d):
    return {n: hashlib.sha256(open(os.path.join(d, n), "rb").read()).hexdigest() for n in sorted(os.listdir(d))}


def _seqdict_bytes(items):
    """seqdict.json as serde_json writes it: the objects back to back, no separator (idsketch.rs:186-189)"""
    return "".join('{"id":{"path":%s,"fasta_id":%s},"len":%d}' % (json.dumps(path), json.dumps(fid), n) for path, fid, n in items).encode()


# ---- one corpus, one reference and one tohnsw + request for the module -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return Corpus(tmp_path_factory.mktemp("commands"))


@pytest.fixture(scope="module")
def ref(corpus):
    class R:
        pass
    r = R()
    r.db, r.q = Folder(corpus.db), Folder(corpus.queries)
    assert len(r.db.listed) == 15 and len(r.db.paths) == 12 and len(r.q.listed) == 5 and len(r.q.paths) == 4
    assert [os.path.relpath(p, corpus.db) for p in r.db.paths] == REL                 # name order: a folder's files, then its sub-folders
    r.oix = _oracle_index([r.db.sig])
    r.answers = r.oix.parallel_search(r.q.sig, KNBN, EF_REQ)[:3]
    return r


def _tohnsw(corpus, src, out, **kw):
    import gsearch_amd as G
    args = dict(ef=EFC, algo="optdens", seed=SEED, insert_batch=BATCH)
    args.update(kw)
    return G.tohnsw(src, out, K, S, NBNG, **args)


def _request(corpus, db_dir, tag, **kw):
    import gsearch_amd as G
    out, mt = os.path.join(corpus.root, tag + ".neighbors.txt"), os.path.join(corpus.root, tag + ".matches")
    for p in (out, mt):
        if os.path.exists(p):
            os.remove(p)
    res = G.request(db_dir, kw.pop("query_dir", corpus.queries), KNBN, out=out, matches=mt, ef=EF_REQ, **kw)
    return res, open(out, "rb").read(), (open(mt, "rb").read() if os.path.exists(mt) else None)


@pytest.fixture(scope="module")
def built(corpus, gpu_ctx):
    class B:
        pass
    b = B()
    b.dir = os.path.join(corpus.root, "database")
    b.report = _tohnsw(corpus, corpus.db, b.dir)
    b.request, b.neighbors, b.matches = _request(corpus, b.dir, "first")
    return b


# ---- tohnsw ------------------------------------------------------------------------------------------------------------------------------------------
def test_tohnsw_writes_the_directory_the_oracle_describes(corpus, ref, built):
    import gsearch_amd as G
    from gsearch_amd.state import HnswParams, ProcessingParams, ProcessingState
    d = built.dir
    assert open(os.path.join(d, "seqdict.json"), "rb").read() == _seqdict_bytes(ref.db.items())
    assert open(os.path.join(d, "parameters.json")).read() == ProcessingParams(HnswParams(1_500_000, EFC, NBNG, 1.0), K, S, "optdens", "dna", False).to_json()
    st = ProcessingState.reload_json(d)
    assert (st.nb_file, st.nb_seq) == (15, ref.db.nb_seq) and st.elapsed_t > 0
    rep = built.report
    assert (rep["nb_file"], rep["nb_point"], rep["nb_record"]) == (15, 12, ref.db.nb_seq) and rep["hnswrs_written"] is True and rep["hnswrs_refused"] is None
    assert sorted(os.path.relpath(p, corpus.db) for p in rep["skipped_files"]) == ["a_only_n.fna", "sub_a/capsid_only.fna", "sub_b/empty.fna"]
    assert set(rep["seconds"]) == {"list", "read_sketch", "insert", "dump", "wall"} and "wall_s" in rep["sketch_stats"]
    assert sorted(os.listdir(d)) == ["hnswdump.gsidx", "hnswdump.hnsw.data", "hnswdump.hnsw.graph", "parameters.json", "processing_state.json", "seqdict.json"]
    hn = G.Hnsw.load(os.path.join(d, "hnswdump.gsidx"))
    try:
        assert np.array_equal(hn.get_data().view(np.uint32), ref.db.sig.view(np.uint32))
        assert np.array_equal(hn.get_ids(), np.arange(12, dtype=np.uint64))
        assert (hn.prm.capacity, hn.prm.max_layer, hn.prm.extend_candidates, hn.prm.keep_pruned) == (1_500_000, 16, 1, 0)
        _same_graph(hn.export_graph(), ref.oix.export())
    finally:
        hn.close()


# ---- request -----------------------------------------------------------------------------------------------------------------------------------------
def test_request_texts_equal_the_oracles_answers(corpus, ref, built):
    ids, dist, cnt = ref.answers
    items, seqdict = ref.q.items(), ref.db.items()
    assert [os.path.basename(it[0]) for it in items] == ["q_a_root0.fna", "q_c_root1.fa.gz", "q_d_unrelated.fna", "q_e_root2.fasta"]   # the N-only file shifts no rank
    # the case is what it claims, on the oracle's distances: the unrelated genome has no answer under 0.99, the mutants of roots 0 and 2 have close ones.
    # The roots share no k-mer, so the graph has no edge of a distance under 1 between the families and a search that enters in one may end there: the
    # mutant of root 1 does (all its answers are at 1.0), and a search returns the 4 members of a family, fewer than the 5 asked for
    assert (dist[2] >= np.float32(0.99)).all() and (dist[[0, 3], 0] < np.float32(0.7)).all() and int(cnt.min()) < KNBN
    want = _neighbors_text(items, seqdict, ids, dist, cnt)
    assert built.neighbors == want.encode()
    text = built.neighbors.decode()
    assert "q_d_unrelated" not in text and "q_b_only_n" not in text and "\n0\t%s\tfasta_id:" % items[0][0] in text and "\n3\t%s\tfasta_id:\t\tlength:\t" % items[3][0] in text
    assert built.matches == _matches_rule(items, seqdict, ids, dist, cnt).encode()
    assert ("\n\n request genome : %s\n\t matched genome " % items[2][0]) in built.matches.decode() and "merit : 1.000E0" in built.matches.decode()
    res = built.request
    assert np.array_equal(res["ids"], ids) and np.array_equal(res["distances"].view(np.uint32), dist.view(np.uint32)) and np.array_equal(res["counts"], cnt)
    assert res["items"] == items and [os.path.basename(p) for p in res["skipped_files"]] == ["q_b_only_n.fna"] and res["index_source"] == "hnswdump.gsidx"
    assert res["lines"] == {"neighbors": want.count("\n"), "matches": built.matches.count(b"\n")}
    assert set(res["seconds"]) == {"load", "list", "read_sketch", "search", "text", "wall"}


def test_request_from_the_hnswrs_pair_gives_the_same_bytes(corpus, built):
    copy = os.path.join(corpus.root, "database_pair_only")
    shutil.copytree(built.dir, copy)
    os.remove(os.path.join(copy, "hnswdump.gsidx"))
    res, neighbors, matches = _request(corpus, copy, "pair")
    assert res["index_source"] == "hnswdump" and neighbors == built.neighbors and matches == built.matches


def test_reformat_of_the_request_output(corpus, ref, built):
    import gsearch_amd as G
    out = os.path.join(corpus.root, "first.tsv")
    ids, dist, cnt = ref.answers
    items, seqdict = ref.q.items(), ref.db.items()
    want = []
    for i in range(len(items)):                                            # name order of the queries = request order here; distances ascending per request
        for j in range(int(cnt[i])):
            if dist[i, j] < np.float32(0.99):
                d = float("%.5E" % float(dist[i, j]))                      # the five decimals the answer file carries
                want.append("%s\t%s\t%s\t%d\t%s" % (os.path.basename(items[i][0]), G.rust_display_f64(d), os.path.basename(seqdict[int(ids[i, j])][0]),
                                                     seqdict[int(ids[i, j])][2], G.rust_display_f64(G.ani(d, K, 1))))
    assert G.reformat(K, 1, os.path.join(corpus.root, "first.neighbors.txt"), out) == len(want) > 6
    assert open(out).read() == "Query_Name\tDistance\tNeighbor_Fasta_name\tNeighbor_Seq_Len\tANI\n" + "".join(w + "\n" for w in want)


# ---- block -------------------------------------------------------------------------------------------------------------------------------------------
def test_block_mode(corpus, ref):
    import gsearch_amd as G
    from gsearch_amd.state import ProcessingParams, ProcessingState
    differ = [i for i in range(12) if not np.array_equal(ref.db.block_sig[i], ref.db.sig[i])]
    assert differ, "no file whose junction k-mers change a slot"         # k-mers across the record junctions exist only with block
    d = os.path.join(corpus.root, "database_block")
    rep = _tohnsw(corpus, corpus.db, d, block=True)
    hn = G.Hnsw.load(os.path.join(d, "hnswdump.gsidx"))
    try:
        got = hn.get_data()
    finally:
        hn.close()
    assert np.array_equal(got.view(np.uint32), ref.db.block_sig.view(np.uint32)) and not np.array_equal(got[differ[0]], ref.db.sig[differ[0]])
    assert open(os.path.join(d, "seqdict.json"), "rb").read() == _seqdict_bytes(ref.db.items("-total-sequence"))
    assert ProcessingParams.reload_json(d).block_flag is True
    st = ProcessingState.reload_json(d)
    assert (st.nb_file, st.nb_seq) == (15, 15) and rep["nb_point"] == 12
    res, neighbors, matches = _request(corpus, d, "block")
    assert matches is None and res["lines"]["matches"] is None           # gsearch.rs:926-929
    oix = _oracle_index([ref.db.block_sig])
    ids, dist, cnt, _ = oix.parallel_search(ref.q.block_sig, KNBN, EF_REQ)
    assert neighbors == _neighbors_text(ref.q.items("-total-sequence"), ref.db.items("-total-sequence"), ids, dist, cnt).encode()


# ---- add ---------------------------------------------------------------------------------------------------------------------------------------------
def test_add_continues_ids_and_equals_two_inserts(corpus, ref):
    from gsearch_amd.state import ProcessingState, SeqDict
    import gsearch_amd as G
    first, second = corpus.subset("part1", REL[:8] + ["a_only_n.fna"]), corpus.subset("part2", REL[8:] + ["sub_b/empty.fna"])
    d = os.path.join(corpus.root, "database_grown")
    _tohnsw(corpus, first, d)
    rep = G.add(d, second)
    assert (rep["first_id"], rep["nb_point"], rep["nb_point_total"], rep["nb_file"]) == (8, 4, 12, 5)
    got = SeqDict.reload_json(os.path.join(d, "seqdict.json")).items
    one_step = ref.db.items()
    assert [(os.path.relpath(p, first if i < 8 else second), f, n) for i, (p, f, n) in enumerate(got)] == [(os.path.relpath(p, corpus.db), f, n) for p, f, n in one_step]
    st = ProcessingState.reload_json(d)
    assert (st.nb_file, st.nb_seq) == (9 + 5, ref.db.nb_seq)
    hn = G.Hnsw.load(os.path.join(d, "hnswdump.gsidx"))
    try:
        assert np.array_equal(hn.get_ids(), np.arange(12, dtype=np.uint64)) and np.array_equal(hn.get_data().view(np.uint32), ref.db.sig.view(np.uint32))
    finally:
        hn.close()
    # the build is batch-synchronous: a graph grown by two inserts is not the graph of one. The meaningful comparison is with an oracle index that was
    # also built by two inserts (8, then 4), and that is the only one made
    oix = _oracle_index([ref.db.sig[:8], ref.db.sig[8:]])
    ids, dist, cnt, _ = oix.parallel_search(ref.q.sig, KNBN, EF_REQ)
    res, neighbors, _ = _request(corpus, d, "grown")
    assert neighbors == _neighbors_text(ref.q.items(), got, ids, dist, cnt).encode()
    assert np.array_equal(res["ids"], ids) and np.array_equal(res["distances"].view(np.uint32), dist.view(np.uint32))


def test_add_refuses_a_directory_whose_parameters_disagree_with_the_dump(corpus, built):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID
    copy = os.path.join(corpus.root, "database_edited")
    shutil.copytree(built.dir, copy)
    p = os.path.join(copy, "parameters.json")
    text = open(p).read()
    assert '"sketch_size":512' in text
    open(p, "w").write(text.replace('"sketch_size":512', '"sketch_size":256'))
    before = _dir_digest(copy)
    with pytest.raises(G.GsError) as e:
        G.add(copy, corpus.queries)
    assert e.value.code == GS_ERR_INVALID and _dir_digest(copy) == before


# ---- a layer-0 list the hnsw_rs format cannot hold ---------------------------------------------------------------------------------------------------
HUB_SPOKES, HUB_SEG, HUB_S, HUB_M, HUB_EFC, HUB_B = 290, 3000, 4096, 128, 400, 16


def hub_corpus(root):
    """a hub genome made of HUB_SPOKES segments and one genome per segment: every spoke is close to the hub alone (two spokes share no k-mer), so the hub's
    layer-0 list fills to 2 x 128 = 256 ids by reverse links - one more than the format's one-byte count holds"""
    rng = np.random.default_rng(77)
    segs = [H.dna_ascii(H.rand_dna(rng, HUB_SEG)) for _ in range(HUB_SPOKES)]
    _write(os.path.join(root, "a_hub.fna"), _fasta([(b"hub", b"".join(segs))], 80))
    for i, s in enumerate(segs):
        _write(os.path.join(root, "spokes", "s%03d.fna" % i), _fasta([(b"s", s)], 80))
    return segs


def test_lists_over_255_leave_the_hnswrs_pair_out(corpus):
    import gsearch_amd as G
    src = os.path.join(corpus.root, "hub")
    segs = hub_corpus(src)
    qdir = os.path.join(corpus.root, "hub_queries")
    _write(os.path.join(qdir, "q.fna"), _fasta([(b"q", segs[200])]))
    d = os.path.join(corpus.root, "database_hub")
    genomes = [[b"".join(segs)]] + [[x] for x in segs]
    sig, _ = _oracle_sigs(genomes, m=HUB_S)
    oix = _oracle_index([sig], m=HUB_S, M=HUB_M, efc=HUB_EFC, seed=2, batch=HUB_B)
    assert int(oix.export()["deg0"].max()) == 2 * HUB_M                     # the case is what it claims, on the oracle's graph
    qsig, qsym = _oracle_sigs([[segs[200]]], m=HUB_S)
    ids, dist, cnt, _ = oix.parallel_search(qsig, KNBN, EF_REQ)
    rep = G.tohnsw(src, d, K, HUB_S, HUB_M, ef=HUB_EFC, seed=2, insert_batch=HUB_B)
    assert rep["nb_point"] == HUB_SPOKES + 1 and rep["hnswrs_written"] is False and "one byte" in rep["hnswrs_refused"]
    assert sorted(os.listdir(d)) == ["hnswdump.gsidx", "parameters.json", "processing_state.json", "seqdict.json"]
    hn = G.Hnsw.load(os.path.join(d, "hnswdump.gsidx"))
    try:
        assert int(hn.export_graph()["deg0"].max()) == 2 * HUB_M
    finally:
        hn.close()
    res, neighbors, _ = _request(corpus, d, "hub", query_dir=qdir)
    seqdict = [(os.path.join(src, "a_hub.fna"), "", HUB_SPOKES * HUB_SEG)] + [(os.path.join(src, "spokes", "s%03d.fna" % i), "", HUB_SEG) for i in range(HUB_SPOKES)]
    assert res["index_source"] == "hnswdump.gsidx" and np.array_equal(res["ids"], ids) and np.array_equal(res["distances"].view(np.uint32), dist.view(np.uint32))
    assert neighbors == _neighbors_text([(os.path.join(qdir, "q.fna"), "", int(qsym[0]))], seqdict, ids, dist, cnt).encode() and b"s200.fna" in neighbors
    d2 = os.path.join(corpus.root, "database_hub_cut")
    rep = G.tohnsw(src, d2, K, HUB_S, HUB_M, ef=HUB_EFC, seed=2, insert_batch=HUB_B, truncate_255=True)
    assert rep["hnswrs_written"] is True and {"hnswdump.hnsw.graph", "hnswdump.hnsw.data"} <= set(os.listdir(d2))


# ---- translate="genes" -------------------------------------------------------------------------------------------------------------------------------
AA_K, AA_S = 7, 256


def test_translate_genes_equals_the_sketch_of_the_called_proteomes(corpus, gpu_ctx):
    import gene_cases as GC
    import gsearch_amd as G
    import pyref_orf as RO
    from gsearch_amd._lib import GS_ERR_INVALID
    src, qdir, faa = (os.path.join(corpus.root, n) for n in ("genes_db", "genes_q", "genes_faa"))
    os.makedirs(faa)
    codes = {"ga.fna": GC.planted_genome(7, 30000)[0], "gb.fna": GC.planted_genome(11, 30000)[0]}
    genomes = {n: RO.ascii_of(g) for n, g in codes.items()}
    rng = np.random.default_rng(5)
    for n, a in genomes.items():
        _write(os.path.join(src, n), _fasta([(b"c1", a[:14000]), (b"c2", a[14000:])]))
    _write(os.path.join(src, "short.fna"), _fasta([(b"s", H.dna_ascii(H.rand_dna(rng, 5000)))]))
    mutant = H.dna_ascii(H.mutate(rng, codes["gb.fna"].astype(np.int64), 0.01))
    _write(os.path.join(qdir, "mutant_of_gb.fna"), _fasta([(b"m1", mutant[:14000]), (b"m2", mutant[14000:])]))
    # the route that works without the commands: genecall() writes the .faa, the AA sketcher reads it
    for n in genomes:
        out = G.genecall(os.path.join(src, n), os.path.join(faa, n[:-4]), ctx=gpu_ctx, **GC.SMALL)
        assert out["trained"] and out["n_genes"] > 10
    assert G.genecall(os.path.join(src, "short.fna"), os.path.join(faa, "short"), ctx=gpu_ctx, **GC.SMALL)["trained"] is False
    sk = G.sketcher_for(G.SeqSketcherParams(AA_K, AA_S, "optdens", "aa"), gpu_ctx)
    want, _, want_sym, _ = sk.sketch_files([os.path.join(faa, "ga.faa"), os.path.join(faa, "gb.faa")])
    d = os.path.join(corpus.root, "database_genes")
    with pytest.raises(G.GsError) as e:
        G.tohnsw(src, d, AA_K, AA_S, NBNG, ef=EFC, aa=True, seed=SEED)          # DNA suffixes for an AA database without translate stay an error
    assert e.value.code == GS_ERR_INVALID
    rep = G.tohnsw(src, d, AA_K, AA_S, NBNG, ef=EFC, aa=True, seed=SEED, translate="genes", gene=GC.SMALL)
    assert rep["nb_point"] == 2 and [os.path.basename(p) for p in rep["skipped_files"]] == ["short.fna"]
    hn = G.Hnsw.load(os.path.join(d, "hnswdump.gsidx"))
    try:
        assert np.array_equal(hn.get_data().view(np.uint32), want.view(np.uint32))
    finally:
        hn.close()
    from gsearch_amd.state import ProcessingParams, SeqDict
    assert [(os.path.basename(p), f, n) for p, f, n in SeqDict.reload_json(os.path.join(d, "seqdict.json")).items] == [("ga.fna", "", int(want_sym[0])), ("gb.fna", "", int(want_sym[1]))]
    assert "AA" in open(os.path.join(d, "parameters.json")).read() and ProcessingParams.reload_json(d).data_t == 1
    res, neighbors, _ = _request(corpus, d, "genes", query_dir=qdir, translate="genes", gene=GC.SMALL)
    assert int(res["ids"][0, 0]) == 1 and res["distances"][0, 0] < res["distances"][0, 1] and b"gb.fna" in neighbors


# ---- stale scratch -----------------------------------------------------------------------------------------------------------------------------------
def test_tohnsw_and_request_on_poisoned_scratch(corpus, built, monkeypatch):
    """as tests/test_gpu_stale_scratch.py: every new device allocation and scratch slot filled with 0xA5, the index's per-call buffers before every call"""
    import gsearch_amd as G
    ctx = G.Context(0)
    for name in ("parallel_insert", "search_arrays"):
        orig = getattr(G.Hnsw, name)

        def poked(self, *a, _orig=orig, **kw):
            self.debug_fill_scratch(0xA5)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(G.Hnsw, name, poked)
    d = os.path.join(corpus.root, "database_poisoned")
    try:
        G.debug_mem_fill(0xA5)
        _tohnsw(corpus, corpus.db, d, ctx=ctx)
        res, neighbors, matches = _request(corpus, d, "poisoned", ctx=ctx)
    finally:
        G.debug_mem_fill(None)
        ctx.close()
    assert neighbors == built.neighbors and matches == built.matches
    for n in ("seqdict.json", "parameters.json", "hnswdump.hnsw.graph", "hnswdump.hnsw.data"):
        assert open(os.path.join(d, n), "rb").read() == open(os.path.join(built.dir, n), "rb").read(), n
