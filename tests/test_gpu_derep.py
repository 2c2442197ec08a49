"""derep on the device (gs_derep.hip, SPEC.md 18): gs_index_components and gs_index_derep against the numpy restatement tests/pyref_derep.py, `==` on
every output word and info field, on the case table of tests/derep_cases.py (n <= 600, m = 96): on clean and on poisoned scratch, in every element
type, through caller ids, in one block of rows and in several (GS_JOIN_MAXQ = 64 and 96); the representatives against Hnsw.count_matrix without the
restatement; every refusal; and derep() end to end on a database tohnsw built from FASTA files."""
import os

import numpy as np
import pytest

import derep_cases as D
import helpers as H
import pyref_derep as R

pytestmark = pytest.mark.gpu

FILLS = [None, 0x00, 0xFF]
DTYPES = [np.float32, np.uint32, np.uint64, np.uint16]


def _index(G, db, M=8):
    """an index over db without an HNSW build: an empty layer-0 graph is imported (derep never reads the graph)"""
    n = len(db)
    hn = G.Hnsw.new(M, max(n, 1024), 16, 40, G.DistHamming(), dtype=db.dtype)
    hn.import_graph(db, dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32),
                             cnt0=np.zeros((n, 2 * M), np.uint32), upidx=np.full(n, -1, np.int32), n_upper=0))
    return hn


def _same(comp, der, ref, ids=None):
    c_max, rc, rg = ref
    n = len(rc["label"])
    ids = np.arange(n, dtype=np.uint64) if ids is None else ids
    assert comp.label_node.dtype == np.uint64 and np.array_equal(comp.label_node, rc["label"])
    assert np.array_equal(comp.label_id, ids[rc["label"].astype(np.int64)])
    assert (comp.n_clusters, comp.n_singletons, comp.largest, comp.c_max) == (rc["n_clusters"], rc["n_singletons"], rc["largest"], c_max)
    assert der.rep_node.dtype == np.uint64 and der.rep_count.dtype == np.uint16
    assert np.array_equal(der.rep_node, rg["rep_node"]) and np.array_equal(der.rep_count, rg["rep_count"])
    assert np.array_equal(der.rep_id, ids[rg["rep_node"].astype(np.int64)]) and np.array_equal(der.reps, rg["reps"])
    assert np.array_equal(der.sizes, np.bincount(rg["rep_node"].astype(np.int64), minlength=n)[rg["reps"].astype(np.int64)])
    assert (der.n_clusters, der.n_singletons, der.largest, der.c_max) == (rg["n_clusters"], rg["n_singletons"], rg["largest"], c_max)


class _Fill:
    """newly taken scratch slots and the index's own per-call buffers hold `byte` (None: as they are)"""

    def __init__(self, G, hn, byte):
        self.G, self.byte = G, byte
        if byte is not None:
            G.debug_mem_fill(byte)
            hn.debug_fill_scratch(byte)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.G.debug_mem_fill(None)


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "clean" if f is None else "fill%02x" % f)
@pytest.mark.parametrize("name", D.NAMES)
def test_every_word_equals_the_restatement(gpu_ctx, name, fill):
    import gsearch_amd as G
    db, max_dist, prio = D.case(name)
    ref = D.reference(name)
    hn = _index(G, db)
    try:
        with _Fill(G, hn, fill):
            comp = hn.components(max_dist)
            der = hn.derep(max_dist, prio)
            _same(comp, der, ref)
            # without the restatement: no two representatives are linked, by the index's own count matrix
            reps = der.reps.astype(np.int64)
            sub = hn.count_matrix(db[reps])[:, reps].astype(np.int64)
            sub[np.arange(len(reps)), np.arange(len(reps))] = 1 << 20
            assert (sub > der.c_max).all()
    finally:
        hn.close()
    if name.startswith("chain3"):
        assert comp.label_node.tolist() == [0, 0, 0] and comp.n_clusters == 1
    if name == "chain3_a_first":
        assert der.rep_node.tolist() == [0, 0, 2]                          # B is no representative and does not cover C
    if name in ("all_linked", "beyond_one"):
        assert comp.n_clusters == 1 and der.n_clusters == 1 and der.c_max == D.M and np.array_equal(der.rep_count, R.counts(db[:1], db)[0])
    if name == "none_linked":
        assert comp.n_clusters == der.n_clusters == len(db) and der.n_singletons == len(db)
    if name == "duplicates":
        assert der.c_max == 0 and (der.rep_count == 0).all() and der.n_singletons == 0
    if name in ("path600", "ring600"):
        assert comp.n_clusters == 1 and comp.largest == 600


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_element_types(gpu_ctx, dtype):
    import gsearch_amd as G
    db, max_dist, prio = D.case("n257")
    hn = _index(G, D.as_dtype(db, dtype))
    try:
        _same(hn.components(max_dist), hn.derep(max_dist, prio), D.reference("n257", np.dtype(dtype).name))
    finally:
        hn.close()


def test_caller_ids(gpu_ctx):
    """labels and representatives come back as node numbers and as the caller's ids; the arithmetic sees node numbers only"""
    import gsearch_amd as G
    db, max_dist, prio = D.case("families_ties")
    hn = _index(G, db)
    ids = (7_000_000_000 + 3 * np.random.default_rng(1).permutation(len(db))).astype(np.uint64)
    hn.set_ids(ids)
    try:
        _same(hn.components(max_dist), hn.derep(max_dist, prio), D.reference("families_ties"), ids)
    finally:
        hn.close()


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "clean" if f is None else "fill%02x" % f)
@pytest.mark.parametrize("maxq", [64, 96])
@pytest.mark.parametrize("name", ["straddle", "inblock", "n257", "ring600"])
def test_blocks_give_the_one_block_answers(gpu_ctx, monkeypatch, name, maxq, fill):
    """GS_JOIN_MAXQ (read at every call) cuts the rows into several blocks: the forest is carried from block to block, the greedy cover comes
    from earlier blocks and the mask from the row's own"""
    import gsearch_amd as G
    db, max_dist, prio = D.case(name)
    ref = D.reference(name)
    assert len(db) > 96
    hn = _index(G, db)
    try:
        one = hn.components(max_dist), hn.derep(max_dist, prio)
        monkeypatch.setenv("GS_JOIN_MAXQ", str(maxq))
        with _Fill(G, hn, fill):
            many = hn.components(max_dist), hn.derep(max_dist, prio)
    finally:
        hn.close()
    _same(one[0], one[1], ref)
    _same(many[0], many[1], ref)
    if name == "inblock":
        order, _ = R.ranks(len(db), prio)
        assert many[1].rep_node[order[D.INBLOCK["x"]]] == order[D.INBLOCK["r1"]] and many[1].rep_count[order[D.INBLOCK["x"]]] == 3


def test_refusals(gpu_ctx):
    import ctypes as C
    import gsearch_amd as G
    from gsearch_amd import _lib
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_STATE, GS_ERR_UNSUPPORTED
    db = D.case("families")[0]
    n = len(db)
    hn = _index(G, db)

    def code(f, *a, **kw):
        with pytest.raises(G.GsError) as e:
            f(*a, **kw)
        return e.value.code
    for bad in (float("nan"), -0.5, float("-inf")):
        assert code(hn.components, bad) == GS_ERR_INVALID and code(hn.derep, bad) == GS_ERR_INVALID
    assert code(hn.derep, 0.3, np.zeros(n + 1, np.uint64)) == GS_ERR_INVALID
    lab, rep, cnt, info = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint16), _lib.DerepInfoC()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    L = hn.ctx.L
    assert L.gs_index_components(hn.h, 0.3, None, C.byref(info)) == GS_ERR_INVALID
    assert L.gs_index_components(hn.h, 0.3, p(lab), None) == GS_ERR_INVALID
    assert L.gs_index_derep(hn.h, 0.3, None, None, p(cnt), C.byref(info)) == GS_ERR_INVALID
    assert L.gs_index_derep(hn.h, 0.3, None, p(rep), None, C.byref(info)) == GS_ERR_INVALID
    assert L.gs_index_derep(hn.h, 0.3, None, p(rep), p(cnt), None) == GS_ERR_INVALID
    assert L.gs_index_components(None, 0.3, p(lab), C.byref(info)) == GS_ERR_INVALID
    assert L.gs_index_components(hn.h, 0.3, p(lab), C.byref(info)) == 0 and L.gs_index_derep(hn.h, 0.3, None, p(rep), p(cnt), C.byref(info)) == 0
    hn.close()
    empty = G.Hnsw.new(8, 1000, 16, 40, G.DistHamming())
    assert code(empty.components, 0.3) == GS_ERR_STATE and code(empty.derep, 0.3) == GS_ERR_STATE
    empty._ensure(32)
    assert code(empty.components, 0.3) == GS_ERR_STATE and code(empty.derep, 0.3) == GS_ERR_STATE
    assert L.gs_index_components(empty.h, 0.3, p(lab), C.byref(info)) == GS_ERR_STATE
    assert L.gs_index_derep(empty.h, 0.3, None, p(rep), p(cnt), C.byref(info)) == GS_ERR_STATE
    empty.close()
    big = _index(G, np.zeros((4, 70000), np.float32))
    assert code(big.components, 0.3) == GS_ERR_UNSUPPORTED and code(big.derep, 0.3) == GS_ERR_UNSUPPORTED
    big.close()


# ---- derep() on files -------------------------------------------------------------------------------------------------------------------------------
K, S, LEN = 21, 512, 20000


def _fasta(records, width=70):
    out = []
    for name, s in records:
        out.append(b">" + name + b"\n")
        out += [s[o:o + width] + b"\n" for o in range(0, len(s), width)]
    return b"".join(out)


def test_derep_end_to_end(gpu_ctx, tmp_path):
    """a dozen FASTA files: three roots with three or four 1 % mutants each (11 files) and one 10 % mutant of the first root; tohnsw, then derep at
    ANI 95: both files byte for byte the restatement's on the database's signatures, the families recovered, the outlier alone"""
    import gsearch_amd as G
    rng = np.random.default_rng(77)
    src, fam = tmp_path / "genomes", {}
    os.makedirs(src)
    roots = [H.rand_dna(rng, LEN - 1500 * f) for f in range(3)]                         # families of different genome lengths
    for f, size in enumerate((4, 4, 3)):
        for i in range(size):
            name = "f%d_m%d.fna" % (f, i)
            fam[name] = f
            (src / name).write_bytes(_fasta([(b"ctg0 " + name.encode(), H.dna_ascii(H.mutate(rng, roots[f], 0.01)))], 60 + i))
    fam["outlier.fna"] = 3
    (src / "outlier.fna").write_bytes(_fasta([(b"far", H.dna_ascii(H.mutate(rng, roots[0], 0.10)))]))
    dbdir, out = str(tmp_path / "database"), tmp_path / "out"
    rep = G.tohnsw(str(src), dbdir, K, S, 8, ef=64, algo="optdens", seed=3, insert_batch=64)
    assert rep["nb_point"] == 12
    hn = G.Hnsw.load(os.path.join(dbdir, "hnswdump.gsidx"))
    sigs, ids = hn.get_data(), hn.get_ids().astype(np.int64)
    hn.close()
    import json
    items = G.state.SeqDict.reload_json(os.path.join(dbdir, "seqdict.json")).items
    paths = [items[i][0] for i in ids]
    lengths = np.array([int(items[i][2]) for i in ids], np.uint64)
    c_max, max_dist = R.ani_cut(95.0, K, 1, S)
    for linkage in ("greedy", "single"):
        res = G.derep(dbdir, ani=95.0, model=1, linkage=linkage, out_dir=out)
        assert res["c_max"] == c_max and res["max_dist"] == max_dist
        if linkage == "greedy":
            want = R.greedy_sequential(sigs, c_max, lengths)
            text, reps = R.clusters_text(paths, want["rep_node"], want["rep_count"], S, K, 1), want["reps"]
            node = res["result"].rep_node
            assert np.array_equal(node, want["rep_node"]) and np.array_equal(res["result"].rep_count, want["rep_count"])
        else:
            want = R.components(sigs, c_max)
            text, reps = R.clusters_text(paths, want["label"], None, S, K, 1), np.unique(want["label"])
            node = res["result"].label_node
            assert np.array_equal(node, want["label"])
        assert open(res["clusters"], "rb").read() == text.encode() and open(res["representatives"], "rb").read() == R.representatives_text(paths, reps).encode()
        # the planted families, and the outlier on its own
        family = np.array([fam[os.path.basename(p)] for p in paths])
        assert len(set(node.tolist())) == 4
        for f in range(4):
            assert len(set(node[family == f].tolist())) == 1
    assert json.load(open(os.path.join(dbdir, "parameters.json")))                        # the database is left as it was
    with pytest.raises(G.GsError):
        G.derep(dbdir, out_dir=out)
    with pytest.raises(G.GsError):
        G.derep(dbdir, ani=95, max_dist=0.5, out_dir=out)
    # max_dist and an array of priorities
    res = G.derep(dbdir, max_dist=max_dist, priority=np.arange(12, dtype=np.uint64), out_dir=out)
    assert np.array_equal(res["result"].rep_node, R.greedy_sequential(sigs, c_max, np.arange(12))["rep_node"])
