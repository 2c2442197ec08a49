"""The restatement of SPEC 18 (tests/pyref_derep.py) held to the definitions, without a device: the two greedy definitions agree, representatives are
pairwise unlinked, members are linked to their representative at the stated count, greedy clusters lie inside components, labels are component
minima; ani_cut against the forward transform; the two texts against literals; the cases are what their names claim."""
import numpy as np
import pytest

import derep_cases as D
import pyref_derep as R


@pytest.mark.parametrize("name", D.NAMES)
def test_definitions_on_every_case(name):
    db, max_dist, prio = D.case(name)
    c_max, comp, seq = D.reference(name)
    n = len(db)
    cm, L = R.links(db, c_max)
    peel = R.greedy_peeling(db, c_max, prio)
    for k in seq:
        assert np.array_equal(seq[k], peel[k]), k
    rep_node, rep_count, reps = seq["rep_node"].astype(np.int64), seq["rep_count"], seq["reps"].astype(np.int64)
    assert not L[np.ix_(reps, reps)].any()                                   # pairwise unlinked
    order, rank_of = R.ranks(n, prio)
    assert [order.index(r) for r in reps] == sorted(order.index(r) for r in reps)
    for v in range(n):
        r = rep_node[v]
        if r == v:
            assert rep_count[v] == 0
        else:
            assert L[r, v] and cm[r, v] == rep_count[v] and rank_of[r] < rank_of[v] and rep_node[r] == r
        assert comp["label"][v] == comp["label"][r]                          # a greedy cluster lies inside one component
    label = comp["label"].astype(np.int64)
    for lab in np.unique(label):
        mem = np.nonzero(label == lab)[0]
        assert mem.min() == lab
        assert not L[np.ix_(mem, np.nonzero(label != lab)[0])].any()         # no link leaves a component
    # connected: the closure of {lab} under L is the whole class
    reach = np.eye(n, dtype=bool) | L
    for _ in range(int(np.ceil(np.log2(max(n, 2)))) + 1):
        reach = reach | ((reach.astype(np.int32) @ reach.astype(np.int32)) > 0)
    assert np.array_equal(reach, label[:, None] == label[None, :])
    assert seq["n_clusters"] == len(reps) and comp["n_clusters"] == len(np.unique(label)) and comp["c_max"] == seq["c_max"] == c_max


def test_the_cases_are_what_they_claim():
    c_max, comp, seq = D.reference("families")
    fam = R.families(0)[1]
    assert comp["n_clusters"] == 6 + 9 and comp["n_singletons"] == 9 and comp["largest"] == 12
    for f in range(6):
        assert len(set(comp["label"][fam == f].tolist())) == 1
    assert len(D.case("n257")[0]) == 257
    db, md, _ = D.case("boundary")
    cm = R.counts(db, db)
    assert (cm[0, 1:] == [9, 10, 11]).all() and R.c_max_of(md, D.M) == 10
    _, _, g = D.reference("boundary")
    assert g["rep_node"][1] == 0 and g["rep_node"][2] == 0 and g["rep_node"][3] != 0
    c_max, comp, seq = D.reference("duplicates")
    db = D.case("duplicates")[0]
    assert c_max == 0 and 1 < comp["n_clusters"] < len(db) and comp["n_singletons"] == 0
    assert all((db[v] == db[int(r)]).all() for v, r in enumerate(comp["label"]))
    assert np.array_equal(comp["label"], seq["rep_node"])                    # node order: the first duplicate is label and representative
    # the chain: B first covers both; A first leaves C a representative, because B is none; single linkage joins all three
    assert D.reference("chain3_b_first")[2]["rep_node"].tolist() == [1, 1, 1]
    assert D.reference("chain3_a_first")[2]["rep_node"].tolist() == [0, 0, 2]
    assert D.reference("chain3_c_first")[2]["rep_node"].tolist() == [0, 2, 2]
    assert D.reference("chain3_a_first")[1]["label"].tolist() == [0, 0, 0]
    for name in ("path600", "ring600"):
        c_max, comp, seq = D.reference(name)
        deg = R.links(D.case(name)[0], c_max)[1].sum(axis=1)
        assert comp["n_clusters"] == 1 and (np.bincount(deg, minlength=3)[1:].tolist() == ([2, 598] if name == "path600" else [0, 600]))
    for name in ("all_linked", "beyond_one"):
        c_max, comp, seq = D.reference(name)
        db = D.case(name)[0]
        assert c_max == D.M and comp["n_clusters"] == 1 and seq["n_clusters"] == 1 and np.array_equal(seq["rep_count"], R.counts(db[:1], db)[0])
    assert D.reference("none_linked")[1]["n_clusters"] == len(D.case("none_linked")[0])
    # ties go by node number; reversed priorities change the representatives
    assert not np.array_equal(D.reference("families")[2]["rep_node"], D.reference("families_reversed")[2]["rep_node"])
    assert np.array_equal(D.reference("families")[2]["rep_node"], D.reference("families_equal")[2]["rep_node"])
    c_max, comp, seq = D.reference("straddle")
    assert 280 <= len(D.case("straddle")[0]) <= 320 and comp["largest"] == 130 and 1 < seq["n_clusters"] < 300
    # an in-block representative nearer than the cover of an earlier block
    db, md, prio = D.case("inblock")
    order, _ = R.ranks(len(db), prio)
    c_max, comp, seq = D.reference("inblock")
    r0, r1, x = (order[D.INBLOCK[k]] for k in ("r0", "r1", "x"))
    cm = R.counts(db, db)
    assert cm[r0, x] == 9 and cm[r1, x] == 3 and cm[r0, r1] == 12 and seq["rep_node"][x] == r1 and seq["rep_count"][x] == 3 and seq["rep_node"][r1] == r1
    for bq in (50, 75):
        assert D.INBLOCK["r1"] // bq == D.INBLOCK["x"] // bq != D.INBLOCK["r0"] // bq


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("k,m", [(16, 96), (21, 18000), (7, 1000), (32, 65535), (21, 512)])
def test_ani_cut_is_the_boundary_of_the_forward_transform(model, k, m):
    import gsearch_amd as G
    for a in (99.5, 95.0, 90.0, 70.0, 100.0, 0.0):
        c, d = G.ani_cut(a, k, model, m)
        assert d == R.f32_dist(c, m)
        assert G.ani(R.f32_dist(c, m), k, model) >= a
        assert c == m or G.ani(R.f32_dist(c + 1, m), k, model) < a
        assert R.ani(R.f32_dist(c, m), k, model) >= a and (c == m or R.ani(R.f32_dist(c + 1, m), k, model) < a)
        if m <= 1000:
            assert (c, d) == R.ani_cut(a, k, model, m)
        assert R.c_max_of(d, m) == c if m <= 1000 else True
    with pytest.raises(G.GsError):
        G.ani_cut(100.5, k, model, m)
    with pytest.raises(G.GsError):
        G.ani_cut(95, k, 3, m)


PATHS = ["/db/a.fna", "/db/sub/b.fa.gz", "/db/c.fasta", "/db/d.fna"]
CLUSTERS = ("genome\trepresentative\tdistance\tani\tcluster_size\n"
            "/db/a.fna\t/db/c.fasta\t3.12500E-2\t99.89999786658474\t3\n"
            "/db/sub/b.fa.gz\t/db/sub/b.fa.gz\t0.00000E0\t100\t1\n"
            "/db/c.fasta\t/db/c.fasta\t0.00000E0\t100\t3\n"
            "/db/d.fna\t/db/c.fasta\t7.08333E-1\t95.03168861167413\t3\n")
SINGLE = ("genome\trepresentative\tdistance\tani\tcluster_size\n"
          "/db/a.fna\t/db/a.fna\t-\t-\t2\n/db/sub/b.fa.gz\t/db/sub/b.fa.gz\t-\t-\t1\n/db/c.fasta\t/db/a.fna\t-\t-\t2\n/db/d.fna\t/db/d.fna\t-\t-\t1\n")


def test_the_two_texts():
    import gsearch_amd as G
    node, cnt = np.array([2, 1, 2, 2], np.uint64), np.array([3, 0, 0, 68], np.uint16)
    for f in (R.clusters_text, G.derep_clusters_text):
        assert f(PATHS, node, cnt, 96, 16, 1) == CLUSTERS
        assert f(PATHS, np.array([0, 1, 0, 3], np.uint64), None, 96, 16, 1) == SINGLE
    for f in (R.representatives_text, G.derep_representatives_text):
        assert f(PATHS, np.array([2, 1], np.uint64)) == "/db/c.fasta\n/db/sub/b.fa.gz\n"
    assert R.clusters_text(PATHS, node, cnt, 96, 21, 2) == G.derep_clusters_text(PATHS, node, cnt, 96, 21, 2)
