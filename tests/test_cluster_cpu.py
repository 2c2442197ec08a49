"""hnswcore without a device: the rules of SPEC.md 10 as tests/pyref_cluster.py restates them must do what a clustering is for (recover planted
families, iterate on a database without clear families), and the host pieces of the feature (the membership CSV, the ctypes mirrors of the two
structs, the type names hnswcore() serves) are checked as they stand. The device is held to pyref_cluster bit for bit in test_gpu_cluster.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyref_cluster as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANTED_SEEDS = [0, 1, 2, 3, 4, 5]
# (k, seed) on the mutation chain; the ones in LOOPING must take 3 or more iterations (the planted case takes 1 or 2, which does not exercise the loop)
CHAIN_CASES = [(3, 0), (5, 0), (8, 0), (3, 3), (8, 3), (8, 2)]
LOOPING = [(5, 0), (3, 3), (8, 3)]


@pytest.fixture(scope="module")
def chains():
    return {s: R.chain(s) for s in {s for _, s in CHAIN_CASES}}


@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_families_are_recovered(seed):
    """8 families x 40 rows, m = 256, 30 % of the slots re-randomised per member: the final clusters are exactly the families"""
    db, fam = R.planted(seed)
    n = len(db)
    r = R.cluster(db, 8, 0.1, 15, seed)
    print("seed %d: p = %d, iterations %d, cost_core %d, cost_all %d" % (seed, r["n_core"], r["iterations"], r["cost_core"], r["cost_all"]))
    med = r["medoids"].astype(np.int64)
    assert len(set(fam[med])) == 8 and (np.diff(med) > 0).all()
    cen = r["centre_node"].astype(np.int64)
    assert np.array_equal(fam[cen], fam)                                 # every node's centre is of its own family ...
    assert len(set(cen)) == 8                                            # ... and a family has one centre
    assert int(r["core_weight"].sum()) == n and int(r["sizes"].sum()) == n and (r["sizes"] == 40).all()
    assert r["converged"] == 1 and 8 <= r["n_core"] <= n
    assert (np.diff(r["core_nodes"].astype(np.int64)) > 0).all()
    assert r["cost_all"] == int(r["centre_count"].astype(np.int64).sum())


@pytest.mark.parametrize("k,seed", sorted(CHAIN_CASES))
def test_mutation_chain_iterates(chains, k, seed):
    """row i = row i-1 with 4 % of the slots redrawn: no clear families, so the Voronoi iteration has work to do"""
    db = chains[seed]
    r = R.cluster(db, k, 0.25, 15, seed)
    print("k %d seed %d: p = %d, iterations %d, cost_core %d, cost_all %d" % (k, seed, r["n_core"], r["iterations"], r["cost_core"], r["cost_all"]))
    assert 1 <= r["iterations"] < 15 and r["converged"] == 1
    assert int(r["core_weight"].sum()) == len(db) == int(r["sizes"].sum())
    assert len(set(r["medoids"].tolist())) == k and set(r["medoids"].tolist()) <= set(r["core_nodes"].tolist())
    # the dispatch is a nearest-centre rule: no medoid is closer than the centre
    cm = R.counts(db[r["medoids"].astype(np.int64)], db)
    assert np.array_equal(cm.min(axis=0), r["centre_count"].astype(np.int64))
    if (k, seed) in LOOPING:
        assert r["iterations"] >= 3
        one = R.cluster(db, k, 0.25, 1, seed)
        assert one["iterations"] == 1 and one["converged"] == 0
        assert one["cost_all"] >= 0 and one["n_core"] == r["n_core"] and np.array_equal(one["core_weight"], r["core_weight"])


def test_coreset_only():
    db = R.chain(1)
    r = R.cluster(db, 0, 0.25, 15, 9)
    C_ = r["core_nodes"].astype(np.int64)
    assert r["iterations"] == 0 and r["converged"] == 1 and r["cost_core"] == 0 and len(r["medoids"]) == 0
    assert set(r["centre_node"].tolist()) <= set(C_.tolist())
    assert (r["centre_count"][C_] == 0).all()                            # a coreset point is at count 0 from itself (or an earlier duplicate)
    assert abs(len(C_) - 100) < 40                                       # about fraction x n


def test_sampling_hash_known_answers():
    """h(r, i) = the first SplitMix64 output from seed ^ (r << 56) ^ i: state 0 gives the published first output of SplitMix64(0)"""
    assert int(R.h(0, 0, np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert int(R.h(5, 0, np.array([5], np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert int(R.h(0, 1, np.array([1 << 56], np.uint64))[0]) == 0xE220A8397B1DCDAF


def test_membership_csv(tmp_path):
    import gsearch_amd as G
    path = tmp_path / "clustercoreset.csv"
    ids = np.array([10, 11, 2 ** 63 + 5, 0], np.uint64)
    cen = np.array([10, 10, 0, 0], np.uint64)
    assert G.write_cluster_csv(str(path), ids, cen) == 4
    assert path.read_text() == "10,10\n11,10\n9223372036854775813,0\n0,0\n"
    with pytest.raises(G.GsError):
        G.write_cluster_csv(str(path), ids, cen[:3])


def _c_struct(name):
    hdr = open(os.path.join(ROOT, "include", "gsearch_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        if words:
            fields += [(w, words[0]) for w in words[1:]]
    return fields


@pytest.mark.parametrize("cname,pyname", [("gs_cluster_params", "ClusterParamsC"), ("gs_cluster_info", "ClusterInfoC")])
def test_ctypes_structs_mirror_the_header(cname, pyname):
    from gsearch_amd import _lib
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    fields = _c_struct(cname)
    cls = getattr(_lib, pyname)
    assert [(n, ctype[t]) for n, t in fields] == list(cls._fields_)

    class Ref(C.Structure):                                              # the C layout rules applied to the header's own field list
        _fields_ = [(n, ctype[t]) for n, t in fields]
    assert C.sizeof(cls) == C.sizeof(Ref) == 32


def test_default_parameters_are_hnswcores():
    import gsearch_amd as G
    p = G.load().gs_cluster_params_default()
    assert (p.n_cluster, p.fraction, p.max_iter) == (0, 0.1, 15)        # hnswcore.rs:328 (fraction), :272 (nb_max_kmedoid_iter)


def test_hnswcore_type_names():
    """u16 / u32 / u64 / f32 are served; the other names of hnswcore.rs:163-170 are refused with a message that says so, before anything is read"""
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID, GS_ERR_UNSUPPORTED
    for t in ("f64", "i32", "i64"):
        with pytest.raises(G.GsError) as e:
            G.hnswcore("/nonexistent", "x", t)
        assert e.value.code == GS_ERR_UNSUPPORTED and t in str(e.value) and "u16" in str(e.value)
    with pytest.raises(G.GsError) as e:
        G.hnswcore("/nonexistent", "x", "float")
    assert e.value.code == GS_ERR_INVALID
