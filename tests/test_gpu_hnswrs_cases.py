"""hnsw_rs dumps from another program on the device (SPEC.md 16.1): every valid hand-built case of hnswrs_cases.py loads into exactly the index the
restatement (pyref_hnswrs.expected_index) says - graph, vectors, ids, all compared with == -, a loaded case dumps to files that verify to the same index,
and every refused case and hostile header raises its code, hands back no index and leaves the context fit for the next load and search."""
import numpy as np
import pytest

import hnswrs_cases as Cs
import pyref_hnswrs as R

pytestmark = pytest.mark.gpu


def _files(tmp_path, name, g, d):
    (tmp_path / (name + ".hnsw.graph")).write_bytes(g)
    (tmp_path / (name + ".hnsw.data")).write_bytes(d)
    return tmp_path / name


def _assert_index_is(hn, ex):
    g = hn.export_graph()
    assert hn.get_nb_point() == ex["n"] and g["entry"] == ex["entry"] and g["n_upper"] == ex["n_upper"]
    for key in ("levels", "deg0", "nbr0", "cnt0", "upidx", "degU", "nbrU", "cntU"):
        assert g[key].shape == ex[key].shape and np.array_equal(g[key], ex[key]), key
    data = hn.get_data()
    assert data.dtype == ex["data"].dtype and data.tobytes() == ex["data"].tobytes()
    assert np.array_equal(hn.get_ids(), ex["ids"])


def _by_id(ex):
    """an index keyed by DataId instead of node number: a dump of caller ids numbers its nodes anew"""
    ids = [int(x) for x in ex["ids"]]
    out = {}
    for i in range(ex["n"]):
        lists = [sorted((int(ex["cnt0"][i, t]), ids[ex["nbr0"][i, t]]) for t in range(ex["deg0"][i]))]
        for l in range(1, int(ex["levels"][i]) + 1):
            u = ex["upidx"][i]
            lists.append(sorted((int(ex["cntU"][u, l - 1, t]), ids[ex["nbrU"][u, l - 1, t]]) for t in range(ex["degU"][u, l - 1])))
        out[ids[i]] = (int(ex["levels"][i]), ex["data"][i].tobytes(), lists)
    return out, ids[ex["entry"]]


@pytest.mark.parametrize("name", sorted(Cs.VALID))
def test_valid_case_loads_as_the_restatement_says(gpu_ctx, tmp_path, name):
    import gsearch_amd as G
    mo, _ = Cs.VALID[name]
    ex = R.expected_index(mo)
    hn = G.Hnsw.load_hnswrs(_files(tmp_path, "in", *R.write(mo)), ctx=gpu_ctx)
    assert hn.dtype == np.dtype(R.DTYPE[mo["T"]]) and hn.prm.max_nb_conn == mo["M"] and hn.prm.ef_construction == mo["ef"] and hn.prm.m == mo["vectors"].shape[1]
    _assert_index_is(hn, ex)
    # dumped again, the files verify - in the restatement and in the library - to the same index
    hn.file_dump_hnswrs(tmp_path / "out")
    g2, d2 = (tmp_path / "out.hnsw.graph").read_bytes(), (tmp_path / "out.hnsw.data").read_bytes()
    code, back = R.verify(g2, d2)
    assert code == R.OK
    ex2 = R.expected_index(back)
    assert _by_id(ex2) == _by_id(ex)
    got = G.hnswrs_verify(tmp_path / "out")
    assert got["digest"] == R.digest(ex2) and got["nb_point"] == ex["n"]
    if ex["dense"]:
        assert got["digest"] == R.digest(ex) and got["entry"] == ex["entry"] and got["n_upper"] == ex["n_upper"]
    hn.close()


def test_three_point_case_searches(gpu_ctx, tmp_path):
    import gsearch_amd as G
    hn = G.Hnsw.load_hnswrs(_files(tmp_path, "three", *R.write(Cs.three_points())), ctx=gpu_ctx)
    ids, dist, cnt, _ = hn.search_arrays(np.array([[1, 2, 3, 4]], np.float32), 3, 10)
    assert ids[0].tolist() == [0, 1, 2] and dist[0].tolist() == [0.0, 0.25, 1.0] and cnt[0] == 3
    hn.close()


def test_refused_cases_raise_their_code_and_leave_the_context_clean(gpu_ctx, tmp_path):
    """one context through all of them: no index comes back, and afterwards a valid case still loads and searches on it - a scratch slot still on lease, or a
    half-built index still holding the stream, would fail that with GS_ERR_STATE or a wrong answer"""
    import gsearch_amd as G
    assert len(Cs.HOSTILE) == 3
    for name in sorted(Cs.REFUSED):
        g, d, code, _ = Cs.REFUSED[name]
        hn = None
        with pytest.raises(G.GsError) as e:
            hn = G.Hnsw.load_hnswrs(_files(tmp_path, "bad", g, d), ctx=gpu_ctx)
        assert e.value.code == code and hn is None, (name, e.value.code, code)
    for _ in range(2):
        mo = Cs.VALID["layers_0_1_5_15_with_empty_layers_between"][0]
        hn = G.Hnsw.load_hnswrs(_files(tmp_path, "good", *R.write(mo)), ctx=gpu_ctx)
        ex = R.expected_index(mo)
        _assert_index_is(hn, ex)
        ids, dist, cnt, _ = hn.search_arrays(ex["data"][:4], 1, 24)
        assert cnt.tolist() == [1] * 4 and dist[:, 0].tolist() == [0.0] * 4
        assert all((ex["data"][int(ids[q, 0])] == ex["data"][q]).all() for q in range(4))
        hn.close()
        gpu_ctx.release_scratch()


def test_import_refuses_two_nodes_on_one_upper_row(gpu_ctx):
    """gs_index_import shares its host validation with the dump reader (gs::graph_validate); a dump cannot name one upper row twice, an imported graph can"""
    import gsearch_amd as G
    mo = Cs.base()
    ex = R.expected_index(mo)
    graph = {k: ex[k] for k in ("levels", "entry", "deg0", "nbr0", "cnt0", "upidx", "n_upper", "degU", "nbrU", "cntU")}
    hn = G.Hnsw.new(mo["M"], 100, 16, 24, G.DistHamming(), ctx=gpu_ctx)
    hn.import_graph(ex["data"], graph)
    _assert_index_is(hn, ex)
    hn.close()
    shared = dict(graph, upidx=ex["upidx"].copy())
    up = np.flatnonzero(ex["upidx"] >= 0)
    shared["upidx"][up[1]] = shared["upidx"][up[0]]
    h2 = G.Hnsw.new(mo["M"], 100, 16, 24, G.DistHamming(), ctx=gpu_ctx)
    with pytest.raises(G.GsError) as e:
        h2.import_graph(ex["data"], shared)
    assert e.value.code == -1 and "upidx" in str(e.value)
    assert h2.get_nb_point() == 0
    h2.close()
