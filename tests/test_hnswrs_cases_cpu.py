"""hnsw_rs dumps as files from another program (SPEC.md 16.1): the hand-built cases of hnswrs_cases.py keep the promise of their names on the restatement
(pyref_hnswrs), and the library's host-only gs_hnswrs_verify / gs_hnswrs_describe give the restatement's verdict on every one of them and on every file
of the prefix and byte sweeps: the same code, and for an accepted file the same description and the same loaded graph (SPEC 16.3 digest). No GPU."""
import pytest

import hnswrs_cases as Cs
import pyref_hnswrs as R


def _lib_verdict(tmp_path, g, d, name="x"):
    """(code, what hnswrs_verify returns or None) of the library on these bytes"""
    import gsearch_amd as G
    (tmp_path / (name + ".hnsw.graph")).write_bytes(g)
    (tmp_path / (name + ".hnsw.data")).write_bytes(d)
    try:
        return 0, G.hnswrs_verify(tmp_path / name)
    except G.GsError as e:
        return e.code, None


def _same_as_model(got, g, mo):
    """the library's verify result against the restatement's model of the same bytes"""
    ex = R.expected_index(mo)
    _, ds = R.describe(g)
    want = dict(ds, distance=ds["distance"].decode("utf-8", "replace"), t_name=ds["t_name"].decode("utf-8", "replace"), n_upper=ex["n_upper"], entry=ex["entry"],
                ids_are_nodes=int(ex["dense"]), digest=R.digest(ex))
    return got == want, (got, want)


@pytest.mark.parametrize("name", sorted(Cs.VALID))
def test_valid_case_keeps_its_promise_and_round_trips(name):
    mo, promise = Cs.VALID[name]
    assert promise(mo), name
    g, d = R.write(mo)
    code, back = R.verify(g, d)
    assert code == R.OK and R.same_model(back, mo) and R.write(back) == (g, d)
    assert len(g) + len(d) < 1 << 20


@pytest.mark.parametrize("name", sorted(Cs.REFUSED))
def test_refused_case_keeps_its_promise(name):
    g, d, code, promise = Cs.REFUSED[name]
    assert code in (R.IO, R.UNSUPPORTED, R.INVALID) and promise(), name
    assert R.verify(g, d) == (code, None)


@pytest.mark.parametrize("name", sorted(Cs.VALID))
def test_library_accepts_valid_case_with_the_model_of_the_restatement(tmp_path, name):
    mo, _ = Cs.VALID[name]
    g, d = R.write(mo)
    code, got = _lib_verdict(tmp_path, g, d)
    assert code == 0
    same, both = _same_as_model(got, g, mo)
    assert same, both


@pytest.mark.parametrize("name", sorted(Cs.REFUSED))
def test_library_refuses_with_the_code_of_the_case(tmp_path, name):
    g, d, code, _ = Cs.REFUSED[name]
    assert _lib_verdict(tmp_path, g, d) == (code, None)


def test_describe_returns_the_description_alone(tmp_path):
    """gs_hnswrs_describe reads the head of the graph file and nothing else: no data file is needed, and what verify refuses later is still described"""
    import gsearch_amd as G
    subjects = [(n, R.write(Cs.VALID[n][0])[0]) for n in sorted(Cs.VALID)]
    subjects += [(n, Cs.REFUSED[n][0]) for n in sorted(Cs.REFUSED)]
    seen = {0: 0, R.IO: 0, R.UNSUPPORTED: 0}
    for name, g in subjects:
        (tmp_path / "only.hnsw.graph").write_bytes(g)
        code, want = R.describe(g)
        seen[code] += 1
        if code:
            with pytest.raises(G.GsError) as e:
                G.hnswrs_describe(tmp_path / "only")
            assert e.value.code == code, name
            continue
        got = G.hnswrs_describe(tmp_path / "only")
        want = dict(want, distance=want["distance"].decode("utf-8", "replace"), t_name=want["t_name"].decode("utf-8", "replace"), n_upper=0, entry=0, ids_are_nodes=0, digest=0)
        assert got == want, name
    assert all(seen.values()), seen
    hostile = G.hnswrs_describe(_write(tmp_path, "h", *Cs.REFUSED[Cs.HOSTILE[0]][:2]))
    assert hostile["nb_point"] == hostile["dimension"] == (1 << 31) - 1 and hostile["t_name"] == "u64" and hostile["kind"] == 2


def _write(tmp_path, name, g, d):
    (tmp_path / (name + ".hnsw.graph")).write_bytes(g)
    (tmp_path / (name + ".hnsw.data")).write_bytes(d)
    return tmp_path / name


def test_prefix_and_byte_sweeps_agree_with_the_restatement(tmp_path):
    """every proper prefix of each file with the other intact is refused; every byte once 0xFF and once ^ 1: the library's verdict is the restatement's for
    every file of the sweep - the code, and for an accepted file (a changed payload byte, distance, ef ...) the description and the loaded graph"""
    sweep = Cs.sweep_files()
    g0, d0 = R.write(Cs.three_points())
    assert len(sweep) == 3 * (len(g0) + len(d0)) - (g0 + d0).count(b"\xff")
    differ, accepted, prefixes = [], 0, 0
    for tag, g, d, code, mo in sweep:
        if tag[1] == "p":
            prefixes += 1
            assert code != R.OK, tag                                    # the restatement refuses every proper prefix
        got_code, got = _lib_verdict(tmp_path, g, d)
        if got_code != code:
            differ.append((tag, got_code, code))
        elif code == R.OK:
            accepted += 1
            same, both = _same_as_model(got, g, mo)
            if not same:
                differ.append((tag,) + both)
    assert prefixes == len(g0) + len(d0) and accepted > 100
    assert not differ, (len(differ), differ[:10])
