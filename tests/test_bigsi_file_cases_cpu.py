""".gsbx files as files from another program (SPEC.md 16.2): the hand-built cases of bigsi_file_cases.py keep the promise of their names on the restatement
(pyref_bigsi_file), and the library's host-only gs_bigsi_verify / gs_bigsi_describe give the restatement's verdict on every one of them and on every file of
the prefix and byte sweeps: the same code, and for an accepted file the same header and the same digest of everything behind it (SPEC 16.3). No GPU."""
import pytest

import bigsi_file_cases as Cs
import pyref_bigsi_file as R


def _lib_verdict(tmp_path, b):
    import gsearch_amd as G
    (tmp_path / "x.gsbx").write_bytes(b)
    try:
        return 0, G.Bigsi.verify(tmp_path / "x.gsbx")
    except G.GsError as e:
        return e.code, None


def _want(b, mo):
    _, h = R.describe(b)
    return dict(h, has_accessions=int(any(mo["names"])), digest=R.digest(b))


@pytest.mark.parametrize("name", sorted(Cs.VALID))
def test_valid_case_keeps_its_promise_and_round_trips(name):
    mo, promise = Cs.VALID[name]
    assert promise(mo), name
    b = R.write(mo)
    code, back = R.verify(b)
    assert code == R.OK and R.same_model(back, mo) and R.write(back) == b
    assert len(b) < 1 << 20


@pytest.mark.parametrize("name", sorted(Cs.REFUSED))
def test_refused_case_keeps_its_promise(name):
    b, code, promise = Cs.REFUSED[name]
    assert code in (R.IO, R.INVALID) and promise(), name
    assert R.verify(b) == (code, None)


@pytest.mark.parametrize("name", sorted(Cs.VALID))
def test_library_accepts_valid_case_with_the_model_of_the_restatement(tmp_path, name):
    mo, _ = Cs.VALID[name]
    b = R.write(mo)
    assert _lib_verdict(tmp_path, b) == (0, _want(b, mo))


@pytest.mark.parametrize("name", sorted(Cs.REFUSED))
def test_library_refuses_with_the_code_of_the_case(tmp_path, name):
    b, code, _ = Cs.REFUSED[name]
    assert _lib_verdict(tmp_path, b) == (code, None)


def test_describe_returns_the_header_alone(tmp_path):
    """gs_bigsi_describe reads the fixed header and judges magic and version only: what verify refuses later is still described"""
    import gsearch_amd as G
    subjects = [(n, R.write(Cs.VALID[n][0])) for n in sorted(Cs.VALID)] + [(n, Cs.REFUSED[n][0]) for n in sorted(Cs.REFUSED)]
    seen = {0: 0, R.IO: 0}
    for name, b in subjects:
        (tmp_path / "h.gsbx").write_bytes(b)
        code, want = R.describe(b)
        seen[code] += 1
        if code:
            with pytest.raises(G.GsError) as e:
                G.Bigsi.describe(tmp_path / "h.gsbx")
            assert e.value.code == code, name
        else:
            assert G.Bigsi.describe(tmp_path / "h.gsbx") == dict(want, has_accessions=0, digest=0), name
    assert all(seen.values()), seen


def test_prefix_and_byte_sweeps_agree_with_the_restatement(tmp_path):
    sweep = Cs.sweep_files()
    b0 = R.write(Cs.base())
    assert len(sweep) == 3 * len(b0) - b0.count(b"\xff")
    differ, accepted, prefixes = [], 0, 0
    for tag, b, code, mo in sweep:
        if tag[0] == "p":
            prefixes += 1
            assert code != R.OK, tag
        got = _lib_verdict(tmp_path, b)
        want = (code, _want(b, mo) if code == R.OK else None)
        accepted += code == R.OK
        if got != want:
            differ.append((tag, got, want))
    assert prefixes == len(b0) and accepted > 50
    assert not differ, (len(differ), differ[:10])
