""".gsbx files from another program on the device (SPEC.md 16.2): every valid hand-built case of bigsi_file_cases.py loads into exactly the index its model
says - rows, t_c, nk_c, accessions, parameters, compared with == - and saves back to the writer's bytes; every refused case raises its code; a short file
that names 2^40 rows is refused from its size, GS_ERR_IO, before the device is asked for a byte."""
import numpy as np
import pytest

import bigsi_file_cases as Cs
import pyref_bigsi_file as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(Cs.VALID))
def test_valid_case_loads_as_its_model_and_saves_back(gpu_ctx, tmp_path, name):
    import gsearch_amd as G
    mo, _ = Cs.VALID[name]
    b = R.write(mo)
    (tmp_path / "in.gsbx").write_bytes(b)
    bx = G.Bigsi.load(tmp_path / "in.gsbx", ctx=gpu_ctx)
    n, B = len(mo["names"]), mo["bloom_size"]
    cap = max(n, 1)
    assert bx.info() == dict(k=mo["k"], num_hash=mo["num_hash"], bloom_size=B, data_t=mo["data_t"], n_colours=n, colour_capacity=cap, row_words=(cap + 63) // 64,
                             minimizer_len=mo["m"])
    rows = bx.rows(np.arange(B, dtype=np.uint64))
    want = mo["rows"] if n else np.zeros((B, 1), np.uint64)
    assert rows.shape == want.shape and np.array_equal(rows, want)
    t, q = bx.bits_set(return_kmers=True)
    assert np.array_equal(t, mo["t"]) and np.array_equal(q, mo["q"])
    assert bx.accessions() == [x.decode() for x in mo["names"]]
    bx.save(tmp_path / "out.gsbx")
    assert (tmp_path / "out.gsbx").read_bytes() == b
    bx.close()
    # a larger capacity widens the rows on the device, not what they hold
    if n:
        bx = G.Bigsi.load(tmp_path / "in.gsbx", ctx=gpu_ctx, capacity=n + 64)
        wide = bx.rows(np.arange(B, dtype=np.uint64))
        W = R.words(n)
        assert wide.shape == (B, R.words(n + 64)) and np.array_equal(wide[:, :W], mo["rows"]) and not wide[:, W:].any()
        bx.close()


def test_refused_cases_raise_their_code(gpu_ctx, tmp_path):
    import gsearch_amd as G
    for name in sorted(Cs.REFUSED):
        b, code, _ = Cs.REFUSED[name]
        (tmp_path / "bad.gsbx").write_bytes(b)
        bx = None
        with pytest.raises(G.GsError) as e:
            bx = G.Bigsi.load(tmp_path / "bad.gsbx", ctx=gpu_ctx)
        assert e.value.code == code and bx is None, (name, e.value.code, code)
    # the context is as fit as before
    mo = Cs.VALID["colours_65"][0]
    (tmp_path / "good.gsbx").write_bytes(R.write(mo))
    bx = G.Bigsi.load(tmp_path / "good.gsbx", ctx=gpu_ctx)
    assert np.array_equal(bx.rows(np.arange(37, dtype=np.uint64)), mo["rows"])
    bx.close()


def test_2p40_rows_in_100_bytes_is_an_io_error_not_a_device_error(gpu_ctx, tmp_path):
    import gsearch_amd as G
    b, code, _ = Cs.REFUSED["bloom_size_2p40_in_100_bytes"]
    assert code == R.IO and len(b) == 100
    (tmp_path / "h.gsbx").write_bytes(b)
    with pytest.raises(G.GsError) as e:
        G.Bigsi.load(tmp_path / "h.gsbx", ctx=gpu_ctx)
    assert e.value.code == -5 and "cut short" in str(e.value)
    # the largest bloom_size the parameters allow, in a file as short: still the size of the file that refuses it (a device allocation of 2^40 - 1 rows would be GS_ERR_HIP)
    b = R.header(dict(version=1, k=31, num_hash=3, data_t=0, m=0, bloom_size=(1 << 40) - 1), n=1) + bytes(60)
    (tmp_path / "h.gsbx").write_bytes(b)
    with pytest.raises(G.GsError) as e:
        G.Bigsi.load(tmp_path / "h.gsbx", ctx=gpu_ctx)
    assert e.value.code == -5
