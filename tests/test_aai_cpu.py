"""superaai (SPEC 9) without a GPU: the pinned arithmetic of the numpy reference (tests/pyref_aai.py) and of the library's host functions
(gs_frac_max_hash, gs_aai, the list reader and the output writer), and the refusals of the device entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pyref_aai as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superaai")
NAN = float("nan")


def test_smhasher_verification_value():
    assert PR.smhasher_verification() == 0x6384BA69


def test_max_hash_literals():
    import gsearch_amd as G
    want = {0: 0, 1: 2 ** 64 - 1, 100: 184467440737095520, 1000: 18446744073709552}
    assert want[100] == 0x028F5C28F5C28F60
    for s, v in want.items():
        assert PR.max_hash(s) == v
        assert G.frac_max_hash(s) == v


@pytest.mark.parametrize("num", [1, 7, 64])
@pytest.mark.parametrize("scaled", [0, 1, 3])
def test_sourmash_restatement_is_order_independent(num, scaled):
    """upstream adds hashes one by one (its list depends on their order and may grow past num); what it prints equals SPEC 9's definition"""
    rng = np.random.default_rng(1000 * num + scaled)
    for trial in range(6):
        pool = rng.integers(0, 2 ** 64, 300, dtype=np.uint64, endpoint=False)
        a = rng.choice(pool, 150)
        b = np.concatenate([rng.choice(pool, 100), rng.integers(0, 2 ** 64, 50, dtype=np.uint64)])
        ref_a, ref_b = _spec_sketch(a, scaled, num), _spec_sketch(b, scaled, num)
        want = PR.similarity(ref_a, ref_b, num) if not (num == 0 and scaled == 0) else 0.0
        for order in range(4):
            oa, ob = (a, b) if order == 0 else (rng.permutation(a), rng.permutation(b))
            if order == 3:
                oa, ob = np.sort(oa)[::-1], np.sort(ob)[::-1]
            ma, mb = PR.SourmashMinHash(num, scaled), PR.SourmashMinHash(num, scaled)
            for h in oa:
                ma.add_hash(int(h))
            for h in ob:
                mb.add_hash(int(h))
            assert set(ref_a.tolist()) <= set(ma.mins) and set(ma.mins[:num]) == set(ref_a.tolist())
            assert ma.jaccard(mb) == want


def _spec_sketch(hashes, scaled, num):
    mh = PR.max_hash(scaled)
    h = np.unique(np.asarray(hashes, np.uint64))
    if mh:
        h = h[h <= np.uint64(mh)]
    return h[:num] if num else h


AAI_TABLE = [(0.0, 7, "0", "-inf"), (1.0, 7, "1", "1"), (0.5, 7, "0.5", "0.9420764131274051"), (0.25, 7, "0.25", "0.8691013240179779"),
             (1 / 5120, 7, "0.0001953125", "-0.12113683298608646"), (2.0 ** -33, 7, "0.00000000011641532182693481", "-2.1686728254335237"),
             (0.5, 12, "0.5", "0.9662112409909863")]


@pytest.mark.parametrize("sim,k,s_txt,a_txt", AAI_TABLE)
def test_aai_and_display_literals(sim, k, s_txt, a_txt, tmp_path):
    import gsearch_amd as G
    assert PR.display(sim) == s_txt and PR.display(PR.aai(sim, k)) == a_txt
    assert PR.display(G.aai(sim, k)) == a_txt
    out = tmp_path / "one.txt"
    G.write_superaai(out, ["q"], ["r"], np.array([[sim]]), k)
    assert out.read_bytes() == ("q\tr\t%s\t%s" % (s_txt, a_txt)).encode()


def test_display_rules():
    for x, t in [(1e21, "1000000000000000000000"), (1e-7, "0.0000001"), (123.456, "123.456"), (-2.5, "-2.5"), (float("-inf"), "-inf")]:
        assert PR.display(x) == t


def test_list_reader(tmp_path):
    import gsearch_amd as G
    cases = [(b"a\r\nb\n\nc", ["a", "b", "", "c"]), (b"a\n", ["a"]), (b"", []), (b"\n", [""]), (b"x\r", ["x\r"]), (b"a\xff\nb\r\n", ["b"]),
             (b"one\r\n\r\ntwo", ["one", "", "two"])]
    for data, want in cases:
        p = tmp_path / "list.txt"
        p.write_bytes(data)
        assert PR.read_list(data) == want, data
        assert G.read_list_lines(str(p)) == want, data


def test_writer_golden(tmp_path):
    import gsearch_amd as G
    q = G.read_list_lines(os.path.join(GOLD, "query_list.txt"))
    r = G.read_list_lines(os.path.join(GOLD, "ref_list.txt"))
    assert len(q) != len(set(q)) and len(r) != len(set(r))              # duplicated paths keep their lines
    fx = json.load(open(os.path.join(GOLD, "sim.json")))
    out = tmp_path / "out.txt"
    G.write_superaai(out, q, r, np.array(fx["sim"]), fx["k"])
    want = open(os.path.join(GOLD, "expected.txt"), "rb").read()
    assert out.read_bytes() == want
    assert PR.output_text(q, r, fx["sim"], fx["k"]).encode() == want
    G.write_superaai(out, [], r, np.zeros((0, len(r))), 7)
    assert out.read_bytes() == b""


def test_superaai_blank_line_is_an_io_error(tmp_path):
    import gsearch_amd as G
    ql, rl, out = tmp_path / "q.txt", tmp_path / "r.txt", tmp_path / "out.txt"
    ql.write_text("\n")
    rl.write_text("")
    with pytest.raises(G.GsError) as e:
        G.superaai(str(ql), str(rl), str(out))
    assert e.value.code == -5 and not out.exists()


def test_compute_calls_refuse_without_gpu():
    import gsearch_amd as G
    L = G.load()
    off = np.zeros(2, np.uint64)
    hp = C.POINTER(C.c_uint64)()
    # k outside 1..32 is refused before anything else
    t = np.frombuffer(b"MKV\0", np.uint8)
    assert L.gs_frac_sketch_batch(None, 33, 100, 5120, t.ctypes.data, 3, None, None, 0, off.ctypes.data, 0, C.byref(hp), off.ctypes.data) == -3
    assert L.gs_frac_sketch_batch(None, 0, 100, 5120, t.ctypes.data, 3, None, None, 0, off.ctypes.data, 0, C.byref(hp), off.ctypes.data) == -1
    try:
        ctx = G.Context(0)
    except G.GsError as e:
        assert e.code == -2
        for call in (lambda: G.FracMinHashSketch(7, 100, 5120).sketch_genomes([[b"MKVLLA"]]),
                     lambda: G.frac_similarity_qxc([np.arange(3, dtype=np.uint64)], [np.arange(3, dtype=np.uint64)], 5120)):
            with pytest.raises(G.GsError):
                call()
        return
    ctx.close()
    pytest.skip("a GPU is present")
