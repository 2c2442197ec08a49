"""Hand-built hnsw_rs dumps (SPEC.md 16.1), in the style of deflate_cases.py: every case has a name that promises a property and a check of that promise
on the restatement (pyref_hnswrs), so that a case cannot quietly stop being what it is called. VALID: name -> (model, promise(model)); REFUSED: name ->
(graph, data, code, promise()) - each differs from the valid model BASE in the named field only. sweep_files(): every proper prefix and every byte
replaced by 0xFF and by itself ^ 1, of the smallest valid case with neighbours, each with the restatement's verdict."""
import struct

import numpy as np

import pyref_hnswrs as R

OK, INVALID, UNSUPPORTED, IO = R.OK, R.INVALID, R.UNSUPPORTED, R.IO


def _dist(vec, a, b):
    return np.float32(int((vec[a] != vec[b]).sum())) / np.float32(vec.shape[1])


def three_points():
    """the dump of test_hnswrs_dump_assembled_by_hand: layer 0 holds ids 0 and 2, layer 1 holds id 1, the entry point; data file in the order 0, 2, 1"""
    vec = np.array([[1, 2, 3, 4], [7, 7, 7, 7], [1, 2, 3, 9]], np.float32)          # data-file order: ids 0, 2, 1
    ids, layer = [0, 2, 1], [0, 0, 1]
    lists = {(0, 0): [(2, _dist(vec, 0, 2)), (1, _dist(vec, 0, 1))], (1, 0): [(0, _dist(vec, 1, 0)), (2, _dist(vec, 1, 2))],
             (2, 0): [(0, _dist(vec, 2, 0)), (1, _dist(vec, 2, 1))]}
    return R.make_model("f32", 4, 10, ids, vec, layer, lists, 2)


def generated(seed, T="f32", n=12, dim=6, M=3, layer=None, ids=None, deg0=None, degU=None):
    """a model with true Hamming distances: every point links to random points that reach the layer, at most deg0 / degU of them"""
    rng = np.random.default_rng(seed)
    vec = rng.integers(0, 3, (n, dim)).astype(R.DTYPE[T])
    layer = list(layer) if layer is not None else [0] * (n - 3) + [1, 1, 2][:min(n, 3)]
    layer = layer[:n]
    ids = list(ids) if ids is not None else list(range(n))
    lists = {}
    for p in range(n):
        for l in range(layer[p] + 1):
            cand = [q for q in range(n) if q != p and layer[q] >= l]
            cap = (2 * M if deg0 is None else deg0) if l == 0 else (M if degU is None else degU)
            pick = [cand[i] for i in rng.permutation(len(cand))[:cap]]
            lists[(p, l)] = [(q, _dist(vec, p, q)) for q in pick]
    return R.make_model(T, M, 24, ids, vec, layer, lists, int(np.argmax(layer)))


def _valid():
    V = {}
    V["three_points_by_hand"] = (three_points(), lambda m: len(m["ids"]) == 3 and m["ids"] == [0, 2, 1] and m["layer"][m["entry"]] == 1)
    for i, T in enumerate(("f32", "u32", "u64", "u16")):
        V["element_type_" + T] = (generated(10 + i, T=T), lambda m, T=T: m["T"] == T and m["vectors"].dtype == R.DTYPE[T])
    perm = [5, 0, 7, 2, 9, 4, 11, 6, 1, 8, 3, 10]
    V["ids_a_permutation_data_in_another_order"] = (generated(20, ids=perm), lambda m: sorted(m["ids"]) == list(range(12)) and m["ids"] != sorted(m["ids"])
                                                   and R.expected_index(m)["dense"] and not np.array_equal(R.expected_index(m)["data"], m["vectors"]))
    V["caller_ids_not_0_to_n"] = (generated(21, ids=[1000 + 7 * i for i in range(11)] + [2 ** 63 + 5]),
                                  lambda m: not R.expected_index(m)["dense"] and np.array_equal(R.expected_index(m)["data"], m["vectors"]))
    V["layers_0_1_5_15_with_empty_layers_between"] = (generated(22, layer=[0] * 6 + [1, 1, 5, 5, 15, 15]),
                                                      lambda m: sorted(set(m["layer"])) == [0, 1, 5, 15] and all(not m["order"][L] for L in (2, 3, 4, 6, 14)))
    V["lists_of_exactly_2M_and_M"] = (generated(23, n=14, M=4, layer=[0] * 8 + [1] * 6),
                                      lambda m: max(len(v) for (p, l), v in m["lists"].items() if l == 0) == 8
                                      and max(len(v) for (p, l), v in m["lists"].items() if l == 1) == 4)
    big = generated(24, n=257, dim=4, M=128, layer=[0] * 256 + [1], deg0=3)
    big["lists"][(0, 0)] = [(q, _dist(big["vectors"], 0, q)) for q in range(256, 1, -1)]
    V["M_128_with_a_255_entry_list"] = (big,
                                        lambda m: m["M"] == 128 and max(len(v) for v in m["lists"].values()) == 255)
    m01 = three_points()
    m01["vectors"] = np.array([[1, 2, 3, 4], [7, 7, 7, 7], [1, 2, 3, 4]], np.float32)
    m01["lists"] = {(0, 0): [(2, np.float32(0.0)), (1, np.float32(1.0))], (1, 0): [(0, np.float32(1.0))], (2, 0): [(0, np.float32(0.0)), (1, np.float32(1.0))]}
    V["distances_0_and_1"] = (m01, lambda m: {float(d) for v in m["lists"].values() for _, d in v} == {0.0, 1.0})
    tie = generated(25, n=9, dim=4, M=4, layer=[0] * 8 + [1])
    tie["lists"][(0, 0)] = [(q, np.float32(0.5)) for q in (7, 3, 5, 1, 6)]
    V["equal_distances_ordered_by_id"] = (tie, lambda m: [q for q, _ in m["lists"][(0, 0)]] == [7, 3, 5, 1, 6]
                                          and R.expected_index(m)["nbr0"][0, :5].tolist() == [1, 3, 5, 6, 7])
    V["a_single_point"] = (R.make_model("u16", 2, 1, [0], np.array([[9, 8, 7]], np.uint16), [0], {}, 0), lambda m: len(m["ids"]) == 1 and not m["lists"])
    long_name = b"x" * (4096 - len(R.DISTNAME)) + R.DISTNAME
    nm = three_points()
    nm["distname"] = long_name
    V["distance_name_of_4096_bytes"] = (nm, lambda m: len(m["distname"]) == 4096)
    return V


VALID = _valid()


def base():
    """seven points, M = 2: p0..p2 on layer 0, p3..p5 on layer 1, p6 on layer 2 (the entry point)"""
    return generated(30, n=7, dim=4, M=2, layer=[0, 0, 0, 1, 1, 1, 2])


def _patch(b, off, fmt, *v):
    raw = struct.pack("<" + fmt, *v)
    return b[:off] + raw + b[off + len(raw):]


def _only_field_differs(new, old, off, size):
    return len(new) == len(old) and new != old and new[:off] == old[:off] and new[off + size:] == old[off + size:]


def _refused():
    Rf = {}
    bm = base()
    g0, d0, off = R.write(bm, layout=True)
    assert R.verify(g0, d0)[0] == OK
    n, dim = 7, 4

    def field(name, code, where, fmt, *v):
        """the base with one named field of one file changed"""
        o, size = off[where], struct.calcsize("<" + fmt)
        g, d = (_patch(g0, o, fmt, *v), d0) if where.startswith("g.") else (g0, _patch(d0, o, fmt, *v))
        Rf[name] = (g, d, code, lambda: _only_field_differs(g, g0, o, size) if where.startswith("g.") else _only_field_differs(d, d0, o, size))

    def model(name, code, change, promise):
        """the base model with one thing changed before it is written (the writer checks nothing)"""
        m = base()
        change(m)
        g, d = R.write(m)
        Rf[name] = (g, d, code, lambda: promise(m))

    # description
    field("format_2_magic", UNSUPPORTED, "g.magic", "I", R.MAGD2)
    field("another_magic", IO, "g.magic", "I", 0x12345678)
    sizes = dict(magic=4, dumpmode=1, M=1, nbl=1, ef=8, n=8, dim=8, distlen=8, dist=len(R.DISTNAME), tlen=8, t=3)
    for f, size in sizes.items():
        cut = off["g." + f] + size // 2
        Rf["description_cut_inside_" + f] = (g0[:cut], d0, IO, lambda cut=cut, f=f, size=size: off["g." + f] <= cut < off["g." + f] + size)
    model("name_length_4097", IO, lambda m: m.update(distname=b"y" * (4097 - len(R.DISTNAME)) + R.DISTNAME), lambda m: len(m["distname"]) == 4097)
    field("light_dump", UNSUPPORTED, "g.dumpmode", "B", 0)
    field("layer_byte_15_in_the_description", IO, "g.nbl", "B", 15)
    field("layer_byte_15_after_the_description", IO, "g.nbl2", "B", 15)
    model("distance_not_hamming", UNSUPPORTED, lambda m: m.update(distname=b"anndists::dist::distances::DistL2"), lambda m: b"DistHamming" not in m["distname"])
    field("unknown_T", UNSUPPORTED, "g.t", "3s", b"f64")
    field("M_1", IO, "g.M", "B", 1)
    field("n_0", IO, "g.n", "Q", 0)
    field("n_2p31", IO, "g.n", "Q", 1 << 31)
    field("dim_0", IO, "g.dim", "Q", 0)
    field("dim_2p31", IO, "g.dim", "Q", 1 << 31)
    field("ef_2p32", IO, "g.ef", "Q", 1 << 32)
    # data file
    field("data_magic_wrong", IO, "d.magic", "I", R.MAGV ^ 1)
    field("data_dimension_differs", IO, "d.dim", "Q", dim + 1)
    field("vector_record_magic_wrong", IO, "d.vec1.magic", "I", R.MAGP)
    field("vector_nbytes_wrong", IO, "d.vec1.nbytes", "Q", 4 * dim - 1)
    Rf["data_cut_inside_the_last_vector"] = (g0, d0[:-2], IO, lambda: len(d0) - 2 > off["d.vec6.payload"])
    extra = struct.pack("<IQQ", R.MAGV, 7, 4 * dim) + bytes(4 * dim)
    Rf["one_vector_too_many"] = (g0, d0 + extra, IO, lambda: len(extra) == 20 + 4 * dim)
    field("an_id_twice", IO, "d.vec1.id", "Q", bm["ids"][0])
    # graph file
    field("layer_header_missing", IO, "g.layer3.magic", "I", 0)
    field("layer_claims_more_points_than_are_left", IO, "g.layer1.np", "Q", 5)
    field("layer_claims_2p64_minus_3_points", IO, "g.layer1.np", "Q", (1 << 64) - 3)
    field("point_magic_wrong", IO, "g.point1.magic", "I", R.MAGL)
    field("point_layer_byte_differs_from_its_layer", IO, "g.point3.layer", "B", 0)
    field("a_point_filed_twice", IO, "g.point1.id", "Q", bm["ids"][0])
    field("a_point_id_the_data_file_lacks", IO, "g.point1.id", "Q", 99)
    field("a_neighbour_id_the_data_file_lacks", IO, "g.point0.nbr0.1.id", "Q", 99)
    field("distance_nan", IO, "g.point0.nbr0.0.dist", "I", 0x7FC00000)
    field("distance_minus_half", IO, "g.point0.nbr0.0.dist", "f", -0.5)
    field("distance_1p5", IO, "g.point0.nbr0.0.dist", "f", 1.5)
    model("neighbours_above_the_points_layer", IO, lambda m: m["lists"].update({(0, 1): [(3, np.float32(0.5))]}), lambda m: m["layer"][0] == 0 and (0, 1) in m["lists"])
    model("layer_0_list_of_2M_plus_1", IO, lambda m: m["lists"].update({(0, 0): [(q, np.float32(0.25)) for q in (1, 2, 3, 4, 5)]}),
          lambda m: len(m["lists"][(0, 0)]) == 2 * m["M"] + 1)
    model("upper_list_of_M_plus_1", IO, lambda m: m["lists"].update({(3, 1): [(q, np.float32(0.25)) for q in (4, 5, 6)]}), lambda m: len(m["lists"][(3, 1)]) == m["M"] + 1)
    model("fewer_points_than_n", IO, lambda m: m["order"][0].remove(2), lambda m: sum(len(o) for o in m["order"]) == len(m["ids"]) - 1)
    Rf["entry_point_missing"] = (g0[:-13], d0, IO, lambda: len(g0) - 13 == off["g.entry.id"])
    Rf["entry_point_cut"] = (g0[:-1], d0, IO, lambda: len(g0) - 1 > off["g.entry.id"])
    field("entry_point_unknown", IO, "g.entry.id", "Q", 99)
    Rf["a_byte_after_the_entry_point"] = (g0 + b"\0", d0, IO, lambda: True)
    field("entry_point_not_on_the_top_layer", INVALID, "g.entry.id", "Q", bm["ids"][3])
    model("upper_link_to_a_point_below_that_layer", INVALID, lambda m: m["lists"].update({(3, 1): [(4, np.float32(0.5)), (0, np.float32(0.5))]}),
          lambda m: m["layer"][0] < 1 and any(q == 0 for q, _ in m["lists"][(3, 1)]))
    # hostile headers: a whole description that names sizes no file of this length can hold - nothing may be allocated from them
    for name, nn, dd, T in (("hostile_n_and_dim_2p31_minus_1_u64", (1 << 31) - 1, (1 << 31) - 1, b"u64"), ("hostile_n_2p31_minus_1_dim_18000_f32", (1 << 31) - 1, 18000, b"f32"),
                            ("hostile_n_2p31_minus_1_dim_1", (1 << 31) - 1, 1, b"f32")):
        g = struct.pack("<IBBBQQQQ", R.MAGD3, 1, 128, 16, 1600, nn, dd, len(R.DISTNAME)) + R.DISTNAME + struct.pack("<Q", 3) + T
        d = struct.pack("<IQ", R.MAGV, dd)
        Rf[name] = (g, d, IO, lambda g=g, d=d: len(g) == 88 and len(d) == 12 and R.describe(g)[0] == OK)
    return Rf


REFUSED = _refused()
HOSTILE = [k for k in REFUSED if k.startswith("hostile_")]
_SWEEP = None


def sweep_files():
    """[(tag, graph, data, code, model or None)] over three_points(): every proper prefix of each file with the other intact, every byte once 0xFF, once ^ 1"""
    global _SWEEP
    if _SWEEP is None:
        g0, d0 = R.write(three_points())
        out = []
        for which, b in (("g", g0), ("d", d0)):
            muts = [("p%d" % i, b[:i]) for i in range(len(b))]
            muts += [("f%d" % i, b[:i] + b"\xff" + b[i + 1:]) for i in range(len(b)) if b[i] != 0xFF]
            muts += [("x%d" % i, b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]) for i in range(len(b))]
            for tag, mb in muts:
                g, d = (mb, d0) if which == "g" else (g0, mb)
                code, mo = R.verify(g, d)
                out.append((which + tag, g, d, code, mo))
        _SWEEP = out
    return _SWEEP
