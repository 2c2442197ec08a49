"""Every operation family against its usual reference on POISONED scratch. Device temporaries (the scratch slots of a context, gs_scratch.hpp; the per-call
buffers of an index) are never cleared between uses, and the rest of the suite runs each operation in one order on one context, mostly on first use of
its memory. Here gs_debug_mem_fill / gs_index_debug_fill_scratch fill that memory with a chosen byte before it is handed out: a kernel that reads a
counter, a bitmap word, a table entry or a tail element nothing wrote gives a wrong answer instead of a right one by luck.

Each case is a function run(ctx, poke) -> tuple of arrays and a reference computed once (the oracle, or the pyref_* restatement the family's own test
uses; shapes, generators and environment switches are those of the named tests). A case runs with the fill off, then under 0x00 (what a missing clear
needs), 0x01 (neither zero nor a sentinel, and a small number in every integer width: a stale value used as a length or an index stays modest) and
0xFF (what a missing sentinel needs; NaN as f32), in that order, and every output must equal the reference bit for bit after each run. Within a family
the larger shape comes first, so that the smaller ones run in slots larger than they need; the last test replays every case in reverse order under
0x01, so that each family also runs in another family's leftovers. The context is the module's own: the session context's slots may be gigabytes."""
import functools
import gzip
import os
import zlib

import numpy as np
import pytest

import helpers as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

FILLS = (None, 0x00, 0x01, 0xFF)
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def stale_ctx():
    import gsearch_amd as G
    ctx = G.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture
def fill_guard():
    """no other test ever runs in fill mode"""
    import gsearch_amd as G
    try:
        yield
    finally:
        G.debug_mem_fill(None)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("stale_scratch")


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == bool:
        return a.view(np.uint8)
    assert a.dtype.kind in "ui", a.dtype
    return a


def _same(got, ref):
    """integers by value, floats by their bits: no tolerance"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return False
    if got.dtype.kind == "f" or ref.dtype.kind == "f":
        return got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref))
    return np.array_equal(_bits(got), _bits(ref))


class Case:
    """make(workdir) -> (run, ref): the inputs and the reference are built once, at the first use. run(ctx, poke) -> tuple of arrays; index cases call
    poke(hn) before EVERY index call. err_has / err_lacks: what the verbose output of every run must (not) hold: the device form the case is about ran."""
    def __init__(self, family, name, env, make, err_has=(), err_lacks=()):
        self.family, self.name, self.env, self.make = family, name, env, make
        self.err_has, self.err_lacks = err_has, err_lacks
        self._built = None

    def built(self, workdir):
        if self._built is None:
            self._built = self.make(workdir)
        return self._built


CASES = []


def case(family, name, env=None, **kw):
    def deco(make):
        CASES.append(Case(family, name, dict(env or {}), make, **kw))
        return make
    return deco


def _run_case(c, ctx, workdir, monkeypatch, capfd, fills):
    import gsearch_amd as G
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    run, ref = c.built(workdir)
    for fill in fills:
        G.debug_mem_fill(fill)

        def poke(hn, fill=fill):
            if fill is not None:
                hn.debug_fill_scratch(fill)
        capfd.readouterr()
        got = run(ctx, poke)
        err = capfd.readouterr().err
        G.debug_mem_fill(None)
        tag = (c.family, c.name, "fill off" if fill is None else "fill 0x%02X" % fill)
        assert len(got) == len(ref), tag
        for i, (g, r) in enumerate(zip(got, ref)):
            assert _same(g, r), tag + ("output %d" % i,)
        for s in c.err_has:
            assert s in err, tag + (s, err[-600:])
        for s in c.err_lacks:
            assert s not in err, tag + (s, err[-600:])


# ------------------------------------------------------------------------------------------------------------------------------------------------
# sketchers
def _oracle_sketch(k, m, algo, genomes, data="dna"):
    recs = [r for g in genomes for r in g]
    goff = np.cumsum([0] + [len(g) for g in genomes]).astype(np.uint64)
    seq, rs, rl = O.pack_dna(recs) if data != "aa" else O.filter_aa(recs)
    return O.sketch_batch(O.params(k, m, algo, data), seq, rs, rl, goff, nthreads=min(8, os.cpu_count() or 1))


def _sketch_case(k, m, algo, genomes, data="dna", info=None):
    """info: what ctx.last_sketch_info() must report after the call (the device form the case is about)"""
    import gsearch_amd as G
    ref = _oracle_sketch(k, m, algo, genomes, data)

    def run(ctx, poke):
        sk = G.sketcher_for(G.SeqSketcherParams(k, m, algo, data), ctx)
        got = sk.sketch_genomes(genomes)
        if info:
            got_info = ctx.last_sketch_info()
            assert info(got_info), got_info
        return (got,)
    return run, (ref,)


# --- OPH (test_gpu_parity.py: test_sketch_split_over_workgroups, test_sketch_dna_matches_oracle, test_sketch_densification_matches_oracle)
@case("oph", "one_long_genome_split_over_workgroups")
def _(wd):
    rng = np.random.default_rng(9)
    return _sketch_case(21, 12000, "optdens", [[H.dna_ascii(H.rand_dna(rng, 1200000))]], info=lambda i: i["workgroups_per_genome"] > 1 and i["table_in_lds"])


# the slot table moves to global memory behind the 2-byte LDS filter when m * sizeof(slot) > 160 KB - 256 (gs_sketch.hip min_geom): with the 8-byte
# slots of test_config4_sketch_aa_super2_bench_shape (AA, k = 7, super2; sketch_size 24000 there), stepping down, 20449 is the last that reports it
GLOBAL_TABLE_M = 20449


@case("oph", "smallest_sketch_with_the_slot_table_in_global_memory")
def _(wd):
    import gsearch_amd as G
    rng = np.random.default_rng(404)
    fam = H.family(rng, 400000, [0.02], alphabet=20)
    genomes = [[H.aa_ascii(g)] for g in fam] + [[H.aa_ascii(fam[0])[:150000] + b"*XBZ-", H.aa_ascii(fam[1])[10:170000].lower()]]
    run0, ref = _sketch_case(7, GLOBAL_TABLE_M, "super2", genomes, "aa", info=lambda i: not i["table_in_lds"])

    def run(ctx, poke):
        got = run0(ctx, poke)
        G.sketcher_for(G.SeqSketcherParams(7, GLOBAL_TABLE_M - 1, "super2", "aa"), ctx).sketch_genomes(genomes[:1])
        assert ctx.last_sketch_info()["table_in_lds"]              # one slot fewer still fits the LDS: GLOBAL_TABLE_M is the smallest
        return got
    return run, ref


def _dna_batch(seed, length):
    """test_sketch_dna_matches_oracle: a family, a multi-record genome with N's / lower case / short / empty records, a genome without a k-mer"""
    rng = np.random.default_rng(seed)
    fam = H.family(rng, length, [0.001, 0.01, 0.05])
    genomes = [[H.dna_ascii(g)] for g in fam]
    g0 = H.dna_ascii(fam[0])
    genomes.append([g0[:7000] + b"NNNNnnnn" + g0[7000:9000].lower(), b"ACGT", b"", g0[9000:9031], g0[20000:45003]])
    genomes.append([b"ACGTN"])
    return genomes


@case("oph", "optdens_k16_m1024")
def _(wd):
    return _sketch_case(16, 1024, "optdens", _dna_batch(16 * 1000 + 1024, 50000))


@case("oph", "revoptdens_k14_m700")
def _(wd):
    return _sketch_case(14, 700, "revoptdens", _dna_batch(14 * 1000 + 700, 50000))


@case("oph", "short_genomes_leave_empty_slots_to_densify")
def _(wd):
    rng = np.random.default_rng(5)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (40, 300, 1500, 5000)]
    run, ref = _sketch_case(21, 4096, "optdens", genomes)
    assert (ref[0][1:] != ref[0][0]).any()
    return run, ref


# --- SuperMinHash (test_sketch_super_matches_oracle, test_sketch_super_cold_path_matches_oracle)
def _super_batch(k, m):
    rng = np.random.default_rng(k * 7 + m)
    fam = H.family(rng, 150000, [0.01, 0.05])
    genomes = [[H.dna_ascii(g)] for g in fam]
    genomes.append([H.dna_ascii(fam[0])[:70000], b"ACGTNN", H.dna_ascii(fam[1])[1000:90000]])
    return genomes


@case("smh", "super_k21_m2000")
def _(wd):
    return _sketch_case(21, 2000, "super", _super_batch(21, 2000))


@case("smh", "super2_k21_m2000")
def _(wd):
    return _sketch_case(21, 2000, "super2", _super_batch(21, 2000))


def _cold_batch():
    rng = np.random.default_rng(17)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (30, 500, 3000)] + [[b"ACGT"]]
    genomes.append([H.dna_ascii(H.rand_dna(rng, 40000))])
    genomes.append([H.dna_ascii(H.rand_dna(rng, 700)), b"ACG", H.dna_ascii(H.rand_dna(rng, 90))])
    genomes.append([b"ACGT" * 40])
    return genomes


@case("smh", "super2_cold_path")
def _(wd):
    return _sketch_case(21, 1024, "super2", _cold_batch())


@case("smh", "super2_cold_path_serial", env={"GS_SMH_COLD_SERIAL": "1"})
def _(wd):
    return _sketch_case(21, 1024, "super2", _cold_batch())


@case("smh", "super_cold_path")
def _(wd):
    return _sketch_case(21, 1024, "super", _cold_batch())


# --- ProbMinHash (test_sketch_prob_tiered_form_and_its_exact_fallback, .._hands_flagged_genomes_to_the_sorted_form, .._bucketed_form_matches_oracle)
@functools.lru_cache(maxsize=None)
def _tiered_batch():
    rng = np.random.default_rng(606)
    base = [H.dna_ascii(H.rand_dna(rng, n)) for n in (760_000, 640_000, 700_000)]
    rep = base[0][1000:6000]
    genomes = [
        [base[0]],
        [base[1][:300_000] + rep * 50 + base[1][300_000:]],
        [base[2] + base[2][: len(base[2]) // 4]],
        [base[0][:200_000], b"ACGTNN", base[1][1000:420_000], b"", base[2][5000:150_000].lower()],
        [base[1][:30_000]],
        [base[2][:350_000] + b"A" * 90_000 + base[2][350_000:]],
        [b"ACGT" * 40_000 + base[0][:600_000]],
        [base[1]],
        [base[2][i:i + 997] for i in range(0, 700_000, 997)],
    ]
    return genomes, _oracle_sketch(21, 1000, "prob", genomes)


def _tiered_case():
    import gsearch_amd as G
    genomes, ref = _tiered_batch()

    def run(ctx, poke):
        return (G.sketcher_for(G.SeqSketcherParams(21, 1000, "prob"), ctx).sketch_genomes(genomes),)
    return run, (ref,)


@case("prob", "tiered_cap_fails", env={"GS_PROB_CAP_C": "-6", "GS_PROB_VERBOSE": "1"}, err_has=("tiered form flagged genomes", "[0,"))
def _(wd):
    return _tiered_case()


@case("prob", "tiered_two_walk", env={"GS_PROB_TWOWALK": "1", "GS_PROB_VERBOSE": "1"}, err_has=("tiered form flagged genomes",),
      err_lacks=("no room for the scratch", "flagged genomes [0,"))
def _(wd):
    return _tiered_case()


@case("prob", "flagged_genomes_handed_to_the_sorted_form")
def _(wd):
    rng = np.random.default_rng(77)
    a = H.dna_ascii(H.rand_dna(rng, 150000)); b = H.dna_ascii(H.rand_dna(rng, 120000))
    genomes = [[a], [b[:60000] + b"A" * 90000 + b[60000:]], [b], [b"ACGT" * 40000 + a[:30000]]]
    return _sketch_case(21, 1000, "prob", genomes)


def _prob_batch(k, m, data, length):
    rng = np.random.default_rng(k * 131 + m)
    if data == "dna":
        fam = H.family(rng, length, [0.01, 0.05])
        asc = [H.dna_ascii(g) for g in fam]
        rep = asc[0][:400] * 40
        genomes = [[a] for a in asc]
        genomes.append([asc[0][: length // 2] + rep, b"ACGTNN", asc[1][1000: length // 2], rep, asc[2][: length // 3]])
        genomes.append([asc[1][:5000]])
        genomes.append([asc[2] + asc[2][: length // 4]])
        genomes.append([b"ACG"])
        return genomes
    fam = H.family(rng, length, [0.02], alphabet=20)
    asc = [H.aa_ascii(g) for g in fam]
    rep = asc[0][:150] * 30
    return [[a] for a in asc] + [[asc[0][: length // 2] + rep + b"*", rep, asc[1][: length // 2]], [b"MKV"], [asc[1] + asc[1][: length // 5]]]


PROB_IMPL_ENV = {"tiers": {}, "buckets": {"GS_PROB_IMPL": "buckets"}, "buckets_one_level": {"GS_PROB_IMPL": "buckets", "GS_PROB_ONELEVEL": "1"},
                 "sort": {"GS_PROB_IMPL": "sort"}}
for _k, _m, _data, _len in ((7, 600, "aa", 100000), (16, 512, "dna", 90000)):
    for _impl, _env in PROB_IMPL_ENV.items():
        @case("prob", "%s_k%d_m%d" % (_impl, _k, _m), env=_env)
        def _(wd, k=_k, m=_m, data=_data, length=_len):
            return _sketch_case(k, m, "prob", _prob_batch(k, m, data, length), data)


# --- HLL (test_sketch_hll_register_file_beyond_lds, test_sketch_hll_survivor_lists, test_sketch_hll_matches_oracle, test_sketch_hll_cold_path_matches_oracle)
@case("hll", "register_file_in_global_memory_m50000")
def _(wd):
    rng = np.random.default_rng(50000)
    fam = H.family(rng, 1600000, [0.03])
    genomes = [[H.dna_ascii(g)] for g in fam] + [[H.dna_ascii(H.rand_dna(rng, 5000))], [b"ACGT"]]
    return _sketch_case(21, 50000, "hll", genomes)


@functools.lru_cache(maxsize=None)
def _survivor_batch():
    rng = np.random.default_rng(41)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (1_200_000, 400_011, 2_300_000)]
    genomes.append([H.dna_ascii(H.rand_dna(rng, 700_000)), b"ACGTNNACGT", H.dna_ascii(H.rand_dna(rng, 650_007))])
    return genomes, _oracle_sketch(21, 4000, "hll", genomes)


def _survivor_case():
    import gsearch_amd as G
    genomes, ref = _survivor_batch()

    def run(ctx, poke):
        return (G.sketcher_for(G.SeqSketcherParams(21, 4000, "hll"), ctx).sketch_genomes(genomes),)
    return run, (ref,)


@case("hll", "survivor_lists_overflow", env={"GS_HLL_SURVIVORS": "4096", "GS_HLL_SURVIVORS_MINCHUNKS": "4"})
def _(wd):
    return _survivor_case()


@case("hll", "survivor_lists_off", env={"GS_HLL_SURVIVORS": "0", "GS_HLL_SURVIVORS_MINCHUNKS": "4"})
def _(wd):
    return _survivor_case()


@case("hll", "k21_m2000_150kb")
def _(wd):
    rng = np.random.default_rng(21 * 31 + 2000)
    length = 150000
    fam = H.family(rng, length, [0.01, 0.05])
    genomes = [[H.dna_ascii(g)] for g in fam]
    g0 = H.dna_ascii(fam[0])
    genomes.append([g0[:length // 3] + b"NNNNnn" + g0[length // 3:length // 2].lower(), b"ACGT", g0[length // 2:]])
    return _sketch_case(21, 2000, "hll", genomes)


@case("hll", "cold_path")
def _(wd):
    rng = np.random.default_rng(23)
    genomes = [[H.dna_ascii(H.rand_dna(rng, n))] for n in (30, 400, 3000, 20000)] + [[b"ACGT"], [b""], [b"ACGT" * 50]]
    genomes.append([H.dna_ascii(H.rand_dna(rng, 900)), b"ACG", H.dna_ascii(H.rand_dna(rng, 100))])
    genomes.append([H.dna_ascii(H.rand_dna(rng, 300000))])
    return _sketch_case(21, 1024, "hll", genomes)


# --- HyperMinHash (test_gpu_hmh.py: test_registers_bit_exact, test_split_genome_equals_max_of_pieces, test_counts_exact_on_uneven_shapes)
def _hmh_genome(rng, k, n):
    s = bytearray(H.dna_ascii(H.rand_dna(rng, n)))
    if n > 50:
        s[n // 3:n // 3 + 7] = b"NNNNNNN"
        s[n // 2:n // 2 + 40] = bytes(s[n // 2:n // 2 + 40]).lower()
        cut = n * 2 // 3
        return [bytes(s[:cut]), bytes(s[cut:]), b"ACGTN"[: max(1, k - 1)]]
    return [bytes(s)]


def _hmh_case(genomes, k, info):
    import gsearch_amd as G
    import pyref_hmh as PR
    ref = np.stack([PR.sketch(g, k) for g in genomes])

    def run(ctx, poke):
        got = G.HyperMinHashSketch.for_k(k, ctx).sketch_genomes(genomes)
        got_info = ctx.last_sketch_info()
        assert info(got_info), got_info
        return (got,)
    return run, (ref,)


@case("hmh", "one_genome_split_over_workgroups")
def _(wd):
    return _hmh_case([_hmh_genome(np.random.default_rng(7), 21, 300_000)], 21, lambda i: i["workgroups_per_genome"] > 1)


@case("hmh", "registers_k21")
def _(wd):
    rng = np.random.default_rng(100 + 21)
    genomes = [_hmh_genome(rng, 21, n) for n in (0, 20, 21, 22, 1000, 200_000)] + [[b""]]
    genomes += [_hmh_genome(rng, 21, 3000) for _ in range(600)]          # more genomes than 2 x CUs: one workgroup each
    return _hmh_case(genomes, 21, lambda i: i["workgroups_per_genome"] == 1 and i["table_in_lds"])


@functools.lru_cache(maxsize=None)
def _hmh_rows():
    """test_counts_exact_on_uneven_shapes: all sketches large (the closed branch), Q x R = 131 x 72"""
    import pyref_hmh as PR
    rng = np.random.default_rng(5)
    big = PR.sketch([H.dna_ascii(H.rand_dna(rng, 3_000_000))], 21)
    rows = []
    for i in range(203):
        x = big.copy()
        flip = rng.random(16384) < rng.uniform(0.0, 0.9)
        x[flip] = rng.integers(1 << 10, 12 << 10, int(flip.sum()), dtype=np.uint16)
        if i % 7 == 0:
            x[rng.random(16384) < 0.05] = 0
        rows.append(x)
    S = np.stack(rows)
    card = np.array([PR.cardinality(s) for s in S], np.uint64)
    return S, card


@case("hmh", "similarity_qxc_uneven_shape")
def _(wd):
    import gsearch_amd as G
    import pyref_hmh as PR
    S, card = _hmh_rows()
    Q, R = S[:131], S[131:]
    qi = np.arange(0, 131, 5)
    ref = np.array([[PR.similarity(Q[i], R[j], int(card[i]), int(card[131 + j])) for j in range(len(R))] for i in qi], np.float64)

    def run(ctx, poke):
        return (G.hmh_similarity_qxc(Q, R, ctx=ctx)[qi],)
    return run, (ref,)


@case("hmh", "cardinality")
def _(wd):
    import gsearch_amd as G
    S, card = _hmh_rows()
    rows = np.concatenate([S[:37], np.zeros((1, 16384), np.uint16)])

    def run(ctx, poke):
        return (np.asarray(G.hmh_cardinality(rows, ctx=ctx), np.uint64),)
    return run, (np.concatenate([card[:37], np.zeros(1, np.uint64)]),)


# --- FracMinHash (test_gpu_aai.py: test_sketch_large_proteome_split_and_mixed_batch, test_similarity_counts_exact)
AA = b"ACDEFGHIKLMNPQRSTVWY"


def _protein(rng, n):
    return bytes(np.frombuffer(AA, np.uint8)[rng.integers(0, len(AA), n)])


def _csr(rows):
    return (np.concatenate([np.asarray(r, np.uint64) for r in rows] + [np.zeros(0, np.uint64)]), np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64))


@case("frac", "sketch_batch_with_a_large_split_proteome")
def _(wd):
    import gsearch_amd as G
    import pyref_aai as PR
    rng = np.random.default_rng(12)
    big = [_protein(rng, 400_000) for _ in range(4)]
    genomes = [big, [_protein(rng, 5000)], [b"MKVL"], [_protein(rng, 200_000), _protein(rng, 7)]]
    shapes = [(100, 5120), (1, 5120)]                       # scaled = 1: every hash survives the filter (the radix path of the large proteome)
    ref = sum((_csr([PR.sketch(g, 7, scaled, num) for g in genomes]) for scaled, num in shapes), ())

    def run(ctx, poke):
        return sum((_csr(G.FracMinHashSketch(7, scaled, num, ctx=ctx).sketch_genomes(genomes)) for scaled, num in shapes), ())
    return run, ref


@case("frac", "similarity_qxc_130x70")
def _(wd):
    import gsearch_amd as G
    import pyref_aai as PR
    nq, nr, num = 130, 70, 64
    rng = np.random.default_rng(nq * 1000 + nr)

    def family(n, size, share):
        base = np.unique(rng.integers(0, 2 ** 64, size * 2, dtype=np.uint64))
        out = []
        for _ in range(n):
            m = int(rng.integers(0, size + 1))
            keep = base[rng.random(len(base)) < share]
            own = rng.integers(0, 2 ** 64, m, dtype=np.uint64)
            s = np.unique(np.concatenate([keep, own]))
            out.append(s[: min(len(s), int(rng.integers(0, num + 1)))])
        return out
    Q, R = family(nq, 80, 0.4), family(nr, 80, 0.4)
    Q[0] = np.zeros(0, np.uint64); Q[1] = R[0].copy(); Q[2] = R[2][:num].copy()
    com, uni = np.zeros((nq, nr), np.uint32), np.zeros((nq, nr), np.uint32)
    for i, a in enumerate(Q):
        for j, b in enumerate(R):
            com[i, j], uni[i, j] = PR.similarity_counts(a, b, num)
    sim = com.astype(np.float64) / np.maximum(1, uni).astype(np.float64)

    def run(ctx, poke):
        s, c, u = G.frac_similarity_qxc(Q, R, num, return_counts=True, ctx=ctx)
        return np.asarray(s, np.float64), np.asarray(c).astype(np.uint32), np.asarray(u).astype(np.uint32)
    return run, (sim, com, uni)


# --- the host-pointer sketch call (gs_sketch_batch stages through the SKB_* slots; every sketch case above goes through it with larger inputs)
@case("hostptr", "sketch_batch_small_after_large")
def _(wd):
    rng = np.random.default_rng(0)
    fam = H.family(rng, 60000, [0.01, 0.05])
    return _sketch_case(21, 2000, "optdens", [[H.dna_ascii(g)] for g in fam])


# ------------------------------------------------------------------------------------------------------------------------------------------------
# files (test_gpu_inflate.py: test_sketch_files_bgzf_members_on_the_device, test_inflate_matches_zlib)
def _fasta(records, width, nl=b"\n"):
    out = []
    for name, s in records:
        out.append(b">" + name + nl)
        out += [s[o:o + width] + nl for o in range(0, len(s), width)]
    return b"".join(out)


@case("files", "sketch_files_plain_gzip_bgzf", env={"GS_GZIP_DEVICE": "1"})
def _(wd):
    import gsearch_amd as G
    rng = np.random.default_rng(11)
    seqs = [H.dna_ascii(H.rand_dna(rng, n)) for n in (150_000, 90_011, 200_000, 60_000)]
    texts = [_fasta([(b"g0 synthetic", seqs[0][:70_000] + b"NNNNNNNNNN" + seqs[0][70_000:110_000].lower() + seqs[0][110_000:])], 70),
             _fasta([(b"c%d" % i, seqs[1][i * 9000:(i + 1) * 9000 + 9]) for i in range(10)], 80, b"\r\n"),
             _fasta([(b"x", seqs[2][:120_000]), (b"rec2 capsid protein", b"ACGTACGTACGTACGTACGTACGTACGTACGTAC"), (b"y", seqs[2][120_000:])], 60),
             _fasta([(b"only", seqs[3])], 61)]
    paths, genomes = [], []
    for i, t in enumerate(texts):
        for ext, blob in ((".fna", t), (".fna.gz", gzip.compress(t, 6)), (".bgz.fna.gz", H.bgzf_bytes(t, block=20_000 + 9000 * i))):
            p = wd / ("f%d%s" % (i, ext))
            p.write_bytes(blob)
            paths.append(str(p))
            genomes.append([t[b:e] for _, b, e in G.fasta_scan(t)])
    ref = _oracle_sketch(21, 1500, "optdens", genomes)
    _, _, orl = O.pack_dna([r for g in genomes for r in g])
    goff = np.cumsum([0] + [len(g) for g in genomes])
    nrec = np.array([len(g) for g in genomes], np.uint64)
    nsym = np.array([int(orl[goff[i]:goff[i + 1]].sum()) for i in range(len(genomes))], np.uint64)

    def run(ctx, poke):
        sk = G.OptDensHashSketch.new(G.SeqSketcherParams(21, 1500, "optdens"), ctx)
        sig, nr, ns, st = sk.sketch_files(paths, pio=4, threads=2)
        assert st["gz_members_inflated_on_device"] > 0, st
        return sig, np.asarray(nr, np.uint64), np.asarray(ns, np.uint64)
    return run, (ref, nrec, nsym)


# both pipelines of gs_sketch_files at work, each on its own context (test_gpu_ingest_deal.py test_both_pipelines_run_groups_until_they_meet at its
# smallest shape): the .gz files dealt between the host decoders and the device inflater, the device side offered 128 members at every claim
@case("files", "sketch_files_dealt_between_both_pipelines", env={"GS_GZIP_DEVICE": "1", "GS_GZIP_DEAL_SHARE": "128"})
def _(wd):
    import gsearch_amd as G
    import ingest_deal_cases as D
    sub = wd / "dealt"
    sub.mkdir()
    corpus = D.Corpus(sub, D.N_DEALT)
    order = corpus.dealt(D.N_DEALT)
    paths = corpus.paths(order)
    ref = D.Reference(corpus.entries).rows(order, False)

    def run(ctx, poke):
        sk = G.OptDensHashSketch.new(G.SeqSketcherParams(D.K, D.M, D.ALGO), ctx)
        sig, nr, ns, st = sk.sketch_files(paths, pio=D.P, threads=4)
        assert 0 < st["gz_members_inflated_on_device"] < D.N_DEALT, st
        return sig, np.asarray(nr, np.uint64), np.asarray(ns, np.uint64)
    return run, ref


@case("files", "gunzip_batch")
def _(wd):
    import gsearch_amd as G
    rng = np.random.default_rng(77)

    def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
        return c.compress(data) + c.flush()
    dna = _fasta([(b"seq some description", H.dna_ascii(H.rand_dna(rng, 120_000)))], 80)
    members = [gz(b""), gz(b"A"), gz(dna, 1), gz(dna, 9), gz(dna[:50_000], 6, zlib.Z_FIXED), gz(b"A" * 30_000 + b"CG" * 20_000 + b"ACGTT" * 9_000),
               gz(bytes(rng.integers(0, 256, 40_000, dtype=np.uint8)), 6), gz(dna[:70_000], 0)]
    ref = tuple(np.frombuffer(zlib.decompress(m, 31), np.uint8) for m in members) + (np.zeros(len(members), np.int32),)

    def run(ctx, poke):
        res = G.gunzip_batch(ctx, members)
        return tuple(np.frombuffer(t, np.uint8) for _, t in res) + (np.array([st for st, _ in res], np.int32),)
    return run, ref


# ------------------------------------------------------------------------------------------------------------------------------------------------
# hamming (test_hamming_matches_oracle: m = 37, 70 x 100; the widening slots HAM_WIDE_* / HAMP_WIDE_* only exist for u16)
for _dt in (np.float32, np.uint32, np.uint64, np.uint16):
    @case("hamming", "qxc_and_pairs_%s" % np.dtype(_dt).name)
    def _(wd, dtype=_dt):
        import gsearch_amd as G
        db = H.synth_sig_db(5, 20, 37, 1, dtype=dtype)
        q = H.queries_from(db, 70, 2)
        rng = np.random.default_rng(3)
        ia, ib = rng.integers(0, len(q), 200), rng.integers(0, len(db), 200)
        ref = (O.hamming_qxc(q, db), O.hamming_pairs(q, db, ia, ib))

        def run(ctx, poke):
            dh = G.DistHamming(ctx)
            return dh.eval_qxc(q, db), dh.eval_pairs(q, db, ia, ib)
        return run, ref


# ------------------------------------------------------------------------------------------------------------------------------------------------
# index
def _graph_outputs(g, og):
    """the comparable part of an exported graph: adjacency beyond a node's degree is unspecified, so both sides are cut at the REFERENCE's degrees"""
    def cut(a, deg):
        a = np.asarray(a)
        return np.where(np.arange(a.shape[-1]) < np.asarray(og[deg])[..., None], a, 0).astype(np.uint32)
    out = [np.array([g["entry"], g["n_upper"]], np.int64), g["levels"], g["upidx"], g["deg0"], cut(g["nbr0"], "deg0"), cut(g["cnt0"], "deg0")]
    if og["n_upper"]:
        out += [g["degU"], cut(g["nbrU"], "degU")]
    return tuple(out)


def _search_case(db, oix, q, knbn, ef, M, efc, dtype=np.float32):
    """search on the oracle's graph, imported"""
    import gsearch_amd as G
    og = oix.export()
    ref = oix.parallel_search(q, knbn, ef, nthreads=min(8, os.cpu_count() or 1))

    def run(ctx, poke):
        hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(ctx), dtype=dtype, ctx=ctx)
        hn.import_graph(db, og)
        poke(hn)
        got = hn.search_arrays(q, knbn, ef)
        hn.close()
        return got
    return run, ref


# the build comes first: 6500 nodes, the largest index of the family (test_insert_prepass_builds_the_oracle_graph f32 M = 12 efc = 60;
# GS_SPARSE_L of test_insert_with_sparse_pair_rows_builds_the_oracle_graph - the list length is settled at the index's first dense batch, so it holds for the whole build)
@case("index", "build_search_insert_search", env={"GS_DIST_MODE": "dense", "GS_SPARSE_L": "192"})
def _(wd):
    import gsearch_amd as G
    m, M, efc, B = 64, 12, 60, 256
    db = H.synth_sig_db(130, 50, m, 321, jlo=0.05, jhi=0.9)
    first = 20 * B                                                     # whole batches (the graph depends on the batch boundaries); the pre-pass runs past 4096 nodes
    q = np.concatenate([H.queries_from(db[:first], 120, 5, frac=0.25), db[:20]])
    oix = O.Index(np.float32, m, M, efc, scale_modify=1.0, seed=4)
    refs, ographs = [], []
    for part in (db[:first], db[first:]):
        oix.parallel_insert(part, batch=B)
        ographs.append(oix.export())
        refs.append(oix.parallel_search(q, 10, 80, nthreads=min(8, os.cpu_count() or 1)))
    assert (ographs[1]["levels"][4096:] > 0).sum() >= 3
    ref = _graph_outputs(ographs[0], ographs[0]) + refs[0] + _graph_outputs(ographs[1], ographs[1]) + refs[1]

    def run(ctx, poke):
        hn = G.Hnsw.new(M, 100000, 16, efc, G.DistHamming(ctx), seed=4, insert_batch=B, ctx=ctx)
        hn.modify_level_scale(1.0); hn.set_extend_candidates(True)
        out = ()
        for step, part in enumerate((db[:first], db[first:])):
            poke(hn)
            hn.parallel_insert(part)
            poke(hn)
            out += _graph_outputs(hn.export_graph(), ographs[step])
            poke(hn)
            out += hn.search_arrays(q, 10, 80)
        hn.close()
        return out
    return run, ref


# the heavy-block path of the match-join: labels, pair lists, tile lists (test_gpu_join_blocks.py test_count_matrix_of_redundant_batches, its first shape)
@case("index", "count_matrix_of_a_redundant_batch", env={"GS_JOIN_VERBOSE": "1"}, err_has=("clusters",), err_lacks=(" 0 clusters",))
def _(wd):
    import gsearch_amd as G
    dtype, m, universe = np.float32, 800, 1600
    rng = np.random.default_rng(m + universe % 97)

    def rnd(shape):
        return rng.integers(0, universe, shape).astype(np.float32)
    roots = rnd((12, m))
    db = np.repeat(roots, 700, axis=0)
    J = rng.uniform(0.25, 0.95, (len(db), 1))
    mk = rng.random(db.shape) > J
    db[mk] = rnd(db.shape)[mk]
    db = np.ascontiguousarray(db[rng.permutation(len(db))])
    n = len(db)
    fam = rng.integers(0, 5, 550)
    q = roots[fam].copy()
    Jq = rng.uniform(0.2, 0.98, (len(q), 1))
    mk = rng.random(q.shape) > Jq
    q[mk] = rng.integers(0, universe, q.shape).astype(np.float32)[mk]
    un = rng.integers(0, universe, (60, m))
    q = np.concatenate([q, db[[5, 5, 77, 77]], un.astype(np.float32), db[rng.integers(0, n, 26)]])
    q[3, :40] = np.nan; q[4, 40:60] = -0.0; db[9, 40:60] = 0.0; db[10, :8] = np.nan
    q = np.ascontiguousarray(q[rng.permutation(len(q))])
    want = np.rint(O.hamming_qxc(q, db, nthreads=os.cpu_count()).astype(np.float64) * m).astype(np.uint16)
    graph = dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 16), np.uint32), cnt0=np.zeros((n, 16), np.uint32),
                 upidx=np.full(n, -1, np.int32), n_upper=0)

    def run(ctx, poke):
        hn = G.Hnsw.new(8, n, 16, 16, G.DistHamming(ctx), dtype=dtype, seed=1, ctx=ctx)
        hn.import_graph(db, graph)
        poke(hn)
        got = hn.count_matrix(q)
        hn.close()
        return (got,)
    return run, (want,)


@functools.lru_cache(maxsize=None)
def _noise_index():
    """test_dense_traversal_small_and_odd_ef: 3000 noise rows, every pair agrees in 19 +- 4 of 96 slots"""
    m = 96
    db = np.random.default_rng(502).integers(0, 5, (3000, m)).astype(np.float32)
    oix = O.Index(np.float32, m, 10, 40, seed=31)
    oix.parallel_insert(db, batch=128)
    q = np.concatenate([np.random.default_rng(503).integers(0, 5, (100, m)).astype(np.float32), db[7:11]])
    return db, oix, q


for _knbn, _ef in ((50, 65), (1, 1)):
    @case("index", "dense_search_knbn%d_ef%d" % (_knbn, _ef), env={"GS_DIST_MODE": "dense"})
    def _(wd, knbn=_knbn, ef=_ef):
        db, oix, q = _noise_index()
        return _search_case(db, oix, q, knbn, ef, 10, 40)


@functools.lru_cache(maxsize=None)
def _ties_index():
    """test_dense_traversal_placements_and_regimes, "ties": many small unrelated families, most pairs share no slot"""
    m = 200
    db = H.synth_sig_db(150, 8, m, 77, jlo=0.0, jhi=0.6)
    oix = O.Index(np.float32, m, 8, 64, seed=9)
    oix.parallel_insert(db, batch=64)
    q = np.concatenate([H.queries_from(db, 300, 5, frac=0.25), db[:40]])
    return db, oix, q


for _vis in ("lds", "global", "split"):
    @case("index", "dense_search_visited_%s" % _vis, env={"GS_DIST_MODE": "dense", "GS_DENSE_VIS": _vis, "GS_SPLIT_W": "1024"})
    def _(wd):
        db, oix, q = _ties_index()
        run, ref = _search_case(db, oix, q, 10, 400, 8, 64)
        assert (ref[1] == 1.0).mean() > 0.3
        return run, ref


@functools.lru_cache(maxsize=None)
def _u64_index():
    """test_dense_strategies_for_every_signature_kind: u64, m = 97, n = 1201"""
    m = 97
    db = H.synth_sig_db(30, 40, m, 55, dtype=np.uint64, jlo=0.02, jhi=0.9)[:1201]
    oix = O.Index(np.uint64, m, 12, 48, seed=4)
    oix.parallel_insert(db, batch=100)
    q = np.concatenate([H.queries_from(db, 150, 3, frac=0.2), db[5:9]])
    return db, oix, q


for _impl in ("join", "tile"):
    @case("index", "dense_search_%s" % _impl, env={"GS_DIST_MODE": "dense", "GS_DENSE_IMPL": _impl})
    def _(wd):
        db, oix, q = _u64_index()
        return _search_case(db, oix, q, 15, 300, 12, 48, np.uint64)


@case("index", "gather_search_on_an_imported_graph", env={"GS_DIST_MODE": "gather"})
def _(wd):
    m = 256
    db = H.synth_sig_db(30, 40, m, 4, jlo=0.05, jhi=0.95)
    oix = O.Index(np.float32, m, 8, 32, seed=123)
    oix.parallel_insert(db, batch=1)
    return _search_case(db, oix, H.queries_from(db, 64, 6, frac=0.3), 10, 48, 8, 32)


for _mode in ("dense", "gather"):
    @case("index", "extend_candidates_small_efc_%s" % _mode, env={"GS_DIST_MODE": _mode})
    def _(wd):
        """test_extend_candidates_with_small_ef_construction, its first shape: efc < 2M, every layer-0 selection extends (ext_keys)"""
        import gsearch_amd as G
        m, M, efc, B = 256, 8, 8, 16
        db = H.synth_sig_db(20, 25, m, 5, jlo=0.05, jhi=0.95)
        half = len(db) // 2 + 1
        oix = O.Index(np.float32, m, M, efc, scale_modify=1.0, seed=3)
        for part in (db[:half], db[half:]):
            oix.parallel_insert(part, batch=B)
        og = oix.export()
        q = H.queries_from(db, 24, 6, frac=0.3)
        ref = _graph_outputs(og, og) + oix.parallel_search(q, 10, 50)

        def run(ctx, poke):
            hn = G.Hnsw.new(M, 10000, 16, efc, G.DistHamming(ctx), seed=3, insert_batch=B, ctx=ctx)
            hn.modify_level_scale(1.0); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
            for part in (db[:half], db[half:]):
                poke(hn)
                hn.parallel_insert(part)
            poke(hn)
            out = _graph_outputs(hn.export_graph(), og)
            poke(hn)
            out += hn.search_arrays(q, 10, 50)
            hn.close()
            return out
        return run, ref


def _empty_graph(n, M=8):
    return dict(levels=np.zeros(n, np.uint8), entry=0, deg0=np.zeros(n, np.uint32), nbr0=np.zeros((n, 2 * M), np.uint32), cnt0=np.zeros((n, 2 * M), np.uint32),
                upidx=np.full(n, -1, np.int32), n_upper=0)


def _self_graph(db, knbn):
    ids, dist = O.bruteforce_topk(db, db, knbn + 1, min(8, os.cpu_count() or 1))
    n = len(db)
    oi, od = np.full((n, knbn), U64MAX), np.full((n, knbn), np.inf, np.float32)
    for i in range(n):
        keep = ids[i] != np.uint64(i)
        if keep.all():
            keep[-1] = False
        oi[i], od[i] = ids[i][keep], dist[i][keep]
    return oi, od, np.full(n, min(knbn, n - 1), np.uint32)


@case("index", "exact_search_knn_graph_bruteforce_nearest_of")
def _(wd):
    """test_gpu_exact_knn.py (_tie_db, m = 1000: duplicates, n = 303 no multiple of 8), test_bruteforce_matches_oracle, test_gpu_cluster.py nearest_of"""
    import gsearch_amd as G
    import pyref_cluster as RC
    db = H.synth_sig_db(13, 23, 1000, 11 + 1000, jlo=0.9, jhi=0.9999)
    db = np.ascontiguousarray(np.concatenate([db, db[[0, 5, 5, 100]]]))
    n = len(db)
    q = np.ascontiguousarray(np.concatenate([H.queries_from(db, 40, 3, frac=0.05), db[[0, 7, 302]]]))
    cand = np.random.default_rng(n).choice(n, 130, replace=False).astype(np.uint64)
    cand[:6] = [200, 3, 150, 201, 7, 200]
    ei, ed = O.bruteforce_topk(db, q, 50, 8)
    near = RC.nearest_of(db, cand)
    ref = (ei, ed, np.full(len(q), 50, np.uint32)) + _self_graph(db, 32) + (ei[:, :12].copy(), ed[:, :12].copy()) + (np.asarray(near[0], np.uint32), np.asarray(near[1], np.uint16))

    def run(ctx, poke):
        hn = G.Hnsw.new(8, 1024, 16, 40, G.DistHamming(ctx), ctx=ctx)
        hn.import_graph(db, _empty_graph(n))
        poke(hn)
        out = tuple(hn.exact_search_arrays(q, 50))
        poke(hn)
        out += tuple(hn.knn_graph(32))
        poke(hn)
        out += tuple(hn.bruteforce_search(q, 12))
        poke(hn)
        out += tuple(hn.nearest_of(cand))
        hn.close()
        return out
    return run, ref


@case("index", "cluster_planted_families")
def _(wd):
    import gsearch_amd as G
    import pyref_cluster as RC
    db = RC.planted(0)[0]
    r = RC.cluster(db, 8, 0.1, 15, 0)
    ref = (r["core_nodes"], r["core_weight"], r["centre_node"], r["centre_count"], r["medoids"], r["sizes"],
           np.array([r["n_core"], r["iterations"], r["converged"], r["cost_core"], r["cost_all"]], np.uint64))

    def run(ctx, poke):
        hn = G.Hnsw.new(8, max(len(db), 1024), 16, 40, G.DistHamming(ctx), dtype=db.dtype, ctx=ctx)
        hn.import_graph(db, _empty_graph(len(db)))
        poke(hn)
        g = hn.cluster(8, 0.1, 15, 0, return_coreset=True)
        hn.close()
        return (g.core_nodes, g.core_weight, g.centre_node, g.centre_count, g.medoids, g.sizes,
                np.array([g.n_core, g.iterations, g.converged, g.cost_core, g.cost_all], np.uint64))
    return run, tuple(np.asarray(a) for a in ref)


@case("index", "embed_knn_graph_and_stats")
def _(wd):
    """test_gpu_embed.py: test_positions_random_graph (dim 2, seeded), test_stats_equal_numpy"""
    import gsearch_amd as G
    import pyref_embed as RE
    n, knbn = 2000, 8
    rng = np.random.default_rng(3 + 2)
    ids = np.full((n, knbn), U64MAX)
    dist = np.full((n, knbn), np.inf, np.float32)
    cnt = rng.integers(0, knbn + 1, n).astype(np.uint32)
    for i in range(n):
        c = int(cnt[i])
        nb = rng.choice(n - 1, c, replace=False)
        ids[i, :c] = nb + (nb >= i)
        dist[i, :c] = np.sort(np.asarray(rng.integers(0, 1 << 12, c) * np.float32(2.0 ** -12), np.float32))
    kw = dict(dim=2, epochs=40, seed=99)
    st = RE.stats(ids, dist, cnt)

    def stat_arrays(s):
        return (np.array([s["n"], s["knbn"], s["n_edges"], s["n_empty"], s["max_occ"]], np.uint64), np.array(s["hubs"], np.uint64),
                np.array([s["occ_mean"], s["occ_std"], s["occ_skew"]], np.float64), np.asarray(s["occ"], np.uint32), np.asarray(s["hist"], np.uint64),
                np.asarray(s["q_first"], np.float32), np.asarray(s["q_last"], np.float32))
    ref = (np.asarray(RE.embed(ids, dist, cnt, RE.defaults(**kw)), np.float32),) + stat_arrays(st)

    def run(ctx, poke):
        return (G.embed_knn_graph(ids, dist, cnt, G.EmbedParams(**kw), ctx=ctx),) + stat_arrays(G.knn_graph_stats(ids, dist, cnt, ctx=ctx))
    return run, ref


# ------------------------------------------------------------------------------------------------------------------------------------------------
# bigsig (test_gpu_bigsi.py test_colour_words_and_lane_mapping at 130 colours; added in two calls: the second starts at colour 65, inside a word)
@case("bigsig", "build_in_two_calls_rows_bits_query_classify")
def _(wd):
    import gsearch_amd as G
    import pyref_bigsi as RB
    rng = np.random.default_rng(130)
    k, h, B, n = 21, 3, 4099, 130

    def seq(length):
        return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)])
    genomes = [[seq(300)] for _ in range(n)]
    reads = []
    for _ in range(48):
        g = genomes[int(rng.integers(n))][0]
        s = int(rng.integers(0, len(g) - 100 + 1))
        reads.append([g[s:s + 100]])
    reads += [[seq(100)] for _ in range(16)]
    rb = RB.Index(k, h, B)
    for g in genomes:
        rb.add(g)
    rnk, rbc, rbh, rcnt = rb.query(reads)
    rtl, racc = rb.classify(rnk, rbc, rbh, 1e-3)
    ref = (rb.row_words(np.arange(B), 3), np.asarray(rb.t(), np.uint64), np.asarray(rb.nk, np.uint64), np.asarray(rnk, np.uint32), np.asarray(rbc, np.uint32),
           np.asarray(rbh, np.uint32), np.asarray(rcnt, np.uint32), np.asarray(rtl, np.float64), np.asarray(racc, bool))

    def run(ctx, poke):
        bx = G.Bigsi(k, h, B, n, ctx=ctx)
        bx.add_genomes(genomes[:65])
        bx.add_genomes(genomes[65:])
        assert bx.info()["row_words"] == 3
        t, nk = bx.bits_set(return_kmers=True)
        qn, qc, qh, cnt = bx.query(reads, dense=True)
        tl, acc = bx.classify(qn, qc, qh, 1e-3)
        out = (bx.rows(np.arange(B)), t, nk, qn, qc, qh, cnt, tl, acc)
        bx.close()
        return out
    return run, ref


# ------------------------------------------------------------------------------------------------------------------------------------------------
# comm (test_topk_merge_of_db_shards_on_the_device)
@case("comm", "topk_merge_dev_with_id_offsets")
def _(wd):
    import gsearch_amd as G
    from gsearch_amd import sharding as Sh
    S, nq, kin, kout = 3, 41, 7, 10
    rng = np.random.default_rng(S * 1000 + nq)
    per = 100000
    ids = np.stack([np.sort(rng.choice(per, (nq, kin)), axis=1) for _ in range(S)]).astype(np.uint64)
    dist = np.sort((rng.integers(0, 40, (S, nq, kin)) / np.float32(64)).astype(np.float32), axis=2)
    short = rng.random((S, nq)) < 0.2
    for s_ in range(S):
        for q_ in np.nonzero(short[s_])[0]:
            cut = int(rng.integers(0, kin))
            ids[s_, q_, cut:] = U64MAX; dist[s_, q_, cut:] = np.inf
    off = np.arange(S, dtype=np.uint64) * np.uint64(per)
    glob = np.where(ids == U64MAX, ids, ids + off[:, None, None])
    want_i, want_d = Sh.merge_topk_shards([glob[s_] for s_ in range(S)], [dist[s_] for s_ in range(S)], kout)

    def run(ctx, poke):
        ptrs = [ctx.alloc(ids.nbytes), ctx.alloc(dist.nbytes), ctx.alloc(nq * kout * 8), ctx.alloc(nq * kout * 4)]
        try:
            ctx.upload(ptrs[0], ids); ctx.upload(ptrs[1], dist)
            G.topk_merge_dev(ctx, ptrs[0], ptrs[1], S, nq, kin, kout, ptrs[2], ptrs[3], id_offset=off)
            return ctx.download(ptrs[2], (nq, kout), np.uint64), ctx.download(ptrs[3], (nq, kout), np.float32)
        finally:
            for p_ in ptrs:
                ctx.free(p_)
    return run, (np.asarray(want_i, np.uint64), np.asarray(want_d, np.float32))


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the primitives of gs_radix.hip on their own (test_gpu_radix.py runs their whole tables under 0x00 and 0xFF; here a large shape in front of a small one,
# and the replay in other families' leftovers)
def _radix_case(names, cases, call, ref):
    picked = [next(c for c in cases if c["name"] == n) for n in names]
    want = tuple(np.asarray(x) for c in picked for x in ref(c))

    def run(ctx, poke):
        return tuple(np.asarray(x) for c in picked for x in call(ctx, c))
    return run, want


@case("radix", "sort_three_tiles_then_65_keys")
def _(wd):
    import gsearch_amd as G
    import pyref_radix as RR
    import radix_cases as RC
    return _radix_case(("size_%d_e24" % (3 * RC.TILE + 17), "size_65_e64"), RC.sort_cases(), lambda ctx, c: (G.debug_radix_sort(c["keys"], c["endbit"], ctx=ctx),),
                       lambda c: (RR.sort(c["keys"], c["endbit"]),))


@case("radix", "run_lengths_five_tiles_then_65_keys")
def _(wd):
    import gsearch_amd as G
    import pyref_radix as RR
    import radix_cases as RC
    return _radix_case(("size_%d" % (4 * RC.TILE + 1), "size_65"), RC.rle_cases(), lambda ctx, c: G.debug_run_lengths(c["a"], ctx=ctx), lambda c: RR.run_lengths(c["a"]))


@case("radix", "scan_4608_then_5_counts")
def _(wd):
    import gsearch_amd as G
    import pyref_radix as RR
    import radix_cases as RC

    def call(ctx, c):
        out, total = G.debug_scan(c["v"], ctx=ctx)
        return out, np.uint32(total)
    return _radix_case(("size_4608", "size_5"), RC.scan_cases(), call, lambda c: (RR.scan(c["v"])[0], np.uint32(RR.scan(c["v"])[1])))


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the two drivers of the compare kernels of gs_hamming.hip on their own (test_gpu_hamming.py runs their whole tables under 0x00 and 0xFF): the K-split
# forms add to / take off cells that the driver itself has to set first, whatever the slot held
@case("hamming", "strided_split_u32_counts")
def _(wd):
    import gsearch_amd as G
    import hamming_cases as HC
    c = next(c for c in HC.dense_cases() if c["name"].startswith("split_float32_129x130_m515"))
    want = HC.counts(c["q"], c["c"], c["m"]).astype(np.uint32)

    def run(ctx, poke):
        out = np.full((c["nq"], c["nc"] + 3), 0xC5C5C5C5, np.uint32)
        parts = G.debug_hamming_strided(c["qw"], c["cw"], c["m"], out, 1, dtype=c["dtype"], ctx=ctx)
        return out[:, :c["nc"]], out[:, c["nc"]:], np.uint32(parts > 1)
    return run, (want, np.full((c["nq"], 3), 0xC5C5C5C5, np.uint32), np.uint32(1))


def _blocks_case(name, n_thin_of, split):
    import gsearch_amd as G
    import hamming_cases as HC
    c = next(c for c in HC.blocks_cases() if c["name"] == name)
    ld = HC.LDS[1]
    want = HC.blocks_expected(c, ld)[0]

    def run(ctx, poke):
        out = np.full((c["nq_rows"], ld), HC.CANARY16, np.uint16)
        parts = G.debug_hamming_blocks(c["qw"], c["cw"], c["m"], c["items"], c["qlist"], c["clist"], n_thin_of(c), out, dtype=c["dtype"], ctx=ctx)
        return out, np.uint32(parts > 1)
    return run, (want, np.uint32(split))


@case("hamming", "work_list_split_three_items")
def _(wd):
    return _blocks_case("three_uint32_m515_r256_3", lambda c: 0, True)


@case("hamming", "work_list_thin_items")
def _(wd):
    return _blocks_case("thin_float32_m1003_r256_30", lambda c: c["eligible"], True)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# hmmsearch (gs_hmm.hip): its host forms stage their arguments in one set of slots and its forms over pairs share their lists, so every form runs in
# what the one before it left - first on nine records, then on two of them, so that each slot is also used smaller after larger. Three synthetic profiles
# in two kernel classes (10 and 64 nodes: one node a lane, 70: two); records on both sides of the 64-residue reload, an empty one, and copies of the
# consensus, so that there are domains and envelopes; every (record, profile) pair in a shuffled order, and one GS_HMM_NO_HIT entry.
HMM_SLOTS = 4                       # domain and envelope slots a pair


@functools.lru_cache(maxsize=None)
def _hmm_sets():
    """-> texts, floors and per record set (records, packed, pair_rec, pair_prof, what the restatements say): the Viterbi matrix, the MSV, Viterbi and
    Forward matrices behind the floors of P = 0.02 and 1e-3, Forward behind the Viterbi floor alone, trace-back, envelopes and their rows"""
    import pyref_hmm as R
    import pyref_hmm_forward as F
    import pyref_hmm_msv as V
    import pyref_hmm_posterior as P
    import pyref_hmm_trace as T
    rng = np.random.default_rng(1361)
    texts = [R.write_hmm(R.synth_model(rng, M)) for M in (10, 64, 70)]
    models = [m for t in texts for m in R.parse_hmm(t)]
    mfl, vfl = V.floors([s for t in texts for s in F.stats_lines(t)]), F.floors(models)
    c10, c64, c70 = (R.consensus(m["tables"]) for m in models)
    nine = [b"", R.background(rng, 1), R.background(rng, 63), R.background(rng, 64), R.background(rng, 65), c70 + R.background(rng, 60), c64 + c64,
            c10 + R.background(rng, 20) + c10, c70]
    assert [len(r) for r in nine] == [0, 1, 63, 64, 65, 130, 128, 40, 70]
    sets = []
    for records in (nine, [nine[5], nine[2]]):
        order = rng.permutation(len(records) * len(models))
        pr = np.append((order // len(models)).astype(np.uint32), np.uint32(R.NO_HIT))
        pp = np.append((order % len(models)).astype(np.uint32), np.uint32(1))
        rl = np.array([len(r) for r in records], np.uint64)
        packed = (np.frombuffer(b"".join(records) + bytes(8), np.uint8), np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64), rl)
        msv, fvit, fwd = V.search_filtered(models, records, floor=mfl, forward=True, vit_floor=vfl)
        *env, outs, conts = P.envelope_pairs(models, records, pr, pp, HMM_SLOTS, rows=True)
        rows = lambda xs: np.concatenate([np.zeros(0, np.int32)] + [x for x in xs if x is not None])     # noqa: E731
        want = {"vit": R.search(models, records), "msv": msv, "fvit": fvit, "fwd": fwd, "fwd_all": F.search_forward(models, records, floor=vfl)[1],
                "trace": T.trace_pairs(models, records, pr, pp, HMM_SLOTS), "env": tuple(env) + (rows(outs), rows(conts))}
        assert (want["fvit"] == R.NO_SCORE).any() and (want["fwd"] != R.NO_SCORE).any() and want["trace"][1].max() >= 1 and want["env"][2].max() >= 1
        sets.append((records, packed, pr, pp, want))
    assert sets[0][4]["trace"][1].max() == 2 and sets[0][4]["env"][2].max() == HMM_SLOTS        # a pair with two domains, one that fills its envelope slots
    return texts, mfl, vfl, sets


@case("hmm", "host_forms_nine_records_then_two")
def _(wd):
    import gsearch_amd as G
    texts, mfl, vfl, sets = _hmm_sets()

    def run(ctx, poke):
        db, got = G.HmmDb(texts, ctx, texts=True), ()
        try:
            for _, packed, pr, pp, _ in sets:
                *env, outs, conts = db.envelopes_packed(*packed, pr, pp, max_env=HMM_SLOTS, rows=True)
                got += ((db.search_packed(*packed),) + db.search_filtered_packed(*packed, msv_floor=mfl, forward=True, floor=vfl) +
                        db.trace_packed(*packed, pr, pp, max_dom=HMM_SLOTS) + tuple(env) + (np.concatenate(outs), np.concatenate(conts)))
        finally:
            db.close()
        return got
    return run, tuple(x for *_, w in sets for x in (w["vit"], w["msv"], w["fvit"], w["fwd"]) + w["trace"] + w["env"])


@case("hmm", "dev_forms_without_the_unwanted_matrices")
def _(wd):
    """the _dev forms on the same sets; the Viterbi matrix of gs_hmm_search_forward_dev and the MSV matrix of gs_hmm_search_filtered_dev are not asked
    for, so both go to their slots"""
    import gsearch_amd as G
    texts, mfl, vfl, sets = _hmm_sets()

    def run(ctx, poke):
        db, got, bufs = G.HmmDb(texts, ctx, texts=True), (), []

        def up(a):
            bufs.append(ctx.alloc(max(a.nbytes, 16)))
            ctx.upload(bufs[-1], np.ascontiguousarray(a))
            return bufs[-1]
        try:
            for records, packed, pr, pp, _ in sets:
                n_rec, n, n_prof = len(records), len(pr), len(db)
                ro = np.concatenate([[0], np.cumsum([packed[2][r] if r < n_rec else 0 for r in pr])]).astype(np.uint64)
                aa, rs, rl, d_pr, d_pp, d_ro, d_mfl, d_vfl = (up(a) for a in packed + (pr, pp, ro, mfl, vfl))
                mat, per_pair = np.zeros((n_rec, n_prof), np.int32), np.zeros(n, np.int32)
                vit, fvit, fwd, fwd_all, raw, nd, dom, efwd, ebck, ne, env, outs, conts = (up(a) for a in (
                    mat, mat, mat, mat, per_pair, per_pair, np.zeros((n, HMM_SLOTS, 8), np.int32), per_pair, per_pair, per_pair, np.zeros((n, HMM_SLOTS, 4), np.int32),
                    np.zeros(int(ro[-1]), np.int32), np.zeros(int(ro[-1]), np.int32)))
                db.search_dev(aa, rs, rl, n_rec, vit)
                db.search_filtered_dev(aa, rs, rl, n_rec, d_mfl, d_vfl, None, fvit, fwd)
                db.search_forward_dev(aa, rs, rl, n_rec, d_vfl, None, fwd_all)
                db.trace_dev(aa, rs, rl, n_rec, d_pr, d_pp, n, HMM_SLOTS, raw, nd, dom)
                db.envelopes_dev(aa, rs, rl, n_rec, d_pr, d_pp, n, HMM_SLOTS, efwd, ebck, ne, env, d_ro, outs, conts)
                got += tuple(ctx.download(p, mat.shape, np.int32) for p in (vit, fvit, fwd, fwd_all))
                got += (ctx.download(raw, (n,), np.int32), ctx.download(nd, (n,), np.uint32), ctx.download(dom, (n, HMM_SLOTS, 8), np.int32),
                        ctx.download(efwd, (n,), np.int32), ctx.download(ebck, (n,), np.int32), ctx.download(ne, (n,), np.uint32),
                        ctx.download(env, (n, HMM_SLOTS, 4), np.int32), ctx.download(outs, (int(ro[-1]),), np.int32), ctx.download(conts, (int(ro[-1]),), np.int32))
        finally:
            for p in bufs:
                ctx.free(p)
            db.close()
        return got
    return run, tuple(x for *_, w in sets for x in (w["vit"], w["fvit"], w["fwd"], w["fwd_all"]) + w["trace"] + w["env"])


# ------------------------------------------------------------------------------------------------------------------------------------------------
# one test function per case, in the order of the list, then the replay
def _make_test(c):
    def test(stale_ctx, fill_guard, workdir, monkeypatch, capfd):
        _run_case(c, stale_ctx, workdir, monkeypatch, capfd, FILLS)
    test.__name__ = test.__qualname__ = "test_%s_%s" % (c.family, c.name)
    test.__doc__ = "%s / %s: equal to its reference with the fill off and under 0x00, 0x01 and 0xFF" % (c.family, c.name)
    return test


assert len({(c.family, c.name) for c in CASES}) == len(CASES)
for _c in CASES:
    globals()["test_%s_%s" % (_c.family, _c.name)] = _make_test(_c)
del _c


def test_zz_replay_of_every_case_in_reverse_order(stale_ctx, fill_guard, workdir, monkeypatch, capfd):
    """what only shows when one family runs in another family's leftovers: the whole list once more, backwards, under 0x01 on the same context"""
    for c in reversed(CASES):
        with monkeypatch.context() as mp:
            _run_case(c, stale_ctx, workdir, mp, capfd, (0x01,))


def test_debug_fill_arguments(stale_ctx, fill_guard):
    import gsearch_amd as G
    from gsearch_amd._lib import GS_ERR_INVALID
    L = stale_ctx.L
    assert L.gs_debug_mem_fill(256) == GS_ERR_INVALID and L.gs_debug_mem_fill(-2) == GS_ERR_INVALID
    assert L.gs_debug_mem_fill(0xAB) == 0
    p = stale_ctx.alloc(64)                                            # gs_dev_alloc fills too: the output buffers of the _dev forms
    try:
        assert (stale_ctx.download(p, 64, np.uint8) == 0xAB).all()
    finally:
        stale_ctx.free(p)
    G.debug_mem_fill(None)
    hn = G.Hnsw.new(8, 1000, 16, 32, G.DistHamming(stale_ctx), ctx=stale_ctx)
    hn.debug_fill_scratch(1)                                           # no index yet: nothing to fill
    hn._ensure(32)
    assert L.gs_index_debug_fill_scratch(hn.h, 256) == GS_ERR_INVALID and L.gs_index_debug_fill_scratch(hn.h, -1) == GS_ERR_INVALID
    hn.debug_fill_scratch(0xFF)
    hn.close()
