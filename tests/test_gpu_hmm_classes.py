"""Every kernel class of gs_hmm.hip on the device, the lane scan of the D states under load, bytes that are no residue, and the two length limits, against
the numpy restatements (tests/pyref_hmm.py, tests/pyref_hmm_forward.py). Every comparison is `==` on int32 and every device output sits between
canaries. The expected matrices are computed once per module; those of the length limits come from tests/golden/hmm_limits.json.

k_hmm_viterbi<Q> and k_hmm_forward<Q> exist for Q = 1, 2, 3, 4, 6, 8, 12, 16 and 20 nodes per lane; a profile runs in the smallest Q with 64 Q >= M:

    M      64  65 128 129 192 193 256 257 384 385 512 513 768 769 1024 1025 1280   300 900
    Q       1   2   2   3   3   4   4   6   6   8   8  12  12  16   16   20   20     6  16

The set below holds a profile on both sides of every edge and GS_HMM_MAX_M itself (all 64 lanes full of 20 nodes), so all 18 instances run, among them
those where the code changes shape: Forward reads its transition rows from LDS in every row from Q = 12 on and Viterbi above 16; from Q = 12 on both
kernels, and at Q = 8 Forward alone, need the attribute for more than 64 KB of dynamic LDS. The profiles are deletion-friendly (hmm_classes_case.py)
and the records leave out between a few and most of the nodes: tests/test_hmm_classes_cpu.py shows on the restatement that each of the six scan
steps, cut out, changes one of these expected scores in every profile (but step 5 at M = 65, which reaches no node), for Viterbi and for Forward."""
import json
import os
import time

import numpy as np
import pytest

import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_forward as F
from test_gpu_hmm import CANARY, GUARD, _Dev, search_dev  # noqa: F401
from test_gpu_hmm_forward import forward_dev, mismatches

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GS_OK = 0
BAD_BYTES = (ord("X"), ord("B"), ord("*"), 0x00, 0xFF, ord("-"))


def build_set():
    """the 19 profiles in an order that is not by M, the six records of every deletion-friendly profile and background on both sides of the
    64-residue block, and both expected matrices"""
    rng = np.random.default_rng(1301)
    texts = [K.model_text(M) for M in K.SET_ORDER]
    models = [m for t in texts for m in R.parse_hmm(t)]
    records, first = [], {}
    for p, m in enumerate(models):
        if m["M"] in K.CLASS_M:
            first[p] = len(records)
            records += K.deletion_records(R.consensus(m["tables"]), m["M"])
    records += [R.background(rng, L) for L in (1, 63, 64, 65, 129)]
    # viterbi_batch walks every record to the longest one's end: the few long records apart, which leaves each record's score what it is
    short = np.array([len(r) <= 50 for r in records])
    vit = np.zeros((len(records), len(models)), np.int32)
    for sel in (np.flatnonzero(short), np.flatnonzero(~short)):
        vit[sel] = R.search(models, [records[r] for r in sel])
    vit, fwd = F.search_forward(models, records, vit=vit)
    return {"texts": texts, "models": models, "records": records, "first": first, "vit": vit, "fwd": fwd}


@pytest.fixture(scope="module")
def cset():
    return build_set()


def check_set(ctx, db, cset):
    """the four ways to a score matrix against the restatement"""
    vit, fwd = cset["vit"], cset["fwd"]
    got = db.search(cset["records"])
    assert got.dtype == np.int32 and got.shape == vit.shape and not mismatches(got, vit)
    assert not mismatches(search_dev(ctx, db, cset["records"]), vit)
    hvit, hfwd = db.search_forward(cset["records"], filter_p=None)
    assert not mismatches(hfwd, fwd) and not mismatches(hvit, vit)
    dvit, dfwd = forward_dev(ctx, db, cset["records"])
    assert not mismatches(dfwd, fwd) and not mismatches(dvit, vit)


def test_all_classes_in_one_set(cset, gpu_ctx):
    import gsearch_amd as G
    models, vit, fwd = cset["models"], cset["vit"], cset["fwd"]
    assert vit.shape == fwd.shape == (107, 19) and len(cset["first"]) == 17 and max(len(r) for r in cset["records"]) == 129
    assert (vit != R.NO_SCORE).all() and (fwd >= vit).all()
    for p, r in cset["first"].items():                                           # the planted pieces are hits, so the comparison is not one of noise
        assert vit[r, p] > models[p]["ga_units"] == 25600, (models[p]["M"], int(vit[r, p]))
    db = G.HmmDb(cset["texts"], gpu_ctx, texts=True)
    try:
        assert [int(x) for x in db.M] == list(K.SET_ORDER) and [int(x) for x in db.M] != sorted(int(x) for x in db.M)
        assert {F.group_size(int(M)) for M in db.M} == set(F.CLASS_G) == {1, 2, 3, 4, 6, 8, 12, 16, 20}
        for p in (0, 2, 8):                                                      # Q = 12, Q = 20 with every lane full, and an ordinary profile
            assert np.array_equal(db.tables(p), models[p]["tables"]), p
        check_set(gpu_ctx, db, cset)
    finally:
        db.close()


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_all_classes_on_poisoned_scratch(cset, gpu_ctx, byte):
    """the same set twice on scratch and allocations filled with a chosen byte: the classes run one after another on the same LDS, the large tables
    after the small ones, and nothing reads what nothing wrote"""
    import gsearch_amd as G
    G.debug_mem_fill(byte)
    try:
        gpu_ctx.release_scratch()
        db = G.HmmDb(cset["texts"], gpu_ctx, texts=True)
        try:
            for _ in range(2):
                check_set(gpu_ctx, db, cset)
        finally:
            db.close()
    finally:
        G.debug_mem_fill(None)


def build_bad_case():
    """packed records as the device forms take them, unfiltered: 600 of 1 .. 40 residues, one in ten with a byte that is no residue, four of 200
    residues with that byte in the first block, on both sides of the block edge and at the end, and ten good records again in lower case"""
    rng = np.random.default_rng(1303)
    Ms = (65, 193, 385)                                                          # Q = 2, 4, 8
    texts = [K.model_text(M) for M in Ms]
    models = [m for t in texts for m in R.parse_hmm(t)]
    cons = R.consensus(models[1]["tables"])
    records = [bytearray(R.background(rng, int(L))) for L in rng.integers(1, 41, size=600)]
    for j in range(0, 600, 37):                                                  # some carry a piece of a consensus
        records[j] = bytearray(cons[j % 50:][:len(records[j])])
    bad = np.zeros(614, bool)
    for j in np.flatnonzero(rng.random(600) < 0.1):
        records[j][int(rng.integers(len(records[j])))] = BAD_BYTES[int(rng.integers(len(BAD_BYTES)))]
        bad[j] = True
    for k, at in enumerate((0, 63, 64, 199)):
        rec = bytearray(cons[:100] + R.background(rng, 100))
        rec[at] = BAD_BYTES[k]
        records.append(rec)
        bad[600 + k] = True
    lower_of = [int(j) for j in np.flatnonzero(~bad[:600] & (np.array([len(r) for r in records[:600]]) >= 10))[:10]]
    records += [bytearray(bytes(records[j]).lower()) for j in lower_of]
    assert len(records) == 614 and 40 < bad.sum() < 90 and all(bytes(records[600 + k]) != bytes(records[j]) for k, j in zip(range(4, 14), lower_of))
    good = np.flatnonzero(~bad[:600])
    vit = np.full((614, 3), R.NO_SCORE, np.int32)
    fwd = vit.copy()
    vit[good], fwd[good] = F.search_forward(models, [bytes(records[j]) for j in good])
    vit[604:], fwd[604:] = vit[lower_of], fwd[lower_of]
    rl = np.array([len(r) for r in records], np.uint64)
    rs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64)
    aa = np.frombuffer(b"".join(bytes(r) for r in records) + bytes(8), np.uint8)
    return {"texts": texts, "packed": (aa, rs, rl), "bad": bad, "vit": vit, "fwd": fwd}


def test_bytes_that_are_no_residue_and_lower_case(gpu_ctx):
    """SPEC 13: a byte that is no residue gives GS_HMM_NO_SCORE, and either case is read. The Python layer filters such bytes away first, so only the
    packed forms reach these sentences. 614 records are more than the 512 wavefronts of a profile's row of workgroups: a wavefront takes a second record
    after a refused one"""
    import gsearch_amd as G
    c = build_bad_case()
    vit, fwd, bad = c["vit"], c["fwd"], c["bad"]
    assert (vit[bad] == R.NO_SCORE).all() and (fwd[bad] == R.NO_SCORE).all() and (vit[~bad] != R.NO_SCORE).all() and (fwd[~bad] >= vit[~bad]).all()
    db = G.HmmDb(c["texts"], gpu_ctx, texts=True)
    try:
        assert not mismatches(search_dev(gpu_ctx, db, packed=c["packed"]), vit)
        dvit, dfwd = forward_dev(gpu_ctx, db, packed=c["packed"])
        assert not mismatches(dvit, vit) and not mismatches(dfwd, fwd)
        assert not mismatches(db.search_packed(*c["packed"]), vit)                                       # gs_hmm_search on the same arrays
        hvit, hfwd = db.search_forward_packed(*c["packed"], filter_p=None)                               # gs_hmm_search_forward
        assert not mismatches(hvit, vit) and not mismatches(hfwd, fwd)
        # with a floor below every score Forward still runs for no refused record
        floor = np.full(3, F.FLOOR_ALL, np.int32)
        assert not mismatches(forward_dev(gpu_ctx, db, packed=c["packed"], floor=floor, want_vit=False)[1], fwd)
    finally:
        db.close()


@pytest.fixture(scope="module")
def limits():
    with open(os.path.join(HERE, "golden", "hmm_limits.json")) as f:
        cases = json.load(f)["cases"]
    assert [(c["score"], c["kind"], c["M"], c["L"]) for c in cases] == list(K.LIMIT_CASES)
    return cases


def limit_set(limits, score, profiles):
    """the texts of `profiles` (kind, M), checked against the file's sha256, the lengths of the score's cases, and raw[length, profile] where the file
    has it"""
    texts = [K.limit_text(kind, M) for kind, M in profiles]
    mine = [c for c in limits if c["score"] == score]
    lens = sorted({c["L"] for c in mine}, reverse=True)
    want = {}
    for c in mine:
        p = profiles.index((c["kind"], c["M"]))
        assert K.sha256(texts[p]) == c["sha256"], "the profile text is not the one the golden file was computed from"
        want[lens.index(c["L"]), p] = c["raw"]
    return texts, lens, want


def test_the_length_limits(limits, gpu_ctx):
    """b"W" * L at GS_HMM_MAX_L = 2^18 for Viterbi and GS_HMM_FWD_MAX_L = 65536 for Forward, and one residue less, against the profiles whose cells grow
    fastest: raw scores of 1.6e9 (Viterbi, above 2^30) and 5.5e8 to 8.5e8 (Forward), where the int32 headroom of SPEC 13 and the unsigned difference
    inside lse (hi - lo up to 1.4e9) are what is computed with. A single wavefront walks each record; the device calls of this test are timed and
    printed."""
    import gsearch_amd as G
    t_dev = 0.0
    # Viterbi
    texts, lens, want = limit_set(limits, "viterbi", [("zero", 64), ("w_only", 64)])
    assert lens == [1 << 18, (1 << 18) - 1, 1 << 16] == [R.MAX_L, R.MAX_L - 1, 1 << 16] and len(want) == 4
    assert max(want.values()) > (1 << 30)
    records = [b"W" * L for L in lens]
    db = G.HmmDb(texts, gpu_ctx, texts=True)
    try:
        t0 = time.perf_counter()
        host = db.search(records)                                                # a return code other than GS_OK raises
        dev = search_dev(gpu_ctx, db, records)
        t_dev += time.perf_counter() - t0
        assert np.array_equal(host, dev) and (host != R.NO_SCORE).all()
        assert {k: int(host[k]) for k in want} == want
        assert host[0, 0] - host[1, 0] == want[0, 0] - want[1, 0] > 6000         # the last residue counts: nothing is clamped
        aa, rs, rl = G.filter_aa_records(records[:1])
        out = np.zeros((1, 2), np.int32)
        assert gpu_ctx.L.gs_hmm_search(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, out.ctypes.data) == GS_OK
        assert np.array_equal(out, host[:1])
    finally:
        db.close()
    # Forward
    texts, lens, want = limit_set(limits, "forward", [("zero", 64), ("zero", 1280)])
    assert lens == [F.FWD_MAX_L, F.FWD_MAX_L - 1] and len(want) == 3
    assert max(c["max_hi_lo"] for c in limits if c["score"] == "forward") > (1 << 30)
    records = [b"W" * L for L in lens]
    db = G.HmmDb(texts, gpu_ctx, texts=True)
    try:
        t0 = time.perf_counter()
        hvit, host = db.search_forward(records, filter_p=None)
        dvit, dev = forward_dev(gpu_ctx, db, records)
        t_dev += time.perf_counter() - t0
        assert np.array_equal(host, dev) and np.array_equal(hvit, dvit) and (host > hvit).all() and (hvit != R.NO_SCORE).all()
        assert {k: int(host[k]) for k in want} == want
        assert host[0, 0] - host[1, 0] == want[0, 0] - want[1, 0] > 6000
        aa, rs, rl = G.filter_aa_records(records[:1])
        vit1, fwd1 = np.zeros((1, 2), np.int32), np.zeros((1, 2), np.int32)
        rc = gpu_ctx.L.gs_hmm_search_forward(gpu_ctx.h, db.h, aa.ctypes.data, rs.ctypes.data, rl.ctypes.data, 1, None, vit1.ctypes.data, fwd1.ctypes.data)
        assert rc == GS_OK and np.array_equal(fwd1, host[:1]) and np.array_equal(vit1, hvit[:1])
    finally:
        db.close()
    print("length limits: %.3f s in the device calls" % t_dev)
