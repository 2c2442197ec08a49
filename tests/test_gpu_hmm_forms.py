"""The two entries of every hmmsearch pair of the ABI - over host pointers and over device pointers (_dev) - run one body (gs_hmm.hip, hmm_*_form), and
what that body refuses it refuses for both with one code: a missing output, a profile set of another context, a record over the length limit, and
for the forms over pairs a pair that names a missing record or profile and a row_off that leaves a pair too few words. The accepted call comes first,
so that a refusal is the refusal of the one argument that changed. (That both forms equal the restatement is what the test_gpu_hmm*.py of each
operation and the hmm family of test_gpu_stale_scratch.py hold them to.)"""
import numpy as np
import pytest

import pyref_hmm as R

pytestmark = pytest.mark.gpu

GS_OK, GS_ERR_INVALID, GS_ERR_UNSUPPORTED = 0, -1, -3
N_REC, N_PAIRS, SLOTS = 3, 2, 2
# the arguments of each pair behind (ctx, db), in the order of the ABI: names of arrays, or plain numbers
OPS = {
    "search": ("aa rs rl n_rec mat0", "mat0"),
    "search_msv": ("aa rs rl n_rec mat0", "mat0"),
    "search_forward": ("aa rs rl n_rec floor mat0 mat1", "mat1"),
    "search_filtered": ("aa rs rl n_rec floor floor mat0 mat1 mat2", "mat1"),
    "trace": ("aa rs rl n_rec pr pp n_pairs slots zero pair0 pair1 items8", "pair0"),
    "envelopes": ("aa rs rl n_rec pr pp n_pairs slots zero pair0 pair1 pair2 items4 ro rows0 rows1", "pair2"),
}


@pytest.fixture(scope="module")
def db(gpu_ctx):
    import gsearch_amd as G
    d = G.HmmDb([R.write_hmm(R.synth_model(np.random.default_rng(1362), 10))], gpu_ctx, texts=True)
    yield d
    d.close()


def good():
    """three records of 10 residues, the pairs (0, 0) and (2, 0)"""
    mat, pair = np.zeros((N_REC, 1), np.int32), np.zeros(N_PAIRS, np.int32)
    return {"aa": np.frombuffer(b"ACDEFGHIKL" * 3 + bytes(8), np.uint8), "rs": np.array([0, 10, 20], np.uint64), "rl": np.array([10, 10, 10], np.uint64), "n_rec": N_REC,
            "floor": np.zeros(1, np.int32), "mat0": mat, "mat1": mat.copy(), "mat2": mat.copy(), "pr": np.array([0, 2], np.uint32), "pp": np.zeros(N_PAIRS, np.uint32),
            "n_pairs": N_PAIRS, "slots": SLOTS, "zero": 0, "pair0": pair, "pair1": pair.copy(), "pair2": pair.copy(), "items8": np.zeros((N_PAIRS, SLOTS, 8), np.int32),
            "items4": np.zeros((N_PAIRS, SLOTS, 4), np.int32), "ro": np.array([0, 10, 20], np.uint64), "rows0": np.zeros(20, np.int32), "rows1": np.zeros(20, np.int32)}


def call(ctx, db, op, dev, **changed):
    """the code of one entry with the arguments of good(), some of them changed"""
    args, bufs, vals = [], [], dict(good(), **changed)
    try:
        for name in OPS[op][0].split():
            v = vals[name]
            if isinstance(v, np.ndarray) and dev:
                bufs.append(ctx.alloc(max(v.nbytes, 16)))
                ctx.upload(bufs[-1], v)
                v = bufs[-1]
            elif isinstance(v, np.ndarray):
                bufs.append(v)                                      # (kept alive)
                v = v.ctypes.data
            args.append(v)
        return getattr(ctx.L, "gs_hmm_" + op + ("_dev" if dev else ""))(ctx.h, db.h, *args)
    finally:
        for p in bufs if dev else ():
            ctx.free(p)


@pytest.mark.parametrize("op", sorted(OPS))
def test_both_entries_refuse_alike(gpu_ctx, db, op):
    import gsearch_amd as G
    both = lambda **changed: (call(gpu_ctx, db, op, False, **changed), call(gpu_ctx, db, op, True, **changed))         # noqa: E731
    assert both() == (GS_OK, GS_OK)
    assert both(**{OPS[op][1]: None}) == (GS_ERR_INVALID, GS_ERR_INVALID)                                                # the output it cannot do without
    over = dict(rl=np.array([10, (1 << 18) + 1, 10], np.uint64), rs=np.array([0, 0, 10], np.uint64), pr=np.array([0, 1], np.uint32))
    assert both(**over) == (GS_ERR_UNSUPPORTED, GS_ERR_UNSUPPORTED)                                                    # a faked length: refused before anything reads record 1
    other = G.Context(0)
    try:
        assert (call(other, db, op, False), call(other, db, op, True)) == (GS_ERR_INVALID, GS_ERR_INVALID)
    finally:
        other.close()
    if "pr" in OPS[op][0].split():
        assert both(pr=np.array([0, N_REC], np.uint32)) == (GS_ERR_INVALID, GS_ERR_INVALID)
        assert both(pp=np.array([0, 1], np.uint32)) == (GS_ERR_INVALID, GS_ERR_INVALID)
        assert both(pr=np.array([0, R.NO_HIT], np.uint32)) == (GS_OK, GS_OK)
    if "ro" in OPS[op][0].split():
        assert both(ro=np.array([0, 10, 19], np.uint64)) == (GS_ERR_INVALID, GS_ERR_INVALID)                            # the second pair's 10 rows do not fit 9 words
        assert both(ro=np.array([0, 11, 10], np.uint64)) == (GS_ERR_INVALID, GS_ERR_INVALID)                            # offsets that decrease
        assert both(rows1=None) == (GS_ERR_INVALID, GS_ERR_INVALID)                                                    # row_off, out_rows and cont_rows go together
