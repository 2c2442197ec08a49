"""gs_hmm_hit_records_dev (gs_hmm_hits.hip; SPEC 13.8) `==` the numpy restatement (tests/pyref_hit_records.py) on every output word and byte, on the
constructed cases of tests/hit_records_cases.py: n_genomes in {1, 3, 70} x n_prof in {1, 2, 120, 130} (the span kernel's 256-thread blocks and the copy
kernel's four wavefronts a block end inside, at and behind those), an all-NO_HIT matrix, an empty genome first, in the middle and last, a record chosen
by two profiles, record and span lengths 1 .. 4097 (below, at and above a wavefront's 64 bytes a trip) at source and destination offsets of every residue
mod 8, spans with n_item = 0, 1 and max_item with i_from = 1 and i_to = L, the three slot widths. The outputs are pre-filled: nothing is written at or
behind n_out, and a refusal writes nothing at all. Everything runs on scratch poisoned with 0x00 and 0xFF too (tests/test_gpu_stale_scratch.py's way).
The cases' own promises are checked by tests/test_hit_records_cpu.py; the references are computed once."""
import numpy as np
import pytest

import hit_records_cases as HC
import pyref_hit_records as R

pytestmark = pytest.mark.gpu
PATTERN = 0xA5


@pytest.fixture(scope="module")
def world():
    cases = HC.all_cases()
    return [(c, R.hit_records(c["best_rec"], c["aa"], c["rec_start"], c["rec_len"], c["n_item"], c["item"])) for c in cases]


class _Dev:
    """a case on the device, pattern-filled outputs of the given room beside it"""

    def __init__(self, G, ctx, case, room_rec, room_aa):
        self.G, self.ctx, self.bufs = G, ctx, []
        self.ng, self.npf = case["best_rec"].shape
        self.n_rec = len(case["rec_len"])
        self.rec, self.aa, self.rs, self.rl = (self.up(case[k]) for k in ("best_rec", "aa", "rec_start", "rec_len"))
        self.spans = {}
        if case["item"] is not None:
            self.spans = dict(n_item_dev=self.up(case["n_item"]), item_dev=self.up(case["item"]), item_words=case["item"].shape[2], max_item=case["item"].shape[1])
        self.shape = ((room_aa + 7) // 8 * 8 + 8, 8 * (room_rec + 2), 8 * (room_rec + 2), 8 * (self.ng + 1))
        self.out = [self.up(np.full(n, PATTERN, np.uint8)) for n in self.shape]

    def up(self, a):
        a = np.ascontiguousarray(a)
        ptr = self.ctx.alloc(max(a.nbytes, 16))
        self.bufs.append(ptr)
        if a.nbytes:
            self.ctx.upload(ptr, a)
        return ptr

    def run(self, cap_rec, cap_aa):
        return self.G.hit_records_dev(self.ctx, self.rec, self.ng, self.npf, self.aa, self.rs, self.rl, self.n_rec, cap_rec, cap_aa, *self.out, **self.spans)

    def read(self):
        return [self.ctx.download(p, (n,), np.uint8) for p, n in zip(self.out, self.shape)]

    def close(self):
        for p in self.bufs:
            self.ctx.free(p)


def _check(G, ctx, case, want):
    n_hit, n_aa = len(want[1]), len(want[0])
    d = _Dev(G, ctx, case, n_hit, n_aa)
    try:
        assert d.run(n_hit, n_aa) == (n_hit, n_aa), case["name"]
        aa, start, ln, goff = d.read()
    finally:
        d.close()
    assert np.array_equal(aa[:n_aa], want[0]) and (aa[n_aa:] == PATTERN).all(), case["name"]
    for got, w in ((start, want[1]), (ln, want[2])):
        assert np.array_equal(got[:8 * n_hit].view(np.uint64), w) and (got[8 * n_hit:] == PATTERN).all(), case["name"]
    assert np.array_equal(goff.view(np.uint64), want[3]), case["name"]


@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_device_form_is_the_restatement(gpu_ctx, world, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        gpu_ctx.release_scratch()                            # the slots are leased anew: poisoned when a fill is on
        for case, want in world:
            _check(G, gpu_ctx, case, want)
    finally:
        G.debug_mem_fill(None)


@pytest.mark.parametrize("fill", [None, 0xFF])
def test_refusals_write_nothing(gpu_ctx, fill):
    import gsearch_amd as G
    G.debug_mem_fill(fill)
    try:
        for what, case, cap_rec, cap_aa in HC.error_cases():
            with pytest.raises(R.Refused) as want:
                R.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"], cap_rec, cap_aa)
            d = _Dev(G, gpu_ctx, case, 64, 4096)
            try:
                with pytest.raises(G.GsError) as got:
                    d.run(64 if cap_rec is None else cap_rec, 4096 if cap_aa is None else cap_aa)
                outs = d.read()
            finally:
                d.close()
            assert got.value.code == want.value.code == G._lib.GS_ERR_INVALID, what
            assert got.value.counts == want.value.counts, what
            assert all((o == PATTERN).all() for o in outs), what
    finally:
        G.debug_mem_fill(None)


def test_counts_first_then_a_call_with_room(gpu_ctx, world):
    """room for nothing: the refusal carries the counts, and a second call sized by them gives the restatement"""
    import gsearch_amd as G
    case, want = next((c, w) for c, w in world if c["name"] == "shape 3x120")
    d = _Dev(G, gpu_ctx, case, len(want[1]), len(want[0]))
    try:
        with pytest.raises(G.GsError) as e:
            d.run(0, 0)
        assert e.value.counts == (len(want[1]), len(want[0])) and all((o == PATTERN).all() for o in d.read())
        assert d.run(*e.value.counts) == e.value.counts
        assert np.array_equal(d.read()[0][:len(want[0])], want[0])
    finally:
        d.close()


def test_device_form_is_its_host_twin(gpu_ctx, world):
    import gsearch_amd as G
    for case, want in world[:4]:
        got = G.hit_records(case["best_rec"], case["aa"], case["rec_start"], case["rec_len"], case["n_item"], case["item"])
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
