"""The three kinds of device targets under hmmsearch() and universal_genes() (`_DevProteins`, `_DevOrfs`, `_DevGenes`: one `_DevTargets`) where the one
body over them can go wrong: a target set with nothing to search in every form, the host copy a protein source answers residues() from against the
device copy the searches read, and the alignment slots with and without their columns. The genomes are those of tests/universal_case.py: two profiles,
three contigs a genome."""
import numpy as np
import pytest

import pyref_hmm as RH
import universal_case as U

pytestmark = pytest.mark.gpu
FORMS = {"faa": False, "orfs": True, "genes": "genes"}
REGIONS = ("protein", "aligned", "envelope", "alignment")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """two planted genomes (both profiles' genes; one gene) in every form, and per form a file that holds no target: a protein record without a residue
    letter, a contig too short for an ORF or a gene"""
    d = tmp_path_factory.mktemp("targets")
    cons = [RH.consensus(m["tables"]) for m in U.models()]
    files = {form: [] for form in FORMS}
    for g, planted in enumerate(((0, 1), (0,))):
        contigs, proteins, _ = U.genome(40 + g, cons, planted, fraction=0.1)
        paths = U.write_genome(d, "g%d" % g, contigs, proteins, forms=("faa", "fna"))
        for form in FORMS:
            files[form].append(paths["faa" if form == "faa" else "fna"])
    empty = {}
    for name, text in (("faa", b">x\nXXXX\n"), ("fna", b">c\nACGT\n")):
        path = str(d / ("empty." + name))
        with open(path, "wb") as f:
            f.write(text)
        empty.update({"faa": path} if name == "faa" else {"orfs": path, "genes": path})
    return {"files": files, "empty": empty, "profiles": U.profile_paths()}


@pytest.mark.parametrize("form", list(FORMS))
def test_hmmsearch_of_nothing_to_search(gpu_ctx, world, tmp_path, form):
    """every output of hmmsearch() on a file without a target: no score, and four tables of their first line alone. The .faa keeps its one (empty) record,
    a row of HMM_NO_SCORE; the nucleotide forms have no target and no row"""
    import gsearch_amd as G
    out = [str(tmp_path / n) for n in ("table", "dom", "env", "ali")]
    got = G.hmmsearch(world["empty"][form], world["profiles"], out[0], ctx=gpu_ctx, score="forward", bias=True, domains=out[1], envelopes=out[2],
                      alignments=out[3], translate=FORMS[form])
    ids, scores, texts = got[0], got[1], got[2:]
    assert len(got) == 6 and len(ids) == (1 if form == "faa" else 0) and (form != "faa" or ids == ["x"])
    assert scores.shape == (len(ids), 2) and scores.dtype == np.int32 and (scores == RH.NO_SCORE).all()
    firsts = (b"target\tprofile\tacc\tbits\tevalue\tpass_ga\tbias\n", b"target\tprofile\tacc\tdom\tn_dom\t", b"target\tprofile\tacc\tenv\tn_env\t", b"# == target\t")
    for text, path, first in zip(texts, out, firsts):
        assert text.startswith(first) and text.count(b"\n") == 1 and text.endswith(b"\n"), text
        assert open(path, "rb").read() == text


@pytest.mark.parametrize("form", list(FORMS))
def test_universal_genes_around_a_genome_without_targets(gpu_ctx, world, form):
    """[planted, nothing to search, planted]: the middle genome gets no hit and a row of HMM_NO_HIT, the outer two what a call over each alone returns -
    with the best hits taken on the device (Viterbi) and on the host behind the bias correction (Forward), in every region"""
    import gsearch_amd as G
    a, b = world["files"][form]
    db = G.HmmDb(world["profiles"], gpu_ctx)
    try:
        for opts in ({}, {"score": "forward", "bias": True}):
            for region in REGIONS:
                run = lambda files: G.universal_genes(files, db, region=region, translate=FORMS[form], **opts)      # noqa: E731
                got, alone = run([a, world["empty"][form], b]), [run([a]), run([b])]
                assert len(got) == len(alone[0]) == (3 if FORMS[form] else 2), (form, region)
                assert got[0][1] == [] and got[1].shape == (3, 2) and got[1].dtype == np.uint32 and (got[1][1] == RH.NO_HIT).all()
                assert [len(x[0][0]) for x in alone] == [2, 1], (form, region, opts)
                for at, one in zip((0, 2), alone):
                    assert got[0][at] == one[0][0], (form, region, opts, at)
                    assert all(np.array_equal(x[at], y[0]) for x, y in zip(got[1:], one[1:])), (form, region, opts, at)
                if FORMS[form]:
                    assert got[2].shape == (3, 2, 4) and (got[2][1] == -1).all()
    finally:
        db.close()


def test_protein_residues_are_the_device_copy(gpu_ctx, world):
    """_DevProteins answers residues() from the host arrays it uploaded: the same bytes read back from d_aa, for the first and the last record, an empty
    cut and an inner one; the names are the records' ids"""
    from gsearch_amd import api as A
    dev = A._DevProteins(gpu_ctx, world["files"]["faa"])
    try:
        assert dev.n == 96 and dev.genome_orf_off.tolist() == [0, 48, 96] and dev.n_long == 0
        assert dev.names() == ["g%d_p%d" % (g, i) for g in range(2) for i in range(48)]
        for j, a, b in ((0, 0, None), (dev.n - 1, 0, None), (0, 5, 5), (dev.n - 1, 451, 451), (50, 17, 203), (1, 450, 451)):
            e = int(dev.aa_len[j]) if b is None else b
            want = gpu_ctx.download(dev.d_aa + int(dev.aa_start[j]) + a, (e - a,), np.uint8).tobytes() if e > a else b""
            got = dev.residues(j, a, b)
            assert isinstance(got, bytes) and got == want and len(got) == e - a, (j, a, b)
        assert len(dev.residues(0)) == 451 and dev.residues(0)[:1] == b"M"
    finally:
        dev.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_align_listed_slots_without_columns(gpu_ctx, world, form):
    """align_listed(columns=False) builds no column and returns the slots of columns=True, on the best hits of a planted genome"""
    import gsearch_amd as G
    from gsearch_amd import api as A
    db = G.HmmDb(world["profiles"], gpu_ctx)
    dev = A._dev_targets(gpu_ctx, world["files"][form][:1], FORMS[form], G._lib.ORF_MIN_AA, A._orf_max_aa(True, False), 11)
    try:
        rec, _ = db.best_hits(dev.search(db, True, 1e-3), dev.genome_orf_off)
        assert rec.shape == (1, 2) and (rec != RH.NO_HIT).all()
        pr, pp = rec.reshape(-1), np.arange(2, dtype=np.uint32)
        _, _, ne, env = dev.envelopes_all(db, pr, pp)
        slots, cols = dev.align_listed(db, pr, pp, ne, env)
        alone = dev.align_listed(db, pr, pp, ne, env, columns=False)
        assert ne.all() and slots[:, 0, 5].all() and [len(c) for c in cols] == [int(n) for n in ne]
        assert isinstance(alone, np.ndarray) and alone.dtype == slots.dtype and np.array_equal(alone, slots)
        got = dev.align_all(db, pr, pp, columns=False)
        assert len(got) == 4 and np.array_equal(got[1], ne) and np.array_equal(got[2], env) and np.array_equal(got[3], slots)
        if form == "faa":                                                   # HmmDb.align_all, the host form of the same pass, over the host copy
            host = db.align_all(dev.aa, dev.aa_start, dev.aa_len, pr, pp, columns=False)
            assert len(host) == 4 and all(np.array_equal(x, y) for x, y in zip(host, got))
            host = db.align_all(dev.aa, dev.aa_start, dev.aa_len, pr, pp)
            assert len(host) == 5 and np.array_equal(host[3], slots) and [len(c) for c in host[4]] == [len(c) for c in cols]
            assert all(np.array_equal(a, b) for x, y in zip(host[4], cols) for u, v in zip(x, y) for a, b in zip(u, v))
    finally:
        dev.close()
        db.close()
