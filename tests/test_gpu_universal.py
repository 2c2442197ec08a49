"""gsearch_amd.universal_sketch (SPEC 17 item 11) against the host composition it replaces: the kept rows `==` sketcher.sketch_genomes(universal_genes(...)[0])
bit for bit, best_rec `==` universal_genes' local matrix, the hit and residue counts those of its lists. Three planted genomes (tests/universal_case.py):
both profiles' genes, one gene, none - as protein FASTA, as nucleotide FASTA searched through its six-frame ORFs and through its called genes (the
third file compressed). Every target form x region x score x prefilter, each with the optdens and the prob sketcher at k = 5, s = 256. universal_genes is
run once per combination and shared by both sketchers."""
import numpy as np
import pytest

import pyref_hmm as RH
import universal_case as U

pytestmark = pytest.mark.gpu
FORMS = {"faa": None, "orfs": True, "genes": "genes"}
REGIONS = ("protein", "aligned", "envelope", "alignment")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("universal")
    cons = [RH.consensus(m["tables"]) for m in U.models()]
    files = {"faa": [], "orfs": [], "genes": []}
    for g, planted in enumerate(((0, 1), (0,), ())):
        contigs, proteins, _ = U.genome(40 + g, cons, planted, fraction=0.1)
        paths = U.write_genome(d, "g%d" % g, contigs, proteins)
        files["faa"].append(paths["faa"])
        for form in ("orfs", "genes"):
            files[form].append(paths["fna.gz" if g == 2 else "fna"])
    return {"files": files, "profiles": U.profile_paths()}


@pytest.fixture(scope="module")
def sketchers(gpu_ctx):
    import gsearch_amd as G
    return [G.sketcher_for(G.SeqSketcherParams(5, 256, algo, "aa"), gpu_ctx) for algo in ("optdens", "prob")]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _compare(G, sk, files, profiles, ctx, want, **opts):
    genomes, local = want
    sig, nrec, nsym, best, stats = G.universal_sketch(files, profiles, sk, ctx=ctx, **opts)
    assert sig.shape == (len(files), 256) and sig.dtype == sk.sig_dtype()
    assert [int(v) for v in nrec] == [len(g) for g in genomes] and [int(v) for v in nsym] == [sum(len(r) for r in g) for g in genomes], opts
    assert best.dtype == np.uint32 and np.array_equal(best, local), opts
    kept = [i for i, g in enumerate(genomes) if g]
    rows = sk.sketch_genomes([genomes[i] for i in kept])
    assert np.array_equal(_bits(sig[kept]), _bits(rows)), (opts, sk.params.c.algo)
    assert set(stats["stage_s"]) == set(G.UNIVERSAL_STAGES)
    return sig, nrec, nsym, best


@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("form", list(FORMS))
def test_rows_are_the_host_composition(gpu_ctx, world, sketchers, form, region):
    import gsearch_amd as G
    files, profiles = world["files"][form], world["profiles"]
    for score in ("viterbi", "forward"):
        for prefilter in (None, "msv+vit16"):
            opts = dict(region=region, score=score, prefilter=prefilter, translate=FORMS[form])
            want = G.universal_genes(files, profiles, ctx=gpu_ctx, **dict(opts, translate=FORMS[form] or False))[:2]
            print(form, region, score, prefilter, [[len(r) for r in g] for g in want[0]])
            assert [len(g) for g in want[0]] == [2, 1, 0]                  # both genes, one, none: the third file is skipped by the commands
            for sk in sketchers:
                _compare(G, sk, files, profiles, gpu_ctx, want, **opts)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_genome_a_round_gives_the_arrays_of_the_default(gpu_ctx, world, sketchers, form):
    import gsearch_amd as G
    files, profiles = world["files"][form], world["profiles"]
    db = G.HmmDb(profiles, gpu_ctx)                                         # an HmmDb is taken as it is
    a = G.universal_sketch(files, db, sketchers[0], region="envelope", score="forward", translate=FORMS[form])
    b = G.universal_sketch(files, db, sketchers[0], region="envelope", score="forward", translate=FORMS[form], genomes_per_call=1)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b[:4]))
    assert a[4]["rounds"] == 1 and b[4]["rounds"] == 3 and int(a[1].sum()) == 3
    db.close()


def test_refusals(gpu_ctx, world, sketchers):
    import gsearch_amd as G
    files, profiles = world["files"]["faa"], world["profiles"]
    with pytest.raises(ValueError):
        G.universal_sketch(files, profiles, sketchers[0], ctx=gpu_ctx, score="forward", bias=True)
    with pytest.raises(ValueError):
        G.universal_sketch(files, profiles, sketchers[0], ctx=gpu_ctx, region="domain")
    with pytest.raises(ValueError):
        G.universal_sketch(files, profiles, G.sketcher_for(G.SeqSketcherParams(16, 256, "optdens", "dna"), gpu_ctx), ctx=gpu_ctx)
    sig, nrec, nsym, best, _ = G.universal_sketch([], profiles, sketchers[0], ctx=gpu_ctx)
    assert sig.shape == (0, 256) and best.shape == (0, 2) and len(nrec) == len(nsym) == 0
