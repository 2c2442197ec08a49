"""Every function include/gsearch_amd.h declares is exercised by name somewhere in the suite: in a file under tests/ or a fuzzer under
tools/, directly (ctx.L.gs_xxx) or through the Python method of gsearch_amd that wraps it. Entry points that are left out on purpose are
listed below with the reason; none of them launches a kernel. The check reads source text only: no GPU, no library call."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# declared, and deliberately named by no test: each with its reason. A function that launches a kernel does not belong here.
UNTESTED_ON_PURPOSE = {
    "gs_version": "returns a constant string; host only",
    "gs_last_error": "the message of the last failure; read by _lib.check whenever any test sees an error code",
    "gs_sig_elem_bytes": "table look-up on the host; its values are implied by every signature dtype the tests compare",
    "gs_value_bits": "table look-up on the host",
    "gs_ctx_stream": "hands the context's stream to a host that shares it; nothing to compare on one stream",
    "gs_comm_rank": "returns the rank the communicator was created with; host only",
    "gs_sig_kind": "table look-up on the host, reached through SeqSketcherParams.sig_dtype (test_abi_cpu.py)",
    "gs_ctx_device_info": "reports the device's name and size; host only, nothing to compare with",
    "gs_ctx_timer_start": "event stopwatch of the benchmark; measures, computes nothing",
    "gs_ctx_timer_stop": "event stopwatch of the benchmark; measures, computes nothing",
    "gs_ctx_profile": "switches the per-family event timers of the profiling tools on; measures, computes nothing",
    "gs_ctx_profile_read": "reads the per-family event timers of the profiling tools; measures, computes nothing",
    "gs_index_dump_hnswrs": "one line on the host: gs_index_dump_hnswrs_ex with flags = 0, which the dump tests call",
}

# host loops that only go round more than once at shapes of their own: the test that reaches them has to stay
SHAPE_TESTS = {
    "gs_hmh_similarity_qxc": ("test_gpu_hmh_passes.py", "test_similarity_across_passes_and_blocks"),
    "gs_hmh_similarity_qxc_dev": ("test_gpu_hmh_passes.py", "test_similarity_across_passes_and_blocks"),
}


def _declared():
    hdr = open(os.path.join(ROOT, "include", "gsearch_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", hdr)))


def _corpus():
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*_fuzz.py"))
    return {f: open(f).read() for f in files if os.path.abspath(f) != os.path.abspath(__file__)}


def _wrappers():
    """gs_ name -> patterns that match a use of a Python wrapper of it: `name(` for a module function, `.name(` for a method, the name of the
    class or of a subclass for a constructor"""
    out = {}
    for path in glob.glob(os.path.join(ROOT, "gsearch_amd", "*.py")):
        if os.path.basename(path) == "_lib.py":
            continue
        src = open(path).read()
        tree = ast.parse(src)
        classes = [n for n in tree.body if isinstance(n, ast.ClassDef)]
        family = {c.name: {c.name} for c in classes}
        for _ in classes:                                            # subclasses, transitively
            for c in classes:
                for b in c.bases:
                    if isinstance(b, ast.Name) and b.id in family:
                        family[b.id] |= family[c.name]
        defs = [(None, n) for n in tree.body if isinstance(n, ast.FunctionDef)]
        defs += [(c.name, n) for c in classes for n in c.body if isinstance(n, ast.FunctionDef)]
        for cls, fn in defs:
            if cls is None:
                pats = [r"\b%s\(" % re.escape(fn.name)]
            elif fn.name in ("__init__", "new"):
                pats = [r"\b%s\b" % re.escape(c) for c in family[cls]]
            elif fn.name.startswith("__"):
                continue
            else:
                pats = [r"\.%s\(" % re.escape(fn.name)]
            for name in set(re.findall(r"\bgs_[a-z0-9_]+\b", ast.get_source_segment(src, fn))):
                out.setdefault(name, []).extend(pats)
    return out


def _uncovered(corpus):
    text = "\n".join(corpus.values())
    wrap = _wrappers()
    return [n for n in _declared() if not re.search(r"\b%s\b" % n, text) and not any(re.search(p, text) for p in wrap.get(n, []))]


def test_every_declared_function_is_named_by_a_test():
    declared = _declared()
    assert len(declared) > 100
    stale = sorted(set(UNTESTED_ON_PURPOSE) - set(declared))
    assert not stale, "listed but no longer declared: %s" % stale
    missing = sorted(set(_uncovered(_corpus())) - set(UNTESTED_ON_PURPOSE))
    assert not missing, "declared in include/gsearch_amd.h and named by no test, fuzzer or tested wrapper: %s" % missing
    assert all(len(r) > 10 for r in UNTESTED_ON_PURPOSE.values())


def test_the_check_notices_a_missing_test():
    """without the files that hold the only tests of the device forms the check reports them"""
    corpus = _corpus()
    for gone, names in (("test_gpu_aai_dev.py", {"gs_frac_sketch_batch_dev", "gs_frac_similarity_qxc_dev"}),
                        ("test_gpu_dev_forms.py", {"gs_index_parallel_search_pid_dev", "gs_index_parallel_insert_ids_dev", "gs_filter_aa_dev"})):
        rest = {f: t for f, t in corpus.items() if os.path.basename(f) != gone}
        assert len(rest) == len(corpus) - 1 and names <= set(_uncovered(rest)), gone


def test_shape_dependent_loops_keep_their_tests():
    for name, (fname, test) in SHAPE_TESTS.items():
        assert name in _declared()
        src = open(os.path.join(ROOT, "tests", fname)).read()
        assert re.search(r"^def %s\(" % test, src, flags=re.M) and "pytest.mark.gpu" in src, (name, fname, test)
        assert "skip" not in src and "xfail" not in src, fname
