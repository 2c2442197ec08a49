"""The host-only readers as a Rust or C++ host meets them: tests/host/loader_sweep.cpp, its own main linked with nothing but gs_hnswio_parse.cpp,
gs_bigsi_file.cpp and gs_hmm_parse.cpp (plain g++, no HIP, no sanitizer), runs as a child process over every hand-built case and the sweeps of the three formats. It limits its own
address space to 2 GiB first - a condition, not a measurement: the valid cases are under 1 MB and must pass under it, and a hostile header that got as
far as an allocation would not - and counts as a surprise any code that differs from the restatement's and any C++ exception that reaches its main."""
import os
import re
import subprocess

import loader_case_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsearch_amd", "csrc")


def test_loader_sweep_under_two_gib(tmp_path):
    exe = str(tmp_path / "loader_sweep")
    src = [os.path.join(ROOT, "tests", "host", "loader_sweep.cpp"), os.path.join(CSRC, "gs_hnswio_parse.cpp"), os.path.join(CSRC, "gs_bigsi_file.cpp"),
           os.path.join(CSRC, "gs_hmm_parse.cpp")]
    for s in src[1:] + [os.path.join(CSRC, h) for h in ("gs_hnswio_parse.hpp", "gs_bigsi_file.hpp", "gs_hmm_parse.hpp", "gs_host.hpp")]:        # plain C++: no HIP header behind the units
        assert not re.search(r"#\s*include\s*[<\"](hip/|gs_internal|gs_spec|gs_scratch)", open(s).read()), s
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe] + src)
    assert "setrlimit(RLIMIT_AS" in open(src[0]).read()
    cases = tmp_path / "cases"
    listed = loader_case_dir.write_case_dir(str(cases))
    assert listed > 16000           # (14 000 of them cuts and byte flips of the two profile texts)
    out = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    last = out.stdout.strip().split("\n")[-1]
    assert out.returncode == 0 and last == "%d files, 0 surprises" % listed, out.stdout[-2000:]
