"""Writes the hand-built dump and index files of hnswrs_cases.py / bigsi_file_cases.py into a directory, with cases.txt: the list of names, sweep positions
and the codes the restatements give (format: tests/host/loader_sweep.cpp). For tests/test_loader_sweep_cpu.py, and by hand for the sanitizer build:
    python tests/loader_case_dir.py DIR && make -C gsearch_amd/csrc loader_sweep_san && gsearch_amd/csrc/loader_sweep_san DIR"""
import os
import sys

import bigsi_file_cases as Bc
import hnswrs_cases as Hc
import pyref_bigsi_file as Rb
import pyref_hnswrs as Rh


def write_case_dir(path):
    """-> the number of files cases.txt lists"""
    os.makedirs(path, exist_ok=True)
    lines = []

    def put(name, data):
        with open(os.path.join(path, name), "wb") as f:
            f.write(data)
    for name in sorted(Hc.VALID):
        g, d = Rh.write(Hc.VALID[name][0])
        put(name + ".hnsw.graph", g); put(name + ".hnsw.data", d)
        lines.append("hnswrs %s 0" % name)
    for name in sorted(Hc.REFUSED):
        g, d, code, _ = Hc.REFUSED[name]
        put(name + ".hnsw.graph", g); put(name + ".hnsw.data", d)
        lines.append("hnswrs %s %d" % (name, code))
    for name in sorted(Bc.VALID):
        put(name + ".gsbx", Rb.write(Bc.VALID[name][0]))
        lines.append("gsbx %s 0" % name)
    for name in sorted(Bc.REFUSED):
        put(name + ".gsbx", Bc.REFUSED[name][0])
        lines.append("gsbx %s %d" % (name, Bc.REFUSED[name][1]))
    g, d = Rh.write(Hc.three_points())
    put("sweep_base.hnsw.graph", g); put("sweep_base.hnsw.data", d)
    for tag, _, _, code, _ in Hc.sweep_files():
        lines.append("sweep_hnswrs sweep_base %s %s %s %d" % (tag[0], tag[1], tag[2:], code))
    put("sweep_base.gsbx", Rb.write(Bc.base()))
    for tag, _, code, _ in Bc.sweep_files():
        lines.append("sweep_gsbx sweep_base %s %s %d" % (tag[0], tag[1:], code))
    with open(os.path.join(path, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


if __name__ == "__main__":
    print(write_case_dir(sys.argv[1]), "files listed in", sys.argv[1])
