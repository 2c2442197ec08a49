"""Writes the hand-built dump and index files of hnswrs_cases.py / bigsi_file_cases.py and two synthetic profile texts into a directory, with cases.txt: the
list of names, sweep positions and the codes the restatements give (format: tests/host/loader_sweep.cpp). For tests/test_loader_sweep_cpu.py, and by hand for the sanitizer build:
    python tests/loader_case_dir.py DIR && make -C gsearch_amd/csrc loader_sweep_san && gsearch_amd/csrc/loader_sweep_san DIR"""
import os
import sys

import numpy as np

import bigsi_file_cases as Bc
import hnswrs_cases as Hc
import pyref_bigsi_file as Rb
import pyref_hmm as Rm
import pyref_hnswrs as Rh


def hmm_code(text):
    """the code gs_hmm_parse_mem gives a text, from the restatement: accepted, unsupported (M over the limit), or invalid"""
    try:
        Rm.parse_hmm(text)
    except Rm.HmmError as e:
        return -3 if str(e).startswith("unsupported") else -1
    return 0


def hmm_texts():
    """two single-model texts of 3 nodes, one per dialect, with and without a COMPO line"""
    return {"sweep_compo": Rm.write_hmm(Rm.synth_model(np.random.default_rng(31), 3), "f", True),
            "sweep_plain": Rm.write_hmm(Rm.synth_model(np.random.default_rng(32), 3), "b", False)}


def hmm_sweep(text):
    """(kind, pos, code) of every cut and of both flips of every byte. A cut is accepted from the offset just past the final `//` on, and only from there."""
    end = text.rindex(b"//") + 2
    for pos in range(len(text) + 1):
        yield "p", pos, 0 if pos >= end else -1
    for pos in range(len(text)):
        yield "f", pos, hmm_code(text[:pos] + b"\xff" + text[pos + 1:])
        yield "x", pos, hmm_code(text[:pos] + bytes([text[pos] ^ 1]) + text[pos + 1:])


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
    for name, text in sorted(hmm_texts().items()):
        put(name + ".hmm", text)
        lines.append("hmm %s 0" % name)
        lines += ["sweep_hmm %s %s %d %d" % ((name,) + c) for c in hmm_sweep(text)]
    with open(os.path.join(path, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


if __name__ == "__main__":
    print(write_case_dir(sys.argv[1]), "files listed in", sys.argv[1])
