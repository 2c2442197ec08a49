#!/usr/bin/env python3
"""Rates of superaai on the device on seeded synthetic proteome families: `fam` families of `members` proteomes of `length`
residues, each member its family's base with `subst` substitutions per residue, so that similarities within a family are not zero.

  sketch   k-mers/s of FracMinHashSketch.sketch_genomes at the defaults (k 7, scaled 100, num 5120), batches of `batch` proteomes
  pairs    pairs/s of frac_similarity_qxc for nq x nr of those sketches
  writer   seconds of write_superaai for the nq x nr matrix
  files    files/s of sketch_files over `files` .faa.gz files
  check    sampled rows compared with the numpy reference (tests/pyref_aai.py): the expected difference is 0

usage: aai_rate.py [--n 10000] [--nq 2000] [--length 1200000] [--files 1000] [--file-length 300000]"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


def family_members(seed, n, length, members, subst):
    """proteome i of the run: base of family i // members, with subst * length substitutions drawn from the member's own stream"""
    bases = {}
    for i in range(n):
        f = i // members
        if f not in bases:
            bases = {f: AA[np.random.default_rng((seed, f)).integers(0, 20, length)]}
        s = bases[f].copy()
        rng = np.random.default_rng((seed, f, i))
        pos = rng.integers(0, length, int(subst * length))
        s[pos] = AA[rng.integers(0, 20, len(pos))]
        yield s.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--length", type=int, default=1_200_000)
    ap.add_argument("--members", type=int, default=10)
    ap.add_argument("--subst", type=float, default=0.03)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--file-length", type=int, default=300_000)
    ap.add_argument("--check", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import gsearch_amd as G
    import pyref_aai as PR
    k, scaled, num = 7, 100, 5120
    sk = G.FracMinHashSketch(k, scaled, num)
    res = {"n": a.n, "length": a.length, "members": a.members, "subst": a.subst}
    sketches, t_dev, windows, gen_s = [], 0.0, 0, 0.0
    it = family_members(a.seed, a.n, a.length, a.members, a.subst)
    sample = {}
    want_rows = set(np.linspace(0, a.n - 1, a.check).astype(int).tolist()) if a.check else set()
    for b0 in range(0, a.n, a.batch):
        t0 = time.perf_counter()
        batch = [next(it) for _ in range(min(a.batch, a.n - b0))]
        gen_s += time.perf_counter() - t0
        for j, s in enumerate(batch):
            if b0 + j in want_rows:
                sample[b0 + j] = s
        t0 = time.perf_counter()
        sketches.extend(sk.sketch_genomes([[s] for s in batch]))
        t_dev += time.perf_counter() - t0
        windows += sum(len(s) - k + 1 for s in batch)
    res["sketch"] = {"proteomes": a.n, "kmers": windows, "wall_s": round(t_dev, 3), "kmers_per_s": windows / t_dev, "generate_s": round(gen_s, 1),
                     "mean_len": float(np.mean([len(x) for x in sketches]))}
    print(json.dumps({"sketch": res["sketch"]}), flush=True)
    Q = sketches[: a.nq]
    G.frac_similarity_qxc(Q[:2], sketches[:2], num)                       # first launch out of the timing
    t0 = time.perf_counter()
    sim = G.frac_similarity_qxc(Q, sketches, num)
    dt = time.perf_counter() - t0
    res["pairs"] = {"nq": len(Q), "nr": len(sketches), "wall_s": round(dt, 3), "pairs_per_s": len(Q) * len(sketches) / dt,
                    "mean_sim_same_family": float(np.mean([sim[i, j] for i in range(min(50, len(Q))) for j in range((i // a.members) * a.members,
                                                                                                                    (i // a.members + 1) * a.members) if j != i]))}
    print(json.dumps({"pairs": res["pairs"]}), flush=True)
    with tempfile.TemporaryDirectory() as td:
        qp = ["q/%06d.faa" % i for i in range(len(Q))]
        rp = ["r/%06d.faa.gz" % i for i in range(len(sketches))]
        t0 = time.perf_counter()
        G.write_superaai(os.path.join(td, "out.txt"), qp, rp, sim, k)
        dt = time.perf_counter() - t0
        res["writer"] = {"lines": len(qp) * len(rp), "bytes": os.path.getsize(os.path.join(td, "out.txt")), "wall_s": round(dt, 3)}
        print(json.dumps({"writer": res["writer"]}), flush=True)
    # sampled rows against the numpy reference: sketches and one similarity row each
    diffs = 0
    for i, s in sample.items():
        ref = PR.sketch([s], k, scaled, num)
        diffs += int(not np.array_equal(ref, sketches[i]))
        if i < len(Q):
            row = np.array([PR.similarity(ref, sketches[j], num) for j in range(0, len(sketches), max(1, len(sketches) // 500))])
            diffs += int(np.count_nonzero(row != sim[i, :: max(1, len(sketches) // 500)]))
    res["check"] = {"rows": sorted(sample), "differences": diffs}
    print(json.dumps({"check": res["check"]}), flush=True)
    if a.files:
        with tempfile.TemporaryDirectory() as td:
            paths = []
            t0 = time.perf_counter()
            for i, s in enumerate(family_members(a.seed + 1, a.files, a.file_length, a.members, a.subst)):
                p = os.path.join(td, "p%05d.faa.gz" % i)
                text = b">p%d\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n"
                with open(p, "wb") as f:
                    f.write(gzip.compress(text, compresslevel=1))
                paths.append(p)
            gen = time.perf_counter() - t0
            t0 = time.perf_counter()
            fs, nrec, nb, st = sk.sketch_files(paths, return_stats=True)
            dt = time.perf_counter() - t0
            res["files"] = {"files": len(paths), "residues_per_file": a.file_length, "wall_s": round(dt, 3), "files_per_s": len(paths) / dt,
                            "generate_s": round(gen, 1), "stats": {x: round(y, 3) for x, y in st.items()}}
            print(json.dumps({"files": res["files"]}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
