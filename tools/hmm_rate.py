#!/usr/bin/env python3
"""Rate of hmmsearch on the device: a synthetic proteome of `n` proteins (lengths drawn around 300 residues, background
composition) against 120 synthetic profiles with the node counts of the bacterial universal-gene set
(tests/golden/hmm/bacteria_node_counts.txt).

  search   cells/s of gs_hmm_search_dev (cells = residues of the proteome x nodes of the set), device arrays in place, the best of `repeat` runs
  best     seconds of gs_hmm_best_hits_dev over the score matrix, the proteome as one genome
  check    `check` sampled (protein, profile) pairs compared with the numpy restatement (tests/pyref_hmm.py): the expected difference is 0

usage: hmm_rate.py [--n 4000] [--repeat 3] [--check 8] [--log profiles/hmm_rate.log]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "hmm_rate.log"))
    a = ap.parse_args()
    import gsearch_amd as G
    import pyref_hmm as R
    rng = np.random.default_rng(a.seed)
    nodes = [int(x) for x in open(os.path.join(ROOT, "tests", "golden", "hmm", "bacteria_node_counts.txt")).read().split()]
    texts = [R.write_hmm(R.synth_model(rng, M, name="SYN%03d_%d" % (i, M))) for i, M in enumerate(nodes)]
    ctx = G.default_context()
    db = G.HmmDb(texts, ctx, texts=True)
    lens = np.clip(rng.gamma(3.0, 100.0, size=a.n).astype(np.int64), 30, 3000)
    recs = [R.background(rng, int(L)) for L in lens]
    for j in range(0, a.n, 40):                                  # one protein in 40 carries the consensus of a profile, as a proteome would
        recs[j] = R.consensus(R.parse_hmm(texts[(j // 40) % len(texts)])[0]["tables"])
    aa, rs, rl = G.filter_aa_records(recs)
    cells = int(rl.sum()) * sum(nodes)
    res = {"proteins": a.n, "residues": int(rl.sum()), "profiles": len(nodes), "nodes": sum(nodes), "cells": cells}
    goff = np.array([0, a.n], np.uint64)
    thr = db.thresholds("ga")
    arrays = (aa, rs, rl, goff, thr)
    ptrs = [ctx.alloc(max(x.nbytes, 16)) for x in arrays]
    for p, x in zip(ptrs, arrays):
        ctx.upload(p, x)
    d_score = ctx.alloc(4 * a.n * len(db))
    d_rec, d_best = ctx.alloc(4 * len(db)), ctx.alloc(4 * len(db))
    best = float("inf")
    for run in range(a.repeat + 1):                              # the first run pays for the module load and the scratch: not counted
        ctx.sync()
        t = time.perf_counter()
        db.search_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_score)
        ctx.sync()
        if run:
            best = min(best, time.perf_counter() - t)
    res["search_s"] = best
    res["cells_per_s"] = cells / best
    t = time.perf_counter()
    db.best_hits_dev(d_score, a.n, ptrs[3], 1, ptrs[4], d_rec, d_best)
    ctx.sync()
    res["best_hits_s"] = time.perf_counter() - t
    scores = ctx.download(d_score, (a.n, len(db)), np.int32)
    hit = ctx.download(d_rec, (len(db),), np.uint32)
    res["profiles_with_a_hit"] = int((hit != R.NO_HIT).sum())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(len(db)))
        diff += int(scores[r, p]) != R.viterbi(R.parse_hmm(texts[p])[0]["tables"], recs[r])
    res["check_pairs"], res["check_differences"] = a.check, diff
    for p in ptrs + [d_score, d_rec, d_best]:
        ctx.free(p)
    db.close()
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
