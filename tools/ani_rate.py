#!/usr/bin/env python3
"""Rates of superani on the device on seeded synthetic genome families made on the device (gs_synth_dna_family_dev, one root per
family, members at 1-5 % substitutions).

  seeds    seeds/s and windows/s of gs_ani_sketch_batch_dev (k 16, c 30) over `n` genomes of `length` bases, `batch` at a time
  pairs    pairs/s and anchors/s of gs_ani_pairs_dev for `nq` genomes, each against the `members` genomes of its family
  chain    anchors/s of the chaining program alone (gs_ani_chain_dev) on diagonal anchors cut into contigs of `contig` anchors
  check    sampled pairs compared with the numpy restatement (tests/pyref_ani.py): the expected difference is 0

usage: ani_rate.py [--n 10000] [--length 5000000] [--batch 250] [--nq 1000] [--members 50] [--check 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K, C_ = 16, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--chain-pairs", type=int, default=2000)
    ap.add_argument("--chain-anchors", type=int, default=100_000)
    ap.add_argument("--contig", type=int, default=2000)
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    import gsearch_amd as G
    from gsearch_amd._lib import check
    import pyref_ani as PR
    ctx = G.default_context()
    L = ctx.L
    res = {"n": a.n, "length": a.length, "nq": a.nq, "members": a.members}
    words = (a.length + 31) // 32
    cap = int(a.length / C_ * 1.15) + 1024

    def sketch(first_seed, n):
        """n genomes of one family on the device -> (seeds (n, cap, 4) device pointer, counts, seconds)"""
        d_seq = ctx.alloc(n * words * 8 + 64)
        check(L.gs_synth_dna_family_dev(ctx.h, first_seed, 0, n, a.length, 1, 0.01, 0.05, d_seq))
        rs = (np.arange(n, dtype=np.uint64) * np.uint64(words * 32))
        rl = np.full(n, a.length, np.uint64)
        go = np.arange(n + 1, dtype=np.uint64)
        d = [ctx.alloc(x.nbytes) for x in (rs, rl, go)]
        for p, x in zip(d, (rs, rl, go)):
            ctx.upload(p, x)
        d_out, d_cnt = ctx.alloc(16 * n * cap), ctx.alloc(4 * n)
        ctx.sync()
        t = time.perf_counter()
        check(L.gs_ani_sketch_batch_dev(ctx.h, K, C_, d_seq, n * words * 8, d[0], d[1], n, d[2], n, cap, d_out, d_cnt))
        ctx.sync()
        dt = time.perf_counter() - t
        cnt = ctx.download(d_cnt, (n,), np.uint32)
        for p in d + [d_seq, d_cnt]:
            ctx.free(p)
        return d_out, cnt, dt

    # seeds
    t_dev, n_seeds = 0.0, 0
    for b0 in range(0, a.n, a.batch):
        nb = min(a.batch, a.n - b0)
        d_out, cnt, dt = sketch(a.seed + 1000 + b0, nb)
        ctx.free(d_out)
        if b0:                                           # the first batch sizes the scratch slots
            t_dev += dt; n_seeds += int(cnt.sum())
    nb_timed = max(a.n - a.batch, 0)
    if t_dev:
        res["seeds_per_s"] = n_seeds / t_dev
        res["windows_per_s"] = nb_timed * (a.length - K + 1) / t_dev
        res["sketch_genomes_per_s"] = nb_timed / t_dev

    # pairs: families of `members`, every genome against its family
    fams = max(a.nq // a.members, 1)
    q_rows, q_off, pq, pr = [], [0], [], []
    for f in range(fams):
        d_out, cnt, _ = sketch(a.seed + f, a.members)
        rows = ctx.download(d_out, (a.members, cap, 4), np.uint32)
        ctx.free(d_out)
        for g in range(a.members):
            q_rows.append(rows[g, :cnt[g]].copy())
            q_off.append(q_off[-1] + int(cnt[g]))
        pq += [f * a.members + i for i in range(a.members) for _ in range(a.members)]
        pr += [f * a.members + j for _ in range(a.members) for j in range(a.members)]
    flat, off = np.concatenate(q_rows), np.array(q_off, np.uint64)
    pq, pr = np.array(pq, np.uint32), np.array(pr, np.uint32)
    arrs = [flat, off, pq, pr]
    d = [ctx.alloc(x.nbytes) for x in arrs]
    for p, x in zip(d, arrs):
        ctx.upload(p, x)
    d_res = ctx.alloc(64 * len(pq))
    ng = len(off) - 1
    for rep in range(2):                                 # the first run sizes the scratch slots
        ctx.sync()
        t = time.perf_counter()
        check(L.gs_ani_pairs_dev(ctx.h, K, d[0], d[1], ng, d[0], d[1], ng, d[2], d[3], len(pq), d_res, 0))
        ctx.sync()
        dt = time.perf_counter() - t
    out = ctx.download(d_res, (len(pq), 8), np.uint64)
    res["pairs"] = len(pq)
    res["pairs_per_s"] = len(pq) / dt
    res["anchors_per_s"] = int(out[:, 0].sum()) / dt
    res["anchors_per_pair"] = float(out[:, 0].mean())
    rng = np.random.default_rng(a.seed)
    bad = 0
    for p in rng.choice(len(pq), min(a.check, len(pq)), replace=False):
        want = PR.pair_counts(q_rows[pq[p]], q_rows[pr[p]], K)
        bad += int(out[p].tolist() != want)
    res["checked_pairs"], res["checked_pairs_differing"] = int(min(a.check, len(pq))), bad
    for p in d + [d_res]:
        ctx.free(p)

    # the chaining program alone
    n_a = a.chain_pairs * a.chain_anchors
    i = np.arange(a.chain_anchors, dtype=np.uint32)
    one = [i // np.uint32(a.contig), i * np.uint32(40), i // np.uint32(a.contig), i * np.uint32(40) + (i % np.uint32(7)), np.zeros_like(i)]
    cols = [np.tile(x, a.chain_pairs) for x in one]
    offs = (np.arange(a.chain_pairs + 1, dtype=np.uint64) * np.uint64(a.chain_anchors))
    d = [ctx.alloc(x.nbytes) for x in cols + [offs]]
    for p, x in zip(d, cols + [offs]):
        ctx.upload(p, x)
    d_o = [ctx.alloc(4 * n_a) for _ in range(3)]
    for rep in range(2):
        ctx.sync()
        t = time.perf_counter()
        check(L.gs_ani_chain_dev(ctx.h, *d[:5], d[5], a.chain_pairs, *d_o))
        ctx.sync()
        dt = time.perf_counter() - t
    res["chain_anchors_per_s"] = n_a / dt
    f = ctx.download(d_o[0], (n_a,), np.int32)[:a.chain_anchors]
    wf, _, _ = PR.chain({"rcontig": one[0], "rpos": one[1], "qcontig": one[2], "qpos": one[3], "strand": one[4]}) if a.chain_anchors <= 200_000 else (f, 0, 0)
    res["chain_f_differing"] = int((f != wf).sum())
    for p in d + d_o:
        ctx.free(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
