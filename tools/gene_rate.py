#!/usr/bin/env python3
"""Rates of the gene caller on the device (SPEC 15, DESIGN 3.21, gs_gene.hip), next to gs_orf_translate_dev on the same input.

  input       `genomes` genomes of `len` bases, one record each: uniform random bases with genes planted by the recipe of the method test
              (tests/gene_cases.py: a gamma(0.5) codon usage per genome, ATG + 58..598 codons + a stop, random strand, gaps of 20..399). `distinct`
              different genomes are made on the host and repeated in turn, since making one takes seconds.
  orf         gs_orf_translate_dev (descriptors and residues), the yardstick
  call        gs_gene_call_dev, count-only and with outputs: the whole pipeline of `rounds` rounds
  train       gs_gene_train_dev on the round-1 intervals (the ORFs of train_min_aa codons and more): both histograms and the tables
  score       gs_gene_score_dev on every ORF under the tables of the call
All by events on the context's stream, a warm-up and then the best of `repeat` runs.

usage: gene_rate.py [--genomes 16 64] [--len 5000000] [--distinct 2] [--repeat 3] [--log profiles/gene_rate.log]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pack(codes):
    c = np.concatenate([codes, np.zeros((-len(codes)) % 4, np.uint8)]).reshape(-1, 4)
    return ((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8)


def best_of(ctx, repeat, fn):
    best = float("inf")
    for run in range(repeat + 1):
        ctx.sync()
        ctx.timer_start()
        out = fn()
        ms = ctx.timer_stop()
        if run:
            best = min(best, ms * 1e-3)
    return best, out


def measure(G, GC, ctx, N, L, distinct, repeat):
    made = [pack(GC.planted_genome(100 + i, L)[0]) for i in range(min(distinct, N))]
    stride = (len(made[0]) + 63) // 64 * 64
    seq = np.zeros(N * stride, np.uint8)
    for g in range(N):
        seq[g * stride:g * stride + len(made[0])] = made[g % len(made)]
    rs, rl, goff = np.arange(N, dtype=np.uint64) * np.uint64(4 * stride), np.full(N, L, np.uint64), np.arange(N + 1, dtype=np.uint64)
    ptrs = []

    def up(a):
        p = ctx.alloc(max(a.nbytes, 16))
        ctx.upload(p, a)
        ptrs.append(p)
        return p

    def new(n):
        p = ctx.alloc(max(int(n), 16))
        ptrs.append(p)
        return p
    d_seq, d_rs, d_rl, d_goff = up(seq), up(rs), up(rl), up(goff)
    res = {"genomes": N, "len": L, "bases": N * L, "distinct": len(made)}
    prm = G.gene_params()
    # the yardstick
    n_orf, n_aa, _ = G.orf_translate_dev(ctx, d_seq, seq.nbytes, d_rs, d_rl, N)
    o_orf, o_aa, o_as, o_al, o_off = new(16 * n_orf), new(n_aa), new(8 * n_orf), new(8 * n_orf), new(8 * (N + 1))
    res["orf_translate_s"], _ = best_of(ctx, repeat, lambda: G.orf_translate_dev(ctx, d_seq, seq.nbytes, d_rs, d_rl, N, n_orf, n_aa, o_orf, o_aa, o_as, o_al, o_off))
    res["orfs"], res["orf_residues"] = n_orf, n_aa
    # the whole call
    d_info, d_tab = new(16 * N), new(4 * 4096 * N)
    res["call_count_s"], (n_gene, n_gaa) = best_of(ctx, repeat, lambda: G.gene_call_dev(ctx, d_seq, seq.nbytes, d_rs, d_rl, N, d_goff, N, d_info, tables_out_dev=d_tab))
    g_gene, g_aa, g_as, g_al, g_off = new(32 * n_gene), new(n_gaa), new(8 * n_gene), new(8 * n_gene), new(8 * (N + 1))
    res["call_s"], _ = best_of(ctx, repeat, lambda: G.gene_call_dev(ctx, d_seq, seq.nbytes, d_rs, d_rl, N, d_goff, N, d_info, n_gene, n_gaa, g_gene, g_aa, g_as, g_al, g_off,
                                                                    tables_out_dev=d_tab))
    info = ctx.download(d_info, (N, 2), np.uint64)
    res.update(genes=n_gene, gene_residues=n_gaa, trained=int((info[:, 1] & 1).sum()), call_over_orf=res["call_s"] / res["orf_translate_s"])
    # the stage entries on the same ORFs
    orf, olen = ctx.download(o_orf, (n_orf,), G.ORF_DTYPE), ctx.download(o_al, (n_orf,), np.uint64)
    keep = olen >= prm.train_min_aa
    iv = np.zeros(int(keep.sum()), G.GENE_INTERVAL_DTYPE)
    iv["begin"], iv["n"], iv["rec"], iv["strand"] = orf["begin"][keep], olen[keep], orf["rec"][keep], orf["strand"][keep]
    d_iv, t_tab, t_info = up(iv), new(4 * 4096 * N), new(16 * N)
    lib = ctx.L
    res["train_s"], rc = best_of(ctx, repeat, lambda: lib.gs_gene_train_dev(ctx.h, C.byref(prm), d_seq, seq.nbytes, d_rs, d_rl, N, d_goff, N, d_iv, len(iv), t_tab, t_info))
    assert rc == 0
    s_j, s_s, s_f = new(8 * n_orf), new(8 * n_orf), new(4 * n_orf)
    res["score_s"], rc = best_of(ctx, repeat, lambda: lib.gs_gene_score_dev(ctx.h, C.byref(prm), d_seq, seq.nbytes, d_rs, d_rl, N, d_goff, N, d_tab, o_orf, o_al, n_orf, s_j, s_s, s_f))
    assert rc == 0
    res["train_intervals"] = len(iv)
    for p in ptrs:
        ctx.free(p)
    print("%d x %d bases: orf_translate %.2f ms (%d ORFs); gene_call %.2f ms (count only %.2f) = %.1f x; train %.2f ms (%d intervals), score %.2f ms; %d genes, %d of %d trained"
          % (N, L, res["orf_translate_s"] * 1e3, n_orf, res["call_s"] * 1e3, res["call_count_s"] * 1e3, res["call_over_orf"], res["train_s"] * 1e3, len(iv),
             res["score_s"] * 1e3, n_gene, res["trained"], N), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--len", type=int, default=5000000)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "gene_rate.log"))
    a = ap.parse_args()
    import gsearch_amd as G
    import gene_cases as GC
    ctx = G.default_context()
    for N in a.genomes:
        line = json.dumps(measure(G, GC, ctx, N, a.len, a.distinct, a.repeat))
        print(line)
        if a.log:
            os.makedirs(os.path.dirname(a.log), exist_ok=True)
            with open(a.log, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
