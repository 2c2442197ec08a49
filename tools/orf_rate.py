#!/usr/bin/env python3
"""Rates of the orfs stage on the device (SPEC 14, DESIGN 3.20, gs_orf.hip).

  translate   `genomes` synthetic genomes of `len` bases generated in HBM (gs_synth_dna_dev, the bench's generator), one record each:
              gs_orf_translate_dev timed by events on the context's stream, a warm-up and then the best of `repeat` runs - the whole call (count
              passes, the read-back of the counts, emit) and the count-only form, so that the difference is the emit pass. bases/s, ORFs and residues out.
  check       the first `check_bases` bases of genome 0 as a record of their own against the restatement (tests/pyref_orf.py): every array `==`
  universal   `search_genomes` of the same genomes written as FASTA files, then universal_genes(translate=True) against 120 synthetic profiles with the
              node counts of the bacterial universal-gene set (tests/golden/hmm/bacteria_node_counts.txt): the wall time of the call, and beside it
              the stages of the same work run one after the other - reading, split + pack + upload + translation + descriptors back, the Viterbi
              search of the ORFs (the yardstick of the translation), best hits.
  --prefilter also the same call with prefilter="msv" (SPEC 13.3): its wall time, the seconds of the filtered search of the ORFs (MSV,
              selection, Viterbi over the selected lists) beside the Viterbi stage, and whether the hits are the same.

  --vit16     also the same call with prefilter="vit16" and "msv+vit16" (SPEC 13.7; vf_floor = the GA cutoffs): wall times, the seconds of
              the staged search of the ORFs beside the Viterbi stage, the share of the pairs that go on to int32 Viterbi, and whether the hits are the same

usage: orf_rate.py [--genomes 64] [--len 5000000] [--search-genomes 64] [--repeat 3] [--min-aa 30] [--prefilter] [--vit16] [--log profiles/orf_rate.log]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ascii_of(packed, n):
    b = np.frombuffer(packed, np.uint8)
    codes = ((b[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).reshape(-1)[:n]
    return np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--len", type=int, default=5000000)
    ap.add_argument("--search-genomes", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--min-aa", type=int, default=30)
    ap.add_argument("--check-bases", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=14)
    ap.add_argument("--prefilter", action="store_true")
    ap.add_argument("--vit16", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "orf_rate.log"))
    a = ap.parse_args()
    import gsearch_amd as G
    from gsearch_amd import api as A
    import pyref_hmm as R
    import pyref_orf as P
    ctx = G.default_context()
    lib = ctx.L
    N, L = a.genomes, a.len
    words = (L + 31) // 32
    res = {"genomes": N, "len": L, "bases": N * L, "min_aa": a.min_aa, "tile": G.ORF_TILE}

    # ---- translate ------------------------------------------------------------------------------------------------------------------------
    seq_bytes = N * words * 8
    d_seq = ctx.alloc(seq_bytes + 64)
    G._lib.check(lib.gs_synth_dna_dev(ctx.h, a.seed, 0, N, L, d_seq))
    rs = np.arange(N, dtype=np.uint64) * np.uint64(words * 32)
    rl = np.full(N, L, np.uint64)
    d_rs, d_rl = ctx.alloc(rs.nbytes), ctx.alloc(rl.nbytes)
    ctx.upload(d_rs, rs); ctx.upload(d_rl, rl)
    max_aa = G._lib.HMM_MAX_L
    n_orf, n_aa, n_long = G.orf_translate_dev(ctx, d_seq, seq_bytes, d_rs, d_rl, N, min_aa=a.min_aa, max_aa=max_aa)          # count only; also the warm-up
    outs = [ctx.alloc(max(n, 16)) for n in (16 * n_orf, n_aa, 8 * n_orf, 8 * n_orf, 8 * (N + 1))]
    best = {"count": float("inf"), "full": float("inf")}
    for run in range(a.repeat + 1):
        for name, args in (("count", (0, 0, None, None, None, None, None)), ("full", (n_orf, n_aa) + tuple(outs))):
            ctx.sync()
            ctx.timer_start()
            G.orf_translate_dev(ctx, d_seq, seq_bytes, d_rs, d_rl, N, *args, min_aa=a.min_aa, max_aa=max_aa)
            ms = ctx.timer_stop()
            if run:
                best[name] = min(best[name], ms * 1e-3)
    res.update(orfs=n_orf, residues=n_aa, long_dropped=n_long, translate_s=best["full"], count_passes_s=best["count"], emit_s=best["full"] - best["count"],
               bases_per_s=N * L / best["full"], residues_per_s=n_aa / best["full"])
    print("translate: %d x %d bases -> %d ORFs, %d residues in %.2f ms (count passes %.2f, emit %.2f): %.3g bases/s" %
          (N, L, n_orf, n_aa, best["full"] * 1e3, best["count"] * 1e3, (best["full"] - best["count"]) * 1e3, res["bases_per_s"]), flush=True)

    # ---- check ----------------------------------------------------------------------------------------------------------------------------
    cb = min(a.check_bases, L)
    head = ctx.download(d_seq, ((cb + 3) // 4 + 8,), np.uint8)
    got = G.orf_translate_packed(head, [0], [cb], min_aa=a.min_aa, max_aa=max_aa, ctx=ctx)
    want = P.translate_records([P.codes(ascii_of(head.tobytes(), cb))], min_aa=a.min_aa, max_aa=max_aa)
    res["check_bases"] = cb
    res["check_equal"] = bool(all(np.array_equal(got[k], want[k]) for k in ("orf", "aa", "aa_start", "aa_len", "rec_orf_off")) and got["n_long"] == want["n_long"])
    print("check: %d bases of genome 0, %d ORFs against the restatement: %s" % (cb, len(want["orf"]), "equal" if res["check_equal"] else "MISMATCH"), flush=True)

    # ---- universal genes ------------------------------------------------------------------------------------------------------------------
    K = min(a.search_genomes, N)
    if K > 0:
        rng = np.random.default_rng(a.seed)
        nodes = [int(x) for x in open(os.path.join(ROOT, "tests", "golden", "hmm", "bacteria_node_counts.txt")).read().split()]
        texts = [R.write_hmm(R.synth_model(rng, M, name="SYN%03d_%d" % (i, M))) for i, M in enumerate(nodes)]
        db = G.HmmDb(texts, ctx, texts=True)
        with tempfile.TemporaryDirectory() as tmp:
            files = []
            for g in range(K):
                packed = ctx.download(d_seq + g * words * 8, (words * 8,), np.uint8)
                files.append(os.path.join(tmp, "g%03d.fna" % g))
                with open(files[-1], "wb") as f:
                    f.write(b">g%03d\n" % g + ascii_of(packed.tobytes(), L) + b"\n")
            for p in outs:
                ctx.free(p)
            outs = []
            t = time.perf_counter()
            genomes, local, where = G.universal_genes(files, db, ctx=ctx, translate=True, min_aa=a.min_aa)
            ctx.sync()
            res["universal_genes_s"] = time.perf_counter() - t
            res["search_genomes"] = K
            res["hits"] = int((local != R.NO_HIT).sum())
            # the stages of the same work, one after the other
            t = time.perf_counter()
            contigs = [A._fna_contigs(p) for p in files]
            res["read_s"] = time.perf_counter() - t
            t = time.perf_counter()
            dev = A._DevOrfs(ctx, contigs, a.min_aa, A._orf_max_aa(False, False), 11)
            ctx.sync()
            res["split_pack_translate_s"] = time.perf_counter() - t
            t = time.perf_counter()
            d_score = dev.search_dev(db, False, None)
            ctx.sync()
            res["viterbi_s"] = time.perf_counter() - t
            res["search_orfs"], res["search_residues"] = int(dev.n), int(dev.aa_len.sum())
            res["cells"] = res["search_residues"] * sum(nodes)
            res["cells_per_s"] = res["cells"] / res["viterbi_s"]
            res["translate_share_of_viterbi"] = (best["full"] * K / N) / res["viterbi_s"]
            d_goff, d_thr = dev.mem.up(dev.genome_orf_off), dev.mem.up(db.thresholds("ga"))
            d_rec, d_sc = dev.mem.new(4 * K * len(db)), dev.mem.new(4 * K * len(db))
            t = time.perf_counter()
            db.best_hits_dev(d_score, dev.n, d_goff, K, d_thr, d_rec, d_sc)
            ctx.sync()
            res["best_hits_s"] = time.perf_counter() - t
            if a.prefilter:
                dev.search_dev(db, False, None, True, 0.02)                  # the warm-up of the MSV and selected-Viterbi kernels
                ctx.sync()
                t = time.perf_counter()
                d_fscore = dev.search_dev(db, False, None, True, 0.02)
                ctx.sync()
                res["filtered_search_s"] = time.perf_counter() - t
                res["filtered_over_viterbi"] = res["filtered_search_s"] / res["viterbi_s"]
                fsc = ctx.download(d_fscore, (dev.n, len(db)), np.int32)
                res["pairs_through_the_filter"] = float((fsc != R.NO_SCORE).mean())
                t = time.perf_counter()
                _, flocal, _ = G.universal_genes(files, db, ctx=ctx, translate=True, min_aa=a.min_aa, prefilter="msv")
                ctx.sync()
                res["universal_genes_prefilter_s"] = time.perf_counter() - t
                res["prefilter_hits"], res["prefilter_same_hits"] = int((flocal != R.NO_HIT).sum()), bool(np.array_equal(flocal, local))
                print("prefilter=msv: filtered search %.2f s (%.3f of the Viterbi stage, %.4f of the pairs go on), universal_genes %.2f s, same hits: %s" %
                      (res["filtered_search_s"], res["filtered_over_viterbi"], res["pairs_through_the_filter"], res["universal_genes_prefilter_s"],
                       res["prefilter_same_hits"]), flush=True)
            if a.vit16:
                vfl = db.vf_floor(False, None, "ga")
                for label, pre, msv in (("vit16", "vit16", False), ("msv_vit16", "msv+vit16", True)):
                    dev.mem.free(dev.search_dev(db, False, None, msv, 0.02, vfl))           # the warm-up of the int16 kernels
                    ctx.sync()
                    t = time.perf_counter()
                    d_fscore = dev.search_dev(db, False, None, msv, 0.02, vfl)
                    ctx.sync()
                    res[label + "_search_s"] = time.perf_counter() - t
                    res[label + "_over_viterbi"] = res[label + "_search_s"] / res["viterbi_s"]
                    res[label + "_pairs_to_viterbi"] = float((ctx.download(d_fscore, (dev.n, len(db)), np.int32) != R.NO_SCORE).mean())
                    dev.mem.free(d_fscore)
                    t = time.perf_counter()
                    _, flocal, _ = G.universal_genes(files, db, ctx=ctx, translate=True, min_aa=a.min_aa, prefilter=pre)
                    ctx.sync()
                    res["universal_genes_%s_s" % label] = time.perf_counter() - t
                    res[label + "_same_hits"] = bool(np.array_equal(flocal, local))
                    print("prefilter=%s: staged search %.2f s (%.3f of the Viterbi stage, %.5f of the pairs go on to Viterbi), universal_genes %.2f s, same hits: %s" %
                          (pre, res[label + "_search_s"], res[label + "_over_viterbi"], res[label + "_pairs_to_viterbi"], res["universal_genes_%s_s" % label],
                           res[label + "_same_hits"]), flush=True)
            dev.close()
        db.close()
        print("universal_genes(translate=True): %d genomes, %d ORFs, %d residues: %.2f s in all; read %.2f s, split + pack + translate %.2f s, Viterbi %.2f s "
              "(%.3g cells/s), best hits %.4f s; the translation kernels are %.4f of the Viterbi stage" %
              (K, res["search_orfs"], res["search_residues"], res["universal_genes_s"], res["read_s"], res["split_pack_translate_s"], res["viterbi_s"], res["cells_per_s"],
               res["best_hits_s"], res["translate_share_of_viterbi"]), flush=True)
    for p in [d_seq, d_rs, d_rl] + outs:
        ctx.free(p)
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
