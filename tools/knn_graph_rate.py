#!/usr/bin/env python3
"""Rate of the database's own exact k-NN graph (gs_index_knn_graph, hnsw2knn) at the bench's database: N synthetic 5 Mbp genomes from the
generator bench.py builds its request database with (gs_synth_dna_family_dev, seed 2024, one root per 100 genomes, mutation 0.001..0.08),
sketched with OptDens k=21 s=18000 and inserted into the HNSW of bench.py (M=128, efc=1600, scale 0.25).
Reports: wall time of knn_graph(knbn) over all rows, its count-matrix / select split (context profile: FAM_HAMMING = the count producers,
FAM_SEARCH = the select, in a second run), the select's bytes / time against 8 TB/s, a check of sampled rows against the CPU oracle, and the
recall of the approximate answer (parallel_search of sampled rows at ef = 5000, the row's own node removed).
usage: knn_graph_rate.py [--db-genomes N] [--knbn K] [--check-rows R] [--recall-rows Q] [--no-check]"""
import argparse, os, sys, time
import ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsearch_amd as G
from bench import HBM_PEAK_GBS

ap = argparse.ArgumentParser()
ap.add_argument("--db-genomes", type=int, default=300000)
ap.add_argument("--knbn", type=int, default=32)
ap.add_argument("--check-rows", type=int, default=512)
ap.add_argument("--recall-rows", type=int, default=10000)
ap.add_argument("--no-check", action="store_true", help="skip the oracle check and the recall (profiling runs)")
a = ap.parse_args()

N, L, k, m, seed, per_root = a.db_genomes, 5_000_000, 21, 18000, 2024, 100
ctx = G.Context(0)
lib, chk = ctx.L, G._lib.check
prm = G.SeqSketcherParams(k, m, "optdens")
hn = G.Hnsw.new(128, 1_500_000, 16, 1600, G.DistHamming(ctx), dtype=np.float32, seed=seed, insert_batch=256, ctx=ctx)
hn.modify_level_scale(0.25); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
hn._ensure(m)
words = (L + 31) // 32
gbytes = words * 8
chunk = min(8192, N)
d_seq, d_sig = ctx.alloc(chunk * gbytes + 64), ctx.alloc(chunk * m * 4)
rs = np.arange(chunk, dtype=np.uint64) * np.uint64(words * 32)
d_rs, d_rl, d_goff = ctx.alloc(rs.nbytes), ctx.alloc(rs.nbytes), ctx.alloc(8 * (chunk + 1))
ctx.upload(d_rs, rs); ctx.upload(d_rl, np.full(chunk, L, np.uint64)); ctx.upload(d_goff, np.arange(chunk + 1, dtype=np.uint64))
t0 = time.perf_counter()
for g0 in range(0, N, chunk):
    n = min(chunk, N - g0)
    chk(lib.gs_synth_dna_family_dev(ctx.h, seed, g0, n, L, max(N // per_root, 1), 0.001, 0.08, d_seq))
    chk(lib.gs_sketch_batch_dev(ctx.h, C.byref(prm.c), d_seq, n * gbytes + 64, d_rs, d_rl, n, d_goff, n, d_sig))
    chk(lib.gs_index_parallel_insert_dev(hn.h, d_sig, n))
ctx.sync()
for p in (d_seq, d_sig, d_rs, d_rl, d_goff):
    ctx.free(p)
chk(lib.gs_index_release_build_scratch(hn.h))
print("# database: %d genomes x %.1f Mbp, k=%d s=%d, HNSW M=128 efc=1600 built in %.1f s" % (N, L / 1e6, k, m, time.perf_counter() - t0), flush=True)

K = a.knbn
hn.knn_graph(K, 1.0, 0, min(N, 4096))              # warm-up: code objects, the count-matrix buffer
t0 = time.perf_counter()
ids, dist, cnt = hn.knn_graph(K)
wall = time.perf_counter() - t0
print("knn_graph(%d) over %d rows: wall %.3f s (%.0f rows/s), host answers included" % (K, N, wall, N / wall), flush=True)
ctx.profile(True)
ctx.profile_read(1); ctx.profile_read(2)
t0 = time.perf_counter()
ids2, dist2, cnt2 = hn.knn_graph(K)
wall_p = time.perf_counter() - t0
cm_ms, cm_n = ctx.profile_read(1)
sel_ms, sel_n = ctx.profile_read(2)
ctx.profile(False)
assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2) and np.array_equal(cnt, cnt2), "two runs differ"
ld = (N + 7) // 8 * 8
sel_bytes = 3.0 * 2.0 * ld * N                       # upper bound: three passes over each count row (pass 3 may stop early)
print("profiled run: wall %.3f s; count matrix %.1f ms (%d launches), select %.1f ms (%d launches) = %.1f %% of the two" %
      (wall_p, cm_ms, cm_n, sel_ms, sel_n, 100.0 * sel_ms / max(cm_ms + sel_ms, 1e-9)), flush=True)
print("select: <= %.1f GB read (3 passes x %d rows x %.2f MB) in %.1f ms = %.2f TB/s, %.1f %% of %.1f TB/s" %
      (sel_bytes / 1e9, N, 2.0 * ld / 1e6, sel_ms, sel_bytes / (sel_ms * 1e-3) / 1e12, 100.0 * sel_bytes / (sel_ms * 1e-3) / (HBM_PEAK_GBS * 1e9), HBM_PEAK_GBS / 1e3), flush=True)
print("neighbours per row: min %d max %d; distance of the %d-th neighbour: median %.4f" % (cnt.min(), cnt.max(), K, float(np.median(dist[:, K - 1]))), flush=True)
if a.no_check:
    sys.exit(0)

import oracle_lib as O
db = hn.get_data()
rng = np.random.default_rng(7)
rows = np.sort(rng.choice(N, min(a.check_rows, N), replace=False))
t0 = time.perf_counter()
oi, od = O.bruteforce_topk(db, db[rows], K + 1, os.cpu_count() or 16)
ok = 0
for i, r in enumerate(rows):
    keep = oi[i] != np.uint64(r)
    if keep.all():
        keep[-1] = False
    ok += int(np.array_equal(ids[r], oi[i][keep]) and np.array_equal(dist[r], od[i][keep]))
print("oracle check: %d / %d sampled rows bit-identical (CPU brute force %.1f s)" % (ok, len(rows), time.perf_counter() - t0), flush=True)

qrows = np.sort(rng.choice(N, min(a.recall_rows, N), replace=False))
t0 = time.perf_counter()
ai, ad, ac, _ = hn.search_arrays(db[qrows], K + 1, 5000)
t_s = time.perf_counter() - t0
rec, exact_lists = 0.0, 0
for i, r in enumerate(qrows):
    sel = ai[i][:ac[i]] != np.uint64(r)
    got_d = ad[i][:ac[i]][sel][:K]
    kth = dist[r, K - 1]
    # tie-aware recall@K: approximate neighbours no farther than the exact K-th one, at most K
    rec += min(int((got_d <= kth).sum()), K) / K
    exact_lists += int(np.array_equal(ai[i][:ac[i]][sel][:K], ids[r]))
print("approximate answer (parallel_search ef=5000 of %d rows, self removed, %.2f s): recall@%d %.4f, identical lists %.4f" %
      (len(qrows), t_s, K, rec / len(qrows), exact_lists / len(qrows)), flush=True)
print("RESULT ok" if ok == len(rows) else "RESULT MISMATCH", flush=True)
