#!/usr/bin/env python3
"""Rate of hnswcore (gs_index_cluster, SPEC 10) at the bench's database: N synthetic 5 Mbp genomes from the generator bench.py builds its request
database with (gs_synth_dna_family_dev, seed 2024, one root per 100 genomes, mutation 0.001..0.08), sketched with OptDens k=21 s=18000 and
inserted into the HNSW of bench.py (M=128, efc=1600, scale 0.25) - the database of tools/knn_graph_rate.py.
Reports: the wall time of cluster(k, fraction); then, from a second run with GS_CLUSTER_VERBOSE=1, the library's own per-stage times (coreset
passes, building P, initial medoids, every k-medoid iteration, final dispatch) and the update kernel's bytes/s next to the measured HBM copy
rate; the cluster sizes; and a check of sampled nodes' centres against numpy (the centre of a node is its nearest medoid by (count, node)).
usage: cluster_rate.py [--db-genomes N] [--cluster K] [--fraction F] [--check-rows R]"""
import argparse, os, sys, time
import ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import gsearch_amd as G

HBM_COPY_TBS = 6.29        # MI355X_MICROARCH.md: float4 copy, 79 % of the 8.0 TB/s of the data sheet

ap = argparse.ArgumentParser()
ap.add_argument("--db-genomes", type=int, default=300000)
ap.add_argument("--cluster", type=int, default=5)
ap.add_argument("--fraction", type=float, default=0.1)
ap.add_argument("--check-rows", type=int, default=2000)
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

K, F = a.cluster, a.fraction
hn.nearest_of(np.arange(min(N, 64), dtype=np.uint64))          # warm-up: code objects, the column copy of the signatures, the count-matrix buffer
t0 = time.perf_counter()
res = hn.cluster(K, F, seed=seed, return_coreset=True)
wall = time.perf_counter() - t0
print("cluster(k=%d, fraction=%g) over %d nodes: wall %.3f s; coreset p = %d, %d iterations, converged %d, cost_core %d, cost_all %d (mean distance to the centre %.4f)"
      % (K, F, N, wall, res.n_core, res.iterations, res.converged, res.cost_core, res.cost_all, res.cost_all / N / m), flush=True)
print("count matrix of the whole database at the recorded 2.4 s per 300 000 x 300 000: the %d + %d rows of the two coreset passes would take %.3f s" %
      ((res.n_core + 1) // 2, res.n_core, 2.4 * (N / 300000.0) * (1.5 * res.n_core) / 300000.0), flush=True)
print("# stages as the library times them (GS_CLUSTER_VERBOSE=1, the stream drained at every stage); update kernel against the %.2f TB/s HBM copy rate:" % HBM_COPY_TBS, flush=True)
sys.stdout.flush()
os.environ["GS_CLUSTER_VERBOSE"] = "1"
t0 = time.perf_counter()
res2 = hn.cluster(K, F, seed=seed, return_coreset=True)
wall2 = time.perf_counter() - t0
del os.environ["GS_CLUSTER_VERBOSE"]
sys.stderr.flush()
same = all(np.array_equal(x, y) for x, y in zip(res, res2) if isinstance(x, np.ndarray)) and res.cost_all == res2.cost_all
print("second run: wall %.3f s, %s" % (wall2, "same answers" if same else "ANSWERS DIFFER"), flush=True)
print("cluster sizes: %s; medoids (node numbers): %s" % (res.sizes.tolist(), res.medoids.tolist()), flush=True)
print("coreset weights: min %d median %d max %d, %d of weight 0" % (res.core_weight.min(), int(np.median(res.core_weight)), res.core_weight.max(),
                                                                    int((res.core_weight == 0).sum())), flush=True)

# sampled nodes against numpy: the centre is the medoid of smallest (count, node number)
rng = np.random.default_rng(7)
rows = np.sort(rng.choice(N, min(a.check_rows, N), replace=False))
ok = 0
if K:
    med = hn.get_data(0, N)[res.medoids.astype(np.int64)] if N <= 20000 else np.stack([hn.get_data(int(x), 1)[0] for x in res.medoids])
    for r in rows:
        c = (med != hn.get_data(int(r), 1)[0]).sum(axis=1)
        t = int(c.argmin())
        ok += int(res.centre_node[r] == res.medoids[t] and res.centre_count[r] == c[t])
    print("numpy check: %d / %d sampled nodes at their nearest medoid with the right count" % (ok, len(rows)), flush=True)
print("RESULT ok" if same and (not K or ok == len(rows)) else "RESULT MISMATCH", flush=True)
