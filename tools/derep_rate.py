#!/usr/bin/env python3
"""Rate of derep (gs_index_components / gs_index_derep, SPEC 18) at the bench's database: N synthetic 5 Mbp genomes from the generator bench.py
builds its request database with (gs_synth_dna_family_dev, seed 2024, one root per 100 genomes, mutation 0.001..0.08; --skew-alpha A: the skewed
form of bench.py's `request_skewed` leg, gs_synth_dna_family_skew_dev, power-law family sizes), sketched with OptDens k=21 s=18000 and inserted
into the HNSW of bench.py - the database of tools/knn_graph_rate.py and tools/cluster_rate.py.
Reports, per entry point: the wall time of the whole call; from a second, profiled run the count-matrix time inside it (context profile family
1 = the count producers) and the time of the gs_derep.hip kernels (family 2), with their share; the clusters found against the planted families;
that two runs give the same words. The yardstick is Hnsw.knn_graph(32) on the same index in the same session (same producer; family 2 = its
select). A library built with -DGS_DEREP_STATS prints the successful and failed CASes of k_derep_union on stderr.
usage: derep_rate.py [--db-genomes N] [--max-dist D] [--skew-alpha A] [--check-rows R]"""
import argparse, os, sys, time
import ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import gsearch_amd as G

ap = argparse.ArgumentParser()
ap.add_argument("--db-genomes", type=int, default=300000)
ap.add_argument("--max-dist", type=float, default=0.99, help="the cut: unrelated genomes are at 1.0, the members of a planted family below it")
ap.add_argument("--skew-alpha", type=float, default=0.0)
ap.add_argument("--check-rows", type=int, default=64)
a = ap.parse_args()

N, L, k, m, seed, per_root = a.db_genomes, 5_000_000, 21, 18000, 2024, 100
n_roots = max(N // per_root, 1)
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
    if a.skew_alpha > 0:
        chk(lib.gs_synth_dna_family_skew_dev(ctx.h, seed + 1, g0, n, L, n_roots, 0.001, 0.08, a.skew_alpha, d_seq))
    else:
        chk(lib.gs_synth_dna_family_dev(ctx.h, seed, g0, n, L, n_roots, 0.001, 0.08, d_seq))
    chk(lib.gs_sketch_batch_dev(ctx.h, C.byref(prm.c), d_seq, n * gbytes + 64, d_rs, d_rl, n, d_goff, n, d_sig))
    chk(lib.gs_index_parallel_insert_dev(hn.h, d_sig, n))
ctx.sync()
for p in (d_seq, d_sig, d_rs, d_rl, d_goff):
    ctx.free(p)
chk(lib.gs_index_release_build_scratch(hn.h))
print("# database: %d genomes x %.1f Mbp in %d families%s, k=%d s=%d, HNSW M=128 efc=1600 built in %.1f s" % (
    N, L / 1e6, n_roots, " of power-law sizes (alpha %.1f)" % a.skew_alpha if a.skew_alpha > 0 else "", k, m, time.perf_counter() - t0), flush=True)

D = a.max_dist
hn.nearest_of(np.arange(min(N, 64), dtype=np.uint64))          # warm-up: code objects, the column copy of the signatures, the count-matrix buffer


def timed(label, call, words):
    t0 = time.perf_counter()
    r1 = call()
    wall = time.perf_counter() - t0
    ctx.profile(True)
    ctx.profile_read(1); ctx.profile_read(2)
    t0 = time.perf_counter()
    r2 = call()
    wall2 = time.perf_counter() - t0
    cm_ms, cm_n = ctx.profile_read(1)
    k_ms, k_n = ctx.profile_read(2)
    ctx.profile(False)
    same = all(np.array_equal(x, y) for x, y in zip(words(r1), words(r2)))
    print("%s: wall %.3f s; profiled run: wall %.3f s, count matrix %.1f ms (%d launches), the other kernels %.1f ms (%d scopes) = %.1f %% of the two; %s"
          % (label, wall, wall2, cm_ms, cm_n, k_ms, k_n, 100 * k_ms / max(cm_ms + k_ms, 1e-9), "same words twice" if same else "WORDS DIFFER"), flush=True)
    return r1, wall, cm_ms, k_ms, same


ok = True
comp, w_c, cm_c, k_c, s = timed("components(%g)" % D, lambda: hn.components(D), lambda r: (r.label_node,))
ok &= s
print("  c_max %d: %d components, %d singletons, largest %d (planted: %d families)" % (comp.c_max, comp.n_clusters, comp.n_singletons, comp.largest, n_roots), flush=True)
der, w_d, cm_d, k_d, s = timed("derep(%g)" % D, lambda: hn.derep(D), lambda r: (r.rep_node, r.rep_count))
ok &= s
print("  %d representatives, %d singletons, largest cluster %d; mean distance to the representative %.4f" % (
    der.n_clusters, der.n_singletons, der.largest, float(der.rep_count.astype(np.float64).mean()) / m), flush=True)
g, w_g, cm_g, k_g, s = timed("knn_graph(32)", lambda: hn.knn_graph(32), lambda r: r)
ok &= s
print("ratios to knn_graph(32): components %.2f, derep %.2f of its wall time; clustering share %.1f %% and %.1f %% against the select's %.1f %%" % (
    w_c / w_g, w_d / w_g, 100 * k_c / (cm_c + k_c), 100 * k_d / (cm_d + k_d), 100 * k_g / (cm_g + k_g)), flush=True)

# sampled nodes against the index's own count matrix: a representative has no linked representative; a member is linked to its representative at
# the stated count and to no representative of earlier rank that is nearer; a label's row links only nodes of its component
rng = np.random.default_rng(7)
rows = np.sort(rng.choice(N, min(a.check_rows, N), replace=False))
is_rep = der.rep_node == np.arange(N, dtype=np.uint64)
bad = 0
for v in rows.tolist():
    c = hn.count_matrix(hn.get_data(v, 1))[0].astype(np.int64)
    link = c <= der.c_max
    link[v] = False
    bad += int((comp.label_node[link] != comp.label_node[v]).any())
    earlier = link & is_rep & (np.arange(N) < v)             # (no priorities: rank = node number)
    if is_rep[v]:
        bad += int(earlier.any())
    else:
        cand = np.nonzero(earlier)[0]
        best = cand[np.lexsort((cand, c[cand]))[0]] if len(cand) else -1
        bad += int(best != der.rep_node[v] or c[best] != der.rep_count[v])
print("count-matrix check: %d sampled nodes, %d violations" % (len(rows), bad), flush=True)
print("RESULT ok" if ok and bad == 0 else "RESULT MISMATCH", flush=True)
