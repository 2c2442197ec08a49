#!/usr/bin/env python3
"""Rate of ann (SPEC.md 8) at the bench's database: N synthetic 5 Mbp genomes from the generator of tools/knn_graph_rate.py (seed 2024, one root
per 100 genomes, mutation 0.001..0.08), sketched with OptDens k=21 s=18000 and inserted into the HNSW of bench.py.
Reports: knn_graph(8) wall time; on that device graph, the calibration + adjacency time (epochs = 0) and the per-epoch time (E epochs minus
that, over E) with the gathers per second and the bytes an epoch moves; the total Hnsw.embed wall time; the k-NN graph statistics; the family
purity of the 10 nearest 2-D neighbours of sampled points (families = connected components of the graph's edges at distance < 0.99);
--quality [KQ]: after the embedding, its quality by neighbourhood conservation (SPEC.md 8.1) on the graph above, timed per pass on the device;
--check: the whole embedding against tests/pyref_embed.py (slow: numpy).
usage: embed_rate.py [--db-genomes N] [--epochs E] [--sample S] [--quality [KQ]] [--check]"""
import argparse, os, sys, time
import ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsearch_amd as G

ap = argparse.ArgumentParser()
ap.add_argument("--db-genomes", type=int, default=300000)
ap.add_argument("--epochs", type=int, default=None)
ap.add_argument("--sample", type=int, default=3000)
ap.add_argument("--check", action="store_true")
ap.add_argument("--skip-purity", action="store_true")
ap.add_argument("--quality", type=int, nargs="?", const=200, default=None, metavar="KQ")
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

K = 8
ep = G.EmbedParams() if a.epochs is None else G.EmbedParams(epochs=a.epochs)
E, S, D = ep.epochs, ep.neg_samples, ep.dim
hn.knn_graph(K, 1.0, 0, min(N, 4096))                  # warm-up
t0 = time.perf_counter()
ids, dist, cnt = hn.knn_graph(K)
t_graph = time.perf_counter() - t0
print("knn_graph(%d) over %d rows: wall %.3f s" % (K, N, t_graph), flush=True)

# the embedding alone, on the device graph (the bench's index has no caller ids: knn_graph_dev answers node numbers)
di, dd, dc, dp = ctx.alloc(8 * N * K), ctx.alloc(4 * N * K), ctx.alloc(4 * N), ctx.alloc(4 * N * D)
hn.knn_graph_dev(K, 0, N, di, dd, dc)
ctx.sync()
zero = G.EmbedParams(epochs=0)
G.embed_knn_graph_dev(ctx, N, K, di, dd, dc, dp, zero)       # warm-up (pools, code objects)
t0 = time.perf_counter()
G.embed_knn_graph_dev(ctx, N, K, di, dd, dc, dp, zero)
t_setup = time.perf_counter() - t0
t0 = time.perf_counter()
G.embed_knn_graph_dev(ctx, N, K, di, dd, dc, dp, ep)
t_full = time.perf_counter() - t0
xy_dev = ctx.download(dp, (N, D), np.float32)
for p in (di, dd, dc, dp):
    ctx.free(p)
per_epoch = (t_full - t_setup) / max(E, 1)
# adjacency length: every kept entry once from its row, plus each entry whose reverse is not kept once more (the reverse-only side)
slot = np.arange(K)[None, :] < cnt[:, None].astype(np.int64)
src = np.repeat(np.arange(N, dtype=np.int64), K).reshape(N, K)[slot]
dst = ids[slot].astype(np.int64)
fwd = np.sort(src * N + dst)
rk = dst * N + src
pos = np.minimum(np.searchsorted(fwd, rk), len(fwd) - 1)
rev_only = int((fwd[pos] != rk).sum())
adj = len(src) + rev_only
deg = np.bincount(src, minlength=N) + np.bincount(dst[fwd[pos] != rk], minlength=N)
gathers = adj + N * S
bytes_epoch = adj * (4 + 4 + 4 * D) + N * S * 4 * D + N * (16 + 4 + 4 * D + 4 * D)
print("calibration + adjacency + initial positions: %.1f ms (epochs = 0)" % (1e3 * t_setup), flush=True)
print("epochs: E = %d, S = %d, dim %d: %.1f ms in all, %.3f ms per epoch; adjacency %d entries (%d reverse-only), max degree %d, nodes above L_H: %d"
      % (E, S, D, 1e3 * (t_full - t_setup), 1e3 * per_epoch, adj, rev_only, deg.max(), int((deg > 64).sum())), flush=True)
print("per epoch: %d gathers (%.2e gathers/s), ~%.1f MB moved (%.2f TB/s effective), positions %.1f MB" %
      (gathers, gathers / per_epoch, bytes_epoch / 1e6, bytes_epoch / per_epoch / 1e12, 4.0 * N * D / 1e6), flush=True)
t0 = time.perf_counter()
xy = hn.embed(K, ep)
t_embed = time.perf_counter() - t0
print("Hnsw.embed(%d) wall %.3f s (graph + calibration + adjacency + %d epochs + copies); equals the device-graph form: %s"
      % (K, t_embed, E, np.array_equal(xy.view(np.uint32), xy_dev.view(np.uint32))), flush=True)
st = hn.knn_graph_stats(K)
print("stats: n_edges %d, occ mean %.3f std %.3f hubness %.3f max %d, q_first %s, q_last %s" % (st["n_edges"], st["occ_mean"], st["occ_std"], st["occ_skew"],
      st["max_occ"], np.round(st["q_first"], 4).tolist(), np.round(st["q_last"], 4).tolist()), flush=True)

if a.quality is not None:
    G.embed_quality(ids, dist, cnt, xy, 1, ctx=ctx)                 # warm-up (pools, code objects)
    t0 = time.perf_counter()
    q = G.embed_quality(ids, dist, cnt, xy, a.quality, ctx=ctx)
    t_q = time.perf_counter() - t0
    ms = G.embed_quality_last_ms(ctx)
    dev_ms = ms["edge"] + ms["rank"] + sum(ms["radius"]) + ms["finish"]
    print("quality (kq %d) of the embedding, %d x %d pairs per pass: edge pass %.3f ms, rank pass %.1f ms, rank finish %.3f ms, radius %.1f ms in %d passes (%s), "
          "summary on the host %.1f ms; device %.1f ms, wall %.3f s with the copies = %.3f x knn_graph(%d), %.1f x the %d epochs"
          % (q["kq_eff"], N, N, ms["edge"], ms["rank"], ms["finish"], sum(ms["radius"]), len(ms["radius"]), " ".join("%.1f" % t for t in ms["radius"]),
             ms["summary"], dev_ms, t_q, t_q / t_graph, K, t_q / max(t_full - t_setup, 1e-9), E), flush=True)
    print("quality: frac_conserved %.6g, n_nomatch %d of %d rows, mean conserved per matched row %.6g, hist %s" %
          (q["frac_conserved"], q["n_nomatch"], q["n_rows"], q["mean_conserved"], q["hist_conserved"].tolist()), flush=True)
    sys.stdout.write(G.embed_quality_text(q))
    sys.stdout.flush()

if not a.skip_purity:
    par = np.arange(N)

    def find(x):
        r = x
        while par[r] != r:
            r = par[r]
        while par[x] != r:
            par[x], x = r, par[x]
        return r
    close = dist[slot] < 0.99
    for s_, d_ in zip(src[close], dst[close]):
        ra, rb = find(s_), find(d_)
        if ra != rb:
            par[ra] = rb
    fam = np.array([find(i) for i in range(N)])
    rng = np.random.default_rng(3)
    smp = rng.choice(N, min(a.sample, N), replace=False)
    xyd = xy.astype(np.float64)
    pur = 0.0
    for i in smp:
        d2 = ((xyd - xyd[i]) ** 2).sum(1)
        d2[i] = np.inf
        nn = np.argpartition(d2, 10)[:10]
        pur += (fam[nn] == fam[i]).mean()
    print("family purity of the 10 nearest 2-D neighbours, %d sampled points: %.4f (%d families)" % (len(smp), pur / len(smp), len(np.unique(fam))), flush=True)

if a.check:
    import pyref_embed as R
    t0 = time.perf_counter()
    ref = R.embed(ids, dist, cnt, R.defaults(epochs=E))
    ok = np.array_equal(ref.view(np.uint32), xy.view(np.uint32))
    print("reference check (%.0f s): %s" % (time.perf_counter() - t0, "bit-identical" if ok else "MISMATCH"), flush=True)
    print("RESULT ok" if ok else "RESULT MISMATCH", flush=True)
