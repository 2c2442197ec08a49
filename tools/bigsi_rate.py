#!/usr/bin/env python3
"""Rates of bigsig on the device (SPEC 11, gs_bigsi.hip): an index of synthetic genomes generated in HBM (gs_synth_dna_dev, the bench's generator), then the
identification of reads cut from them (and of reads from genomes that are not in the index), all through the device forms.
Reports genomes/s and bit-sets/s of the build; reads/s, row look-ups/s and gathered bytes/s of the query next to a device-to-device copy rate taken in
the same run; the classify time; and checks a sample of reads and one column against the numpy restatement (tests/pyref_bigsi.py).
--minimizer M adds, after the plain legs and in the same run, the same build and query on a minimizer index of window K and minimizer length M (SPEC 11.1),
with the share of the query time spent in k_bigsi_minimizers; --min-count F adds the build of a few colours under the coverage filter with its split into
emit / sort / fill (on the plain index, and on the minimizer index when --minimizer is given). The splits come from the event timers of gs_ctx_profile.
--ties runs the same reads through the query with ties (SPEC 11.2) next to the plain query, in the same run: on the index above, where no tie is planted, and
on a second index in which colour c holds genome c // 8, so that every read is tied 8 ways; with --minimizer also on the minimizer index.
usage: bigsi_rate.py [--genomes N] [--mbp L] [--log2-rows R] [--hashes H] [--k K] [--reads Q] [--down-sample D] [--minimizer M] [--min-count F] [--ties]
                     [--max-ties T]"""
import argparse, os, sys, time
import ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsearch_amd as G
import pyref_bigsi as PR
import pyref_bigsi_mini as PM

ap = argparse.ArgumentParser()
ap.add_argument("--genomes", type=int, default=4096)
ap.add_argument("--mbp", type=float, default=5.0)
ap.add_argument("--log2-rows", type=int, default=26)
ap.add_argument("--hashes", type=int, default=3)
ap.add_argument("--k", type=int, default=31)
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--down-sample", type=int, default=1)
ap.add_argument("--chunk", type=int, default=512)
ap.add_argument("--minimizer", type=int, default=0)
ap.add_argument("--min-count", type=int, default=0)
ap.add_argument("--filter-colours", type=int, default=4)
ap.add_argument("--ties", action="store_true")
ap.add_argument("--max-ties", type=int, default=16)
a = ap.parse_args()

ctx = G.Context(0)
lib, chk = ctx.L, G._lib.check
N, L, B, h, k = a.genomes, int(a.mbp * 1e6), 1 << a.log2_rows, a.hashes, a.k
words = (L + 31) // 32
chunk = min(a.chunk, N)
seed = 1
print("# %s; index: %d genomes x %.1f Mbp, bloom_size 2^%d, num_hash %d, k %d: matrix %.2f GB" % (ctx.device_info()["name"], N, L / 1e6, a.log2_rows, h, k,
                                                                                               B * ((N + 63) // 64) * 8 / 1e9), flush=True)


def ascii_of(packed, n):
    codes = np.stack([(packed >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[:n]
    return bytes(np.frombuffer(b"ACGT", np.uint8)[codes])


# ---- device copy rate of this run ---------------------------------------------------------------------------------------------------------------
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
nb = 2 << 30
d_a, d_b = ctx.alloc(nb), ctx.alloc(nb)
ctx.memset(d_a, 1, nb); ctx.memset(d_b, 2, nb); ctx.sync()
best = 1e9
for _ in range(4):
    t0 = time.perf_counter()
    assert hip.hipMemcpy(d_b, d_a, nb, 3) == 0          # hipMemcpyDeviceToDevice
    ctx.sync()
    best = min(best, time.perf_counter() - t0)
copy_rate = 2 * nb / best
print("device copy: %.2f GB in %.2f ms: %.2f TB/s (bytes read + written)" % (nb / 1e9, best * 1e3, copy_rate / 1e12), flush=True)
ctx.free(d_a); ctx.free(d_b)

# ---- build ------------------------------------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
bx = G.Bigsi(k, h, B, N, ctx=ctx)
print("create (allocate + zero the matrix): %.3f s" % (time.perf_counter() - t0), flush=True)
d_seq = ctx.alloc(chunk * words * 8 + 64)
rs = np.arange(chunk, dtype=np.uint64) * np.uint64(words * 32)
d_rs, d_rl, d_go = ctx.alloc(rs.nbytes), ctx.alloc(rs.nbytes), ctx.alloc(8 * (chunk + 1))
ctx.upload(d_rs, rs); ctx.upload(d_rl, np.full(chunk, L, np.uint64)); ctx.upload(d_go, np.arange(chunk + 1, dtype=np.uint64))
t_build, per_chunk = 0.0, []
for g0 in range(0, N, chunk):
    c = min(chunk, N - g0)
    chk(lib.gs_synth_dna_dev(ctx.h, seed, g0, c, L, d_seq))
    ctx.sync()
    t0 = time.perf_counter()
    bx.add_genomes_dev(d_seq, c * words * 8 + 64, d_rs, d_rl, c, d_go, c)
    ctx.sync()
    per_chunk.append(time.perf_counter() - t0)
    t_build += per_chunk[-1]
nk = N * (L - k + 1)
print("build: %d genomes in %.3f s (%d chunks of %d; first %.3f s, the others %.3f s each): %.1f genomes/s, %.3g bit-sets/s, %d workgroup(s) per genome" %
      (N, t_build, len(per_chunk), chunk, per_chunk[0], np.mean(per_chunk[1:]) if len(per_chunk) > 1 else per_chunk[0], N / t_build, nk * h / t_build,
       ctx.last_sketch_info()["workgroups_per_genome"]), flush=True)
t = bx.bits_set()
print("build: bits set per column: mean %.0f (%.4f of the rows), expected %.0f" % (t.mean(), t.mean() / B, B * (1 - np.exp(-h * (L - k + 1) / B))), flush=True)
# the last genome of the last chunk against the restatement
g_last = N - 1
head = ctx.download(d_seq + ((g_last % chunk) * words * 8), (words * 8,), np.uint8)
ref = PR.Index(k, h, B)
ref.add([ascii_of(head, L)])
rows = ref.cols[0][:: max(len(ref.cols[0]) // 4000, 1)]
rows = np.unique(np.concatenate([rows, np.random.default_rng(1).integers(0, B, 4000).astype(np.uint64)]))
got = (bx.rows(rows)[:, g_last >> 6] >> np.uint64(g_last & 63)) & np.uint64(1)
ok = np.array_equal(got.astype(bool), np.isin(rows, ref.cols[0])) and int(t[g_last]) == len(ref.cols[0])
print("build: column %d (%d rows sampled, t_c) against pyref_bigsi: %s" % (g_last, len(rows), "bit-exact" if ok else "MISMATCH"), flush=True)

# ---- reads: records inside a buffer of `own` indexed genomes (colours 0 ..) and `other` genomes of another seed -------------------------------------
own, other = min(chunk, N), max(min(chunk, N) // 8, 1)
ctx.free(d_seq)
d_seq = ctx.alloc((own + other) * words * 8 + 64)
chk(lib.gs_synth_dna_dev(ctx.h, seed, 0, own, L, d_seq))
chk(lib.gs_synth_dna_dev(ctx.h, seed + 77, 0, other, L, d_seq + own * words * 8))
Q, RL = a.reads, a.read_len
rng = np.random.default_rng(2)
src = rng.integers(0, own + other, Q).astype(np.uint64)
start = src * np.uint64(words * 32) + rng.integers(0, L - RL, Q).astype(np.uint64)
for p in (d_rs, d_rl, d_go):
    ctx.free(p)
d_rs, d_rl, d_go = ctx.alloc(8 * Q), ctx.alloc(8 * Q), ctx.alloc(8 * (Q + 1))
ctx.upload(d_rs, start); ctx.upload(d_rl, np.full(Q, RL, np.uint64)); ctx.upload(d_go, np.arange(Q + 1, dtype=np.uint64))
d_n, d_c, d_h, d_t, d_acc = ctx.alloc(4 * Q), ctx.alloc(4 * Q), ctx.alloc(4 * Q), ctx.alloc(8 * Q), ctx.alloc(Q)
sb = (own + other) * words * 8 + 64
bx.query_dev(d_seq, sb, d_rs, d_rl, Q, d_go, min(Q, 20000), d_n, d_c, d_h, down_sample=a.down_sample)       # warm-up
ctx.sync()
times = []
for _ in range(3):
    t0 = time.perf_counter()
    bx.query_dev(d_seq, sb, d_rs, d_rl, Q, d_go, Q, d_n, d_c, d_h, down_sample=a.down_sample)
    ctx.sync()
    times.append(time.perf_counter() - t0)
tq = min(times)
n_used = ctx.download(d_n, Q, np.uint32)
look = int(n_used.sum()) * h
W = bx.info()["row_words"]
print("query: %d reads of %d bp (%.0f %% from indexed genomes), down_sample %d: %.4f s (runs: %s): %.3g reads/s, %.3g row look-ups/s, %.3g gathered bytes/s = %.2f of the copy rate "
      "(%d words per row)" % (Q, RL, 100.0 * own / (own + other), a.down_sample, tq, " ".join("%.4f" % x for x in times), Q / tq, look / tq, look * W * 8 / tq,
                              look * W * 8 / tq / copy_rate, W), flush=True)
t0 = time.perf_counter()
bx.classify_dev(Q, d_n, d_c, d_h, 1e-3, d_t, d_acc)
ctx.sync()
tc = time.perf_counter() - t0
col, hits, acc = ctx.download(d_c, Q, np.uint32), ctx.download(d_h, Q, np.uint32), ctx.download(d_acc, Q, np.uint8).astype(bool)
planted = src < own
print("classify: %d reads in %.4f s (%.3g reads/s); accepted %d, of the planted reads %d of %d with their own colour, of the others %d accepted" %
      (Q, tc, Q / tc, acc.sum(), int((acc & planted & (col == src)).sum()), int(planted.sum()), int((acc & ~planted).sum())), flush=True)
# a sample of reads against the restatement, on the sampled genome's column only where that is all the restatement holds: n and the planted hits
g0 = ascii_of(ctx.download(d_seq, (words * 8,), np.uint8), L)
mine = np.nonzero(src == 0)[0][:50]
ok = True
for r in mine:
    s = int(start[r])
    v = PR.kmers([g0[s:s + RL]], k)[:: a.down_sample]
    ok = ok and int(n_used[r]) == len(v) and int(hits[r]) == len(v) and int(col[r]) == 0
print("query: %d reads cut from genome 0 against pyref_bigsi (n, best colour, best hits = n): %s" % (len(mine), "equal" if ok else "MISMATCH"), flush=True)


# ---- the query with ties beside the plain query: the same reads, the same run ---------------------------------------------------------------------
def timed(f, repeats=5):
    f(min(Q, 20000))                                                               # warm-up
    ctx.sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f(Q)
        ctx.sync()
        out.append(time.perf_counter() - t0)
    return out


def ties_leg(ix, label, p_rs):
    """plain and ties form in turn on the reads that begin at p_rs; the ties form's arrays against the plain form's"""
    tp = timed(lambda q: ix.query_dev(d_seq, sb, p_rs, d_rl, Q, d_go, q, d_n, d_c, d_h, down_sample=a.down_sample))
    pn, pc, ph = (ctx.download(p, Q, np.uint32) for p in (d_n, d_c, d_h))
    tt = timed(lambda q: ix.query_ties_dev(d_seq, sb, p_rs, d_rl, Q, d_go, q, d_n, d_h, d_nt, d_td, d_sg, down_sample=a.down_sample, max_ties=a.max_ties))
    tn, th, nt, sg = (ctx.download(p, Q, np.uint32) for p in (d_n, d_h, d_nt, d_sg))
    td = ctx.download(d_td, (Q, a.max_ties), np.uint32)
    t0 = time.perf_counter()
    ix.verdict_dev(Q, d_n, d_h, d_nt, d_sg, 1e-3, d_t, d_acc)
    ctx.sync()
    tv = time.perf_counter() - t0
    vd = ctx.download(d_acc, Q, np.uint8)
    same = np.array_equal(pn, tn) and np.array_equal(ph, th) and np.array_equal(td[:, 0][th > 0], pc[th > 0]) and bool((td[:, 0][th == 0] == 0xFFFFFFFF).all())
    print("%s: plain %.4f s (runs: %s; spread %.1f %%), ties %.4f s (runs: %s; spread %.1f %%): ties / plain = %.3f; verdict %.4f s; n_tied: mean %.2f, max %d, "
          "reads with a tie %d; verdicts %s; n, hits and tied[0] against the plain query: %s" %
          (label, min(tp), " ".join("%.4f" % x for x in tp), 100 * (max(tp) - min(tp)) / min(tp), min(tt), " ".join("%.4f" % x for x in tt),
           100 * (max(tt) - min(tt)) / min(tt), min(tt) / min(tp), tv, nt.mean(), nt.max(), int((nt > 1).sum()), np.bincount(vd, minlength=5).tolist(),
           "equal" if same else "MISMATCH"), flush=True)
    return nt


if a.ties:
    d_nt, d_td, d_sg = ctx.alloc(4 * Q), ctx.alloc(4 * Q * a.max_ties), ctx.alloc(4 * Q)
    ties_leg(bx, "ties, none planted", d_rs)
    # colour c holds genome c // 8: the records of a chunk's 8 x fewer genomes, each named by 8 colours
    n8 = max(min(N // 8, own), 1)
    tx = G.Bigsi(k, h, B, N, ctx=ctx)
    d_gen8 = ctx.alloc((chunk // 8 + 1) * words * 8 + 64)
    t_rs, t_rl, t_go = ctx.alloc(8 * chunk), ctx.alloc(8 * chunk), ctx.alloc(8 * (chunk + 1))
    ctx.upload(t_rs, (np.arange(chunk, dtype=np.uint64) // np.uint64(8)) * np.uint64(words * 32)); ctx.upload(t_rl, np.full(chunk, L, np.uint64))
    ctx.upload(t_go, np.arange(chunk + 1, dtype=np.uint64))
    for first in range(0, N // 8 * 8, chunk):
        c = min(chunk, N // 8 * 8 - first)
        chk(lib.gs_synth_dna_dev(ctx.h, seed, first // 8, (c + 7) // 8, L, d_gen8))
        tx.add_genomes_dev(d_gen8, ((c + 7) // 8) * words * 8 + 64, t_rs, t_rl, c, t_go, c)
    ctx.sync()
    start8 = rng.integers(0, n8, Q).astype(np.uint64) * np.uint64(words * 32) + rng.integers(0, L - RL, Q).astype(np.uint64)
    d_rs8 = ctx.alloc(8 * Q)
    ctx.upload(d_rs8, start8)
    nt8 = ties_leg(tx, "ties, every read cut from a genome held by 8 colours", d_rs8)
    print("ties: reads with n_tied >= 8: %d of %d" % (int((nt8 >= 8).sum()), Q), flush=True)
    tx.close()
    for p in (d_gen8, t_rs, t_rl, t_go, d_rs8):
        ctx.free(p)


# ---- the minimizer index and the coverage filter, beside the plain legs above -------------------------------------------------------------------------
FAM_SKETCH, FAM_HAMMING, FAM_SEARCH, FAM_INSERT = 0, 1, 2, 3           # gs_internal.hpp: the families the steps of gs_bigsi.hip are timed as
if a.minimizer or a.min_count > 1:
    bx.close()
    for p in (d_seq, d_rs, d_rl, d_go):
        ctx.free(p)
    d_gen = ctx.alloc(chunk * words * 8 + 64)
    g_rs, g_rl, g_go = ctx.alloc(8 * chunk), ctx.alloc(8 * chunk), ctx.alloc(8 * (chunk + 1))
    ctx.upload(g_rs, np.arange(chunk, dtype=np.uint64) * np.uint64(words * 32)); ctx.upload(g_rl, np.full(chunk, L, np.uint64))
    ctx.upload(g_go, np.arange(chunk + 1, dtype=np.uint64))


def filter_leg(m, label):
    nf = min(a.filter_colours, chunk)
    fx = G.Bigsi(k, h, B, nf, ctx=ctx, minimizer_len=m)
    chk(lib.gs_synth_dna_dev(ctx.h, seed, 0, nf, L, d_gen))
    ctx.sync()
    ctx.profile(True)
    for fam in (FAM_SKETCH, FAM_HAMMING, FAM_INSERT):
        ctx.profile_read(fam)
    t0 = time.perf_counter()
    fx.add_genomes_dev(d_gen, nf * words * 8 + 64, g_rs, g_rl, nf, g_go, nf, min_count=a.min_count)
    ctx.sync()
    tb = time.perf_counter() - t0
    emit, srt, fill = (ctx.profile_read(fam)[0] / 1e3 for fam in (FAM_SKETCH, FAM_HAMMING, FAM_INSERT))
    ctx.profile(False)
    t, nk_ = fx.bits_set(return_kmers=True)
    print("%s build with min_count %d: %d colours of %.1f Mbp in %.3f s: %.2f genomes/s; emit %.3f s, sort + run lengths %.3f s, fill %.4f s (kernels); "
          "kept occurrences %d, bits %d (synthetic genomes repeat no value: the filter keeps nothing)" %
          (label, a.min_count, nf, L / 1e6, tb, nf / tb, emit, srt, fill, int(nk_.sum()), int(t.sum())), flush=True)
    fx.close()


if a.min_count > 1:
    filter_leg(0, "plain")
if a.minimizer:
    m = a.minimizer
    w = k - m + 1
    mx = G.Bigsi(k, h, B, N, ctx=ctx, minimizer_len=m)
    t_build, per_chunk = 0.0, []
    for first in range(0, N, chunk):
        c = min(chunk, N - first)
        chk(lib.gs_synth_dna_dev(ctx.h, seed, first, c, L, d_gen))
        ctx.sync()
        t0 = time.perf_counter()
        mx.add_genomes_dev(d_gen, c * words * 8 + 64, g_rs, g_rl, c, g_go, c)
        ctx.sync()
        per_chunk.append(time.perf_counter() - t0)
        t_build += per_chunk[-1]
    t, nkm = mx.bits_set(return_kmers=True)
    print("minimizer (%d, %d) build: %d genomes in %.3f s (first chunk %.3f s, the others %.3f s each): %.1f genomes/s, %.3g bit-sets/s; occurrences per window %.4f "
          "(2 / (w + 1) = %.4f); bits set per column: mean %.0f" %
          (k, m, N, t_build, per_chunk[0], np.mean(per_chunk[1:]) if len(per_chunk) > 1 else per_chunk[0], N / t_build, float(nkm.sum()) * h / t_build,
           float(nkm.mean()) / (L - k + 1), 2.0 / (w + 1), t.mean()), flush=True)
    g_last = N - 1
    head = ctx.download(d_gen + ((g_last % chunk) * words * 8), (words * 8,), np.uint8)
    ref = PM.Index(k, m, h, B)
    ref.add([ascii_of(head, L)])
    rows = np.unique(np.concatenate([ref.cols[0][:: max(len(ref.cols[0]) // 4000, 1)], np.random.default_rng(1).integers(0, B, 4000).astype(np.uint64)]))
    got = (mx.rows(rows)[:, g_last >> 6] >> np.uint64(g_last & 63)) & np.uint64(1)
    ok = np.array_equal(got.astype(bool), np.isin(rows, ref.cols[0])) and int(t[g_last]) == len(ref.cols[0]) and int(nkm[g_last]) == ref.nk[0]
    print("minimizer build: column %d (%d rows sampled, t_c, nk_c) against pyref_bigsi_mini: %s" % (g_last, len(rows), "bit-exact" if ok else "MISMATCH"), flush=True)
    # the same reads
    d_seq = ctx.alloc((own + other) * words * 8 + 64)
    chk(lib.gs_synth_dna_dev(ctx.h, seed, 0, own, L, d_seq))
    chk(lib.gs_synth_dna_dev(ctx.h, seed + 77, 0, other, L, d_seq + own * words * 8))
    d_rs, d_rl, d_go = ctx.alloc(8 * Q), ctx.alloc(8 * Q), ctx.alloc(8 * (Q + 1))
    ctx.upload(d_rs, start); ctx.upload(d_rl, np.full(Q, RL, np.uint64)); ctx.upload(d_go, np.arange(Q + 1, dtype=np.uint64))
    mx.query_dev(d_seq, sb, d_rs, d_rl, Q, d_go, min(Q, 20000), d_n, d_c, d_h, down_sample=a.down_sample)       # warm-up
    ctx.sync()
    mtimes = []
    for _ in range(3):
        t0 = time.perf_counter()
        mx.query_dev(d_seq, sb, d_rs, d_rl, Q, d_go, Q, d_n, d_c, d_h, down_sample=a.down_sample)
        ctx.sync()
        mtimes.append(time.perf_counter() - t0)
    tm = min(mtimes)
    ctx.profile(True)
    for fam in (FAM_SKETCH, FAM_SEARCH):
        ctx.profile_read(fam)
    mx.query_dev(d_seq, sb, d_rs, d_rl, Q, d_go, Q, d_n, d_c, d_h, down_sample=a.down_sample)
    ctx.sync()
    pre, srch = ctx.profile_read(FAM_SKETCH)[0] / 1e3, ctx.profile_read(FAM_SEARCH)[0] / 1e3
    ctx.profile(False)
    mn_used = ctx.download(d_n, Q, np.uint32)
    mlook = int(mn_used.sum()) * h
    print("minimizer query: %d reads of %d bp, down_sample %d: %.4f s (runs: %s): %.3g reads/s, %.3g row look-ups/s, %.3g gathered bytes/s = %.2f of the copy rate; "
          "k_bigsi_minimizers %.4f s, the look-ups %.4f s: the pre-pass is %.2f of the two" %
          (Q, RL, a.down_sample, tm, " ".join("%.4f" % x for x in mtimes), Q / tm, mlook / tm, mlook * W * 8 / tm, mlook * W * 8 / tm / copy_rate, pre, srch,
           pre / (pre + srch)), flush=True)
    print("minimizer against plain, same run: row look-ups %.4f of the plain index's (2 / (w + 1) = %.4f); time per read %.4f of the plain index's" %
          (mlook / look, 2.0 / (w + 1), tm / tq), flush=True)
    mcol, mhits = ctx.download(d_c, Q, np.uint32), ctx.download(d_h, Q, np.uint32)
    ok = True
    for r in mine:
        s_ = int(start[r])
        v = PM.minimizers(g0[s_:s_ + RL], k, m)[0][:: a.down_sample]
        ok = ok and int(mn_used[r]) == len(v) and int(mhits[r]) == len(v) and int(mcol[r]) == 0
    print("minimizer query: %d reads cut from genome 0 against pyref_bigsi_mini (n, best colour, best hits = n): %s" % (len(mine), "equal" if ok else "MISMATCH"), flush=True)
    if a.ties:
        ties_leg(mx, "minimizer (%d, %d) ties, none planted" % (k, m), d_rs)
    mx.close()
    if a.min_count > 1:
        filter_leg(m, "minimizer (%d, %d)" % (k, m))
