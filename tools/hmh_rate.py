#!/usr/bin/env python3
"""Rates of hypermash on the device (HyperMinHash, SPEC 7): k_sketch_hmh on synthetic genomes generated in HBM (gs_synth_dna_dev), one long
input split over many workgroups, the all-pairs similarity in both branches, and the files path on FASTQ.gz files.
usage: hmh_rate.py [--genomes N] [--big-gbp G] [--pairs-big P] [--pairs-small S] [--files F]"""
import argparse, gzip, os, sys, tempfile, time
import ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsearch_amd as G
import pyref_hmh as PR

ap = argparse.ArgumentParser()
ap.add_argument("--genomes", type=int, default=10000)
ap.add_argument("--big-gbp", type=float, default=4.0)
ap.add_argument("--pairs-big", type=int, default=10000)
ap.add_argument("--pairs-small", type=int, default=2000)
ap.add_argument("--files", type=int, default=300)
a = ap.parse_args()

ctx = G.Context(0)
lib, chk = ctx.L, G._lib.check
k, M = 21, 16384
prm = G.SeqSketcherParams(k, M, "hmh")


def synth_sketch(n, L, seed, d_out, chunk=4096):
    """n genomes of L bases from gs_synth_dna_dev, sketched in chunks into d_out; returns kernel-inclusive seconds (synthesis excluded)"""
    words = (L + 31) // 32
    chunk = min(chunk, n)
    d_seq = ctx.alloc(chunk * words * 8 + 64)
    rs = np.arange(chunk, dtype=np.uint64) * np.uint64(words * 32)
    d_rs, d_rl, d_go = ctx.alloc(rs.nbytes), ctx.alloc(rs.nbytes), ctx.alloc(8 * (chunk + 1))
    ctx.upload(d_rs, rs); ctx.upload(d_rl, np.full(chunk, L, np.uint64)); ctx.upload(d_go, np.arange(chunk + 1, dtype=np.uint64))
    t = 0.0
    for g0 in range(0, n, chunk):
        c = min(chunk, n - g0)
        chk(lib.gs_synth_dna_dev(ctx.h, seed, g0, c, L, d_seq))
        ctx.sync()
        t0 = time.perf_counter()
        chk(lib.gs_sketch_batch_dev(ctx.h, C.byref(prm.c), d_seq, c * words * 8 + 64, d_rs, d_rl, c, d_go, c, d_out + g0 * M * 2))
        ctx.sync()
        t += time.perf_counter() - t0
    head = ctx.download(d_seq, (words * 8,), np.uint8)                # the first genome of the last chunk
    for p in (d_seq, d_rs, d_rl, d_go):
        ctx.free(p)
    return t, head, n - c


def ascii_of(packed, L):
    codes = np.stack([(packed >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[:L]
    return bytes(np.frombuffer(b"ACGT", np.uint8)[codes])


# ---- 1. sketch rate: N x 5 Mbp
N, L = a.genomes, 5_000_000
d_sig = ctx.alloc(N * M * 2)
synth_sketch(min(N, 64), L, 1, d_sig)                                 # warm-up
t, head, g_last = synth_sketch(N, L, 1, d_sig)
info = ctx.last_sketch_info()
nk = N * (L - k + 1)
print("sketch: %d genomes x %.1f Mbp, k=%d: %.3f s, %.3g k-mers/s, %d workgroup(s) per genome" % (N, L / 1e6, k, t, nk / t, info["workgroups_per_genome"]), flush=True)
sig = ctx.download(d_sig + g_last * M * 2, (M,), np.uint16)
ok = np.array_equal(sig, PR.sketch([ascii_of(head, L)], k))
print("sketch: genome %d checked against pyref_hmh: %s" % (g_last, "bit-exact" if ok else "MISMATCH"), flush=True)

# ---- 2. similarity: the closed-form branch on the 5 Mbp sketches, the small-set branch on 50 kbp ones
nq = min(a.pairs_big, N)
d_sim = ctx.alloc(nq * nq * 8)
G.hmh_similarity_qxc_dev(ctx, d_sig, min(nq, 256), d_sig, min(nq, 256), d_sim); ctx.sync()
t0 = time.perf_counter()
G.hmh_similarity_qxc_dev(ctx, d_sig, nq, d_sig, nq, d_sim)
ctx.sync()
t = time.perf_counter() - t0
print("similarity (closed form, cards > 2^19): %d x %d pairs in %.3f s, %.3g pairs/s" % (nq, nq, t, nq * nq / t), flush=True)
rows = ctx.download(d_sig, (4, M), np.uint16)
s4 = ctx.download(d_sim, (4, nq), np.float64)[:, :4]
err = max(abs(s4[i, j] - PR.similarity(rows[i], rows[j])) for i in range(4) for j in range(4))
print("similarity: 4 x 4 checked against pyref_hmh, max |diff| %.3g" % err, flush=True)
ctx.free(d_sim); ctx.free(d_sig)

ns = a.pairs_small
d_ss = ctx.alloc(ns * M * 2)
synth_sketch(ns, 50_000, 2, d_ss)
d_sim = ctx.alloc(ns * ns * 8)
G.hmh_similarity_qxc_dev(ctx, d_ss, 64, d_ss, 64, d_sim); ctx.sync()
t0 = time.perf_counter()
G.hmh_similarity_qxc_dev(ctx, d_ss, ns, d_ss, ns, d_sim)
ctx.sync()
t = time.perf_counter() - t0
print("similarity (small-set branch, cards <= 2^19): %d x %d pairs in %.3f s, %.3g pairs/s" % (ns, ns, t, ns * ns / t), flush=True)
rows = ctx.download(d_ss, (3, M), np.uint16)
s3 = ctx.download(d_sim, (3, ns), np.float64)[:, :3]
err = max(abs(s3[i, j] - PR.similarity(rows[i], rows[j])) for i in range(3) for j in range(3))
print("similarity: 3 x 3 checked against pyref_hmh, max |diff| %.3g" % err, flush=True)
ctx.free(d_sim); ctx.free(d_ss)

# ---- 3. one long input (a metagenome-sized single genome)
Lb = int(a.big_gbp * 1e9)
d_one = ctx.alloc(M * 2)
t, _, _ = synth_sketch(1, Lb, 3, d_one)
info = ctx.last_sketch_info()
print("one input of %.2f Gbp: %.3f s, %.3g k-mers/s, %d workgroups" % (Lb / 1e9, t, (Lb - k + 1) / t, info["workgroups_per_genome"]), flush=True)
ctx.free(d_one)

# ---- 4. files: FASTQ.gz of 150 bp reads, 2 Mbp of reads per file
nf = a.files
with tempfile.TemporaryDirectory() as td:
    rng = np.random.default_rng(9)
    paths = []
    for f in range(nf):
        g = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 400_000)])
        st = rng.integers(0, len(g) - 150, 13_334)
        text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, g[s:s + 150], b"I" * 150) for i, s in enumerate(st))
        p = os.path.join(td, "s%04d.fq.gz" % f)
        with open(p, "wb") as fh:
            fh.write(gzip.compress(text, compresslevel=1))
        paths.append(p)
    sk = G.HyperMinHashSketch.for_k(k, ctx)
    sk.sketch_files(paths[:8])
    t0 = time.perf_counter()
    sig, nr, nb, st = sk.sketch_files(paths)
    t = time.perf_counter() - t0
    print("files: %d FASTQ.gz files (%.1f Mbp of reads each) in %.3f s: %.1f files/s; host read+decode+scan %.3f s (summed over threads), "
          "PCIe wait %.3f s, device pack + sketch %.3f s, wall %.3f s" % (nf, nb.mean() / 1e6, t, nf / t, st["host_read_decode_scan_s"], st["pcie_wait_s"],
                                                                        st["device_s"], st["wall_s"]), flush=True)
