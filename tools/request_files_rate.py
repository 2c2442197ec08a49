#!/usr/bin/env python3
"""The whole chain from files to answers: a synthetic folder of .fna.gz genomes -> tohnsw -> request, with the stage split each command
returns, next to the same stages called directly (sketch_files + parallel_insert; sketch_files + search_arrays + ReqAnswer.dump) in the same run.
The difference is the commands' own overhead: listing, the JSON files, the two dumps, the reload of the directory, gsearch.matches.
usage: request_files_rate.py [--db 2000] [--queries 500] [--genome-len 1000000] [--roots 20] [--threads 16] [--pio 0] [--knbn 50] [--workers 16] [--repeats 3]
Parameters are the bench's: k = 21, s = 18000, optdens, M = 128, efc = 1600, level scale 0.25, ef = 5000."""
import argparse
import io
import os
import shutil
import sys
import tempfile
import time
import zlib
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ACGT = np.frombuffer(b"ACGT", np.uint8)


def _write_family(job):
    """one root and its mutants (1 % substitutions each, a further 1 % for the queries) as single-member .fna.gz files, level 1"""
    folder, qfolder, root_no, first, count, qcount, L, seed = job
    rng = np.random.default_rng([seed, root_no])
    root = rng.integers(0, 4, L).astype(np.uint8)

    def dump(path, codes, name):
        seq = ACGT[codes]
        pad = (-L) % 80
        lines = np.concatenate([np.concatenate([seq, np.full(pad, 78, np.uint8)]).reshape(-1, 80), np.full(((L + pad) // 80, 1), 10, np.uint8)], axis=1)
        co = zlib.compressobj(1, zlib.DEFLATED, 31)
        with open(path, "wb") as f:
            f.write(co.compress(b">%s synthetic\n" % name + lines.tobytes()) + co.flush())

    def mutant(base, mu):
        g = base.copy()
        pos = rng.integers(0, L, int(L * mu))
        g[pos] = (g[pos] + rng.integers(1, 4, len(pos)).astype(np.uint8)) & 3
        return g
    for i in range(count):
        dump(os.path.join(folder, "g%06d.fna.gz" % (first + i)), mutant(root, 0.01), b"genome%d" % (first + i))
    for i in range(qcount):
        dump(os.path.join(qfolder, "q%03d_%04d.fna.gz" % (root_no, i)), mutant(root, 0.02), b"query%d_%d" % (root_no, i))
    return count + qcount


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=500)
    ap.add_argument("--genome-len", type=int, default=1_000_000)
    ap.add_argument("--roots", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pio", type=int, default=0)
    ap.add_argument("--knbn", type=int, default=50)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--kmer", type=int, default=21)
    ap.add_argument("--sketch-size", type=int, default=18000)
    ap.add_argument("--max-nb-conn", type=int, default=128)
    ap.add_argument("--ef-construction", type=int, default=1600)
    ap.add_argument("--scale-modify", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import gsearch_amd as G

    work = tempfile.mkdtemp(prefix="gs_request_files_")
    try:
        dbf, qf, out = (os.path.join(work, n) for n in ("db", "queries", "database"))
        os.makedirs(dbf); os.makedirs(qf)
        t0 = time.perf_counter()
        R = max(1, min(args.roots, args.db))
        jobs, first = [], 0
        for r in range(R):
            c, qc = args.db // R + (r < args.db % R), args.queries // R + (r < args.queries % R)
            jobs.append((dbf, qf, r, first, c, qc, args.genome_len, args.seed))
            first += c
        with Pool(max(1, args.workers)) as pool:
            pool.map(_write_family, jobs)
        size = sum(os.path.getsize(os.path.join(d, n)) for d in (dbf, qf) for n in os.listdir(d))
        print("wrote %d + %d files of %.2f Mbp (.fna.gz, %.2f GB on disk, %d families) in %.1fs" % (args.db, args.queries, args.genome_len / 1e6, size / 1e9, R,
                                                                                                 time.perf_counter() - t0), flush=True)
        k, s, M, efc = args.kmer, args.sketch_size, args.max_nb_conn, args.ef_construction
        print("device:", G.default_context().device_info(), flush=True)
        # one pass over every file first (module load, first allocations, the page cache): neither side below pays for being the first
        t = time.perf_counter()
        G.sketcher_for(G.SeqSketcherParams(k, s, "optdens")).sketch_files(G.list_fasta_files(dbf) + G.list_fasta_files(qf), pio=args.pio, threads=args.threads)
        print("warm-up: sketch_files over all %d files in %.2fs (not counted)" % (args.db + args.queries, time.perf_counter() - t), flush=True)

        def stages(d):
            return ", ".join("%s %.3fs" % (n, v) for n, v in d.items())

        def plain(d):
            return ", ".join("%s %s" % (n, ("%.3f" % v) if isinstance(v, float) else v) for n, v in ((n, v.item() if hasattr(v, "item") else v) for n, v in d.items()))
        runs = []
        for rep_no in range(args.repeats):                      # the commands and the direct calls alternate, so both see the same machine
            print("--- repeat %d" % rep_no, flush=True)
            # ---- the commands
            t = time.perf_counter()
            rep = G.tohnsw(dbf, out, k, s, M, ef=efc, algo="optdens", scale_modify=args.scale_modify, pio=args.pio, threads=args.threads, seed=args.seed)
            t_tohnsw = time.perf_counter() - t
            print("tohnsw : %d files -> %d points in %.2fs = %.0f genomes/s | %s | hnsw_rs pair written: %s" % (rep["nb_file"], rep["nb_point"], t_tohnsw, rep["nb_file"] / t_tohnsw,
                                                                                                             stages(rep["seconds"]), rep["hnswrs_written"]), flush=True)
            print("         sketch_files: %s" % plain(rep["sketch_stats"]), flush=True)
            nb, mt = os.path.join(work, "gsearch.neighbors.txt"), os.path.join(work, "gsearch.matches")
            t = time.perf_counter()
            res = G.request(out, qf, args.knbn, out=nb, matches=mt, threads=args.threads, pio=args.pio)
            t_request = time.perf_counter() - t
            print("request: %d files, %d answers each, in %.2fs = %.0f genomes/s | %s | %d + %d lines" % (res["nb_file"], args.knbn, t_request, res["nb_file"] / t_request,
                                                                                                     stages(res["seconds"]), res["lines"]["neighbors"], res["lines"]["matches"]), flush=True)
            print("         sketch_files: %s" % plain(res["sketch_stats"]), flush=True)
            hits = sum(1 for i, it in enumerate(res["items"]) if res["counts"][i] and res["distances"][i, 0] < 0.9)
            print("         %d of %d queries have a neighbour under 0.9" % (hits, len(res["items"])), flush=True)
            # ---- the same stages called directly
            sk = G.sketcher_for(G.SeqSketcherParams(k, s, "optdens"))
            paths, qpaths = G.list_fasta_files(dbf), G.list_fasta_files(qf)
            t = time.perf_counter()
            sig, _, nsym, _ = sk.sketch_files(paths, pio=args.pio, threads=args.threads)
            d_sketch = time.perf_counter() - t
            hn = G.Hnsw.new(M, 1_500_000, 16, efc, G.DistHamming(), seed=args.seed)
            hn.modify_level_scale(args.scale_modify); hn.set_extend_candidates(True); hn.set_keeping_pruned(False)
            t = time.perf_counter()
            hn.parallel_insert(sig, ids=np.arange(len(sig), dtype=np.uint64))
            d_insert = time.perf_counter() - t
            print("direct : sketch_files %.3fs + parallel_insert %.3fs = %.2fs = %.0f genomes/s ; tohnsw adds %.2fs (%.1f %%)" % (
                d_sketch, d_insert, d_sketch + d_insert, len(paths) / (d_sketch + d_insert), t_tohnsw - d_sketch - d_insert, 100 * (t_tohnsw / (d_sketch + d_insert) - 1)), flush=True)
            seqdict = [(p, "", int(n)) for p, n in zip(paths, nsym)]
            t = time.perf_counter()
            qsig, _, qsym, _ = sk.sketch_files(qpaths, pio=args.pio, threads=args.threads)
            q_sketch = time.perf_counter() - t
            t = time.perf_counter()
            ids, dist, cnt, _ = hn.search_arrays(qsig, args.knbn, 5000)
            q_search = time.perf_counter() - t
            t = time.perf_counter()
            buf = io.StringIO()
            for i, p in enumerate(qpaths):
                G.ReqAnswer(i, (p, "", int(qsym[i])), [G.Neighbour(int(ids[i, j]), float(dist[i, j])) for j in range(int(cnt[i]))]).dump(seqdict, float(np.float32(0.99)), buf)
            q_text = time.perf_counter() - t
            same = buf.getvalue() == open(nb, encoding="utf-8").read()
            tot = q_sketch + q_search + q_text
            print("direct : sketch_files %.3fs + search_arrays %.3fs + ReqAnswer.dump %.3fs = %.2fs = %.0f genomes/s ; request adds %.2fs (%.1f %%) ; same answer text: %s" % (
                q_sketch, q_search, q_text, tot, len(qpaths) / tot, t_request - tot, 100 * (t_request / tot - 1), same), flush=True)
            hn.close()
            runs.append((t_tohnsw, d_sketch + d_insert, t_request, tot))
        med = [float(np.median([r[i] for r in runs])) for i in range(4)]
        print("median of %d: tohnsw %.3fs = %.0f genomes/s, direct %.3fs = %.0f genomes/s, the command adds %.3fs | request %.3fs = %.0f genomes/s, direct %.3fs = %.0f genomes/s, the command adds %.3fs" % (
            len(runs), med[0], args.db / med[0], med[1], args.db / med[1], med[0] - med[1], med[2], args.queries / med[2], med[3], args.queries / med[3], med[2] - med[3]), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
