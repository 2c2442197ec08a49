#!/usr/bin/env python3
"""Seconds per stage of universal_sketch (SPEC 17 item 11) beside the host composition it replaces, on the same commit.

  genomes     `genomes` synthetic genomes of `len` uniform random bases, written as .fna files, in each of which the consensus of every one of 120
              synthetic profiles (the node counts of the bacterial universal-gene set, tests/golden/hmm/bacteria_node_counts.txt) is planted as a gene:
              M + the consensus back-translated + a stop, on a random strand, at random non-overlapping places. The targets are the six-frame ORFs
              (translate=True): random bases do not train the gene caller.
  device      universal_sketch(files, profiles, sketcher, translate=True, region=.., prefilter=..): its seconds per stage - targets (read, split, pack,
              upload, translate), search, best hits, spans, hit records (gs_hmm_hit_records_dev), sketch - and the share of the hit-record step
  host        sketcher.sketch_genomes(universal_genes(the same arguments)[0]): the chosen residues come back to the host and go up again
  The two alternate in one session, `rounds` rounds after a warm-up of each; minima and spread ((max - min) / min) of the walls. The rows must be equal.

usage: universal_rate.py [--genomes 16] [--len 2000000] [--rounds 3] [--region protein] [--prefilter msv+vit16] [--algo optdens] [--log profiles/universal_rate.log]"""
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


def planted_genome(rng, length, genes):
    """uniform random bases with `genes` (code arrays) written over them at non-overlapping places, each on a random strand"""
    code = rng.integers(0, 4, length).astype(np.uint8)
    room = length // len(genes)
    for i, g in enumerate(genes):
        assert len(g) + 100 <= room, "the genome is too short for its planted genes"
        at = i * room + int(rng.integers(50, room - len(g) - 49))
        code[at:at + len(g)] = (3 - g)[::-1] if rng.integers(0, 2) else g
    return np.frombuffer(b"ACGT", np.uint8)[code].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=16)
    ap.add_argument("--len", type=int, default=2000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--region", default="protein")
    ap.add_argument("--prefilter", default="msv+vit16")
    ap.add_argument("--algo", default="optdens")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "universal_rate.log"))
    a = ap.parse_args()
    import gsearch_amd as G
    import pyref_hmm as R
    import pyref_orf as P
    ctx = G.default_context()
    rng = np.random.default_rng(a.seed)
    nodes = [int(x) for x in open(os.path.join(ROOT, "tests", "golden", "hmm", "bacteria_node_counts.txt")).read().split()]
    models = [R.synth_model(rng, M, name="SYN%03d_%d" % (i, M)) for i, M in enumerate(nodes)]
    texts = [R.write_hmm(m) for m in models]
    db = G.HmmDb(texts, ctx, texts=True)
    genes = [np.concatenate([P.back_translate(b"M" + db.consensus(p)), np.array([3, 0, 0], np.uint8)]) for p in range(len(db))]       # .. TAA
    sk = G.sketcher_for(G.SeqSketcherParams(5, 1800, a.algo, "aa"), ctx)
    prefilter = None if a.prefilter in ("", "none") else a.prefilter
    opts = dict(region=a.region, prefilter=prefilter)
    res = {"genomes": a.genomes, "len": a.len, "profiles": len(db), "nodes": sum(nodes), "region": a.region, "prefilter": prefilter, "algo": a.algo, "rounds": a.rounds}
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for g in range(a.genomes):
            files.append(os.path.join(tmp, "g%03d.fna" % g))
            with open(files[-1], "wb") as f:
                f.write(b">g%03d\n" % g + planted_genome(rng, a.len, genes) + b"\n")

        def device():
            t = time.perf_counter()
            out = G.universal_sketch(files, db, sk, translate=True, **opts)
            ctx.sync()
            return time.perf_counter() - t, out

        def host():
            t = time.perf_counter()
            lists = G.universal_genes(files, db, ctx=ctx, translate=True, **opts)[0]
            t1 = time.perf_counter()
            rows = sk.sketch_genomes(lists)
            ctx.sync()
            t2 = time.perf_counter()
            return t2 - t, t1 - t, t2 - t1, rows, lists
        device(), host()                                                    # the warm-up of both
        dev_wall, host_wall, host_genes, host_sketch, stages = [], [], [], [], []
        for _ in range(a.rounds):
            w, (sig, nrec, nsym, local, st) = device()
            dev_wall.append(w)
            stages.append(st["stage_s"])
            w, tg, ts, rows, lists = host()
            host_wall.append(w)
            host_genes.append(tg)
            host_sketch.append(ts)
        res["equal_rows"] = bool(np.array_equal(np.ascontiguousarray(sig).view(np.uint8), np.ascontiguousarray(rows).view(np.uint8)))
        res["hits"], res["residues_sketched"] = int(nrec.sum()), int(nsym.sum())
    spread = lambda v: (max(v) - min(v)) / min(v)      # noqa: E731
    best = min(range(a.rounds), key=lambda i: dev_wall[i])
    res["device_wall_s"], res["device_spread"] = min(dev_wall), spread(dev_wall)
    res["host_wall_s"], res["host_spread"] = min(host_wall), spread(host_wall)
    res["host_universal_genes_s"], res["host_sketch_genomes_s"] = min(host_genes), min(host_sketch)
    res["stage_s"] = {k: min(s[k] for s in stages) for k in G.UNIVERSAL_STAGES}
    res["stage_s_of_best_round"] = stages[best]
    res["hit_records_share"] = res["stage_s"]["hit_records"] / res["device_wall_s"]
    res["device_over_host"] = res["device_wall_s"] / res["host_wall_s"]
    db.close()
    print("universal_sketch: %d genomes x %d bases, %d profiles, region=%s prefilter=%s: %d hits, %d residues sketched, rows equal: %s" %
          (a.genomes, a.len, res["profiles"], a.region, prefilter, res["hits"], res["residues_sketched"], res["equal_rows"]))
    print("  device %.3f s (spread %.3f): %s" % (res["device_wall_s"], res["device_spread"], ", ".join("%s %.4f" % (k, res["stage_s"][k]) for k in G.UNIVERSAL_STAGES)))
    print("  hit records %.5f of the call" % res["hit_records_share"])
    print("  host   %.3f s (spread %.3f): universal_genes %.3f, sketch_genomes %.4f; device / host %.3f" %
          (res["host_wall_s"], res["host_spread"], res["host_universal_genes_s"], res["host_sketch_genomes_s"], res["device_over_host"]))
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
