#!/usr/bin/env python3
"""Rates of the split commands (gsearch_amd/split.py, SPEC 17 items 12-18) on files: a folder of N genomes of L bp in families of 20 (a random root,
mutants at 0.1 to 8 %), written as FASTA by this script, and a folder of Q further mutants as queries; OptDens k=21, s sketch slots, HNSW M=128 efc=1600.
  (1) request_split on a database of ONE piece against request on the same directory: what the command itself costs
  (2) on P pieces, request_split against the loop the reference's multiple_search.sh runs - request on every piece (which sketches the queries P
      times) and a merge on the host -, alternating in one session over three rounds: minimum and spread, the per-piece load / search+merge seconds,
      and the merge's share of a search_merge_dev call (the call against search_dev on the same loaded piece)
  (3) a database cut by the nearest of K medoids: request_split at probe = 1, 2 against all pieces - seconds, pieces loaded, and recall@nbanswers
      against the unrouted answers of the same run
usage: split_rate.py [--genomes N] [--length L] [--queries Q] [--sketch S] [--pieces P] [--medoids K] [--nbanswers A] [--workdir DIR]"""
import argparse, os, shutil, sys, tempfile, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import gsearch_amd as G
from gsearch_amd.sharding import merge_topk_shards
from gsearch_amd.state import SeqDict

ap = argparse.ArgumentParser()
ap.add_argument("--genomes", type=int, default=4000)
ap.add_argument("--length", type=int, default=50000)
ap.add_argument("--queries", type=int, default=200)
ap.add_argument("--sketch", type=int, default=4096)
ap.add_argument("--pieces", type=int, default=4)
ap.add_argument("--medoids", type=int, default=8)
ap.add_argument("--nbanswers", type=int, default=10)
ap.add_argument("--workdir", default=None)
a = ap.parse_args()

N, L, Q, S, P, KM, KNBN = a.genomes, a.length, a.queries, a.sketch, a.pieces, a.medoids, a.nbanswers
K, NBNG, EFC, PER, ROUNDS = 21, 128, 1600, 20, 3
ACGT = np.frombuffer(b"ACGT", np.uint8)
work = a.workdir or tempfile.mkdtemp(prefix="split_rate_")
db, qdir = os.path.join(work, "db"), os.path.join(work, "queries")


def mutate(rng, g, mu):
    h = g.copy()
    mask = rng.random(len(g)) < mu
    h[mask] = (h[mask] + rng.integers(1, 4, int(mask.sum()))) % 4
    return h


def write(path, g):
    with open(path, "wb") as f:
        f.write(b">g\n" + ACGT[g].tobytes() + b"\n")


t0 = time.perf_counter()
rng = np.random.default_rng(2024)
os.makedirs(db), os.makedirs(qdir)
roots = []
for i in range(N):
    if i % PER == 0:
        roots.append(rng.integers(0, 4, L))
    write(os.path.join(db, "g%06d.fna" % i), roots[-1] if i % PER == 0 else mutate(rng, roots[-1], rng.uniform(0.001, 0.08)))
for i in range(Q):
    write(os.path.join(qdir, "q%05d.fna" % i), mutate(rng, roots[int(rng.integers(len(roots)))], 0.02))
print("# shape: %d genomes x %d bp in families of %d, %d queries; OptDens k=%d s=%d, HNSW M=%d efc=%d, nbanswers %d, ef %d; files written in %.1f s"
      % (N, L, PER, Q, K, S, NBNG, EFC, KNBN, G.commands.EF_SEARCH, time.perf_counter() - t0), flush=True)
build = dict(ef=EFC, seed=7, capacity=2 * N, hnswrs=False)
out = lambda tag: dict(out=os.path.join(work, tag + ".txt"), matches=os.path.join(work, tag + ".matches"))


def timed(fn, *args, **kw):
    t = time.perf_counter()
    res = fn(*args, **kw)
    return time.perf_counter() - t, res


def spread(ts):
    return "min %.3f s, spread %.3f .. %.3f" % (min(ts), min(ts), max(ts))


# ---- (1) one piece ----------------------------------------------------------------------------------------------------------------------------------
one = os.path.join(work, "one")
t, rep = timed(G.tohnsw_split, db, one, K, S, NBNG, pieces=1, **build)
print("tohnsw_split pieces=1: %.2f s (%s)" % (t, ", ".join("%s %.2f" % kv for kv in rep["seconds"].items())), flush=True)
G.request(os.path.join(one, "part_000"), qdir, KNBN, **out("warm"))                    # code objects, pools
t_req, t_split = [], []
for r in range(ROUNDS):
    t, base = timed(G.request, os.path.join(one, "part_000"), qdir, KNBN, **out("request"))
    t_req.append(t)
    t, res = timed(G.request_split, one, qdir, KNBN, **out("split1"))
    t_split.append(t)
same = open(out("request")["out"], "rb").read() == open(out("split1")["out"], "rb").read()
print("(1) one piece: request %s; request_split %s; overhead of the command %.3f s; answers %s" % (spread(t_req), spread(t_split), min(t_split) - min(t_req),
      "byte-identical" if same else "DIFFER"), flush=True)
ok = same

# ---- (2) P pieces against the per-piece loop --------------------------------------------------------------------------------------------------------
many = os.path.join(work, "many")
t, rep = timed(G.tohnsw_split, db, many, K, S, NBNG, pieces=P, **build)
print("tohnsw_split pieces=%d: %.2f s (%s)" % (P, t, ", ".join("%s %.2f" % kv for kv in rep["seconds"].items())), flush=True)
dirs = [os.path.join(many, p["dir"]) for p in rep["pieces"]]
lengths = [len(SeqDict.reload_json(os.path.join(d, "seqdict.json")).items) for d in dirs]
offs = np.concatenate([[0], np.cumsum(lengths)])[:P].astype(np.uint64)


def loop():
    """request per piece, then a merge of the answers on the host: what multiple_search.sh does with sort -g"""
    ids, dist, secs = [], [], []
    for p, d in enumerate(dirs):
        t, r = timed(G.request, d, qdir, KNBN, **out("loop_piece"))
        secs.append((t, r["seconds"]["read_sketch"]))
        ids.append(np.where(r["ids"] == np.uint64(0xFFFFFFFFFFFFFFFF), r["ids"], r["ids"] + offs[p]))
        dist.append(r["distances"])
    t0 = time.perf_counter()
    m_ids, m_dist = merge_topk_shards(ids, dist, KNBN)
    return m_ids, m_dist, secs, time.perf_counter() - t0


t_loop, t_split = [], []
for r in range(ROUNDS):
    t, (l_ids, l_dist, secs, t_merge) = timed(loop)
    t_loop.append(t)
    t, res = timed(G.request_split, many, qdir, KNBN, **out("splitP"))
    t_split.append(t)
same = np.array_equal(l_ids, res["ids"]) and np.array_equal(l_dist.view(np.uint32), res["distances"].view(np.uint32))
ok = ok and same
print("(2) %d pieces: the per-piece loop %s (last round: per piece %s s of which the query sketch %s s, host merge %.4f s); request_split %s; answers %s"
      % (P, spread(t_loop), " ".join("%.3f" % s[0] for s in secs), " ".join("%.3f" % s[1] for s in secs), t_merge, spread(t_split),
         "identical" if same else "DIFFER"), flush=True)
print("    request_split, last round: %s; per piece load %s s, search+merge %s s" % (", ".join("%s %.3f" % kv for kv in res["seconds"].items()),
      " ".join("%.3f" % p["seconds"]["load"] for p in res["pieces"]), " ".join("%.3f" % p["seconds"]["search_merge"] for p in res["pieces"])), flush=True)
# the merge's share of a call: search_merge_dev against search_dev on the same loaded piece and the same device queries
ctx = G.default_context()
pdb = G.commands._Database(dirs[0], ctx)
nq = len(res["items"])
sig = np.ascontiguousarray(pdb.hn.get_data(0, min(nq, lengths[0])))
nq = len(sig)
d_q, d_ids, d_dist, d_cnt, d_ev = ctx.alloc(sig.nbytes), ctx.alloc(8 * nq * KNBN), ctx.alloc(4 * nq * KNBN), ctx.alloc(4 * nq), ctx.alloc(8 * nq)
ctx.upload(d_q, sig)
t_s, t_m = [], []
for r in range(ROUNDS + 1):
    t_s.append(timed(pdb.hn.search_dev, d_q, nq, KNBN, G.commands.EF_SEARCH, d_ids, d_dist, d_cnt, d_ev)[0])
    G.topk_reset_dev(ctx, nq, KNBN, d_ids, d_dist, d_cnt, d_ev)
    t_m.append(timed(pdb.hn.search_merge_dev, d_q, nq, KNBN, G.commands.EF_SEARCH, d_ids, d_dist, d_cnt, d_ev)[0])
pdb.close()
for p in (d_q, d_ids, d_dist, d_cnt, d_ev):
    ctx.free(p)
print("    one call on piece 0 with %d device queries: search_dev min %.4f s, search_merge_dev min %.4f s: the merge kernel and its launch are %.1f %% of the call"
      % (nq, min(t_s[1:]), min(t_m[1:]), 100.0 * max(min(t_m[1:]) - min(t_s[1:]), 0.0) / min(t_m[1:])), flush=True)

# ---- (3) routed search ------------------------------------------------------------------------------------------------------------------------------
routed = os.path.join(work, "routed")
t, rep = timed(G.tohnsw_split, db, routed, K, S, NBNG, mode="medoid", n_medoids=KM, max_piece=-(-N // P), **build)
print("tohnsw_split mode=medoid n_medoids=%d max_piece=%d: %.2f s (%s); piece sizes %s" % (KM, -(-N // P), t, ", ".join("%s %.2f" % kv for kv in rep["seconds"].items()),
      [p["nb_point"] for p in rep["pieces"]]), flush=True)
t_all, full = timed(G.request_split, routed, qdir, KNBN, **out("routed_all"))
for probe in (1, 2):
    if probe >= KM:
        continue
    ts = []
    for r in range(ROUNDS):
        t, res = timed(G.request_split, routed, qdir, KNBN, probe=probe, **out("routed_%d" % probe))
        ts.append(t)
    hit = sum(len(set(res["ids"][q, :int(res["counts"][q])].tolist()) & set(full["ids"][q, :int(full["counts"][q])].tolist())) for q in range(len(full["ids"])))
    print("(3) probe=%d: %s, %d of %d pieces loaded, %d query rows searched of %d; recall@%d against the unrouted answers %.4f (all pieces: %.3f s)"
          % (probe, spread(ts), sum(p["loaded"] for p in res["pieces"]), len(res["pieces"]), sum(p["rows"] for p in res["pieces"]),
             len(res["pieces"]) * len(full["ids"]), KNBN, hit / max(int(full["counts"].sum()), 1), t_all), flush=True)
if a.workdir is None:
    shutil.rmtree(work)
print("RESULT ok" if ok else "RESULT MISMATCH", flush=True)
