"""Databases of several pieces on one device (SPEC 17 items 12-18): the reference's "Database split" scripts (scripts/split_folder.sh,
multiple_build.sh, multiple_search.sh) and the CoreSet cut of its todo.md, as two commands next to tohnsw / request.

* ``tohnsw_split``  - a folder of FASTA files -> out_dir/part_000 .. part_NNN, each a database directory of its own, cut at random or by the nearest
                      of k medoids (then with a router, out_dir/router, a database of the k medoids), and out_dir/split.json
* ``request_split`` - a folder of query files against all pieces, or against the pieces the router names: the queries are sketched ONCE and stay on
                      the device, the pieces are loaded, searched and closed one after the other (Hnsw.search_merge_dev), and one
                      gsearch.neighbors.txt comes out as if the database were whole

Only one piece is on the device at a time. Everything that touches sequence data runs on the device; there is no CPU fallback."""
import json
import os
import time

import numpy as np

from . import _lib
from ._lib import GsError
from . import api as A
from . import commands as Cm
from .state import DATA_TYPE, SKETCH_ALGO, HnswParams, ProcessingParams, ProcessingState, SeqDict

SPLIT_JSON, ROUTER, SPILL = "split.json", "router", "signatures.spill"
FILES_PER_ROUND, QUERIES_PER_ROUND = 4096, 4096
KNBN_MAX = 1024                                              # gs_index_search_merge_dev, gs_index_exact_search
_M64 = (1 << 64) - 1


# ---- the rules (SPEC 17 items 12-16; restated in tests/pyref_split.py) ---------------------------------------------------------------------------------
def split_key(seed, i):
    """the sort key of position i under `seed`: the splitmix64 finaliser of seed * 0x9E3779B97F4A7C15 + (i + 1) * 0xBF58476D1CE4E5B9 (mod 2^64)"""
    z = (int(seed) * 0x9E3779B97F4A7C15 + (int(i) + 1) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def split_order(n, seed):
    """the seeded permutation of 0..n-1: ascending (split_key, position)"""
    return sorted(range(int(n)), key=lambda i: (split_key(seed, i), i))


def _bounds(n, j, parts):
    base, rem = divmod(n, parts)
    lo = j * base + min(j, rem)
    return lo, lo + base + (1 if j < rem else 0)


def random_pieces(n, pieces, seed):
    """piece j takes positions [lo_j, hi_j) of split_order(n, seed), the bounds those of a contiguous cut whose first n mod pieces parts hold one
    more; inside a piece ascending (list order). pieces = 1: 0..n-1."""
    n, pieces = int(n), int(pieces)
    if not 1 <= pieces <= max(n, 1):
        raise GsError(_lib.GS_ERR_INVALID, "pieces = %d for %d genomes: between 1 and the number of genomes" % (pieces, n))
    order = split_order(n, seed)
    return [sorted(order[slice(*_bounds(n, j, pieces))]) for j in range(pieces)]


def sample_rows(n, size, seed):
    """the first `size` positions of split_order(n, seed), ascending"""
    return sorted(split_order(n, seed)[:max(0, min(int(size), int(n)))])


def medoid_pieces(assign, n_medoids, max_piece=None):
    """assign[i] = the medoid position of genome i -> [(medoid position, ascending genomes)]: medoids in position order, a medoid's n genomes as
    ceil(n / max_piece) consecutive runs whose sizes differ by at most one (max_piece None: one run); a medoid without a genome gives no piece"""
    if max_piece is not None and int(max_piece) < 1:
        raise GsError(_lib.GS_ERR_INVALID, "max_piece must be positive")
    out = []
    for j in range(int(n_medoids)):
        members = [i for i, a in enumerate(assign) if int(a) == j]
        parts = 1 if max_piece is None else -(-len(members) // int(max_piece))
        out += [(j, members[slice(*_bounds(len(members), c, parts))]) for c in range(parts if members else 0)]
    return out


def route_rows(table, counts, piece_medoid):
    """table (nq, probe) = every query's nearest medoid positions, counts (nq,) how many of them are valid -> per piece the ascending rows of the
    queries that chose its medoid (every piece of a shared medoid gets them); piece_medoid[p] None: every row"""
    table, counts = np.asarray(table), np.asarray(counts)
    nq = table.shape[0]
    valid = np.arange(table.shape[1])[None, :] < counts[:, None] if nq else np.zeros(table.shape, bool)
    return [np.arange(nq, dtype=np.uint32) if mp is None else np.nonzero(((table == mp) & valid).any(axis=1))[0].astype(np.uint32) for mp in piece_medoid]


def id_offsets(lengths):
    """piece p's ids start at the sum of the dictionary lengths of the pieces before it"""
    return [int(x) for x in np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])[:len(lengths)]]


def split_json_text(mode, seed, params, pieces, medoids, router):
    """the text of split.json: one object, indent 1, keys in this order. pieces: [(directory relative to out_dir, medoid position or None)];
    medoids: the medoid files' paths as listed; router: its directory relative to out_dir, or None"""
    obj = {"version": 1, "mode": mode, "seed": int(seed),
           "sketch": {"kmer_size": params.kmer_size, "sketch_size": params.sketch_size, "algo": SKETCH_ALGO[params.algo], "data_t": DATA_TYPE[params.data_t]},
           "block_flag": bool(params.block_flag), "router": router, "medoids": list(medoids),
           "pieces": [{"dir": d, "medoid": (None if mp is None else int(mp))} for d, mp in pieces]}
    return json.dumps(obj, indent=1, ensure_ascii=False) + "\n"


# ---- tohnsw_split -----------------------------------------------------------------------------------------------------------------------------------------
def _add_stats(total, stats):
    for k, v in (stats or {}).items():
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            total[k] = total.get(k, 0) + v
    return total


def _build_piece(rows_sig, items, nb_seq, nb_file, out_dir, params, sk, seed, insert_batch, max_layer, extend_candidates, keep_pruned, hnswrs, truncate_255, t_start):
    """one database directory from signatures that are already sketched: ONE parallel_insert with ids 0..n-1, every file of the directory, index closed"""
    hn = Cm._new_index(params, sk.sig_dtype(), sk.ctx, seed, insert_batch, max_layer, extend_candidates, keep_pruned)
    try:
        hn.parallel_insert(rows_sig, ids=np.arange(len(items), dtype=np.uint64))
        state = ProcessingState(nb_seq, nb_file, time.perf_counter() - t_start)
        return Cm._dump_database(hn, out_dir, params, SeqDict(items), state, hnswrs, truncate_255)
    finally:
        hn.close()


def _nearest_medoid(router_dir, spill, keep, ctx, per_round):
    """every kept row of the spill file through exact_search_dev(knbn = 1) on the router: the medoid position that minimises (mismatch count, position)"""
    db = Cm._Database(router_dir, ctx)
    try:
        assign = np.zeros(len(keep), np.int64)
        for a in range(0, len(keep), per_round):
            rows = np.ascontiguousarray(spill[keep[a:a + per_round]])
            with Cm._Scope(db.ctx) as d:
                d_q, d_ids, d_dist, d_cnt = d.up(rows), d.new(8 * len(rows)), d.new(4 * len(rows)), d.new(4 * len(rows))
                db.hn.exact_search_dev(d_q, len(rows), 1, d_ids, d_dist, d_cnt)
                assign[a:a + len(rows)] = db.ctx.download(d_ids, (len(rows),), np.uint64).astype(np.int64)
        return assign
    finally:
        db.close()


def tohnsw_split(dir, out_dir, kmer_size, sketch_size, nbng, pieces=None, mode="random", medoids=None, n_medoids=None, sample_size=None, cluster_fraction=0.1, max_piece=None,
                 files_per_round=FILES_PER_ROUND, ef=400, algo="optdens", aa=False, block=False, scale_modify=1.0, pio=0, threads=0, seed=0, insert_batch=0,
                 hnswrs=True, truncate_255=False, translate=None, ctx=None, capacity=Cm.CAPACITY, max_layer=Cm.MAX_LAYER, extend_candidates=True,
                 keep_pruned=False, gene=None, universal=None, universal_opts=None):
    """tohnsw into several database directories (SPEC 17 items 12-15). The files are listed as tohnsw lists them and sketched once, in rounds of
    files_per_round; a round's signatures are appended to out_dir/signatures.spill (deleted at the end), so the host holds one round plus one piece.
    mode="random": `pieces` pieces from the seeded permutation (random_pieces). mode="medoid": `medoids` = files of the folder, or n_medoids = k
    medoids that Hnsw.cluster (coreset fraction cluster_fraction) finds on a seeded sample of sample_size genomes (default: all); the medoids become out_dir/router, every genome goes
    to its nearest medoid, and a medoid's genomes are cut at max_piece. Every piece is built by ONE parallel_insert with ids 0..n-1 and written
    like tohnsw's directory; split.json names them. Every other argument is tohnsw's; universal is GS_ERR_UNSUPPORTED.
    Returns per piece its directory, medoid and tohnsw-like counts, the skipped files, the summed sketch statistics and seconds per stage."""
    t_start = time.perf_counter()
    if (universal is not None and universal is not False) or universal_opts:
        raise GsError(_lib.GS_ERR_UNSUPPORTED, "tohnsw_split: universal-gene databases are not split (build them with tohnsw)")
    if mode not in ("random", "medoid"):
        raise GsError(_lib.GS_ERR_INVALID, "mode: 'random' or 'medoid', not %r" % (mode,))
    if mode == "random" and (pieces is None or medoids is not None or n_medoids is not None or max_piece is not None):
        raise GsError(_lib.GS_ERR_INVALID, "mode='random' takes pieces, and neither medoids, n_medoids nor max_piece")
    if mode == "medoid" and (pieces is not None or (medoids is None) == (n_medoids is None)):
        raise GsError(_lib.GS_ERR_INVALID, "mode='medoid' takes medoids or n_medoids (one of them), and no pieces")
    if int(files_per_round) < 1:
        raise GsError(_lib.GS_ERR_INVALID, "files_per_round must be positive")
    params = ProcessingParams(HnswParams(capacity, ef, nbng, scale_modify), kmer_size, sketch_size, algo, "aa" if aa else "dna", block)
    sk = A.sketcher_for(A.SeqSketcherParams(kmer_size, sketch_size, params.algo, params.data_t), ctx)
    Cm._check_translate(translate, params.data_t, block, None)
    paths = Cm._list(dir, params.data_t, translate)
    t_list = time.perf_counter()
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    spill_path = os.path.join(out_dir, SPILL)
    n, m, dtype = len(paths), int(sketch_size), sk.sig_dtype()
    nrec, nsym, stats = np.zeros(n, np.uint64), np.zeros(n, np.uint64), {}
    build = dict(params=params, sk=sk, seed=seed, insert_batch=insert_batch, max_layer=max_layer, extend_candidates=extend_candidates, keep_pruned=keep_pruned,
                 hnswrs=hnswrs, truncate_255=truncate_255, t_start=t_start)
    try:
        with open(spill_path, "wb") as f:
            for a in range(0, n, int(files_per_round)):
                sig, r, s, st = Cm._sketch_dir(sk, paths[a:a + int(files_per_round)], block, pio, threads, translate, gene)
                np.ascontiguousarray(sig, dtype=dtype).tofile(f)
                nrec[a:a + len(r)], nsym[a:a + len(s)] = r, s
                _add_stats(stats, st)
        t_sketch = time.perf_counter()
        keep = [i for i in range(n) if int(nsym[i]) > 0]
        skipped = [paths[i] for i in range(n) if int(nsym[i]) == 0]
        if not keep:
            raise GsError(_lib.GS_ERR_INVALID, "none of the %d files under %s has a kept record" % (n, dir))
        spill = np.memmap(spill_path, dtype=dtype, mode="r", shape=(n, m))
        router, medoid_paths = None, []
        if mode == "random":
            cut = [(None, [keep[i] for i in part]) for part in random_pieces(len(keep), pieces, seed)]
        else:
            if medoids is not None:
                where = {os.path.abspath(p): i for i, p in enumerate(paths)}
                med = []
                for p in medoids:
                    i = where.get(os.path.abspath(str(p)))
                    if i is None or int(nsym[i]) == 0:
                        raise GsError(_lib.GS_ERR_INVALID, "medoid %s is no file of %s with a kept record" % (p, dir))
                    med.append(i)
                if not med or len(set(med)) != len(med):
                    raise GsError(_lib.GS_ERR_INVALID, "medoids: at least one file, none of them twice")
            else:
                sample = [keep[i] for i in sample_rows(len(keep), len(keep) if sample_size is None else sample_size, seed)]
                if not 1 <= int(n_medoids) <= len(sample):
                    raise GsError(_lib.GS_ERR_INVALID, "n_medoids = %d for a sample of %d genomes" % (int(n_medoids), len(sample)))
                hn = Cm._new_index(params, dtype, sk.ctx, seed, insert_batch, max_layer, extend_candidates, keep_pruned)
                try:
                    hn.parallel_insert(np.ascontiguousarray(spill[sample]), ids=np.arange(len(sample), dtype=np.uint64))
                    med = [sample[int(j)] for j in hn.cluster(n_cluster=int(n_medoids), fraction=cluster_fraction, seed=seed).medoids]
                finally:
                    hn.close()
            medoid_paths = [paths[i] for i in med]
            router = ROUTER
            _build_piece(np.ascontiguousarray(spill[med]), Cm._items(paths, nsym, med, block), Cm._nb_seq(nrec, med, len(med), block), len(med),
                         os.path.join(out_dir, ROUTER), **build)
            assign = _nearest_medoid(os.path.join(out_dir, ROUTER), spill, keep, sk.ctx, int(files_per_round))
            cut = [(j, [keep[i] for i in members]) for j, members in medoid_pieces(assign, len(med), max_piece)]
        t_route = time.perf_counter()
        report = []
        for p, (mp, files) in enumerate(cut):
            name = "part_%03d" % p
            nb_file = len(files) + (len(skipped) if p == 0 else 0)           # the files without a kept record are counted once, with the first piece
            written, why = _build_piece(np.ascontiguousarray(spill[files]), Cm._items(paths, nsym, files, block), Cm._nb_seq(nrec, files, nb_file, block), nb_file,
                                        os.path.join(out_dir, name), **build)
            report.append({"dir": name, "medoid": mp, "nb_point": len(files), "nb_file": nb_file, "nb_record": int(sum(int(nrec[i]) for i in files)),
                           "hnswrs_written": written, "hnswrs_refused": why})
        del spill
        with open(os.path.join(out_dir, SPLIT_JSON), "w", encoding="utf-8", newline="") as f:
            f.write(split_json_text(mode, seed, params, [(r["dir"], r["medoid"]) for r in report], medoid_paths, router))
    finally:
        if os.path.exists(spill_path):
            os.remove(spill_path)
    t_end = time.perf_counter()
    return {"pieces": report, "nb_file": n, "nb_point": len(keep), "skipped_files": skipped, "medoids": medoid_paths, "router": router, "sketch_stats": stats,
            "seconds": {"list": t_list - t_start, "read_sketch": t_sketch - t_list, "route": t_route - t_sketch, "build": t_end - t_route, "wall": t_end - t_start}}


# ---- request_split ----------------------------------------------------------------------------------------------------------------------------------------
_AGREE = ("kmer_size", "sketch_size", "algo", "data_t", "block_flag")


def _pieces_of(db):
    """-> (piece directories, their medoid positions or None, the router's directory or None, number of medoids)"""
    if isinstance(db, (list, tuple)):
        if not db:
            raise GsError(_lib.GS_ERR_INVALID, "request_split: an empty list of databases")
        return [str(d) for d in db], [None] * len(db), None, 0
    path = os.path.join(str(db), SPLIT_JSON)
    if not os.path.exists(path):
        raise GsError(_lib.GS_ERR_INVALID, "%s has no %s: give the directory tohnsw_split wrote, or a list of database directories" % (db, SPLIT_JSON))
    with open(path, encoding="utf-8") as f:
        o = json.load(f)
    dirs = [os.path.join(str(db), p["dir"]) for p in o["pieces"]]
    if not dirs:
        raise GsError(_lib.GS_ERR_INVALID, "%s names no piece" % path)
    router = os.path.join(str(db), o["router"]) if o.get("router") else None
    return dirs, [p["medoid"] for p in o["pieces"]], router, len(o.get("medoids") or [])


def request_split(db, query_dir, nbanswers, probe=None, out="gsearch.neighbors.txt", matches="gsearch.matches", ef=Cm.EF_SEARCH, threshold=Cm.OUT_THRESHOLD,
                  pio=0, threads=0, translate=None, ctx=None, gene=None, universal=None, universal_opts=None, queries_per_round=QUERIES_PER_ROUND):
    """request against a database of several pieces (SPEC 17 items 16-18). db: the directory tohnsw_split wrote, or a list of database directories
    built separately by tohnsw (no router: probe must be None). The queries are sketched once, in rounds of queries_per_round, and stay on the device
    with their running answers; the pieces are loaded, searched and merged (Hnsw.search_merge_dev) and closed in piece order, piece p's ids offset by
    the dictionary lengths of the pieces before it. probe=j < n_medoids: the router names every query's j nearest medoids first, a piece is searched
    for the queries that chose its medoid, and a piece nobody chose is never loaded. Pieces whose parameters.json disagree are refused with
    GS_ERR_INVALID before anything is written. The two files are request's, over the concatenated dictionary. Returns request's dictionary
    (index_source: per loaded piece) plus `pieces`: per piece its directory, id offset, rows searched and seconds for load and search_merge."""
    t_start = time.perf_counter()
    if (universal is not None and universal is not False) or universal_opts:
        raise GsError(_lib.GS_ERR_UNSUPPORTED, "request_split: universal-gene databases are not split")
    knbn = int(nbanswers)
    if not 1 <= knbn <= KNBN_MAX:
        raise GsError(_lib.GS_ERR_INVALID if knbn < 1 else _lib.GS_ERR_UNSUPPORTED, "nbanswers = %d: between 1 and %d" % (knbn, KNBN_MAX))
    dirs, piece_medoid, router, n_medoids = _pieces_of(db)
    if probe is not None:
        if router is None:
            raise GsError(_lib.GS_ERR_INVALID, "probe needs a router: this database has none")
        if not 1 <= int(probe) <= n_medoids:
            raise GsError(_lib.GS_ERR_INVALID, "probe = %d: between 1 and the %d medoids" % (int(probe), n_medoids))
        if int(probe) == n_medoids:
            probe = None                                     # every piece gets every row: the unrouted call
    all_params = [ProcessingParams.reload_json(d) for d in dirs] + ([ProcessingParams.reload_json(router)] if router and probe is not None else [])
    for d, p in zip(dirs + [router], all_params):
        for key in _AGREE:
            if getattr(p, key) != getattr(all_params[0], key):
                raise GsError(_lib.GS_ERR_INVALID, "%s: %s = %r, but %r in %s" % (d, key, getattr(p, key), getattr(all_params[0], key), dirs[0]))
    params = all_params[0]
    block = params.block_flag
    Cm._check_translate(translate, params.data_t, block, None)
    dicts = [SeqDict.reload_json(os.path.join(d, "seqdict.json")).items for d in dirs]
    offsets = id_offsets([len(x) for x in dicts])
    seqdict = [it for x in dicts for it in x]
    del dicts
    sk = A.sketcher_for(A.SeqSketcherParams(params.kmer_size, params.sketch_size, params.algo, params.data_t), ctx)
    ctx = sk.ctx
    t_load = time.perf_counter()
    paths = Cm._list(query_dir, params.data_t, translate)
    t_list = time.perf_counter()
    m, dtype = params.sketch_size, sk.sig_dtype()
    rowbytes = m * dtype.itemsize
    report = [{"dir": d, "id_offset": offsets[p], "medoid": piece_medoid[p], "rows": 0, "loaded": False, "index_source": None,
               "seconds": {"load": 0.0, "search_merge": 0.0}} for p, d in enumerate(dirs)]
    nsym, stats, items = np.zeros(len(paths), np.uint64), {}, []
    with Cm._Scope(ctx) as dev:
        d_q = dev.new(rowbytes * len(paths))                 # every kept query's signature, in request order
        for a in range(0, len(paths), int(queries_per_round)):
            sig, _, s, st = Cm._sketch_dir(sk, paths[a:a + int(queries_per_round)], block, pio, threads, translate, gene)
            nsym[a:a + len(s)] = s
            _add_stats(stats, st)
            keep = [i for i in range(len(s)) if int(s[i]) > 0]
            if keep:
                ctx.upload(d_q + rowbytes * len(items), np.ascontiguousarray(sig[keep], dtype=dtype))
            items += Cm._items(paths[a:a + len(s)], s, keep, block)
        t_sketch = time.perf_counter()
        nq = len(items)
        ids, dist = np.zeros((nq, knbn), np.uint64), np.zeros((nq, knbn), np.float32)
        cnt, ev = np.zeros(nq, np.uint32), np.zeros(nq, np.uint64)
        if nq:
            d_ids, d_dist, d_cnt, d_ev = dev.new(8 * nq * knbn), dev.new(4 * nq * knbn), dev.new(4 * nq), dev.new(8 * nq)
            A.topk_reset_dev(ctx, nq, knbn, d_ids, d_dist, d_cnt, d_ev)
            rows = [None] * len(dirs)
            if probe is not None:
                rdb = Cm._Database(router, ctx)
                try:
                    j = int(probe)
                    with Cm._Scope(ctx) as d:
                        r_ids, r_dist, r_cnt = d.new(8 * nq * j), d.new(4 * nq * j), d.new(4 * nq)
                        rdb.hn.exact_search_dev(d_q, nq, j, r_ids, r_dist, r_cnt)
                        rows = route_rows(ctx.download(r_ids, (nq, j), np.uint64).astype(np.int64), ctx.download(r_cnt, (nq,), np.uint32), piece_medoid)
                finally:
                    rdb.close()
            for p, d in enumerate(dirs):
                nr = nq if rows[p] is None else len(rows[p])
                report[p]["rows"] = int(nr)
                if nr == 0:
                    continue
                t0 = time.perf_counter()
                pdb = Cm._Database(d, ctx)
                try:
                    t1 = time.perf_counter()
                    with Cm._Scope(ctx) as sc:
                        d_rows = None if rows[p] is None else sc.up(np.ascontiguousarray(rows[p], np.uint32))
                        pdb.hn.search_merge_dev(d_q, nq, knbn, int(ef), d_ids, d_dist, d_cnt, d_ev, d_rows=d_rows, nr=nr, id_offset=offsets[p])
                    report[p].update(loaded=True, index_source=pdb.source)
                finally:
                    pdb.close()
                report[p]["seconds"] = {"load": t1 - t0, "search_merge": time.perf_counter() - t1}
            ids, dist = ctx.download(d_ids, (nq, knbn), np.uint64), ctx.download(d_dist, (nq, knbn), np.float32)
            cnt, ev = ctx.download(d_cnt, (nq,), np.uint32), ctx.download(d_ev, (nq,), np.uint64)
    t_search = time.perf_counter()
    nb_match, lines = Cm._write_answers(items, ids, dist, cnt, seqdict, threshold, out, matches, block)
    t_text = time.perf_counter()
    seconds = {"load": t_load - t_start, "list": t_list - t_load, "read_sketch": t_sketch - t_list, "search": t_search - t_sketch, "text": t_text - t_search,
               "wall": t_text - t_start}
    return {"ids": ids, "distances": dist, "counts": cnt, "evals": ev, "items": items, "nb_file": len(paths), "nb_match": nb_match,
            "skipped_files": [paths[i] for i in range(len(paths)) if int(nsym[i]) == 0], "lines": lines, "sketch_stats": stats, "seconds": seconds,
            "index_source": [r["index_source"] for r in report if r["loaded"]], "pieces": report, "probe": None if probe is None else int(probe)}
