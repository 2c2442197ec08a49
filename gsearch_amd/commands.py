"""The four commands the project was modelled on, on directories of files (SPEC 17):

* ``tohnsw``   - gsearch tohnsw  (gsearch.rs:204-283, dnasketch.rs:60-470, aasketch.rs): a folder of FASTA files -> a database directory
* ``add``      - gsearch add     (gsearch.rs:717-741, dnasketch.rs:106-134): more files into that directory
* ``request``  - gsearch request (gsearch.rs:880-950, dnarequest.rs:240-400, answer.rs, matcher.rs): a folder of query files -> gsearch.neighbors.txt
                 (and gsearch.matches by sequence)
* ``reformat`` - reformat        (src/bin/reformat.rs): gsearch.neighbors.txt -> the ANI table of the README
* ``derep``    - no upstream program (SPEC 18): a database directory -> its clusters and representatives at an ANI cut

They join pieces that are each held to the oracle on their own - list_fasta_files, sketch_files, Hnsw.parallel_insert / search_arrays, the two dump
formats, state.py, ReqAnswer.dump, ani - and add no kernel. Everything that touches sequence data runs on the device; there is no CPU fallback.
Argument parsing and logging of the binaries are not here."""
import decimal
import io
import json
import os
import time

import numpy as np

from . import _lib
from ._lib import GsError
from . import api as A
from .state import HnswParams, ProcessingParams, ProcessingState, SeqDict

GSIDX, HNSWRS = "hnswdump.gsidx", "hnswdump"            # the library's own lossless dump; Hnsw::file_dump(dir, "hnswdump") of dumpload.rs:26-31
CAPACITY, MAX_LAYER = 1_500_000, 16                       # gsearch.rs:269, dnasketch.rs:139
EF_SEARCH, OUT_THRESHOLD = 5000, 0.99                     # gsearch.rs:893, dnarequest.rs:83
MATCHES_LISTED = 5                                        # matcher.rs:266
BLOCK_FASTA_ID = "-total-sequence"                        # dnafiles.rs:268-272, aafiles.rs:91-95
GENES_PER_CALL = 64                                       # genomes called and sketched per device round of translate="genes"
UNIVERSAL = "universal.json"                              # sidecar of a universal-gene database: the profile names in order and the options (SPEC 17 item 11)
UNIVERSAL_OPTS = ("cutoff", "score", "filter_p", "region", "min_aa", "table", "prefilter", "msv_p", "genomes_per_call", "bias")


# ---- Rust's number formats -----------------------------------------------------------------------------------------------------------------------
def rust_display_f64(x):
    """Rust's `{}` of an f64: the shortest digits that round-trip, always positional, no `.0` on integral values (0.54, 0.00001, 0, 100,
    10000000000000000); `inf`, `-inf`, `NaN`, `-0`. Python's repr has the same digits and differs in the layout at both ends (1e-05, 1e+16, 100.0)."""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    s = format(decimal.Decimal(repr(x)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def rust_upper_exp(x, digits):
    """Rust's `{:.<digits>E}` (5.400E-1: no `+`, no exponent padding)"""
    return A._rust_e(x, digits)


# ---- gsearch.matches (matcher.rs) ----------------------------------------------------------------------------------------------------------------
def matches_text(requests, seqdict, threshold=OUT_THRESHOLD, listed=MATCHES_LISTED):
    """The text Matcher::analyze writes (matcher.rs:233-277). requests: (request path, neighbours) in request order, a neighbour anything with
    .d_id and .distance (f32), in answer order; seqdict: (path, fasta_id, len) by d_id. Per request genome its targets grouped by database path, a
    target's merit the f64 product of its distances below the threshold cast to f32, ascending merit, at most `listed` lines. The two orders upstream
    leaves to a HashMap are fixed (SPEC 17): request genomes in request order, equal merits by first appearance among the neighbours."""
    thr = np.float32(threshold)
    genomes = {}                                            # request path -> {target path -> merit}; dicts keep first appearance
    for path, neighbours in requests:
        targets = genomes.setdefault(path, {})
        for n in neighbours:
            tpath = seqdict[int(n.d_id)][0]
            d = np.float32(n.distance)
            merit = targets.setdefault(tpath, 1.0)
            if d < thr:
                targets[tpath] = merit * float(d)
    out = []
    for path, targets in genomes.items():
        out.append("\n\n request genome : %s" % path)
        ranked = sorted(((float(np.float32(m)), t) for t, m in targets.items()), key=lambda e: e[0])      # stable: ties keep first appearance
        for merit, tpath in ranked[:listed]:
            out.append("\n\t matched genome %s  merit : %s" % (tpath, rust_upper_exp(merit, 3)))
    return "".join(out)


# ---- reformat (src/bin/reformat.rs) --------------------------------------------------------------------------------------------------------------
REFORMAT_HEADER = "Query_Name\tDistance\tNeighbor_Fasta_name\tNeighbor_Seq_Len\tANI"          # reformat.rs:61


def _file_name(path):
    return os.path.basename(path.rstrip("/"))


def _ani_string(distance, kmer, model):
    """reformat.rs:80-86"""
    if model not in (1, 2):
        return "Invalid Model"
    return rust_display_f64(A.ani(distance, kmer, model))


def reformat_text(kmer, model, text):
    """reformat.rs on the text of a gsearch.neighbors.txt -> the text of the table"""
    kmer, model = int(kmer), int(model)
    rows = []
    for no, line in enumerate(text.split("\n"), 1):
        if line.endswith("\r"):
            line = line[:-1]
        if not line.startswith("query_id:"):
            continue
        parts = line.split("\t")
        if len(parts) < 8:
            raise ValueError("line %d has %d fields, an answer line has 9: %r" % (no, len(parts), line))
        s = parts[3]
        try:
            if s != s.strip() or "_" in s:
                raise ValueError(s)
            distance = float(s)
        except ValueError:
            raise ValueError("Failed to parse distance %r in line %d: %r" % (s, no, line)) from None
        # reformat.rs:75 takes parts[7], which answer.rs:66-71 makes the label " answer_seq_len:"; the README's table shows the length (SPEC 17)
        rows.append((_file_name(parts[1]).encode(), distance, "%s\t%s\t%s\t%s\t%s" % (
            _file_name(parts[1]), rust_display_f64(distance), _file_name(parts[5]), parts[-1].strip(" "), _ani_string(distance, kmer, model))))
    rows.sort(key=lambda r: (r[0], r[1]))                   # stable: ties keep input order
    return "".join(s + "\n" for s in [REFORMAT_HEADER] + [r[2] for r in rows])


def reformat(kmer, model, input_file, output_file):
    """`reformat kmer model input output`: the answers of `request` as the table Query_Name, Distance, Neighbor_Fasta_name, Neighbor_Seq_Len, ANI,
    sorted by (query name, distance). Returns the number of rows."""
    with open(input_file, encoding="utf-8", newline="") as f:
        out = reformat_text(kmer, model, f.read())
    with open(output_file, "w", encoding="utf-8", newline="") as f:
        f.write(out)
    return out.count("\n") - 1


# ---- files -> signatures -------------------------------------------------------------------------------------------------------------------------
def _check_translate(translate, data_t, block, universal=None):
    if universal is not None and universal is not False:
        if data_t != _lib.DATA["aa"]:
            raise GsError(_lib.GS_ERR_INVALID, "universal genes feed the amino-acid sketchers: the database is not an AA database")
        if block:
            raise GsError(_lib.GS_ERR_UNSUPPORTED, "universal with block: the universal genes of a genome are not one record")
        if translate is not None and translate is not True and translate != "genes":
            raise GsError(_lib.GS_ERR_INVALID, "translate with universal: None, True or 'genes', not %r" % (translate,))
        return
    if translate is None:
        return
    if translate != "genes":
        raise GsError(_lib.GS_ERR_INVALID, "translate: None or 'genes' (True only with universal), not %r" % (translate,))
    if data_t != _lib.DATA["aa"]:
        raise GsError(_lib.GS_ERR_INVALID, "translate='genes' feeds the amino-acid sketchers: the database is not an AA database")
    if block:
        raise GsError(_lib.GS_ERR_UNSUPPORTED, "translate='genes' with block: the genes of a genome are not one record")


def _list(directory, data_t, translate):
    files = A.list_fasta_files(directory, "dna" if translate else data_t)
    if not files:
        raise GsError(_lib.GS_ERR_INVALID, "no %s file under %s" % ("nucleotide FASTA" if translate or data_t == _lib.DATA["dna"] else "protein FASTA", directory))
    return files


class _Scope:
    """device buffers of one round, freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def new(self, nbytes):
        ptr = self.ctx.alloc((max(int(nbytes), 8) + 7) // 8 * 8)
        self.bufs.append(ptr)
        return ptr

    def up(self, arr):
        ptr = self.new(arr.nbytes)
        if arr.nbytes:
            self.ctx.upload(ptr, arr)
        return ptr

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        while self.bufs:
            self.ctx.free(self.bufs.pop())


def _genome_contigs(path):
    """the kept records of one nucleotide file, line breaks removed (the reader's rules: `capsid` records skipped)"""
    text = A.read_fasta_file(path)
    return [bytes(text[b:e]).replace(b"\n", b"").replace(b"\r", b"") for _, b, e in A.fasta_scan(text, skip_capsid=True)]


def _sketch_genes(sk, paths, gene):
    """translate='genes': every genome's proteome is what gene_call gives, called on the device and sketched there by the AA sketcher in the layout
    gene_call_dev leaves (aa, aa_start, aa_len; rec_gene_off gathered at the genome boundaries). The host sees descriptors, never residues.
    -> what sketch_files returns: (signatures, genes per file, residues per file, stats)"""
    ctx, gene = sk.ctx, dict(gene or {})
    n, m = len(paths), sk.params.c.sketch_size
    sig = np.zeros((n, m), sk.sig_dtype())
    nrec, nsym = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    st = {"host_read_decode_scan_s": 0.0, "pcie_wait_s": 0.0, "device_s": 0.0, "wall_s": 0.0, "gz_members_inflated_on_device": 0,
          "gz_members_handed_back_to_host": 0}
    t_all = time.perf_counter()
    min_aa = int(A.gene_params(**gene).min_aa)
    for f0 in range(0, n, GENES_PER_CALL):
        t0 = time.perf_counter()
        recs, goff = [], [0]
        for p in paths[f0:f0 + GENES_PER_CALL]:
            for ctg in _genome_contigs(p):
                recs.extend(ctg[b:b + l] for b, l in A.bigsi_split(ctg))          # cut at every byte outside ACGTacgt, as gene_call does
            goff.append(len(recs))
        ng, n_rec = len(goff) - 1, len(recs)
        t1 = time.perf_counter()
        st["host_read_decode_scan_s"] += t1 - t0
        if n_rec == 0:
            continue
        seq, rs, rl = A.pack_dna_records(recs)
        goff = np.array(goff, np.uint64)
        cap_aa = 2 * int(np.maximum(rl.astype(np.int64) - 2, 0).sum())
        cap_gene = cap_aa // max(min_aa, 1)
        if cap_gene == 0:                                     # no record long enough to hold a gene
            continue
        with _Scope(ctx) as d:
            d_aa, d_as, d_al, d_off = d.new(cap_aa + 8), d.new(8 * cap_gene), d.new(8 * cap_gene), d.new(8 * (n_rec + 1))
            n_gene, _ = A.gene_call_dev(ctx, d.up(seq), seq.nbytes, d.up(rs), d.up(rl), n_rec, d.up(goff), ng, d.new(16 * ng), cap_gene, cap_aa,
                                        d.new(A.GENE_DTYPE.itemsize * cap_gene), d_aa, d_as, d_al, d_off, **gene)
            rec_off = ctx.download(d_off, (n_rec + 1,), np.uint64)
            ggoff = np.ascontiguousarray(rec_off[goff.astype(np.int64)], np.uint64)            # the first gene of every genome
            if n_gene:
                aa_len = ctx.download(d_al, (n_gene,), np.uint64)
                csum = np.concatenate([[0], np.cumsum(aa_len.astype(np.int64))])
                d_sig = d.new(ng * m * sig.dtype.itemsize)
                A.check(ctx.L.gs_sketch_batch_dev(ctx.h, A.C.byref(sk.params.c), d_aa, (cap_aa + 8) // 8 * 8, d_as, d_al, n_gene, d.up(ggoff), ng, d_sig))
                sig[f0:f0 + ng] = ctx.download(d_sig, (ng, m), sig.dtype)
                g0 = ggoff.astype(np.int64)
                nrec[f0:f0 + ng] = g0[1:] - g0[:-1]
                nsym[f0:f0 + ng] = csum[g0[1:]] - csum[g0[:-1]]
        st["device_s"] += time.perf_counter() - t1
    st["wall_s"] = time.perf_counter() - t_all
    return sig, nrec, nsym, st


class _Universal:
    """the profile set and the options of a command's `universal` argument; None and False (files of extracted universal genes, sketched as they are)
    make none. The set is closed with the command when the command made it."""

    def __init__(self, universal, opts, ctx):
        self.db, self.own = None, False
        if universal is None or universal is False:
            if opts:
                raise GsError(_lib.GS_ERR_INVALID, "universal_opts without universal")
            return
        self.opts = dict(opts or {})
        unknown = sorted(set(self.opts) - set(UNIVERSAL_OPTS))
        if unknown:
            raise GsError(_lib.GS_ERR_INVALID, "universal_opts: %s; the options are %s (translate and gene are the command's own)" % (unknown, list(UNIVERSAL_OPTS)))
        self.own = not isinstance(universal, A.HmmDb)
        self.db = A._as_hmm_db(universal, ctx)

    def close(self):
        if self.own and self.db is not None:
            self.db.close()
        self.db = None

    def sidecar(self, translate, gene):
        return {"profiles": list(self.db.names), "options": dict(self.opts, translate=translate, gene=dict(gene or {}))}

    def check_against(self, db_dir, universal):
        """a directory with a sidecar takes universal genes only: of its own profiles, or files that hold them already (universal=False)"""
        path = os.path.join(db_dir, UNIVERSAL)
        if not os.path.exists(path):
            return
        with open(path, encoding="utf-8") as f:
            names = json.load(f)["profiles"]
        if universal is None:
            raise GsError(_lib.GS_ERR_INVALID, "%s is a universal-gene database (%s): give universal, or universal=False for files of extracted genes" % (db_dir, UNIVERSAL))
        if self.db is not None and list(self.db.names) != list(names):
            raise GsError(_lib.GS_ERR_INVALID, "the profiles given differ from the %d that %s was built with (%s)" % (len(names), db_dir, UNIVERSAL))


def _sketch_dir(sk, paths, block, pio, threads, translate, gene, universal=None):
    if universal is not None and universal.db is not None:
        sig, nrec, nsym, _, stats = A.universal_sketch(paths, universal.db, sk, translate=translate, gene=gene, **universal.opts)
        return sig, nrec, nsym, stats
    if translate == "genes":
        return _sketch_genes(sk, paths, gene)
    return sk.sketch_files(paths, block=block, pio=pio, threads=threads)


def _items(paths, nsym, keep, block):
    """the dictionary entries of the kept files: (path as listed, "" by sequence / "-total-sequence" with block, symbols sketched)"""
    fid = BLOCK_FASTA_ID if block else ""
    return [(paths[i], fid, int(nsym[i])) for i in keep]


def _nb_seq(nrec, keep, n_files, block):
    """files.rs:192-194: one per IdSeq a file gives - its kept records by sequence, the file itself with block"""
    return int(n_files) if block else int(sum(int(nrec[i]) for i in keep))


# ---- the database directory ----------------------------------------------------------------------------------------------------------------------
def _new_index(params, dtype, ctx, seed, insert_batch, max_layer=MAX_LAYER, extend_candidates=True, keep_pruned=False):
    h = params.hnsw
    hn = A.Hnsw(h.max_nb_conn, h.capacity, max_layer, h.ef, dtype=dtype, sketch_size=params.sketch_size, seed=seed, insert_batch=insert_batch, ctx=ctx)
    hn.modify_level_scale(h.scale_modification)               # dnasketch.rs:141
    hn.set_extend_candidates(extend_candidates)               # dnasketch.rs:159
    hn.set_keeping_pruned(keep_pruned)                        # dnasketch.rs:160
    return hn


class _Database:
    """a database directory reloaded: parameters.json, seqdict.json, processing_state.json and the index - from hnswdump.gsidx when it is there,
    otherwise from the hnsw_rs pair with a hint built from parameters.json (SPEC 17)"""

    def __init__(self, db_dir, ctx, seed=0, insert_batch=0):
        self.dir = str(db_dir)
        self.params = ProcessingParams.reload_json(self.dir)
        self.seqdict = SeqDict.reload_json(os.path.join(self.dir, "seqdict.json"))
        self.state = ProcessingState.reload_json(self.dir)
        self.sk = A.sketcher_for(A.SeqSketcherParams(self.params.kmer_size, self.params.sketch_size, self.params.algo, self.params.data_t), ctx)
        self.ctx = self.sk.ctx
        own = os.path.join(self.dir, GSIDX)
        self.source = GSIDX if os.path.exists(own) else HNSWRS
        if self.source == GSIDX:
            self.hn = A.Hnsw.load(own, ctx=self.ctx)
        else:
            self.hn = A.Hnsw.load_hnswrs(os.path.join(self.dir, HNSWRS), hint=_new_index(self.params, self.sk.sig_dtype(), self.ctx, seed, insert_batch), ctx=self.ctx)
        try:
            if self.hn.dtype != self.sk.sig_dtype() or int(self.hn.prm.m) != self.params.sketch_size:
                raise GsError(_lib.GS_ERR_INVALID, "parameters.json (%s x %d) disagrees with the dump (%s x %d)" % (
                    self.sk.sig_dtype().name, self.params.sketch_size, self.hn.dtype.name, int(self.hn.prm.m)))
            if self.hn.get_nb_point() != self.seqdict.get_nb_entries():
                raise GsError(_lib.GS_ERR_INVALID, "seqdict.json has %d entries, the dump %d points" % (self.seqdict.get_nb_entries(), self.hn.get_nb_point()))
        except Exception:
            self.hn.close()
            raise

    def close(self):
        self.hn.close()


def _dump_database(hn, out_dir, params, seqdict, state, hnswrs, truncate_255):
    """all files of a database directory -> (hnsw_rs pair written, why not)"""
    os.makedirs(out_dir, exist_ok=True)
    params.dump_json(out_dir)
    seqdict.dump(os.path.join(out_dir, "seqdict.json"))
    state.dump_json(out_dir)
    hn.file_dump(os.path.join(out_dir, GSIDX))
    base = os.path.join(out_dir, HNSWRS)
    pair = [base + ".hnsw.graph", base + ".hnsw.data"]
    written, why = False, None
    if hnswrs:
        try:
            hn.file_dump_hnswrs(base, truncate_255=truncate_255)
            written = True
        except GsError as e:
            # neighbour counts are one byte in that format: a list of more than 255 ids cannot be written, by upstream either. Left out and
            # reported - a build of an hour must not die at its last step; hnswdump.gsidx holds the whole index
            if e.code != _lib.GS_ERR_UNSUPPORTED:
                raise
            why = str(e)
    if not written:
        for p in pair:                                        # no stale or partial pair next to a newer dictionary
            if os.path.exists(p):
                os.remove(p)
    return written, why


def _report(nb_file, items, nrec, keep, skipped, stats, seconds, written, why):
    return {"nb_file": nb_file, "nb_point": len(items), "nb_record": int(sum(int(nrec[i]) for i in keep)), "sketch_stats": stats, "seconds": seconds,
            "skipped_files": skipped, "hnswrs_written": written, "hnswrs_refused": why}


def tohnsw(dir, out_dir, kmer_size, sketch_size, nbng, ef=400, algo="optdens", aa=False, block=False, scale_modify=1.0, pio=0, threads=0, seed=0,
           insert_batch=0, hnswrs=True, truncate_255=False, translate=None, ctx=None, capacity=CAPACITY, max_layer=MAX_LAYER, extend_candidates=True,
           keep_pruned=False, gene=None, universal=None, universal_opts=None):
    """`gsearch tohnsw -d dir -k -s -n --ef --algo [--aa] [--block]`: the accepted files under `dir` (recursive, name order) -> one signature per
    file that has a kept record -> ONE parallel_insert with ids = positions in the dictionary -> `out_dir` with parameters.json, seqdict.json,
    processing_state.json, hnswdump.gsidx and (hnswrs) the hnsw_rs pair. gene: gene_call parameters of translate='genes'.
    universal (SPEC 17 item 11): a profile set (path, directory, list or HmmDb) - every file's signature is that of its universal genes (universal_sketch with
    universal_opts; .faa files, or nucleotide files with translate=True / 'genes'), a file without a hit is skipped, and universal.json is written.
    Returns counts, the sketch_files statistics, seconds per stage, the files skipped and whether the pair was written."""
    t_start = time.perf_counter()
    params = ProcessingParams(HnswParams(capacity, ef, nbng, scale_modify), kmer_size, sketch_size, algo, "aa" if aa else "dna", block)
    sk = A.sketcher_for(A.SeqSketcherParams(kmer_size, sketch_size, params.algo, params.data_t), ctx)
    _check_translate(translate, params.data_t, block, universal)
    uni = _Universal(universal, universal_opts, sk.ctx)
    try:
        paths = _list(dir, params.data_t, translate)
        t_list = time.perf_counter()
        sig, nrec, nsym, stats = _sketch_dir(sk, paths, block, pio, threads, translate, gene, uni)
        sidecar = uni.sidecar(translate, gene) if uni.db is not None else None
    finally:
        uni.close()
    t_sketch = time.perf_counter()
    keep = [i for i in range(len(paths)) if int(nsym[i]) > 0]
    if not keep:
        raise GsError(_lib.GS_ERR_INVALID, "none of the %d files under %s has a kept record" % (len(paths), dir))
    seqdict = SeqDict(_items(paths, nsym, keep, block))
    hn = _new_index(params, sk.sig_dtype(), sk.ctx, seed, insert_batch, max_layer, extend_candidates, keep_pruned)
    try:
        hn.parallel_insert(sig[keep], ids=np.arange(len(keep), dtype=np.uint64))            # dnasketch.rs:421-435
        t_insert = time.perf_counter()
        state = ProcessingState(_nb_seq(nrec, keep, len(paths), block), len(paths), time.perf_counter() - t_start)
        written, why = _dump_database(hn, str(out_dir), params, seqdict, state, hnswrs, truncate_255)
        if sidecar is not None:
            with open(os.path.join(str(out_dir), UNIVERSAL), "w", encoding="utf-8") as f:
                json.dump(sidecar, f, indent=1, default=str)
                f.write("\n")
    finally:
        hn.close()
    t_dump = time.perf_counter()
    seconds = {"list": t_list - t_start, "read_sketch": t_sketch - t_list, "insert": t_insert - t_sketch, "dump": t_dump - t_insert, "wall": t_dump - t_start}
    return _report(len(paths), seqdict.items, nrec, keep, [paths[i] for i in range(len(paths)) if int(nsym[i]) == 0], stats, seconds, written, why)


def add(db_dir, new_dir, pio=0, threads=0, truncate_255=False, translate=None, ctx=None, seed=0, insert_batch=0, hnswrs=True, gene=None, universal=None,
        universal_opts=None):
    """`gsearch add -b db_dir -n new_dir`: everything but the two directories is reloaded from the database (block_flag, algo, kmer_size, data_t and
    sketch_size are the stored ones; seed / insert_batch only matter when the index comes from the hnsw_rs pair). The new files' signatures go in by
    ONE parallel_insert with ids continuing at the dictionary's length; all files of the directory are rewritten. A directory whose parameters.json
    disagrees with the dump is refused with GS_ERR_INVALID before anything is written. universal / universal_opts as tohnsw takes them; a directory that
    has universal.json refuses a call without universal and one whose profile names differ, universal=False: the files hold extracted genes already."""
    t_start = time.perf_counter()
    db = _Database(db_dir, ctx, seed, insert_batch)
    uni = None
    try:
        block = db.params.block_flag
        _check_translate(translate, db.params.data_t, block, universal)
        uni = _Universal(universal, universal_opts, db.ctx)
        uni.check_against(db.dir, universal)
        t_load = time.perf_counter()
        paths = _list(new_dir, db.params.data_t, translate)
        t_list = time.perf_counter()
        sig, nrec, nsym, stats = _sketch_dir(db.sk, paths, block, pio, threads, translate, gene, uni)
        t_sketch = time.perf_counter()
        keep = [i for i in range(len(paths)) if int(nsym[i]) > 0]
        first = db.seqdict.get_nb_entries()
        items = _items(paths, nsym, keep, block)
        if keep:
            db.hn.parallel_insert(sig[keep], ids=np.arange(first, first + len(keep), dtype=np.uint64))
        t_insert = time.perf_counter()
        seqdict = SeqDict(db.seqdict.items + items)
        state = ProcessingState(db.state.nb_seq + _nb_seq(nrec, keep, len(paths), block), db.state.nb_file + len(paths), time.perf_counter() - t_start)
        written, why = _dump_database(db.hn, db.dir, db.params, seqdict, state, hnswrs, truncate_255)
    finally:
        if uni is not None:
            uni.close()
        db.close()
    t_dump = time.perf_counter()
    seconds = {"load": t_load - t_start, "list": t_list - t_load, "read_sketch": t_sketch - t_list, "insert": t_insert - t_sketch, "dump": t_dump - t_insert,
               "wall": t_dump - t_start}
    out = _report(len(paths), items, nrec, keep, [paths[i] for i in range(len(paths)) if int(nsym[i]) == 0], stats, seconds, written, why)
    out.update(first_id=first, nb_point_total=seqdict.get_nb_entries(), index_source=db.source)
    return out


# ---- derep (SPEC 18) -----------------------------------------------------------------------------------------------------------------------------
DEREP_HEADER = "genome\trepresentative\tdistance\tani\tcluster_size"
DEREP_CLUSTERS, DEREP_REPS = "derep.clusters.tsv", "derep.representatives.txt"


def derep_clusters_text(paths, cluster_node, counts, m, kmer, model):
    """derep.clusters.tsv: the header, then one line per genome in node order: its path, the path of its representative (of its component's label
    under single linkage), the distance (f32)count / (f32)m as gsearch.neighbors.txt prints one ({:.5E}), the ANI of that distance as reformat prints
    one, the number of genomes of its cluster. counts None (single linkage): distance and ANI are `-`."""
    cluster_node = np.asarray(cluster_node, np.int64)
    size = np.bincount(cluster_node, minlength=len(paths))
    lines = [DEREP_HEADER]
    for v, r in enumerate(cluster_node.tolist()):
        if counts is None:
            d_s = a_s = "-"
        else:
            d = float(np.float32(int(counts[v])) / np.float32(m))
            d_s, a_s = A._rust_5e(d), _ani_string(d, int(kmer), int(model))
        lines.append("%s\t%s\t%s\t%s\t%d" % (paths[v], paths[r], d_s, a_s, size[r]))
    return "".join(s + "\n" for s in lines)


def derep_representatives_text(paths, reps):
    """derep.representatives.txt: the representatives' paths, one per line, in the order given (rank order)"""
    return "".join("%s\n" % paths[int(r)] for r in reps)


def derep(db_dir, ani=None, max_dist=None, model=1, linkage="greedy", priority="length", out_dir=".", ctx=None):
    """Dereplication of a database directory (SPEC 18): the directory is reloaded as `request` reloads it, its genomes are clustered at the cut and
    out_dir/derep.clusters.tsv and out_dir/derep.representatives.txt are written. The cut is `ani` (percent, through ani_cut with the database's
    k-mer size and `model`) or `max_dist` (a DistHamming distance), exactly one of them. linkage "greedy": Hnsw.derep, representatives by
    `priority` - "length": the symbols sketched per genome (seqdict.json), longer first; None: node order; or one value per node;
    linkage "single": Hnsw.components, the representative of a cluster is its first genome. On an amino-acid or universal-gene database the same
    transform gives an AAI-like cut, not an ANI. Returns the result, c_max, max_dist and the two paths."""
    if (ani is None) == (max_dist is None):
        raise GsError(_lib.GS_ERR_INVALID, "derep: give ani or max_dist, one of them")
    if linkage not in ("greedy", "single"):
        raise GsError(_lib.GS_ERR_INVALID, "derep: linkage is \"greedy\" or \"single\"")
    db = _Database(db_dir, ctx)
    try:
        items, kmer, m = db.seqdict.items, int(db.params.kmer_size), int(db.params.sketch_size)
        if ani is not None:
            max_dist = A.ani_cut(ani, kmer, model, m)[1]
        ids = db.hn.get_ids().astype(np.int64)                   # node v is entry ids[v] of the dictionary (tohnsw and add insert with ids = positions)
        if isinstance(priority, str):
            if priority != "length":
                raise GsError(_lib.GS_ERR_INVALID, "derep: priority is \"length\", None or an array")
            priority = np.array([int(items[i][2]) for i in ids], np.uint64)
        paths = [items[i][0] for i in ids]
        if linkage == "greedy":
            res = db.hn.derep(max_dist, priority)
            text = derep_clusters_text(paths, res.rep_node, res.rep_count, m, kmer, model)
            reps = res.reps
        else:
            res = db.hn.components(max_dist)
            text = derep_clusters_text(paths, res.label_node, None, m, kmer, model)
            reps = np.unique(res.label_node)
    finally:
        db.close()
    os.makedirs(str(out_dir), exist_ok=True)
    out = {"result": res, "c_max": res.c_max, "max_dist": float(max_dist), "clusters": os.path.join(str(out_dir), DEREP_CLUSTERS),
           "representatives": os.path.join(str(out_dir), DEREP_REPS)}
    with open(out["clusters"], "w", encoding="utf-8", newline="") as f:
        f.write(text)
    with open(out["representatives"], "w", encoding="utf-8", newline="") as f:
        f.write(derep_representatives_text(paths, reps))
    return out


def _write_answers(items, ids, dist, cnt, seqdict, threshold, out, matches, block):
    """the two answer files of a request: ReqAnswer.dump per request into `out` (created or truncated) and, by sequence, matcher.rs' text into
    `matches` -> (matches written by ReqAnswer.dump, lines per file)"""
    thr = float(np.float32(threshold))                        # out_threshold is an f32 compared with f32 distances (answer.rs:42,55)
    answers = [[A.Neighbour(int(ids[i, j]), float(dist[i, j])) for j in range(int(cnt[i]))] for i in range(len(items))]
    nb_match, buf = 0, io.StringIO()
    for i, item in enumerate(items):
        nb_match += A.ReqAnswer(i, item, answers[i]).dump(seqdict, thr, buf)
    text = buf.getvalue()
    with open(out, "w", encoding="utf-8", newline="") as f:
        f.write(text)
    lines = {"neighbors": text.count("\n"), "matches": None}
    if not block:                                             # gsearch.rs:926-929: the matcher is run by sequence only
        text = matches_text([(item[0], answers[i]) for i, item in enumerate(items)], seqdict, thr)
        with open(matches, "w", encoding="utf-8", newline="") as f:
            f.write(text)
        lines["matches"] = text.count("\n")
    return nb_match, lines


def request(db_dir, query_dir, nbanswers, out="gsearch.neighbors.txt", matches="gsearch.matches", ef=EF_SEARCH, threshold=OUT_THRESHOLD, pio=0, threads=0,
            translate=None, ctx=None, gene=None, universal=None, universal_opts=None):
    """`gsearch request -b db_dir -r query_dir -n nbanswers`: the query files sketched with the database's parameters and mode, ONE search_arrays over
    all of them, then per request (rank = position among the sketched query files) ReqAnswer.dump into `out` (created or truncated) and, when the
    database was built by sequence, `matches` in matcher.rs' form. Returns ids, distances, counts, evaluation counts, the request items, lines
    written and seconds per stage. universal / universal_opts as add takes them, with the same refusals on a directory that has universal.json."""
    t_start = time.perf_counter()
    db = _Database(db_dir, ctx)
    uni = None
    try:
        block = db.params.block_flag
        _check_translate(translate, db.params.data_t, block, universal)
        uni = _Universal(universal, universal_opts, db.ctx)
        uni.check_against(db.dir, universal)
        t_load = time.perf_counter()
        paths = _list(query_dir, db.params.data_t, translate)
        t_list = time.perf_counter()
        sig, nrec, nsym, stats = _sketch_dir(db.sk, paths, block, pio, threads, translate, gene, uni)
        t_sketch = time.perf_counter()
        keep = [i for i in range(len(paths)) if int(nsym[i]) > 0]
        items = _items(paths, nsym, keep, block)
        knbn = int(nbanswers)
        if keep:
            ids, dist, cnt, ev = db.hn.search_arrays(sig[keep], knbn, int(ef))
        else:
            ids, dist, cnt, ev = np.zeros((0, knbn), np.uint64), np.zeros((0, knbn), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
        seqdict = db.seqdict.items
    finally:
        if uni is not None:
            uni.close()
        db.close()
    t_search = time.perf_counter()
    nb_match, lines = _write_answers(items, ids, dist, cnt, seqdict, threshold, out, matches, block)
    t_text = time.perf_counter()
    seconds = {"load": t_load - t_start, "list": t_list - t_load, "read_sketch": t_sketch - t_list, "search": t_search - t_sketch, "text": t_text - t_search,
               "wall": t_text - t_start}
    return {"ids": ids, "distances": dist, "counts": cnt, "evals": ev, "items": items, "nb_file": len(paths), "nb_match": nb_match,
            "skipped_files": [paths[i] for i in range(len(paths)) if int(nsym[i]) == 0], "lines": lines, "sketch_stats": stats, "seconds": seconds,
            "index_source": db.source}
