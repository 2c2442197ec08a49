"""Host-side mirror of the reference's operator interface for the sketch-and-query hot path.

Names and argument meaning follow the Rust traits gsearch calls (paths relative to /root/reference):

* ``SeqSketcherParams`` / ``*HashSketch.new(params)`` / ``sketch_compressedkmer`` / ``sketch_compressedkmer_seqs``
  — kmerutils::sketching::setsketchert::SeqSketcherT, called at src/dna/dnasketch.rs:336,357,
  src/dna/dnarequest.rs:272,287, src/aa/aasketch.rs:313,329.
* ``DistHamming.eval`` — anndists::dist::DistHamming (src/dna/dnasketch.rs:72, src/bin/bindash.rs:93-99).
* ``Hnsw.new / modify_level_scale / set_extend_candidates / set_keeping_pruned / parallel_insert /
  parallel_search / get_nb_point`` — hnsw_rs::Hnsw (src/dna/dnasketch.rs:139-141,159-160,435; src/dna/dnarequest.rs:353).

Everything here is a thin ctypes shell over the C ABI (include/gsearch_amd.h); the arithmetic runs in the
HIP library. There is no CPU fallback.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import ALGO, DATA, KIND_F32, KIND_U16, KIND_U32, KIND_U64, GsError, IndexParams, SketchParams, check

KIND_DTYPE = {KIND_U16: np.dtype(np.uint16), KIND_U32: np.dtype(np.uint32), KIND_U64: np.dtype(np.uint64),
              KIND_F32: np.dtype(np.float32)}
DTYPE_KIND = {v: k for k, v in KIND_DTYPE.items()}

Neighbour = namedtuple("Neighbour", ["d_id", "distance", "p_id"], defaults=[None])   # hnsw_rs::Neighbour; gsearch reads d_id and distance (answer.rs:42,55-57); p_id = (layer, rank in layer)

# At interpreter exit the HIP runtime may already be torn down when Python finalises leftover objects: destroying device
# objects then would call into a dead runtime. After this flag is set __del__ becomes a no-op (the OS reclaims everything).
_exiting = [False]
import atexit  # noqa: E402
atexit.register(lambda: _exiting.__setitem__(0, True))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
    """One per (process, GPU): owns the HIP stream all calls are enqueued on."""

    def __init__(self, device_id=0, stream=None):
        self.L = _lib.load()
        h = C.c_void_p()
        check(self.L.gs_ctx_create(C.byref(h), device_id, stream))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if not _exiting[0]:
                self.close()
        except Exception:
            pass

    def sync(self):
        check(self.L.gs_ctx_sync(self.h))

    def release_scratch(self):
        """give back the device scratch the context keeps between calls (it grows on demand)"""
        check(self.L.gs_ctx_release_scratch(self.h))

    def device_info(self):
        ncu, hbm, name = C.c_int(), C.c_uint64(), C.create_string_buffer(128)
        check(self.L.gs_ctx_device_info(self.h, C.byref(ncu), C.byref(hbm), name, 128))
        return {"n_cu": ncu.value, "hbm_bytes": hbm.value, "name": name.value.decode()}

    def last_sketch_info(self):
        """form of the slot-min sketch kernel the last sketch call launched (include/gsearch_amd.h gs_ctx_last_sketch_info)"""
        out = np.zeros(4, np.uint32)
        check(self.L.gs_ctx_last_sketch_info(self.h, _p(out)))
        return {"filtered": bool(out[0]), "table_in_lds": bool(out[1]), "workgroups_per_genome": int(out[2]), "launches": int(out[3])}

    # stopwatch / per-family kernel timers (HIP events on the context's stream)
    def timer_start(self):
        check(self.L.gs_ctx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        check(self.L.gs_ctx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile(self, enable=True):
        check(self.L.gs_ctx_profile(self.h, int(enable)))

    def profile_read(self, family, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        check(self.L.gs_ctx_profile_read(self.h, family, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    # device memory
    def alloc(self, nbytes):
        p = C.c_void_p()
        check(self.L.gs_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr):
        check(self.L.gs_dev_free(self.h, ptr))

    def upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        check(self.L.gs_dev_upload(self.h, ptr, _p(arr), arr.nbytes))

    def download(self, ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        check(self.L.gs_dev_download(self.h, _p(out), ptr, out.nbytes))
        return out

    def memset(self, ptr, byte, nbytes):
        check(self.L.gs_dev_memset(self.h, ptr, byte, nbytes))


class Comm:
    """RCCL communicator of the path's one exchange step (include/gsearch_amd.h gs_comm_*): all-gather of the per-rank top-k blocks."""

    def __init__(self, ctx, n_ranks, rank, unique_id):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(self.L.gs_comm_create(ctx.h, int(n_ranks), int(rank), buf, C.byref(h)))
        self.h, self.n_ranks, self.rank = h, int(n_ranks), int(rank)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(_lib.load().gs_comm_unique_id(buf))
        return buf.raw

    def allgather_topk_dev(self, ids_dev, dist_dev, nq_local, knbn, all_ids_dev, all_dist_dev):
        check(self.L.gs_comm_allgather_topk_dev(self.h, ids_dev, dist_dev, nq_local, knbn, all_ids_dev, all_dist_dev))

    def allgatherv_topk_dev(self, ids_dev, dist_dev, nq_local, nq_max, knbn, all_ids_dev, all_dist_dev):
        """unequal shards: this rank's nq_local (<= nq_max, may be 0) rows -> compact concatenation in rank order; returns every rank's count"""
        counts = np.zeros(self.n_ranks, dtype=np.uint64)
        check(self.L.gs_comm_allgatherv_topk_dev(self.h, ids_dev, dist_dev, int(nq_local), int(nq_max), int(knbn), all_ids_dev, all_dist_dev, _p(counts)))
        return counts

    def allgatherv_topk_async_dev(self, ids_dev, dist_dev, nq_local, nq_max, knbn, all_ids_dev, all_dist_dev, counts_dev=None):
        """the exchange queued on the context's stream, no host round trip (gs_comm_allgatherv_topk_async_dev); wait() is the synchronising half"""
        check(self.L.gs_comm_allgatherv_topk_async_dev(self.h, ids_dev, dist_dev, int(nq_local), int(nq_max), int(knbn), all_ids_dev, all_dist_dev, counts_dev))

    def wait(self):
        """waits for the context's stream, checks the last exchange's block shapes, returns every rank's count (gs_comm_wait)"""
        counts = np.zeros(self.n_ranks, dtype=np.uint64)
        check(self.L.gs_comm_wait(self.h, _p(counts)))
        return counts

    def size(self):
        return int(self.L.gs_comm_size(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.gs_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if not _exiting[0]:
                self.close()
        except Exception:
            pass


def topk_block_bytes(nq_max, knbn):
    return int(_lib.load().gs_topk_block_bytes(int(nq_max), int(knbn)))


def topk_pack(ids, dist, nq_max):
    """host form of the exchange's block layout (gs_topk_pack): (nq_local, knbn) ids / distances -> one fixed-size block (uint8 array)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint64); dist = np.ascontiguousarray(dist, dtype=np.float32)
    nq, knbn = ids.shape
    out = np.zeros(topk_block_bytes(nq_max, knbn), dtype=np.uint8)
    check(_lib.load().gs_topk_pack(_p(ids) if nq else None, _p(dist) if nq else None, nq, int(nq_max), knbn, _p(out)))
    return out


def topk_unpack(blocks, n_ranks, nq_max, knbn):
    """n_ranks blocks back to back -> (compact ids, compact distances, counts per rank), rank order (gs_topk_unpack)"""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    counts = np.zeros(n_ranks, dtype=np.uint64)
    check(_lib.load().gs_topk_unpack(_p(blocks), int(n_ranks), int(nq_max), int(knbn), None, None, _p(counts)))
    tot = int(counts.sum())
    ids, dist = np.zeros((tot, knbn), np.uint64), np.zeros((tot, knbn), np.float32)
    check(_lib.load().gs_topk_unpack(_p(blocks), int(n_ranks), int(nq_max), int(knbn), _p(ids), _p(dist), _p(counts)))
    return ids, dist, counts


def topk_merge_dev(ctx, ids_dev, dist_dev, n_shards, nq, knbn_in, knbn_out, out_ids_dev, out_dist_dev, id_offset=None):
    """DB-sharded alternative: merge the answers of n_shards shards for the same nq queries on the device (gs_topk_merge_dev)"""
    off = None if id_offset is None else np.ascontiguousarray(id_offset, dtype=np.uint64)
    check(ctx.L.gs_topk_merge_dev(ctx.h, ids_dev, dist_dev, int(n_shards), int(nq), int(knbn_in), _p(off), int(knbn_out), out_ids_dev, out_dist_dev))


def topk_reset_dev(ctx, nq, knbn, run_ids_dev, run_dist_dev, run_count_dev, run_evals_dev=None):
    """empty running lists for Hnsw.search_merge_dev (gs_topk_reset_dev): ids UINT64_MAX, distances +inf, counts and evaluations 0"""
    check(ctx.L.gs_topk_reset_dev(ctx.h, int(nq), int(knbn), run_ids_dev, run_dist_dev, run_count_dev, run_evals_dev))


_default_ctx = None


def debug_mem_fill(byte):
    """debugging, not for production use: fill every new device allocation and every newly taken scratch slot with `byte` (0..255) from now on,
    in the whole process; None = off (include/gsearch_amd.h gs_debug_mem_fill)"""
    check(_lib.load().gs_debug_mem_fill(-1 if byte is None else int(byte)))


def debug_radix_sort(keys, endbit, ctx=None):
    """debugging, not for production use: the device radix sort of gs_radix.hip on a host array of uint64 keys, stable on bits [0, 8 * ceil(endbit / 8))
    (gs_debug_radix_sort_u64)"""
    ctx = ctx or default_context()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.empty_like(keys)
    check(ctx.L.gs_debug_radix_sort_u64(ctx.h, _p(keys), keys.size, int(endbit), _p(out)))
    return out


def debug_run_lengths(sorted_keys, ctx=None, out=None):
    """debugging, not for production use: the device run-length encoding of gs_radix.hip on a sorted host array (gs_debug_run_lengths_u64): (keys, lengths)
    of the runs. out: a (uint64, uint32) pair of contiguous arrays of len(sorted_keys) entries to write into - what comes back is their first r entries,
    and a test that filled them with a canary looks at the rest."""
    ctx = ctx or default_context()
    a = np.ascontiguousarray(sorted_keys, dtype=np.uint64)
    uniq, lengths = out if out is not None else (np.empty(a.size, np.uint64), np.empty(a.size, np.uint32))
    if not (uniq.dtype == np.uint64 and lengths.dtype == np.uint32 and uniq.shape == lengths.shape == a.shape and uniq.flags.c_contiguous and lengths.flags.c_contiguous):
        raise ValueError("debug_run_lengths: out must be contiguous uint64 and uint32 arrays as long as the input")
    r = C.c_uint64(0)
    check(ctx.L.gs_debug_run_lengths_u64(ctx.h, _p(a), a.size, _p(uniq), _p(lengths), C.byref(r)))
    return uniq[:r.value], lengths[:r.value]


def debug_scan(values, ctx=None):
    """debugging, not for production use: the one-workgroup exclusive prefix sum of gs_radix.hip on a host array of uint32 (gs_debug_scan_u32):
    (prefix sums, total)"""
    ctx = ctx or default_context()
    v = np.ascontiguousarray(values, dtype=np.uint32)
    out = np.empty_like(v)
    total = C.c_uint32(0xFFFFFFFF)
    check(ctx.L.gs_debug_scan_u32(ctx.h, _p(v), v.size, _p(out), C.byref(total)))
    return out, int(total.value)


_HAMMING_FORM_DTYPE = (np.dtype(np.float32), np.dtype(np.uint32), np.dtype(np.uint16))


def _strided_rows(a, name, dtype):
    """a C-contiguous 2-D array of padded rows: of uint32, uint64 or float32 elements (dtype None), or of uint32 words that hold elements of `dtype`
    (a pitch that is no whole number of 8-byte elements can only be written so). Returns (array, kind, row pitch in bytes)."""
    dt = np.dtype(a.dtype if dtype is None else dtype) if isinstance(a, np.ndarray) else None
    if not (dt in DTYPE_KIND and dt != np.uint16 and a.ndim == 2 and a.flags.c_contiguous and (dtype is None or a.dtype == np.uint32)):
        raise ValueError("%s: a C-contiguous 2-D array of uint32, uint64 or float32 rows, or of uint32 words with dtype= given" % name)
    return a, DTYPE_KIND[dt], a.shape[1] * a.dtype.itemsize


def debug_hamming_strided(q, c, m, out, form, shift_bytes=0, dtype=None, ctx=None):
    """debugging, not for production use: the dense DistHamming driver of gs_hamming.hip on host rows (gs_debug_hamming_strided). q, c: 2-D arrays of one
    dtype (uint32, uint64, float32) whose rows are the padded rows - the first m columns count, the row pitch is the array's width - or, with dtype
    given, arrays of uint32 words that hold such rows. out: (nq, ld_out)
    array of float32 (form 0, distances), uint32 (form 1, counts) or uint16 (form 2), written in place in its first nc columns. Returns the number of
    K parts the call used."""
    ctx = ctx or default_context()
    q, kind, sq = _strided_rows(q, "debug_hamming_strided", dtype)
    c, kind_c, sc = _strided_rows(c, "debug_hamming_strided", dtype)
    if kind != kind_c or not (0 <= int(form) <= 2):
        raise ValueError("debug_hamming_strided: q and c of one dtype, form 0, 1 or 2")
    if not (isinstance(out, np.ndarray) and out.ndim == 2 and out.flags.c_contiguous and out.dtype == _HAMMING_FORM_DTYPE[form] and out.shape[0] == q.shape[0]):
        raise ValueError("debug_hamming_strided: out must be a C-contiguous (nq, ld_out) array of the form's dtype")
    parts = C.c_uint32(0)
    check(ctx.L.gs_debug_hamming_strided(ctx.h, kind, int(m), _p(q), q.shape[0], sq, _p(c), c.shape[0], sc, int(shift_bytes), int(form), _p(out), out.shape[1],
                                         C.byref(parts)))
    return int(parts.value)


def debug_hamming_blocks(q, c, m, items, qlist, clist, n_thin, out16, dtype=None, ctx=None):
    """debugging, not for production use: the work-list DistHamming driver of gs_hamming.hip on host rows (gs_debug_hamming_blocks). q, c as for
    debug_hamming_strided; items: (n, 4) uint32 {first entry in qlist, query rows, first entry in clist, candidate rows}; out16: (rows of q, ld_out) uint16,
    written in place in the cells the items name. Returns the number of K parts of the tile kernel's run."""
    ctx = ctx or default_context()
    q, kind, sq = _strided_rows(q, "debug_hamming_blocks", dtype)
    c, kind_c, sc = _strided_rows(c, "debug_hamming_blocks", dtype)
    items = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, 4)
    qlist, clist = np.ascontiguousarray(qlist, dtype=np.uint32), np.ascontiguousarray(clist, dtype=np.uint32)
    if kind != kind_c:
        raise ValueError("debug_hamming_blocks: q and c of one dtype")
    if not (isinstance(out16, np.ndarray) and out16.ndim == 2 and out16.flags.c_contiguous and out16.dtype == np.uint16 and out16.shape[0] == q.shape[0]):
        raise ValueError("debug_hamming_blocks: out16 must be a C-contiguous (rows of q, ld_out) uint16 array")
    parts = C.c_uint32(0)
    check(ctx.L.gs_debug_hamming_blocks(ctx.h, kind, int(m), _p(q), q.shape[0], sq, _p(c), c.shape[0], sc, _p(items), items.shape[0], _p(qlist), qlist.size,
                                        _p(clist), clist.size, int(n_thin), _p(out16), out16.shape[1], C.byref(parts)))
    return int(parts.value)


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ----------------------------------------------------------------------------------------------------------
class SeqSketcherParams:
    """kmerutils::sketcharg::SeqSketcherParams::new(kmer_size, sketch_size, algo, data_t) (gsearch.rs:258-263)."""

    def __init__(self, kmer_size, sketch_size, algo, data_t="dna"):
        self.c = SketchParams(int(kmer_size), int(sketch_size), ALGO[algo] if isinstance(algo, str) else int(algo),
                              DATA[data_t] if isinstance(data_t, str) else int(data_t))
        check(_lib.load().gs_check_params(C.byref(self.c)))

    def get_kmer_size(self):
        return self.c.k

    def get_sketch_size(self):
        return self.c.sketch_size

    def sig_kind(self):
        return _lib.load().gs_sig_kind(C.byref(self.c))

    def sig_dtype(self):
        return KIND_DTYPE[self.sig_kind()]


def pack_dna_records(records):
    """ASCII records -> (packed 2-bit buffer, rec_start, rec_len); each record starts on a byte boundary.
    Same filtering as Sequence::encode_and_add (dnafiles.rs:70-71): non-ACGT dropped, case folded."""
    L = _lib.load()
    total = sum(len(r) for r in records) + 4 * len(records)
    packed = np.zeros(total // 4 + 64, dtype=np.uint8)
    starts = np.zeros(len(records), dtype=np.uint64)
    lens = np.zeros(len(records), dtype=np.uint64)
    off = 0
    for i, r in enumerate(records):
        a = np.frombuffer(r, dtype=np.uint8)
        n = L.gs_pack_dna(_p(a) if len(a) else None, len(a), _p(packed), off)
        starts[i], lens[i] = off, n
        off += (n + 3) // 4 * 4
    return packed[: (off + 3) // 4 + 8], starts, lens


def filter_aa_records(records):
    L = _lib.load()
    outs = []
    starts = np.zeros(len(records), dtype=np.uint64)
    lens = np.zeros(len(records), dtype=np.uint64)
    off = 0
    for i, r in enumerate(records):
        a = np.frombuffer(r, dtype=np.uint8)
        o = np.zeros(max(len(a), 1), dtype=np.uint8)
        n = L.gs_filter_aa(_p(a) if len(a) else None, len(a), _p(o))
        outs.append(o[:n])
        starts[i], lens[i] = off, n
        off += n
    seq = np.concatenate(outs) if outs else np.zeros(0, np.uint8)
    return np.concatenate([seq, np.zeros(8, np.uint8)]), starts, lens


class _SeqSketcher:
    """Common shell of the SeqSketcherT implementations. A genome is a list of records (ASCII bytes)."""
    ALGO_NAME = None

    def __init__(self, params, ctx=None):
        if self.ALGO_NAME is not None and params.c.algo != ALGO[self.ALGO_NAME]:
            raise GsError(_lib.GS_ERR_INVALID, "params.algo does not match %s" % type(self).__name__)
        self.params = params
        self.ctx = ctx or default_context()

    @classmethod
    def new(cls, params, ctx=None):
        return cls(params, ctx)

    def sig_dtype(self):
        return self.params.sig_dtype()

    def sketch_packed(self, seq, rec_start, rec_len, genome_rec_off):
        """Lowest level: already packed input (the layout of include/gsearch_amd.h gs_sketch_batch)."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        rec_start = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rec_len = np.ascontiguousarray(rec_len, dtype=np.uint64)
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        ng = len(goff) - 1
        out = np.zeros((ng, self.params.c.sketch_size), dtype=self.sig_dtype())
        check(self.ctx.L.gs_sketch_batch(self.ctx.h, C.byref(self.params.c), _p(seq), seq.nbytes, _p(rec_start), _p(rec_len),
                                         len(rec_start), _p(goff), ng, _p(out)))
        return out

    def _pack(self, records):
        if self.params.c.data_t != DATA["aa"]:
            return pack_dna_records(records)
        return filter_aa_records(records)

    def sketch_compressedkmer_seqs(self, vseq):
        """All sequences are ONE genome -> exactly one signature (assert at dnasketch.rs:359)."""
        seq, rs, rl = self._pack(list(vseq))
        return [row for row in self.sketch_packed(seq, rs, rl, np.array([0, len(rs)], dtype=np.uint64))]

    def sketch_compressedkmer(self, vseq):
        """One signature per input sequence, in input order (assert at dnasketch.rs:338)."""
        seq, rs, rl = self._pack(list(vseq))
        return [row for row in self.sketch_packed(seq, rs, rl, np.arange(len(rs) + 1, dtype=np.uint64))]

    def sketch_files(self, paths, block=False, pio=0, threads=0):
        """the reader side of sketchandstore_dir_compressedkmer (dnasketch.rs:240-300) for a list of FASTA files (plain / gz / bz2 / xz):
        host threads read + decode + scan groups of `pio` files while the previous group crosses PCIe and the one before is packed and
        sketched. -> ((n_files, m) signatures, records kept per file, symbols sketched per file, stats dict)"""
        paths = [str(x).encode() for x in paths]
        n = len(paths)
        arr = (C.c_char_p * max(n, 1))(*paths)
        out = np.zeros((n, self.params.c.sketch_size), dtype=self.sig_dtype())
        nrec, nsym, st = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(6, np.float64)
        check(self.ctx.L.gs_sketch_files_ex(self.ctx.h, C.byref(self.params.c), arr, n, int(bool(block)), int(pio), int(threads), _p(out), _p(nrec), _p(nsym), _p(st), len(st)))
        return out, nrec[:n], nsym[:n], {"host_read_decode_scan_s": st[0], "pcie_wait_s": st[1], "device_s": st[2], "wall_s": st[3],
                                         "gz_members_inflated_on_device": int(st[4]), "gz_members_handed_back_to_host": int(st[5])}

    def sketch_genomes(self, genomes):
        """Batch form used by the drivers: genomes = list of lists of records -> (n_genomes, m) array."""
        recs, goff = [], [0]
        for g in genomes:
            recs.extend(g)
            goff.append(len(recs))
        seq, rs, rl = self._pack(recs)
        return self.sketch_packed(seq, rs, rl, np.array(goff, dtype=np.uint64))


def is_fasta_file(path, data_t="dna"):
    """files.rs:117-146 is_fasta_dna_file / is_fasta_aa_file"""
    return bool(_lib.load().gs_is_fasta_file(str(path).encode(), DATA[data_t] if isinstance(data_t, str) else int(data_t)))


def read_fasta_file(path):
    """file_to_buffer + needletail's transparent gz / bz2 / xz decoding (files.rs:220-250): the decompressed text as bytes"""
    L = _lib.load()
    p, n = C.c_void_p(), C.c_uint64()
    check(L.gs_read_fasta_file(str(path).encode(), C.byref(p), C.byref(n)))
    try:
        return C.string_at(p, n.value)
    finally:
        L.gs_host_free(p)


def gunzip_batch(ctx, members, out_caps=None):
    """gzip members (bytes objects, one single-member file each) inflated on the device (gs_inflate.hip): list of (status, text bytes).
    status 0 = the deflate data, ISIZE and CRC-32 all check; see gs_gunzip_batch in include/gsearch_amd.h for the others."""
    n = len(members)
    if n == 0:
        return []
    ins = [np.frombuffer(m, dtype=np.uint8) if len(m) else np.zeros(1, np.uint8) for m in members]
    caps = [int(c) for c in out_caps] if out_caps is not None else [
        (int.from_bytes(m[-4:], "little") if len(m) >= 18 else 0) for m in members]
    outs = [np.empty(max(c, 1) + 64, dtype=np.uint8) for c in caps]
    pin = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    pout = (C.c_void_p * n)(*[a.ctypes.data for a in outs])
    lin = (C.c_uint64 * n)(*[len(m) for m in members])
    cap = (C.c_uint64 * n)(*caps)
    lout = (C.c_uint64 * n)()
    st = (C.c_int * n)()
    check(ctx.L.gs_gunzip_batch(ctx.h, pin, lin, n, pout, cap, lout, st))
    return [(int(st[i]), outs[i][:lout[i]].tobytes()) for i in range(n)]


def list_fasta_files(directory, data_t="dna"):
    """recursive directory walk of process_dir (files.rs:148-215): accepted files in name order"""
    L = _lib.load()
    dt = DATA[data_t] if isinstance(data_t, str) else int(data_t)
    n, nb = C.c_uint64(), C.c_uint64()
    check(L.gs_list_fasta_files(str(directory).encode(), dt, None, 0, C.byref(n), C.byref(nb)))
    buf = C.create_string_buffer(max(nb.value, 1))
    check(L.gs_list_fasta_files(str(directory).encode(), dt, buf, nb.value, C.byref(n), C.byref(nb)))
    return [x.decode() for x in buf.raw[:nb.value].split(b"\0") if x]


def fasta_scan(text, skip_capsid=True):
    """record boundaries of a FASTA text (bytes): list of (id, seq_begin, seq_end) — the reader side of dnafiles.rs:43-193"""
    L = _lib.load()
    buf = np.frombuffer(text, dtype=np.uint8)
    n = C.c_uint64()
    check(L.gs_fasta_scan(_p(buf) if len(buf) else None, len(buf), int(skip_capsid), 0, None, None, None, None, C.byref(n)))
    nr = n.value
    sb, se, ib = np.zeros(nr, np.uint64), np.zeros(nr, np.uint64), np.zeros(nr, np.uint64)
    il = np.zeros(nr, np.uint32)
    check(L.gs_fasta_scan(_p(buf) if len(buf) else None, len(buf), int(skip_capsid), nr, _p(sb), _p(se), _p(ib), _p(il), C.byref(n)))
    return [(bytes(text[int(ib[i]):int(ib[i]) + int(il[i])]).decode("ascii", "replace"), int(sb[i]), int(se[i])) for i in range(nr)]


def sketch_fasta_files(sketcher, files, skip_capsid=True):
    """files: list of FASTA texts (bytes), one genome each -> ((n_files, m) signatures, (rec_start, rec_len, packed)).
    Record splitting on the host, filtering + 2-bit packing + sketching on the device; one signature per file, k-mers never
    span records (by-sequence mode, dnasketch.rs:348-363)."""
    ctx, L = sketcher.ctx, sketcher.ctx.L
    text = b"".join(files)
    offs = np.cumsum([0] + [len(f) for f in files])
    sb, se, goff = [], [], [0]
    for fi, f in enumerate(files):
        recs = fasta_scan(f, skip_capsid)
        for _, b, e in recs:
            sb.append(int(offs[fi]) + b)
            se.append(int(offs[fi]) + e)
        goff.append(len(sb))
    nrec = len(sb)
    sb, se = np.array(sb, dtype=np.uint64), np.array(se, dtype=np.uint64)
    tbuf = np.frombuffer(text, dtype=np.uint8)
    d_text = ctx.alloc(len(tbuf) + 64)
    pbytes = len(tbuf) // 4 + 8 * nrec + 128
    d_packed = ctx.alloc(pbytes)
    try:
        ctx.upload(d_text, tbuf)
        ctx.memset(d_packed, 0, pbytes)
        rs, rl = np.zeros(max(nrec, 1), np.uint64), np.zeros(max(nrec, 1), np.uint64)
        check(L.gs_pack_fasta_dev(ctx.h, d_text, len(tbuf), _p(sb), _p(se), nrec, d_packed, _p(rs), _p(rl)))
        m = sketcher.params.c.sketch_size
        ng = len(files)
        goff = np.array(goff, dtype=np.uint64)
        d_rs, d_rl, d_go = ctx.alloc(8 * max(nrec, 1)), ctx.alloc(8 * max(nrec, 1)), ctx.alloc(8 * (ng + 1))
        d_sig = ctx.alloc(ng * m * sketcher.sig_dtype().itemsize)
        try:
            ctx.upload(d_rs, rs); ctx.upload(d_rl, rl); ctx.upload(d_go, goff)
            check(L.gs_sketch_batch_dev(ctx.h, C.byref(sketcher.params.c), d_packed, pbytes // 8 * 8, d_rs, d_rl, nrec, d_go, ng, d_sig))
            out = ctx.download(d_sig, (ng, m), sketcher.sig_dtype())
        finally:
            for p_ in (d_rs, d_rl, d_go, d_sig):
                ctx.free(p_)
        return out, (rs[:nrec], rl[:nrec], ctx.download(d_packed, (pbytes,), np.uint8))
    finally:
        ctx.free(d_text)
        ctx.free(d_packed)


class OptDensHashSketch(_SeqSketcher):
    ALGO_NAME = "optdens"


class RevOptDensHashSketch(_SeqSketcher):
    ALGO_NAME = "revoptdens"


class ProbHash3aSketch(_SeqSketcher):
    ALGO_NAME = "prob"


class SuperHashSketch(_SeqSketcher):
    ALGO_NAME = "super"


class SuperHash2Sketch(_SeqSketcher):
    ALGO_NAME = "super2"


class HyperLogLogSketch(_SeqSketcher):
    """kmerutils HyperLogLogSketch<Kmer, u16>: SetSketch registers with SetSketchParams::default() + set_m(sketch_size)
    (dnasketch.rs:541-574, aasketch.rs:481-500)"""
    ALGO_NAME = "hll"


class HyperMinHashSketch(_SeqSketcher):
    """hyperminhash::Sketch as hypermash builds it (src/bin/hypermash.rs:115-250): 16384 u16 registers of canonical DNA k-mers, k in 1..32
    (15 accepted). Arithmetic: SPEC 7. `HyperMinHashSketch.new(SeqSketcherParams(k, 16384, "hmh"))` or `HyperMinHashSketch.for_k(k)`."""
    ALGO_NAME = "hmh"

    @classmethod
    def for_k(cls, k, ctx=None):
        return cls(SeqSketcherParams(k, _lib.HMH_REGISTERS, "hmh"), ctx)

    def sketch_files(self, paths, threads=0):
        """one sketch per file with hypermash's reader rules: FASTA or FASTQ (plain / gz / bz2 / xz; zstd is refused), no capsid filter,
        records of <= k bases skipped. -> ((n_files, 16384) uint16, records kept per file, bases sketched per file, stats dict)"""
        paths = [str(x).encode() for x in paths]
        n = len(paths)
        arr = (C.c_char_p * max(n, 1))(*paths)
        out = np.zeros((n, _lib.HMH_REGISTERS), dtype=np.uint16)
        nrec, nb, st = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(4, np.float64)
        check(self.ctx.L.gs_hmh_sketch_files(self.ctx.h, self.params.c.k, arr, n, int(threads), _p(out), _p(nrec), _p(nb), _p(st)))
        return out, nrec[:n], nb[:n], {"host_read_decode_scan_s": st[0], "pcie_wait_s": st[1], "device_s": st[2], "wall_s": st[3]}


def sketcher_for(params, ctx=None):
    """(algo) dispatch of dna_process_tohnsw (dnasketch.rs:493-644); hmh: hypermash's sketcher."""
    table = {ALGO["optdens"]: OptDensHashSketch, ALGO["revoptdens"]: RevOptDensHashSketch, ALGO["prob"]: ProbHash3aSketch,
             ALGO["super"]: SuperHashSketch, ALGO["super2"]: SuperHash2Sketch, ALGO["hll"]: HyperLogLogSketch, ALGO["hmh"]: HyperMinHashSketch}
    return table[params.c.algo](params, ctx)


def _hmh_rows(a):
    a = np.ascontiguousarray(a, dtype=np.uint16)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != _lib.HMH_REGISTERS:
        raise GsError(_lib.GS_ERR_INVALID, "HyperMinHash sketches have %d registers" % _lib.HMH_REGISTERS)
    return a


def hmh_cardinality(sigs, ctx=None):
    """Sketch::cardinality of each row of an (n, 16384) uint16 array -> uint64 array (SPEC 7, bit-exact)"""
    ctx = ctx or default_context()
    a = _hmh_rows(sigs)
    out = np.zeros(len(a), np.uint64)
    check(ctx.L.gs_hmh_cardinality(ctx.h, _p(a), len(a), _p(out)))
    return out


def hmh_cardinality_dev(ctx, sigs_dev, n, card_out_dev):
    check(ctx.L.gs_hmh_cardinality_dev(ctx.h, sigs_dev, int(n), card_out_dev))


def hmh_similarity_qxc(Q, R, ctx=None):
    """Sketch::similarity of every (query, reference) pair -> (nq, nr) float64 (SPEC 7)"""
    ctx = ctx or default_context()
    q, r = _hmh_rows(Q), _hmh_rows(R)
    out = np.zeros((len(q), len(r)), np.float64)
    check(ctx.L.gs_hmh_similarity_qxc(ctx.h, _p(q), len(q), _p(r), len(r), _p(out)))
    return out


def hmh_similarity_qxc_dev(ctx, Q_dev, nq, R_dev, nr, sim_out_dev):
    check(ctx.L.gs_hmh_similarity_qxc_dev(ctx.h, Q_dev, int(nq), R_dev, int(nr), sim_out_dev))


def hypermash_distance(sim, kmer_size):
    """hypermash.rs:261-263: 1 - (2 sim / (1 + sim))^(1/k), f64"""
    return _lib.load().gs_hmh_distance(float(sim), int(kmer_size))


def fastq_scan(text):
    """record boundaries of a FASTQ text (bytes): list of (id, seq_begin, seq_end); a truncated or malformed record raises (GS_ERR_IO)"""
    L = _lib.load()
    buf = np.frombuffer(text, dtype=np.uint8)
    n = C.c_uint64()
    check(L.gs_fastq_scan(_p(buf) if len(buf) else None, len(buf), 0, None, None, None, None, C.byref(n)))
    nr = n.value
    sb, se, ib = np.zeros(nr, np.uint64), np.zeros(nr, np.uint64), np.zeros(nr, np.uint64)
    il = np.zeros(nr, np.uint32)
    check(L.gs_fastq_scan(_p(buf) if len(buf) else None, len(buf), nr, _p(sb), _p(se), _p(ib), _p(il), C.byref(n)))
    return [(bytes(text[int(ib[i]):int(ib[i]) + int(il[i])]).decode("ascii", "replace"), int(sb[i]), int(se[i])) for i in range(nr)]


def read_path_list(path):
    """hypermash.rs:103-108: the lines of a list file (line breaks stripped), blank lines dropped"""
    with open(path, "rb") as f:
        lines = f.read().decode("utf-8").split("\n")
    lines = [x[:-1] if x.endswith("\r") else x for x in lines]
    return [x for x in lines if x.strip()]


def write_hypermash_tsv(query_paths, ref_paths, dist, out):
    """hypermash.rs:265-275: `Query\tReference\tDistance`, then one row per pair with six decimals; 0 when the two paths share a file name.
    Rows query-major in the order given [CHOICE: upstream's order is a HashMap's]."""
    import os
    out.write("Query\tReference\tDistance\n")
    for i, q in enumerate(query_paths):
        qb = os.path.basename(q)
        for j, r in enumerate(ref_paths):
            d = 0.0 if qb == os.path.basename(r) else float(dist[i, j])
            out.write("%s\t%s\t%.6f\n" % (q, r, d))


def hypermash(query_paths, ref_paths, k, out, threads=0, ctx=None):
    """hypermash (src/bin/hypermash.rs): HyperMinHash sketches of every query and reference file, the similarity of every pair on the device,
    distance 1 - (2 sim / (1 + sim))^(1/k), written as upstream's TSV to `out` (a path or a text stream). A path listed twice is sketched once,
    as upstream's map does. Returns the (nq, nr) distance matrix."""
    def uniq(xs):
        seen, res = set(), []
        for x in xs:
            if x not in seen:
                seen.add(x)
                res.append(x)
        return res
    qp, rp = uniq([str(x) for x in query_paths]), uniq([str(x) for x in ref_paths])
    sk = HyperMinHashSketch.for_k(k, ctx)
    qs = sk.sketch_files(qp, threads=threads)[0]
    rs = sk.sketch_files(rp, threads=threads)[0]
    sim = hmh_similarity_qxc(qs, rs, sk.ctx) if len(qp) and len(rp) else np.zeros((len(qp), len(rp)))
    with np.errstate(invalid="ignore"):
        dist = 1.0 - np.power(2.0 * sim / (1.0 + sim), 1.0 / float(k))
    if isinstance(out, (str, bytes)) or hasattr(out, "__fspath__"):
        with open(out, "w") as f:
            write_hypermash_tsv(qp, rp, dist, f)
    else:
        write_hypermash_tsv(qp, rp, dist, out)
    return dist


# ----------------------------------------------------------------------------------------------------------
# superaai (binaux/src/bin/superaai.rs): FracMinHash / bottom-k proteome sketches and AAI (SPEC 9)
def _take_csr(L, hp, off):
    """copy a library-allocated CSR into a list of uint64 arrays and release it"""
    n = len(off) - 1
    try:
        tot = int(off[-1])
        flat = np.ctypeslib.as_array(hp, shape=(tot,)).copy() if tot else np.zeros(0, np.uint64)
    finally:
        L.gs_host_free(C.cast(hp, C.c_void_p))
    return [flat[int(off[i]):int(off[i + 1])] for i in range(n)]


def _csr(sketches):
    rows = [np.ascontiguousarray(x, dtype=np.uint64).ravel() for x in sketches]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in rows]) if rows else []
    flat = np.concatenate(rows) if rows and off[-1] else np.zeros(1, np.uint64)
    return flat, off


class FracMinHashSketch:
    """sourmash KmerMinHash as superaai builds it (superaai.rs:119-153): the `num` smallest distinct MurmurHash3 (seed 42) values of the
    k-byte windows of a proteome that pass the `scaled` threshold (SPEC 9). scaled = 0: no threshold; num = 0: no bound."""

    def __init__(self, k=7, scaled=100, num=5120, ctx=None):
        self.k, self.scaled, self.num = int(k), int(scaled), int(num)
        self.ctx = ctx or default_context()

    def max_hash(self):
        return frac_max_hash(self.scaled)

    def sketch_genomes(self, genomes):
        """genomes: list of lists of records (bytes; '\\n' and '\\r' are dropped, every other byte kept) -> list of ascending uint64 arrays"""
        recs, goff = [], [0]
        for g in genomes:
            recs.extend(bytes(r) for r in g)
            goff.append(len(recs))
        lens = np.array([len(r) for r in recs], dtype=np.uint64)
        end = np.cumsum(lens).astype(np.uint64) if len(recs) else np.zeros(0, np.uint64)
        beg = (end - lens).astype(np.uint64)
        text = np.frombuffer(b"".join(recs) + b"\0", dtype=np.uint8)
        goff = np.array(goff, dtype=np.uint64)
        off = np.zeros(len(goff), np.uint64)
        hp = C.POINTER(C.c_uint64)()
        check(self.ctx.L.gs_frac_sketch_batch(self.ctx.h, self.k, self.scaled, self.num, _p(text), len(text) - 1, _p(beg), _p(end), len(recs), _p(goff),
                                              len(goff) - 1, C.byref(hp), _p(off)))
        return _take_csr(self.ctx.L, hp, off)

    def sketch_files(self, paths, threads=0, return_stats=False):
        """one sketch per file with superaai's reader rules: FASTA or FASTQ (plain / gz / bz2 / xz; zstd is refused), no capsid or length
        filter -> list of ascending uint64 arrays (and, with return_stats, records and residues per file and a stats dict)"""
        paths = [str(x).encode() for x in paths]
        n = len(paths)
        arr = (C.c_char_p * max(n, 1))(*paths)
        off = np.zeros(n + 1, np.uint64)
        nrec, nb, st = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(4, np.float64)
        hp = C.POINTER(C.c_uint64)()
        check(self.ctx.L.gs_frac_sketch_files(self.ctx.h, self.k, self.scaled, self.num, arr, n, int(threads), C.byref(hp), _p(off), _p(nrec), _p(nb), _p(st)))
        sk = _take_csr(self.ctx.L, hp, off)
        if return_stats:
            return sk, nrec[:n], nb[:n], {"host_read_decode_scan_s": st[0], "pcie_wait_s": st[1], "device_s": st[2], "wall_s": st[3]}
        return sk


def frac_max_hash(scaled):
    """sourmash max_hash_for_scaled (SPEC 9)"""
    return int(_lib.load().gs_frac_max_hash(int(scaled)))


def frac_similarity_qxc(Q, R, num, return_counts=False, ctx=None):
    """sourmash similarity of every (query, reference) pair of ascending sketches -> (nq, nr) float64; with return_counts also the
    (nq, nr) uint32 arrays of |A n B n U| and |U| (SPEC 9)"""
    ctx = ctx or default_context()
    q, qo = _csr(Q)
    r, ro = _csr(R)
    nq, nr = len(qo) - 1, len(ro) - 1
    sim = np.zeros((nq, nr), np.float64)
    com = np.zeros((nq, nr), np.uint32) if return_counts else None
    uni = np.zeros((nq, nr), np.uint32) if return_counts else None
    check(ctx.L.gs_frac_similarity_qxc(ctx.h, int(num), _p(q), _p(qo), nq, _p(r), _p(ro), nr, _p(sim), _p(com), _p(uni)))
    return (sim, com, uni) if return_counts else sim


def frac_similarity_qxc_dev(ctx, num, Q_dev, q_off_dev, nq, R_dev, r_off_dev, nr, sim_out_dev, common_out_dev=None, union_out_dev=None):
    check(ctx.L.gs_frac_similarity_qxc_dev(ctx.h, int(num), Q_dev, q_off_dev, int(nq), R_dev, r_off_dev, int(nr), sim_out_dev, common_out_dev, union_out_dev))


def aai(sim, k):
    """superaai.rs:159: 1 + ln(2 sim / (1 + sim)) / k, f64 with the C library's log"""
    return _lib.load().gs_aai(float(sim), int(k))


def read_list_lines(path):
    """superaai.rs:97-113 (BufRead::lines().filter_map(Result::ok)): '\\n' or '\\r\\n' stripped, a last line without a terminator kept, a line
    that is not UTF-8 dropped, a blank line KEPT"""
    with open(path, "rb") as f:
        data = f.read()
    lines = data.split(b"\n")
    last = lines.pop()                      # what follows the last '\\n': a line without a terminator, kept as it is (a '\\r' included)
    out = []
    for x in lines + ([last] if last else []):
        if x is not last and x.endswith(b"\r"):
            x = x[:-1]
        try:
            out.append(x.decode("utf-8"))
        except UnicodeDecodeError:
            continue
    return out


def write_superaai(out, query_paths, ref_paths, sim, k):
    """superaai.rs:160,165: `q\\tr\\t{sim}\\t{aai}` per pair, query-major, joined by '\\n', no trailing newline, Rust Display of f64"""
    qp = [str(x).encode() for x in query_paths]
    rp = [str(x).encode() for x in ref_paths]
    sim = np.ascontiguousarray(sim, dtype=np.float64).reshape(len(qp), len(rp))
    qa, ra = (C.c_char_p * max(len(qp), 1))(*qp), (C.c_char_p * max(len(rp), 1))(*rp)
    check(_lib.load().gs_superaai_write(str(out).encode(), qa, len(qp), ra, len(rp), _p(sim), int(k)))


def superaai(query_list, ref_list, out, k=7, scaled=100, sketch=5120, threads=0, ctx=None):
    """superaai (binaux/src/bin/superaai.rs): list files of query and reference proteomes in, upstream's text at `out` (a path). Each distinct
    file is sketched once; the similarity of every pair runs on the device. A blank line of a list is a path: the call then fails with
    GS_ERR_IO before anything is written. Returns the (nq, nr) similarity matrix."""
    import os
    qp, rp = read_list_lines(query_list), read_list_lines(ref_list)
    for x in qp + rp:
        if not os.path.isfile(x):
            raise GsError(_lib.GS_ERR_IO, "cannot open %r" % x)
    uniq = list(dict.fromkeys(qp + rp))
    sk = FracMinHashSketch(k, scaled, sketch, ctx)
    sks = sk.sketch_files(uniq, threads=threads) if uniq else []
    at = {p: sks[i] for i, p in enumerate(uniq)}
    if qp and rp:
        sim = frac_similarity_qxc([at[x] for x in qp], [at[x] for x in rp], sketch, ctx=sk.ctx)
    else:
        sim = np.zeros((len(qp), len(rp)), np.float64)
    write_superaai(out, qp, rp, sim, k)
    return sim


# ---- superani (binaux/src/bin/superani.rs; SPEC 12) -------------------------------------------------------------------------------------
AniGenome = namedtuple("AniGenome", ["seeds", "bases"])     # seeds: (n, 4) uint32 {value, contig, pos, fwd} in position order; bases: kept bases of all records


class AniSketcher:
    """FracMinHash seeds of genomes for the seed-chaining ANI (SPEC 12): every canonical k-mer whose mixed value is <= (2^64-1) / c, in position order."""

    def __init__(self, k=16, c=30, ctx=None):
        self.k, self.c = int(k), int(c)
        self.ctx = ctx or default_context()

    def sketch_packed(self, seq, rec_start, rec_len, genome_rec_off):
        """already packed input (the layout of gs_sketch_batch) -> list of AniGenome"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        ng = len(goff) - 1
        off = np.zeros(ng + 1, np.uint64)
        hp = C.POINTER(C.c_uint32)()
        check(self.ctx.L.gs_ani_sketch_batch(self.ctx.h, self.k, self.c, _p(seq) if seq.nbytes else None, seq.nbytes, _p(rs) if len(rs) else None,
                                             _p(rl) if len(rl) else None, len(rs), _p(goff), ng, C.byref(hp), _p(off)))
        try:
            tot = int(off[-1])
            flat = np.ctypeslib.as_array(hp, shape=(tot * 4,)).copy().reshape(tot, 4) if tot else np.zeros((0, 4), np.uint32)
        finally:
            self.ctx.L.gs_host_free(C.cast(hp, C.c_void_p))
        return [AniGenome(flat[int(off[g]):int(off[g + 1])], int(rl[int(goff[g]):int(goff[g + 1])].sum())) for g in range(ng)]

    def sketch_genomes(self, genomes):
        """genomes: list of lists of records (ASCII bytes; everything but ACGT / acgt is dropped) -> list of AniGenome"""
        recs, goff = [], [0]
        for g in genomes:
            recs.extend(bytes(r) for r in g)
            goff.append(len(recs))
        seq, rs, rl = pack_dna_records(recs)
        return self.sketch_packed(seq, rs, rl, np.array(goff, dtype=np.uint64))

    def sketch_files(self, paths):
        """one genome per FASTA file (plain / gz / bz2 / xz), every record kept (no capsid filter) -> list of AniGenome"""
        genomes = []
        for path in paths:
            text = read_fasta_file(path)
            genomes.append([text[sb:se] for _, sb, se in fasta_scan(text, skip_capsid=False)])
        return self.sketch_genomes(genomes)


def _ani_csr(genomes):
    rows = [np.ascontiguousarray(g.seeds if isinstance(g, AniGenome) else g, dtype=np.uint32).reshape(-1, 4) for g in genomes]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in rows]) if rows else []
    flat = np.concatenate(rows) if rows and off[-1] else np.zeros((1, 4), np.uint32)
    return np.ascontiguousarray(flat), off


def ani_pairs(Q, R, pairs=None, k=16, max_block_anchors=0, ctx=None):
    """the eight integers {n_anchors, n_chains_kept, M_q, C_q, A_q, M_r, C_r, A_r} of SPEC 12 for every listed (query index, reference index);
    pairs = None: every pair, reference-major. Q, R: lists of AniGenome (or of (n, 4) seed arrays) -> (n_pairs, 8) uint64"""
    ctx = ctx or default_context()
    q, qo = _ani_csr(Q)
    r, ro = _ani_csr(R)
    if pairs is None:
        pairs = [(iq, ir) for ir in range(len(R)) for iq in range(len(Q))]
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    pq, pr = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    out = np.zeros((len(pairs), 8), np.uint64)
    check(ctx.L.gs_ani_pairs(ctx.h, int(k), _p(q), _p(qo), len(qo) - 1, _p(r), _p(ro), len(ro) - 1, _p(pq) if len(pq) else None, _p(pr) if len(pr) else None,
                             len(pairs), _p(out) if len(pairs) else None, int(max_block_anchors)))
    return out


def ani_estimate(counts, bases_q, bases_r, k=16):
    """SPEC 12 closed form: (n, 8) integers and the kept bases of both genomes of each pair -> (n, 3) float32 {ani, af_q, af_r}"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1, 8)
    bq = np.ascontiguousarray(np.broadcast_to(np.asarray(bases_q, dtype=np.uint64), (len(counts),)))
    br = np.ascontiguousarray(np.broadcast_to(np.asarray(bases_r, dtype=np.uint64), (len(counts),)))
    out = np.zeros((len(counts), 3), np.float32)
    check(_lib.load().gs_ani_estimate(_p(counts) if len(counts) else None, _p(bq) if len(counts) else None, _p(br) if len(counts) else None, len(counts), int(k),
                                      _p(out) if len(counts) else None))
    return out


def _rust_f32(x):
    """Rust's Display of an f32: the shortest digits that read back to the same f32, positional, no trailing `.0`"""
    return np.format_float_positional(np.float32(x), unique=True, trim="-")


def write_superani(out, query_paths, ref_paths, est):
    """superani.rs:109-145: `query\tref\tani\taf_query\taf_ref\n` per pair, reference-major then query, both in list order (SPEC 12).
    est: (n_ref, n_query, 3) float32 {ani, af_q, af_r}"""
    est = np.asarray(est, dtype=np.float32).reshape(len(ref_paths), len(query_paths), 3)
    with open(out, "wb") as f:
        for j, r in enumerate(ref_paths):
            for i, q in enumerate(query_paths):
                f.write(("%s\t%s\t%s\t%s\t%s\n" % (q, r, _rust_f32(est[j, i, 0]), _rust_f32(est[j, i, 1]), _rust_f32(est[j, i, 2]))).encode("utf-8"))


def superani(query_list, ref_list, out, k=16, c=30, ctx=None):
    """superani (binaux/src/bin/superani.rs): list files of query and reference genomes in, its text at `out` (a path). Each distinct file is
    sketched once; anchors, chaining and the per-side counts of every pair run on the device. Returns the (n_ref, n_query, 3) estimates."""
    import os
    qp, rp = read_list_lines(query_list), read_list_lines(ref_list)
    for x in qp + rp:
        if not os.path.isfile(x):
            raise GsError(_lib.GS_ERR_IO, "cannot open %r" % x)
    uniq = list(dict.fromkeys(qp + rp))
    sk = AniSketcher(k, c, ctx)
    gs = sk.sketch_files(uniq) if uniq else []
    at = {p: gs[i] for i, p in enumerate(uniq)}
    Q, R = [at[x] for x in qp], [at[x] for x in rp]
    if Q and R:
        counts = ani_pairs(Q, R, None, k=k, ctx=sk.ctx)
        est = ani_estimate(counts, [g.bases for _ in R for g in Q], [g.bases for g in R for _ in Q], k).reshape(len(R), len(Q), 3)
    else:
        est = np.zeros((len(R), len(Q), 3), np.float32)
    write_superani(out, qp, rp, est)
    return est


# ---- hmmsearch (`hmmsearch_rs -f proteome.faa -m profile.HMM`; SPEC 13) ------------------------------------------------------------------
def hmm_parse(text, model=0):
    """model number `model` of a HMMER3 ASCII text (bytes) -> (info dict, int32 [27][M + 1] tables, number of models in the text); host only"""
    L = _lib.load()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    info, n = _lib.HmmInfoC(), C.c_uint32()
    check(L.gs_hmm_parse_mem(_p(buf) if len(buf) else None, len(buf), int(model), C.byref(info), None, 0, C.byref(n)))
    tab = np.zeros((_lib.HMM_TABLE_ROWS, info.M + 1), np.int32)
    check(L.gs_hmm_parse_mem(_p(buf), len(buf), int(model), None, _p(tab), tab.size, None))
    return _hmm_info(info), tab, n.value


def _hmm_info(i):
    pair = lambda v, bit: (v[0], v[1]) if i.flags & bit else None
    return {"name": i.name.decode(), "acc": i.acc.decode(), "M": int(i.M), "ga": pair(i.ga, _lib.HMM_HAS_GA), "tc": pair(i.tc, _lib.HMM_HAS_TC),
            "nc": pair(i.nc, _lib.HMM_HAS_NC), "mu": i.mu if i.flags & _lib.HMM_HAS_STATS else None, "lam": i.lam if i.flags & _lib.HMM_HAS_STATS else None,
            "ga_units": int(i.ga_units) if i.flags & _lib.HMM_HAS_GA else None, "tbm": int(i.tbm)}


def hmm_specials(L, M):
    """(tloop, tmove, null, tBM, nloop, nmove) in units for a target of L residues and a profile of M nodes (SPEC 13); host only"""
    out = np.zeros(6, np.int32)
    check(_lib.load().gs_hmm_specials(int(L), int(M), _p(out)))
    return tuple(int(x) for x in out)


def hmm_bits(raw):
    return _lib.load().gs_hmm_bits(int(raw))


def hmm_evalue(bits, mu, lam, n_targets):
    """E = n_targets * P(score >= bits) under the Gumbel of a profile's STATS LOCAL VITERBI line"""
    return _lib.load().gs_hmm_evalue(float(bits), float(mu), float(lam), float(n_targets))


def hmm_forward_evalue(bits, tau, lam, n_targets):
    """E = n_targets * P with P = 1 below tau, exp(-lam (bits - tau)) above: the exponential tail of a profile's STATS LOCAL FORWARD line (SPEC 13.1)"""
    return _lib.load().gs_hmm_forward_evalue(float(bits), float(tau), float(lam), float(n_targets))


def hmm_logsum_table():
    """T of SPEC 13.1 as the library holds it: uint16 [5903]; host only"""
    out = np.zeros(_lib.HMM_LSE_N, np.uint16)
    check(_lib.load().gs_hmm_logsum_table(_p(out), out.size))
    return out


def hmm_exp2_table():
    """EXP2 of SPEC 13.6 as the library holds it: uint32 [1024], EXP2[f] = floor(65536 * 2^(-f / 1024) + 1/2); host only"""
    out = np.zeros(_lib.HMM_EXP2_N, np.uint32)
    check(_lib.load().gs_hmm_exp2_table(_p(out), out.size))
    return out


def hmm_parse_stats(text, model=0):
    """({msv mu, lambda, viterbi mu, lambda, forward tau, lambda} as float64 [6], has) of model number `model` of a HMMER3 text: has bit 0 / 1 / 2 =
    the STATS LOCAL MSV / VITERBI / FORWARD line was there; host only"""
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    out, has = np.zeros(6, np.float64), C.c_uint32()
    check(_lib.load().gs_hmm_parse_stats_mem(_p(buf) if len(buf) else None, len(buf), int(model), _p(out), C.byref(has)))
    return out, has.value


def hmm_viterbi_floor(mu, lam, p=1e-3):
    """the Viterbi score in units whose Gumbel tail mass is p (SPEC 13.1): floor((mu - ln(-ln(1 - p)) / lam) * 1024 + 1/2); host only"""
    out = C.c_int32()
    check(_lib.load().gs_hmm_viterbi_floor(float(mu), float(lam), float(p), C.byref(out)))
    return out.value


def hmm_threshold_units(bits):
    """a caller's cutoff in bits -> units of 2^-10 bit: floor(bits * 1024 + 1/2)"""
    import math
    return int(math.floor(float(bits) * 1024.0 + 0.5))


def _opt(a):
    """the pointer argument of an array that may be missing or empty"""
    return _p(a) if a is not None and a.size else None


def _recs(aa, rec_start, rec_len):
    """-> the three arrays as a host form reads them (the caller holds them until it returns), and its arguments aa, rec_start, rec_len, n_rec"""
    aa, rs, rl = np.ascontiguousarray(aa, dtype=np.uint8), np.ascontiguousarray(rec_start, dtype=np.uint64), np.ascontiguousarray(rec_len, dtype=np.uint64)
    return (aa, rs, rl), (_opt(aa), _opt(rs), _opt(rl), len(rs))


def _pairs(pair_rec, pair_prof):
    """-> both lists as the call reads them and the arguments pair_rec, pair_prof, n_pairs of a host form"""
    pr, pp = np.ascontiguousarray(pair_rec, dtype=np.uint32).reshape(-1), np.ascontiguousarray(pair_prof, dtype=np.uint32).reshape(-1)
    if len(pr) != len(pp):
        raise ValueError("pair_rec and pair_prof: one entry per pair each")
    return pr, pp, (_opt(pr), _opt(pp), len(pr))


def _ali_col_off(lens, n_env, env, M):
    """col_off of gs_hmm_align: per pair room for Ld + M columns of every listed envelope; lens: the pair's record length (0: it names none), M: its
    profile's nodes"""
    max_env = env.shape[1]
    listed = np.where(np.asarray(lens, dtype=np.int64) > 0, np.minimum(n_env, max_env), 0).astype(np.int64)
    ld = np.maximum(env[:, :, 1].astype(np.int64) - env[:, :, 0] + 1, 0)                               # (a bad envelope is refused by the call)
    ld[np.arange(max_env)[None, :] >= listed[:, None]] = 0
    co = np.zeros(len(listed) + 1, np.uint64)
    co[1:] = np.cumsum(ld.sum(axis=1) + listed * np.asarray(M, dtype=np.int64))
    return co


def _ali_columns(slots, cols, co, n_env, env, M):
    """the column words of gs_hmm_align -> per pair the list of its aligned slots' (state, k, i, pp) int32 arrays"""
    out = []
    for j in range(len(slots)):
        at, per = int(co[j]), []
        for e in range(int(min(n_env[j], slots.shape[1]))):
            if not slots[j, e, 5]:                                                         # (a path has a match cell; a pair that got nothing has no slots)
                break
            w = cols[at:at + int(slots[j, e, 5:8].sum())]
            w0 = w[:, 0].astype(np.int64) & 0xFFFFFFFF
            per.append(((w0 >> 28).astype(np.int32), ((w0 >> 16) & 0xFFF).astype(np.int32), ((w0 & 0xFFFF) + 1).astype(np.int32), w[:, 1].copy()))
            at += int(env[j, e, 1]) - int(env[j, e, 0]) + 1 + int(M[j])
        out.append(per)
    return out


def _all_items(run, k):
    """got = run(8), and run again with the largest count when 8 slots a pair do not hold them all; got[k]: the counts, got[k + 1]: the items"""
    got = run(8)
    if len(got[k]) and int(got[k].max()) > got[k + 1].shape[1]:
        got = run(int(got[k].max()))
    return got


class HmmDb:
    """A set of HMMER3 profiles in device memory (SPEC 13). paths_or_dir: a directory (its *.HMM / *.hmm files in name order), one path, a list of
    paths, or - texts=True - a list of bytes objects. Profiles keep the order of the files and of the models inside each."""

    def __init__(self, paths_or_dir, ctx=None, texts=False):
        import os
        self.ctx = ctx or default_context()
        L = self.ctx.L
        h = C.c_void_p()
        if texts:
            bufs = [np.frombuffer(bytes(t), dtype=np.uint8) for t in paths_or_dir]
            ptr = (C.c_void_p * len(bufs))(*[b.ctypes.data if len(b) else None for b in bufs])
            nb = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
            check(L.gs_hmm_db_load_mem(self.ctx.h, ptr, nb, len(bufs), C.byref(h)))
            file_texts = [bytes(t) for t in paths_or_dir]
        else:
            if isinstance(paths_or_dir, (str, bytes, os.PathLike)):
                d = os.fsdecode(paths_or_dir)
                paths = sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(".hmm")) if os.path.isdir(d) else [d]
            else:
                paths = [os.fsdecode(x) for x in paths_or_dir]
            arr = (C.c_char_p * len(paths))(*[x.encode() for x in paths])
            check(L.gs_hmm_db_load(self.ctx.h, arr, len(paths), C.byref(h)))
            file_texts = []
            for x in paths:
                with open(x, "rb") as f:
                    file_texts.append(f.read())
        self.h = h
        n = C.c_uint64()
        check(L.gs_hmm_db_info(self.h, C.byref(n), None, 0))
        infos = (_lib.HmmInfoC * n.value)()
        check(L.gs_hmm_db_info(self.h, C.byref(n), infos, n.value))
        self.info = [_hmm_info(i) for i in infos]
        self.names = [i["name"] for i in self.info]
        self.acc = [i["acc"] for i in self.info]
        self.M = np.array([i["M"] for i in self.info], np.uint32)
        self.ga = np.array([i["ga"][0] if i["ga"] else np.nan for i in self.info])
        self.mu = np.array([i["mu"] if i["mu"] is not None else np.nan for i in self.info])
        self.lam = np.array([i["lam"] if i["lam"] is not None else np.nan for i in self.info])
        self.ga_units = [i["ga_units"] for i in self.info]
        # STATS LOCAL FORWARD tau / lambda of every profile (nan without the line), through gs_hmm_parse_stats_mem
        # and STATS LOCAL MSV mu / lambda (SPEC 13.3), from the same call
        fstats, mstats = [], []
        for t in file_texts:
            n_models = C.c_uint32()
            buf = np.frombuffer(t, dtype=np.uint8)
            check(L.gs_hmm_parse_mem(_p(buf), len(buf), 0, None, None, 0, C.byref(n_models)))
            for k in range(n_models.value):
                st, has = hmm_parse_stats(t, k)
                fstats.append((st[4], st[5]) if has & 4 else (np.nan, np.nan))
                mstats.append((st[0], st[1]) if has & 1 else (np.nan, np.nan))
        assert len(fstats) == len(self.info)
        self.tau = np.array([a for a, _ in fstats])
        self.lam_fwd = np.array([b for _, b in fstats])
        self.mu_msv = np.array([a for a, _ in mstats])
        self.lam_msv = np.array([b for _, b in mstats])

    def __len__(self):
        return len(self.info)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.gs_hmm_db_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if not _exiting[0]:
                self.close()
        except Exception:
            pass

    def tables(self, p):
        """int32 [27][M + 1] of profile p, nodes 1..M read back from the device"""
        tab = np.zeros((_lib.HMM_TABLE_ROWS, int(self.M[p]) + 1), np.int32)
        check(self.ctx.L.gs_hmm_db_tables(self.h, int(p), _p(tab), tab.size))
        return tab

    def consensus(self, p):
        """the consensus of profile p as bytes, a letter per node: the most probable residue of the node's match emission (SPEC 13; host only)"""
        buf = C.create_string_buffer(int(self.M[p]))
        check(self.ctx.L.gs_hmm_db_consensus(self.h, int(p), buf, len(buf)))
        return buf.raw

    def search_packed(self, aa, rec_start, rec_len):
        """residues as filter_aa_records() returns them -> int32 [n_rec, n_prof] raw scores (units of 2^-10 bit; HMM_NO_SCORE for an empty record)"""
        held, recs = _recs(aa, rec_start, rec_len)
        out = np.zeros((recs[3], len(self)), np.int32)
        check(self.ctx.L.gs_hmm_search(self.ctx.h, self.h, *recs, _opt(out)))
        return out

    def search(self, records):
        """records: protein sequences (bytes; everything outside the 20 letters is dropped, as the AA sketchers do) -> int32 [n_rec, n_prof]"""
        return self.search_packed(*filter_aa_records([bytes(r) for r in records]))

    def search_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, score_out_dev):
        check(self.ctx.L.gs_hmm_search_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), score_out_dev))

    def viterbi_floor(self, filter_p=1e-3):
        """int32 [n_prof]: per profile the Viterbi score in units below which Forward is not run (SPEC 13.1) - the score whose Gumbel tail mass under the
        profile's STATS LOCAL VITERBI line is filter_p; a profile without that line: INT32_MIN + 1, every pair that has a Viterbi score"""
        return np.array([hmm_viterbi_floor(i["mu"], i["lam"], filter_p) if i["mu"] is not None else _lib.HMM_FLOOR_ALL for i in self.info], np.int32)

    def _floor(self, filter_p, floor, msv=False):
        """the floors of a call: `floor` when given, else viterbi_floor(filter_p), or msv_floor(filter_p) with msv; None: every pair that has a score"""
        if floor is not None:
            fl = np.ascontiguousarray(floor, dtype=np.int32)
            if fl.shape != (len(self),):
                raise ValueError("%s: one int32 per profile" % ("msv_floor" if msv else "floor"))
            return fl
        return None if filter_p is None else (self.msv_floor if msv else self.viterbi_floor)(filter_p)

    def search_forward_packed(self, aa, rec_start, rec_len, filter_p=1e-3, floor=None):
        """residues as filter_aa_records() returns them -> (vit, fwd), int32 [n_rec, n_prof]: what search_packed() returns, and the Forward raw score of
        the pairs whose Viterbi score reaches the profile's floor (HMM_NO_SCORE for the others)"""
        held, recs = _recs(aa, rec_start, rec_len)
        fl = self._floor(filter_p, floor)
        vit, fwd = np.zeros((recs[3], len(self)), np.int32), np.zeros((recs[3], len(self)), np.int32)
        check(self.ctx.L.gs_hmm_search_forward(self.ctx.h, self.h, *recs, _opt(fl), _opt(vit), _opt(fwd)))
        return vit, fwd

    def search_forward(self, records, filter_p=1e-3, floor=None):
        """records as search() takes them -> (vit, fwd). Forward runs for the pairs with vit >= the profile's floor: `floor` (int32 [n_prof], units) when
        given, else viterbi_floor(filter_p); filter_p=None: every pair that has a Viterbi score"""
        return self.search_forward_packed(*filter_aa_records([bytes(r) for r in records]), filter_p=filter_p, floor=floor)

    def search_forward_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, vit_floor_dev, vit_out_dev, fwd_out_dev):
        """all device memory; vit_floor_dev None: every pair, vit_out_dev None: the Viterbi matrix is not wanted"""
        check(self.ctx.L.gs_hmm_search_forward_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), vit_floor_dev, vit_out_dev, fwd_out_dev))

    def msv_floor(self, filter_p=0.02):
        """int32 [n_prof]: per profile the MSV score in units below which Viterbi is not run (SPEC 13.3) - the score whose Gumbel tail mass under the
        profile's STATS LOCAL MSV line is filter_p (HMMER's F1 = 0.02); a profile without that line: INT32_MIN + 1, every pair that has an MSV score"""
        return np.array([hmm_viterbi_floor(m, l, filter_p) if not np.isnan(m) else _lib.HMM_FLOOR_ALL for m, l in zip(self.mu_msv, self.lam_msv)], np.int32)

    def search_msv_packed(self, aa, rec_start, rec_len):
        """residues as filter_aa_records() returns them -> int32 [n_rec, n_prof] MSV raw scores (SPEC 13.3; HMM_NO_SCORE for an empty record)"""
        held, recs = _recs(aa, rec_start, rec_len)
        out = np.zeros((recs[3], len(self)), np.int32)
        check(self.ctx.L.gs_hmm_search_msv(self.ctx.h, self.h, *recs, _opt(out)))
        return out

    def search_msv(self, records):
        """records as search() takes them -> int32 [n_rec, n_prof] MSV raw scores"""
        return self.search_msv_packed(*filter_aa_records([bytes(r) for r in records]))

    def search_msv_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, msv_out_dev):
        check(self.ctx.L.gs_hmm_search_msv_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), msv_out_dev))

    def search_filtered_packed(self, aa, rec_start, rec_len, msv_p=0.02, msv_floor=None, forward=False, filter_p=1e-3, floor=None):
        """residues as filter_aa_records() returns them -> (msv, vit) or, forward=True, (msv, vit, fwd), int32 [n_rec, n_prof] (SPEC 13.3): the MSV
        score of every pair, what search_packed() returns for the pairs whose MSV score reaches the profile's MSV floor (HMM_NO_SCORE for the others),
        and the Forward score behind that Viterbi matrix as search_forward_packed() computes it"""
        held, recs = _recs(aa, rec_start, rec_len)
        mfl = self._floor(msv_p, msv_floor, msv=True)
        fl = self._floor(filter_p, floor) if forward else None
        msv, vit = np.zeros((recs[3], len(self)), np.int32), np.zeros((recs[3], len(self)), np.int32)
        fwd = np.zeros((recs[3], len(self)), np.int32) if forward else None
        check(self.ctx.L.gs_hmm_search_filtered(self.ctx.h, self.h, *recs, _opt(mfl), _opt(fl), _opt(msv), _opt(vit), _opt(fwd)))
        return (msv, vit, fwd) if forward else (msv, vit)

    def search_filtered(self, records, msv_p=0.02, msv_floor=None, forward=False, filter_p=1e-3, floor=None):
        """records as search() takes them -> (msv, vit[, fwd]). Viterbi runs for the pairs with msv >= the profile's MSV floor: `msv_floor` (int32
        [n_prof], units) when given, else msv_floor(msv_p); msv_p=None: every pair that has an MSV score. forward, filter_p, floor: as search_forward()"""
        return self.search_filtered_packed(*filter_aa_records([bytes(r) for r in records]), msv_p=msv_p, msv_floor=msv_floor, forward=forward, filter_p=filter_p,
                                           floor=floor)

    def search_filtered_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, msv_floor_dev, vit_floor_dev, msv_out_dev, vit_out_dev, fwd_out_dev):
        """all device memory; a floor None: every pair, msv_out_dev None: the MSV matrix is not wanted, fwd_out_dev None: no Forward pass"""
        check(self.ctx.L.gs_hmm_search_filtered_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), msv_floor_dev, vit_floor_dev, msv_out_dev,
                                                    vit_out_dev, fwd_out_dev))

    def tables16(self, p):
        """int16 [27][M + 1] of profile p (SPEC 13.7): h(x) = max(-32768, (x + 1) >> 1) of every word of tables(p), nodes 1..M read back from the device"""
        tab = np.zeros((_lib.HMM_TABLE_ROWS, int(self.M[p]) + 1), np.int16)
        check(self.ctx.L.gs_hmm_db_tables16(self.h, int(p), _p(tab), tab.size))
        return tab

    def search_vit16_packed(self, aa, rec_start, rec_len):
        """residues as filter_aa_records() returns them -> int32 [n_rec, n_prof] vf, the packed int16 Viterbi filter score (SPEC 13.7): at least the
        Viterbi score of the pair, HMM_VF_OVER where the int16 cells overflow, HMM_NO_SCORE for an empty record"""
        held, recs = _recs(aa, rec_start, rec_len)
        out = np.zeros((recs[3], len(self)), np.int32)
        check(self.ctx.L.gs_hmm_search_vit16(self.ctx.h, self.h, *recs, _opt(out)))
        return out

    def search_vit16(self, records):
        """records as search() takes them -> int32 [n_rec, n_prof] vf"""
        return self.search_vit16_packed(*filter_aa_records([bytes(r) for r in records]))

    def search_vit16_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, vf_out_dev):
        check(self.ctx.L.gs_hmm_search_vit16_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), vf_out_dev))

    def vf_floor(self, forward=False, filter_p=1e-3, cutoff=None):
        """int32 [n_prof]: the floor of vf in a staged search (SPEC 13.7) - the lowest Viterbi score a later consumer looks at, so that the filter
        changes no output: viterbi_floor(filter_p) when Forward runs behind it (filter_p=None leaves nothing to cut by: ValueError), else the
        thresholds of `cutoff` when best hits are taken at one, else 0 - the score table lists raw >= 0"""
        if forward:
            if filter_p is None:
                raise ValueError("prefilter 'vit16' cuts Forward by its Viterbi floor: filter_p=None leaves nothing to cut by")
            return self.viterbi_floor(filter_p)
        return np.zeros(len(self), np.int32) if cutoff is None else self.thresholds(cutoff)

    def search_staged_packed(self, aa, rec_start, rec_len, vf_floor, msv=False, msv_p=0.02, msv_floor=None, forward=False, filter_p=1e-3, floor=None):
        """residues as filter_aa_records() returns them -> (vf, vit), with msv=True (msv, vf, vit), with forward=True fwd behind them; int32 [n_rec, n_prof]
        (SPEC 13.7): the MSV score of every pair, vf of every pair or - msv=True - of the pairs at or above the MSV floor, what search_packed() returns
        for the pairs with vf >= vf_floor (int32 [n_prof], units; None: every pair that has a vf), and the Forward score behind that Viterbi matrix as
        search_forward_packed() computes it; HMM_NO_SCORE for the pairs a stage did not run for"""
        held, recs = _recs(aa, rec_start, rec_len)
        mfl = self._floor(msv_p, msv_floor, msv=True) if msv else None
        fl = self._floor(filter_p, floor) if forward else None
        vfl = None if vf_floor is None else np.ascontiguousarray(vf_floor, dtype=np.int32)
        if vfl is not None and vfl.shape != (len(self),):
            raise ValueError("vf_floor: one int32 per profile")
        new = lambda: np.zeros((recs[3], len(self)), np.int32)      # noqa: E731
        m, vf, vit, fwd = new() if msv else None, new(), new(), new() if forward else None
        check(self.ctx.L.gs_hmm_search_staged(self.ctx.h, self.h, *recs, 1 if msv else 0, _opt(mfl), _opt(vfl), _opt(fl), _opt(m), _opt(vf), _opt(vit), _opt(fwd)))
        return ((m,) if msv else ()) + (vf, vit) + ((fwd,) if forward else ())

    def search_staged(self, records, vf_floor, msv=False, msv_p=0.02, msv_floor=None, forward=False, filter_p=1e-3, floor=None):
        """records as search() takes them -> what search_staged_packed() returns"""
        return self.search_staged_packed(*filter_aa_records([bytes(r) for r in records]), vf_floor, msv=msv, msv_p=msv_p, msv_floor=msv_floor, forward=forward,
                                         filter_p=filter_p, floor=floor)

    def search_staged_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, use_msv, msv_floor_dev, vf_floor_dev, vit_floor_dev, msv_out_dev, vf_out_dev, vit_out_dev,
                          fwd_out_dev):
        """all device memory; a floor None: every pair, msv_out_dev / vf_out_dev None: that matrix is not wanted, fwd_out_dev None: no Forward pass"""
        check(self.ctx.L.gs_hmm_search_staged_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), 1 if use_msv else 0, msv_floor_dev, vf_floor_dev,
                                                  vit_floor_dev, msv_out_dev, vf_out_dev, vit_out_dev, fwd_out_dev))

    def trace_packed(self, aa, rec_start, rec_len, pair_rec, pair_prof, max_dom=8, max_block_cells=0):
        """SPEC 13.2: the domains of the Viterbi path of the pairs (pair_rec[j], pair_prof[j]), traced back on the device -> (int32 raw [n_pairs] as
        search_packed() gives it, uint32 n_dom [n_pairs] the true number of domains, int32 dom [n_pairs, max_dom, 8]: i_from, i_to, k_from, k_to (1-based,
        inclusive), seg, n_match, n_ins, n_del of the first max_dom domains in sequence order, zeros behind them). A pair whose record is HMM_NO_HIT, empty
        or holds a byte that is no residue: HMM_NO_SCORE, 0 and zeros. max_block_cells bounds the cells whose back-pointers are alive at once (0: 2^27)"""
        held, recs = _recs(aa, rec_start, rec_len)
        pr, pp, pairs = _pairs(pair_rec, pair_prof)
        raw, nd = np.zeros(len(pr), np.int32), np.zeros(len(pr), np.uint32)
        dom = np.zeros((len(pr), int(max_dom), _lib.HMM_DOM_WORDS), np.int32)
        check(self.ctx.L.gs_hmm_trace(self.ctx.h, self.h, *recs, *pairs, int(max_dom), int(max_block_cells), _opt(raw), _opt(nd), _opt(dom)))
        return raw, nd, dom

    def trace(self, records, pairs, max_dom=8, max_block_cells=0):
        """records as search() takes them; pairs: (record, profile) index pairs -> (raw, n_dom, dom) of trace_packed()"""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return self.trace_packed(*filter_aa_records([bytes(r) for r in records]), pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32), max_dom=max_dom,
                                 max_block_cells=max_block_cells)

    def trace_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, pair_rec_dev, pair_prof_dev, n_pairs, max_dom, raw_out_dev, n_dom_out_dev, dom_out_dev,
                  max_block_cells=0):
        """all device memory; the lengths and the pair list are read back once"""
        check(self.ctx.L.gs_hmm_trace_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), pair_rec_dev, pair_prof_dev, int(n_pairs), int(max_dom),
                                          int(max_block_cells), raw_out_dev, n_dom_out_dev, dom_out_dev))

    def envelopes_packed(self, aa, rec_start, rec_len, pair_rec, pair_prof, max_env=8, rows=False, max_block_rows=0):
        """SPEC 13.4: Forward and Backward scores and the posterior envelopes of the pairs (pair_rec[j], pair_prof[j]), all on the device -> (int32 fwd
        [n_pairs] as search_forward_packed() gives it, int32 bck [n_pairs] = bN[0] - null, uint32 n_env [n_pairs] the true number of envelopes, int32 env
        [n_pairs, max_env, 4]: i_from, i_to (1-based, inclusive), env_raw, peak of the first max_env envelopes in sequence order, zeros behind them) and,
        with rows=True, two lists of per-pair int32 arrays out[1..L] and cont[1..L] in units (empty for a pair that gets no envelopes below). A pair
        whose record is HMM_NO_HIT, empty or holds a byte that is no residue: HMM_NO_SCORE, HMM_NO_SCORE, 0 and zeros. max_block_rows bounds the rows of
        the two passes that are alive at once (0: 2^25)"""
        (_, _, rl), recs = _recs(aa, rec_start, rec_len)
        pr, pp, pairs = _pairs(pair_rec, pair_prof)
        n = len(pr)
        fwd, bck, ne = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
        env = np.zeros((n, int(max_env), _lib.HMM_ENV_WORDS), np.int32)
        ro = o_rows = c_rows = None
        if rows and n:
            named = pr < len(rl)                                                    # (HMM_NO_HIT names no record; another bad index is refused below)
            lens = np.zeros(n, np.uint64)
            lens[named] = rl[pr[named]]
            ro = np.zeros(n + 1, np.uint64)
            ro[1:] = np.cumsum(lens)
            o_rows, c_rows = np.zeros(max(int(ro[-1]), 1), np.int32), np.zeros(max(int(ro[-1]), 1), np.int32)
        check(self.ctx.L.gs_hmm_envelopes(self.ctx.h, self.h, *recs, *pairs, int(max_env), int(max_block_rows), _opt(fwd), _opt(bck), _opt(ne), _opt(env), _opt(ro),
                                          _opt(o_rows), _opt(c_rows)))
        if not rows:
            return fwd, bck, ne, env
        has = fwd != _lib.HMM_NO_SCORE
        cut = lambda a: [a[int(ro[j]):int(ro[j + 1])] if has[j] else a[:0] for j in range(n)]      # noqa: E731
        return fwd, bck, ne, env, cut(o_rows) if n else [], cut(c_rows) if n else []

    def envelopes(self, records, pairs, max_env=8, rows=False, max_block_rows=0, bias=False):
        """records as search() takes them; pairs: (record, profile) index pairs -> what envelopes_packed() returns; bias=True (SPEC 13.5): followed by what
        null2_packed() returns for those envelopes, (slots, seq_bias)"""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        packed = filter_aa_records([bytes(r) for r in records])
        pr, pp = pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32)
        got = self.envelopes_packed(*packed, pr, pp, max_env=max_env, rows=rows, max_block_rows=max_block_rows)
        return got + self.null2_packed(*packed, pr, pp, got[2], got[3]) if bias else got

    def null2_packed(self, aa, rec_start, rec_len, pair_rec, pair_prof, n_env, env, n2=False, occ=False, max_block_cells=0):
        """SPEC 13.5: the null2 bias correction of the envelopes envelopes_packed() listed for the same pairs (n_env, env as it returned them; max_env is
        env's second extent), Forward and Backward over every listed envelope on the device -> (int32 slots [n_pairs, max_env, 4]: corr, dom_bias, seg_raw,
        mass of each listed envelope, zeros behind them; int32 seq_bias [n_pairs]). The corrected scores are env_raw - dom_bias and fwd - seq_bias; both
        biases are >= 0. n2=True: followed by the int32 [n_pairs, max_env, 20] null2 log-odds of the 20 residues; occ=True: followed by two lists, per pair
        the int32 [listed, M] rows occM and occI (log2 of the expected number of residues every match and insert state emits). A pair whose record is
        HMM_NO_HIT, empty or holds a byte that is no residue: zeros, seq_bias 0, no rows. When n_env exceeds max_env the sequence bias counts the listed
        envelopes only. max_block_cells bounds the cells whose Forward rows are alive at once (0: 2^26)"""
        (_, _, rl), recs = _recs(aa, rec_start, rec_len)
        pr, pp, pairs = _pairs(pair_rec, pair_prof)
        n = len(pr)
        ne = np.ascontiguousarray(n_env, dtype=np.uint32).reshape(-1)
        env = np.ascontiguousarray(env, dtype=np.int32)
        if len(ne) != n or env.ndim != 3 or env.shape[0] != n or env.shape[2] != _lib.HMM_ENV_WORDS:
            raise ValueError("n_env and env: as envelopes_packed() returns them for these pairs")
        max_env = env.shape[1]
        slots, sb = np.zeros((n, max_env, _lib.HMM_N2_WORDS), np.int32), np.zeros(n, np.int32)
        v = np.zeros((n, max_env, 20), np.int32) if n2 else None
        oo = o_m = o_i = None
        if occ and n:
            listed = np.minimum(ne, max_env).astype(np.uint64)
            M = np.where(pp < len(self), self.M[np.minimum(pp, len(self) - 1)], 0).astype(np.uint64)      # (a bad profile index is refused below)
            oo = np.zeros(n + 1, np.uint64)
            oo[1:] = np.cumsum(listed * M)
            o_m, o_i = np.zeros(max(int(oo[-1]), 1), np.int32), np.zeros(max(int(oo[-1]), 1), np.int32)
        check(self.ctx.L.gs_hmm_null2(self.ctx.h, self.h, *recs, *pairs, int(max_env), int(max_block_cells), _opt(ne), _opt(env), _opt(slots), _opt(sb), _opt(v), _opt(oo),
                                      _opt(o_m), _opt(o_i)))
        out = (slots, sb) + ((v,) if n2 else ())
        if not occ:
            return out
        residue = np.zeros(256, bool)
        residue[list(b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwy")] = True
        rs_, aa_ = np.ascontiguousarray(rec_start, dtype=np.uint64), np.ascontiguousarray(aa, dtype=np.uint8)
        has = [r < len(rl) and int(rl[r]) > 0 and bool(residue[aa_[int(rs_[r]):int(rs_[r]) + int(rl[r])]].all()) for r in pr]      # the pairs that have a score
        cut = lambda a: [a[int(oo[j]):int(oo[j + 1])].reshape(-1, int(self.M[pp[j]])) if has[j] else a[:0].reshape(0, int(self.M[pp[j]])) for j in range(n)]      # noqa: E731
        return out + ((cut(o_m), cut(o_i)) if n else ([], []))

    def null2(self, records, pairs, n_env, env, n2=False, occ=False, max_block_cells=0):
        """records as search() takes them; pairs: (record, profile) index pairs; n_env, env as envelopes() returned them -> what null2_packed() returns"""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return self.null2_packed(*filter_aa_records([bytes(r) for r in records]), pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32), n_env, env, n2=n2, occ=occ,
                                 max_block_cells=max_block_cells)

    def null2_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, pair_rec_dev, pair_prof_dev, n_pairs, max_env, n_env_dev, env_dev, slot_out_dev, seq_bias_out_dev,
                  n2_out_dev=None, occ_off_dev=None, occm_out_dev=None, occi_out_dev=None, max_block_cells=0):
        """all device memory; the lengths, the pair list, n_env, env and occ_off are read back once"""
        check(self.ctx.L.gs_hmm_null2_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), pair_rec_dev, pair_prof_dev, int(n_pairs), int(max_env),
                                          int(max_block_cells), n_env_dev, env_dev, slot_out_dev, seq_bias_out_dev, n2_out_dev, occ_off_dev, occm_out_dev, occi_out_dev))

    def align_packed(self, aa, rec_start, rec_len, pair_rec, pair_prof, n_env, env, columns=False, max_block_cells=0):
        """SPEC 13.6: the optimal-accuracy alignment of the envelopes envelopes_packed() listed for the same pairs (n_env, env as it returned them), all on
        the device -> int32 slots [n_pairs, max_env, 8]: i_from, i_to (record coordinates, 1-based, inclusive), k_from, k_to, oa, n_match, n_ins, n_del of
        each listed envelope, zeros behind them; the expected accuracy of a slot is oa / (65536 Ld). columns=True: followed by a list, per pair the list of
        its listed slots' columns (state, k, i, pp): int32 arrays of one length, state 0 M / 1 I / 2 D, node k, record row i (1-based; for D the row it sits
        in), pp = pM or pI of the cell in units (0 for D), in order from (i_from, k_from) to (i_to, k_to). A pair whose record is HMM_NO_HIT, empty or
        holds a byte that is no residue: zeros and no columns. A listed envelope of more than HMM_ALI_MAX_LD residues is refused"""
        (_, _, rl), recs = _recs(aa, rec_start, rec_len)
        pr, pp, pairs = _pairs(pair_rec, pair_prof)
        n = len(pr)
        ne = np.ascontiguousarray(n_env, dtype=np.uint32).reshape(-1)
        env = np.ascontiguousarray(env, dtype=np.int32)
        if len(ne) != n or env.ndim != 3 or env.shape[0] != n or env.shape[2] != _lib.HMM_ENV_WORDS:
            raise ValueError("n_env and env: as envelopes_packed() returns them for these pairs")
        max_env = env.shape[1]
        slots = np.zeros((n, max_env, _lib.HMM_ALI_WORDS), np.int32)
        co = cols = None
        if columns and n:
            named = pr < len(rl)                                                    # (HMM_NO_HIT names no record; another bad index is refused below)
            lens = np.zeros(n, np.int64)
            lens[named] = rl[pr[named]]
            M = np.where(pp < len(self), self.M[np.minimum(pp, len(self) - 1)], 0).astype(np.int64)       # (a bad profile index is refused below)
            co = _ali_col_off(lens, ne, env, M)
            cols = np.zeros((max(int(co[-1]), 1), 2), np.int32)
        check(self.ctx.L.gs_hmm_align(self.ctx.h, self.h, *recs, *pairs, int(max_env), int(max_block_cells), _opt(ne), _opt(env), _opt(slots), _opt(co), _opt(cols)))
        if not columns:
            return slots
        return slots, (_ali_columns(slots, cols, co, ne, env, M) if n else [])

    def align(self, records, pairs, n_env, env, columns=False, max_block_cells=0):
        """records as search() takes them; pairs: (record, profile) index pairs; n_env, env as envelopes() returned them -> what align_packed() returns"""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return self.align_packed(*filter_aa_records([bytes(r) for r in records]), pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32), n_env, env, columns=columns,
                                 max_block_cells=max_block_cells)

    def align_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, pair_rec_dev, pair_prof_dev, n_pairs, max_env, n_env_dev, env_dev, slot_out_dev, col_off_dev=None,
                  col_out_dev=None, max_block_cells=0):
        """all device memory; the lengths, the pair list, n_env, env and col_off are read back once"""
        check(self.ctx.L.gs_hmm_align_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), pair_rec_dev, pair_prof_dev, int(n_pairs), int(max_env),
                                          int(max_block_cells), n_env_dev, env_dev, slot_out_dev, col_off_dev, col_out_dev))

    def align_all(self, aa, rec_start, rec_len, pair_rec, pair_prof, columns=True):
        """envelopes_packed() with room for every envelope (_all_items) and align_packed() behind it -> (fwd, n_env, env) + what align_packed() returns"""
        fwd, _, ne, env = _all_items(lambda m: self.envelopes_packed(aa, rec_start, rec_len, pair_rec, pair_prof, m), 2)
        got = self.align_packed(aa, rec_start, rec_len, pair_rec, pair_prof, ne, env, columns=columns)
        return (fwd, ne, env) + (got if columns else (got,))

    def envelopes_dev(self, aa_dev, rec_start_dev, rec_len_dev, n_rec, pair_rec_dev, pair_prof_dev, n_pairs, max_env, fwd_out_dev, bck_out_dev, n_env_out_dev,
                      env_out_dev, row_off_dev=None, out_rows_dev=None, cont_rows_dev=None, max_block_rows=0):
        """all device memory; the lengths, the pair list and row_off are read back once"""
        check(self.ctx.L.gs_hmm_envelopes_dev(self.ctx.h, self.h, aa_dev, rec_start_dev, rec_len_dev, int(n_rec), pair_rec_dev, pair_prof_dev, int(n_pairs), int(max_env),
                                              int(max_block_rows), fwd_out_dev, bck_out_dev, n_env_out_dev, env_out_dev, row_off_dev, out_rows_dev, cont_rows_dev))

    def thresholds(self, cutoff="ga"):
        """int32 [n_prof] in units: every profile's GA1, or the caller's bits for all (a number) or per profile (a sequence)"""
        if isinstance(cutoff, str):
            if cutoff != "ga":
                raise ValueError("cutoff: 'ga' or bits")
            if any(g is None for g in self.ga_units):
                raise GsError(_lib.GS_ERR_INVALID, "a profile of the set has no GA cutoff: give bits")
            return np.array(self.ga_units, np.int32)
        bits = np.broadcast_to(np.asarray(cutoff, dtype=np.float64), (len(self),))
        return np.array([hmm_threshold_units(b) for b in bits], np.int32)

    def best_hits_dev(self, score_dev, n_rec, genome_rec_off_dev, n_genomes, thr_dev, best_rec_out_dev, best_score_out_dev):
        check(self.ctx.L.gs_hmm_best_hits_dev(self.ctx.h, self.h, score_dev, int(n_rec), genome_rec_off_dev, int(n_genomes), thr_dev, best_rec_out_dev,
                                              best_score_out_dev))

    def best_hits(self, scores, genome_rec_off, cutoff="ga"):
        """per genome (records [genome_rec_off[g], genome_rec_off[g+1])) and profile the record with the largest raw score at or above the cutoff, the
        lowest such record on a tie -> (uint32 [n_genomes, n_prof] records, HMM_NO_HIT when none; int32 scores, HMM_NO_SCORE when none)"""
        ctx = self.ctx
        scores = np.ascontiguousarray(scores, dtype=np.int32).reshape(-1, len(self))
        goff = np.ascontiguousarray(genome_rec_off, dtype=np.uint64)
        thr = self.thresholds(cutoff)
        ng, nrec, npf = len(goff) - 1, len(scores), len(self)
        rec, sc = np.zeros((ng, npf), np.uint32), np.zeros((ng, npf), np.int32)
        if ng == 0:
            return rec, sc
        bufs = [ctx.alloc(max(a.nbytes, 16)) for a in (scores, goff, thr, rec, sc)]
        try:
            for ptr, a in zip(bufs[:3], (scores, goff, thr)):
                if a.nbytes:
                    ctx.upload(ptr, a)
            self.best_hits_dev(bufs[0], nrec, bufs[1], ng, bufs[2], bufs[3], bufs[4])
            rec = ctx.download(bufs[3], (ng, npf), np.uint32)
            sc = ctx.download(bufs[4], (ng, npf), np.int32)
        finally:
            for ptr in bufs:
                ctx.free(ptr)
        return rec, sc


def _faa_records(path):
    """(ids, sequences as the reader leaves them) of one protein FASTA file, plain or compressed"""
    text = read_fasta_file(path)
    recs = fasta_scan(text, skip_capsid=False)
    return [r[0] for r in recs], [text[b:e] for _, b, e in recs]


def _as_hmm_db(hmm, ctx):
    return hmm if isinstance(hmm, HmmDb) else HmmDb(hmm, ctx)


def _check_prefilter(prefilter):
    """-> (an MSV stage runs in front, the int16 Viterbi filter runs in front of Viterbi)"""
    if prefilter not in (None, "msv", "vit16", "msv+vit16"):
        raise ValueError("prefilter: None, 'msv', 'vit16' or 'msv+vit16'")
    return prefilter in ("msv", "msv+vit16"), prefilter in ("vit16", "msv+vit16")


def _alignment_text(db, ids, listed, residues_of, n_env, env, slots, cols):
    """the text of hmmsearch(alignments=), SPEC 13.6: per pair of `listed` and aligned envelope a tab-separated header line and the lines model, match,
    target and PP, unwrapped. residues_of(r): the residues of target r"""
    exp2 = hmm_exp2_table().astype(np.int64)
    out = [b"# == target\tprofile\tacc\tenv\tn_env\tali_from\tali_to\thmm_from\thmm_to\tM\tacc\tn_match\tn_ins\tn_del\n"]
    tabs = {}
    for j, (r, p) in enumerate(listed):
        if not cols[j]:
            continue
        inf = db.info[p]
        if p not in tabs:
            tabs[p] = (db.tables(p), db.consensus(p).decode("ascii").lower())
        tab, cons = tabs[p]
        rec = bytes(residues_of(r)).decode("ascii").upper()
        for d, (st, k, i, pp) in enumerate(cols[j]):
            s = [int(v) for v in slots[j, d]]
            Ld = int(env[j, d, 1]) - int(env[j, d, 0]) + 1
            out.append(("==\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\t%d\t%d\t%d\n" % (ids[r], inf["name"], inf["acc"] or "-", d + 1, int(n_env[j]), s[0], s[1], s[2], s[3],
                                                                                          inf["M"], s[4] / (65536.0 * Ld), s[5], s[6], s[7])).encode())
            nu = -pp.astype(np.int64)
            dig = (10 * (exp2[nu & 1023] >> np.minimum(nu >> 10, 31)) + 32768) >> 16
            model, match, target, ppl = [], [], [], []
            for c in range(len(st)):
                res = rec[int(i[c]) - 1]
                if st[c] == 0:
                    m = cons[int(k[c]) - 1]
                    model.append(m); target.append(res)
                    match.append(m if m.upper() == res else ("+" if int(tab[_lib.HMM_AA.index(res), int(k[c])]) > 0 else " "))
                elif st[c] == 1:
                    model.append("."); match.append(" "); target.append(res.lower())
                else:
                    model.append(cons[int(k[c]) - 1]); match.append(" "); target.append("-")
                ppl.append("." if st[c] == 2 else ("*" if dig[c] >= 10 else str(int(dig[c]))))
            out.append("".join("  %-6s %s\n" % (lab, "".join(t)) for lab, t in (("model", model), ("match", match), ("target", target), ("PP", ppl))).encode())
    return b"".join(out)


def _table_pairs(scores, seq_bias):
    """the (record, profile) pairs of the score table of hmmsearch() in its order: those with raw >= 0, by (profile, -(raw - seq_bias), record)"""
    listed = []
    for p in range(scores.shape[1]):
        plain = scores[:, p].astype(np.int64)
        keep = np.flatnonzero((plain != _lib.HMM_NO_SCORE) & (plain >= 0))
        col = plain - seq_bias[:, p]
        listed += [(int(r), p) for r in keep[np.lexsort((keep, -col[keep]))]]
    return listed


def _score_table(db, ids, listed, scores, seq_bias, fwd, bias):
    """the score table of hmmsearch(), SPEC 13 / 13.1 / 13.5: a row per pair of `listed`; seq_bias: int64 as scores, zeros without bias"""
    out = [b"target\tprofile\tacc\tbits\tevalue\tpass_ga" + (b"\tbias\n" if bias else b"\n")]
    for r, p in listed:
        inf = db.info[p]
        raw = int(scores[r, p]) - int(seq_bias[r, p])
        b = hmm_bits(raw)
        if fwd:
            ev = "%.3E" % hmm_forward_evalue(b, db.tau[p], db.lam_fwd[p], len(ids)) if not np.isnan(db.tau[p]) else "-"
        else:
            ev = "%.3E" % hmm_evalue(b, inf["mu"], inf["lam"], len(ids)) if inf["mu"] is not None else "-"
        ga = "-" if inf["ga_units"] is None else ("1" if raw >= inf["ga_units"] else "0")
        tail = "\t%.2f\n" % (int(seq_bias[r, p]) / 1024.0) if bias else "\n"
        out.append(("%s\t%s\t%s\t%.2f\t%s\t%s%s" % (ids[r], inf["name"], inf["acc"] or "-", b, ev, ga, tail)).encode())
    return b"".join(out)


def _domain_table(db, ids, listed, n_dom, dom):
    """the domain table of hmmsearch(domains=), SPEC 13.2: n_dom, dom as trace_all() returns them for the pairs of `listed`"""
    out = [b"target\tprofile\tacc\tdom\tn_dom\ti_from\ti_to\tk_from\tk_to\tM\tseg_bits\tn_match\tn_ins\tn_del\n"]
    for j, (r, p) in enumerate(listed):
        inf = db.info[p]
        for d in range(int(n_dom[j])):
            w = [int(v) for v in dom[j, d]]
            out.append(("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%d\t%d\t%d\n" % (ids[r], inf["name"], inf["acc"] or "-", d + 1, int(n_dom[j]), w[0], w[1], w[2], w[3],
                                                                                          inf["M"], w[4] / 1024.0, w[5], w[6], w[7])).encode())
    return b"".join(out)


def _envelope_table(db, ids, listed, n_env, env, slots=None):
    """the envelope table of hmmsearch(envelopes=), SPEC 13.4: n_env, env as envelopes_all() returns them for the pairs of `listed`; slots: their null2
    slots with bias (SPEC 13.5), which take dom_bias off env_bits and add the column `env_bias`"""
    bias = slots is not None
    out = [b"target\tprofile\tacc\tenv\tn_env\ti_from\ti_to\tenv_bits\tpeak_occ" + (b"\tenv_bias\n" if bias else b"\n")]
    for j, (r, p) in enumerate(listed):
        inf = db.info[p]
        for d in range(int(n_env[j])):
            w = [int(v) for v in env[j, d]]
            db_ = int(slots[j, d, 1]) if bias else 0
            tail = "\t%.2f\n" % (db_ / 1024.0) if bias else "\n"
            out.append(("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%.2f\t%.3f%s" % (ids[r], inf["name"], inf["acc"] or "-", d + 1, int(n_env[j]), w[0], w[1], (w[2] - db_) / 1024.0,
                                                                     1.0 - 2.0 ** (w[3] / 1024.0), tail)).encode())
    return b"".join(out)


def hmmsearch(faa, hmm, output=None, ctx=None, score="viterbi", filter_p=1e-3, domains=None, translate=False, min_aa=_lib.ORF_MIN_AA, table=11, prefilter=None,
              msv_p=0.02, envelopes=None, bias=False, alignments=None):
    """Library counterpart of `hmmsearch_rs -f proteome.faa -m profile.HMM`: every protein of `faa` (.faa, also .gz / .bz2 / .xz) against every profile of
    `hmm` (a path, a directory, a list of paths or an HmmDb). Returns (ids, int32 [n_rec, n_prof] raw scores, table bytes) and writes the table to
    `output` when given. The table (a stated choice, SPEC 13): a header line, then `target profile acc bits evalue pass_ga` separated by tabs for every
    (record, profile) with raw >= 0, sorted by (profile, -raw, record); bits %.2f, evalue %.3E with Z = the number of records (`-` without STATS),
    pass_ga 1 / 0 (`-` without GA), acc `-` when the profile has none.
    score="forward" (SPEC 13.1): the scores are the Forward matrix behind the Viterbi floor of filter_p (None: every pair) - bits and pass_ga of the
    Forward raw, evalue from STATS LOCAL FORWARD (`-` without the line), rows for the pairs that have a Forward raw >= 0.
    domains (a path; SPEC 13.2): the pairs the score table lists are traced back on the device and a second table is written there - a header line, then
    `target profile acc dom n_dom i_from i_to k_from k_to M seg_bits n_match n_ins n_del` for every domain, seg_bits %.2f of seg / 1024, sorted like the
    score table and then by dom (from 1). With score="forward" the pairs are the Forward table's and the path is still the Viterbi path. The return value is
    then (ids, scores, table bytes, domain table bytes).
    envelopes (a path; SPEC 13.4): the pairs the score table lists get a Forward and a Backward pass on the device and a table of their posterior
    envelopes is written there - a header line, then `target profile acc env n_env i_from i_to env_bits peak_occ` for every envelope, env_bits %.2f of
    env_raw / 1024, peak_occ %.3f of 1 - 2^(peak / 1024), sorted like the score table and then by env (from 1). It works with either score and together
    with domains; its bytes are appended to the return value.
    translate=True (SPEC 14): `faa` is a NUCLEOTIDE FASTA; the targets are its stop-to-stop six-frame ORFs of min_aa residues and more under translation
    `table` (11 or 4), translated on the device and searched there without their residues coming back. A target is named `{contig}_{begin+1}_{end}_{+|-}`
    as write_orf_faa() names it, Z is the number of ORFs, the formats are unchanged. The ORFs are not a proteome: no start codons, no frameshifts.
    translate="genes" (SPEC 15): the targets are instead the genes the self-trained caller of gene_call() chooses in that file taken as one genome, called
    on the device and searched there; names, Z and formats follow in the same way. A file too small to train has no targets. Unlike translate=True, which drops and counts an ORF longer than
    the search takes (the smallest of the HMM_*MAX_L limits of the programs the call runs), a called gene that long raises ValueError and ends the call: a
    gene set with one silently left out would no longer be the genome's.
    prefilter="msv" (SPEC 13.3): the MSV score of every pair runs first and Viterbi (and Forward behind it) only for the pairs at or above the MSV floor of
    msv_p (HMMER's F1 = 0.02; None: every pair) - in all three target forms and with both scores. The returned matrix holds HMM_NO_SCORE for the pairs the
    filter left out, the table has rows only for pairs that passed, Z stays the number of records. A pair whose gapped alignment is good and whose
    ungapped diagonals are weak is lost: the filter's stated cost. prefilter=None: no prefilter.
    prefilter="vit16" (SPEC 13.7): the packed int16 Viterbi score vf of every pair runs first and Viterbi (and Forward behind it) only for the pairs with vf at
    or above the lowest Viterbi score the call looks at - 0, the table's raw >= 0, or the Viterbi floor of filter_p with score="forward" (filter_p=None
    then leaves nothing to cut by: ValueError). vf is never below the Viterbi score, so the tables are those of prefilter=None byte for byte; the returned
    matrix holds HMM_NO_SCORE for the pairs the filter left out. prefilter="msv+vit16": MSV first, vf for its survivors, the tables of prefilter="msv".
    bias=True (SPEC 13.5; score="forward" only, ValueError otherwise): the pairs with a Forward raw >= 0 get their posterior envelopes and the null2 bias
    correction on the device. The table gains a last column `bias` (%.2f bits of seq_bias); bits, evalue and pass_ga are those of the corrected score
    fwd - seq_bias, and the rows are sorted by it. The envelope table gains a last column `env_bias` and its env_bits are env_raw - dom_bias. The returned
    matrix stays the uncorrected one. bias=False: no correction, the tables of 13 / 13.1 / 13.4 byte for byte.
    alignments (a path; SPEC 13.6): every posterior envelope of the pairs the score table lists gets its optimal-accuracy alignment on the device, and
    a text is written there, sorted like the envelope table - a legend line, then per envelope a line `== target profile acc env n_env ali_from ali_to
    hmm_from hmm_to M acc n_match n_ins n_del` separated by tabs (acc %.3f of oa / (65536 Ld)) and four unwrapped lines: `model` (the consensus letter of
    the node, lower case; `.` in an insert column), `match` (the letter where residue and consensus agree, `+` where the match score of the residue at
    the node is above 0, else a blank), `target` (upper case on a match state, lower case on an insert state, `-` on a delete state) and `PP` (the digit
    (10 w + 32768) >> 16 of the column's weight, `*` from 10; `.` under a delete column). It works with either score, with or without bias, and together
    with domains and envelopes; its bytes are appended to the return value. An envelope of more than HMM_ALI_MAX_LD = 8192 residues is not aligned by this
    library: the call then raises GsError (GS_ERR_UNSUPPORTED) and writes no alignment text, although records of up to 65 536 residues are searched."""
    if score not in ("viterbi", "forward"):
        raise ValueError("score: 'viterbi' or 'forward'")
    if bias and score != "forward":
        raise ValueError("bias=True corrects Forward scores: score='forward'")
    pre_msv, pre_vit16 = _check_prefilter(prefilter)
    db = _as_hmm_db(hmm, ctx)
    fwd = score == "forward"
    vf_floor = db.vf_floor(fwd, filter_p) if pre_vit16 else None
    enveloped = envelopes is not None or alignments is not None
    dev = _dev_targets(db.ctx, [faa], translate, min_aa, _orf_max_aa(fwd or enveloped, domains is not None), table)
    try:
        ids = dev.names()
        scores = dev.search(db, fwd, filter_p, pre_msv, msv_p, vf_floor)
        seq_bias = np.zeros(scores.shape, np.int64)                      # of the pairs that get a row, with bias
        if bias:
            cand = np.argwhere((scores != _lib.HMM_NO_SCORE) & (scores.astype(np.int64) >= 0))
            b_ne, b_env, b_slots, b_sb = dev.bias_all(db, cand[:, 0].astype(np.uint32), cand[:, 1].astype(np.uint32))[1:]
            seq_bias[cand[:, 0], cand[:, 1]] = b_sb
        listed = _table_pairs(scores, seq_bias)
        texts = [(output, _score_table(db, ids, listed, scores, seq_bias, fwd, bias))]
        if output is not None:                                           # the score table stands even if a pass below refuses its pairs
            with open(output, "wb") as f:
                f.write(texts[0][1])
        pr, pp = np.array([r for r, _ in listed], np.uint32), np.array([p for _, p in listed], np.uint32)
        if domains is not None:
            _, nd, dom = dev.trace_all(db, pr, pp)
            texts.append((domains, _domain_table(db, ids, listed, nd, dom)))
        slots = None
        if enveloped and bias:                                           # the candidates' envelopes, in the table's order
            slot_of = {(int(r), int(p)): j for j, (r, p) in enumerate(cand)}
            order = [slot_of[rp] for rp in listed]
            ne, env, slots = b_ne[order], b_env[order], b_slots[order]
        elif enveloped:
            _, _, ne, env = dev.envelopes_all(db, pr, pp)
        if envelopes is not None:
            texts.append((envelopes, _envelope_table(db, ids, listed, ne, env, slots)))
        if alignments is not None:                                       # every listed envelope aligned, over the envelopes found above
            a_slots, a_cols = dev.align_listed(db, pr, pp, ne, env)
            texts.append((alignments, _alignment_text(db, ids, listed, dev.residues, ne, env, a_slots, a_cols)))
    finally:
        dev.close()
    for path, text in texts[1:]:
        with open(path, "wb") as f:
            f.write(text)
    return (ids, scores) + tuple(text for _, text in texts)


def _bias_best_hits(scores, goff, thr, bias_of):
    """SPEC 13.5, the best hits of universal_genes(bias=True): the candidates are the pairs whose uncorrected Forward raw reaches the profile's cutoff - a
    superset of the final hits, the bias is never negative -, bias_of(pair_rec, pair_prof) gives their seq_bias, and per genome and profile the record
    with the largest corrected score at or above the cutoff is kept, the lowest record on a tie -> uint32 [n_genomes, n_prof], HMM_NO_HIT where none"""
    goff = np.asarray(goff, dtype=np.int64)
    ng, npf = len(goff) - 1, scores.shape[1]
    rec = np.full((ng, npf), _lib.HMM_NO_HIT, np.uint32)
    s = scores.astype(np.int64)
    thr = np.asarray(thr, dtype=np.int64)
    cand = np.argwhere((scores != _lib.HMM_NO_SCORE) & (s >= thr[None, :]))
    cand = cand[(cand[:, 0] >= goff[0]) & (cand[:, 0] < goff[-1])]
    if len(cand) == 0:
        return rec
    sb = np.asarray(bias_of(cand[:, 0].astype(np.uint32), cand[:, 1].astype(np.uint32)), dtype=np.int64)
    corrected = s[cand[:, 0], cand[:, 1]] - sb
    genome = np.searchsorted(goff, cand[:, 0], side="right") - 1
    for j in np.lexsort((cand[:, 0], -corrected)):                      # best first, the lowest record among equals
        g, p = int(genome[j]), int(cand[j, 1])
        if corrected[j] >= thr[p] and rec[g, p] == _lib.HMM_NO_HIT:
            rec[g, p] = cand[j, 0]
    return rec


def _region_spans(dev, db, rec, region):
    """the cut of universal_genes(region=) per hit of the best-hit matrix `rec` over the targets `dev`: {g * n_prof + p: (a, b)}, residues [a, b) of the
    record, from i_from of the hit's first domain ("aligned"), posterior envelope ("envelope") or aligned envelope ("alignment") through i_to of its
    last. A hit that has none is not in the dict: it keeps its whole record, as every hit of region "protein" does"""
    if region == "protein" or not (rec != _lib.HMM_NO_HIT).any():
        return {}
    pr, pp = rec.reshape(-1), np.tile(np.arange(len(db), dtype=np.uint32), rec.shape[0])
    if region == "aligned":
        _, n_item, item = dev.trace_all(db, pr, pp)
    elif region == "envelope":
        _, _, n_item, item = dev.envelopes_all(db, pr, pp)
    else:
        _, n_item, _, item = dev.align_all(db, pr, pp, columns=False)
    return {int(j): (int(item[j, 0, 0]) - 1, int(item[j, int(n_item[j]) - 1, 1])) for j in np.flatnonzero(n_item)}


def universal_genes(faa_files, hmm, ctx=None, cutoff="ga", score="viterbi", filter_p=1e-3, region="protein", translate=False, min_aa=_lib.ORF_MIN_AA, table=11,
                    prefilter=None, msv_p=0.02, bias=False):
    """One genome per protein FASTA file: per genome the residues of its best protein for every profile that has a hit at the cutoff, in profile
    order - the records an AA sketcher takes for `tohnsw` / `request` at the universal-gene level. -> (list of lists of bytes, uint32 [n_genomes, n_prof]
    record numbers inside each genome's file, HMM_NO_HIT where a profile found nothing). score="forward": the best hits are those of the Forward matrix
    (SPEC 13.1) behind the Viterbi floor of filter_p - the score the files' GA cutoffs were gathered on. region="aligned" (SPEC 13.2): every hit is
    traced back on the device and contributes the residues from i_from of its first domain through i_to of its last, not the whole protein.
    region="envelope" (SPEC 13.4): every hit contributes the residues from i_from of its first posterior envelope through i_to of its last - what a
    Forward hit list should be cut by; a hit without an envelope contributes the whole record, and is counted like any other.
    region="alignment" (SPEC 13.6): every hit contributes the residues from i_from of the optimal-accuracy alignment of its first envelope through i_to
    of that of its last - the envelope cut without the flanks the model does not align; a hit without an envelope contributes the whole record. A hit
    with an envelope of more than HMM_ALI_MAX_LD = 8192 residues makes the call raise GsError (GS_ERR_UNSUPPORTED): such an envelope is not aligned.
    translate=True (SPEC 14): one genome per NUCLEOTIDE FASTA file; the candidates are the stop-to-stop six-frame ORFs of min_aa residues and more under
    translation `table`, translated and searched on the device - only the chosen hits' residues come back. The record numbers are then ORF numbers inside
    the genome, and a third value is returned: int64 [n_genomes, n_prof, 4] = (contig index, begin, end, strand) of the chosen ORF in contig coordinates
    (0-based, end exclusive, strand 0 / 1 = + / -), -1 where a profile found nothing. A stop-to-stop ORF overhangs the gene at its 5' end;
    region="aligned" trims that. The ORF set is not a proteome and is not meant for the AA sketchers as a whole.
    translate="genes" (SPEC 15): the candidates are the genes of gene_call(), every file one self-trained genome; the record numbers are gene numbers
    inside the genome and the coordinates are the gene's, from its start codon through its stop codon. A called gene longer than the search takes raises
    ValueError and ends the call (translate=True drops and counts such an ORF; see hmmsearch).
    prefilter="msv" (SPEC 13.3): the best hits are taken among the pairs at or above the MSV floor of msv_p, as hmmsearch(prefilter="msv") scores them.
    prefilter="vit16" (SPEC 13.7): Viterbi runs only for the pairs whose int16 score vf reaches the cutoff in units (score="forward": the Viterbi floor of
    filter_p; filter_p=None: ValueError); vf is never below the Viterbi score, so the result is that of prefilter=None. "msv+vit16": that of "msv".
    bias=True (SPEC 13.5; score="forward" only, ValueError otherwise): every pair whose Forward raw reaches the cutoff gets its posterior envelopes and
    the null2 bias correction on the device, and the best hit per genome and profile is the record with the largest corrected score fwd - seq_bias at or
    above the cutoff (the lowest record on a tie) - the score the files' cutoffs were gathered on. A low-complexity protein that passes a cutoff on its
    composition alone is dropped. It works with all three target forms and every region."""
    if score not in ("viterbi", "forward"):
        raise ValueError("score: 'viterbi' or 'forward'")
    if region not in ("protein", "aligned", "envelope", "alignment"):
        raise ValueError("region: 'protein', 'aligned', 'envelope' or 'alignment'")
    if bias and score != "forward":
        raise ValueError("bias=True corrects Forward scores: score='forward'")
    pre_msv, pre_vit16 = _check_prefilter(prefilter)
    db = _as_hmm_db(hmm, ctx)
    fwd = score == "forward"
    vf_floor = db.vf_floor(fwd, filter_p, cutoff) if pre_vit16 else None
    ctx = db.ctx
    dev = _dev_targets(ctx, faa_files, translate, min_aa, _orf_max_aa(fwd or region in ("envelope", "alignment"), region == "aligned"), table)
    try:
        ng, npf = len(dev.genome_orf_off) - 1, len(db)
        rec, where = np.full((ng, npf), _lib.HMM_NO_HIT, np.uint32), np.full((ng, npf, 4), -1, np.int64)
        if ng and npf and dev.n:
            d_score = dev.search_dev(db, fwd, filter_p, pre_msv, msv_p, vf_floor)
            if bias:
                rec = _bias_best_hits(ctx.download(d_score, (dev.n, npf), np.int32), dev.genome_orf_off, db.thresholds(cutoff), lambda pr, pp: dev.bias_all(db, pr, pp)[4])
            else:
                d_goff, d_thr = dev.mem.up(dev.genome_orf_off), dev.mem.up(db.thresholds(cutoff))
                d_rec, d_sc = dev.mem.new(4 * ng * npf), dev.mem.new(4 * ng * npf)
                db.best_hits_dev(d_score, dev.n, d_goff, ng, d_thr, d_rec, d_sc)
                rec = ctx.download(d_rec, (ng, npf), np.uint32)
        span = _region_spans(dev, db, rec, region)
        genomes = []
        for g in range(ng):
            hits = []
            for p, r in enumerate(rec[g]):
                if r != _lib.HMM_NO_HIT:
                    a, b = span.get(g * npf + p, (0, int(dev.aa_len[r])))
                    hits.append(dev.residues(int(r), a, b))
                    if translate:
                        c, ob, oe, st = dev.coords(int(r))
                        where[g, p] = (c - int(dev.genome_contig0[g]), ob, oe, st)
            genomes.append(hits)
        local = np.where(rec == _lib.HMM_NO_HIT, rec, rec - dev.genome_orf_off[:-1].astype(np.uint32)[:, None]).astype(np.uint32)
        return (genomes, local, where) if translate else (genomes, local)
    finally:
        dev.close()


# ---- orfs (SPEC 14): stop-to-stop six-frame translation on the device ----------------------------------------------------------------------
ORF_DTYPE = np.dtype([("begin", np.uint64), ("rec", np.uint32), ("strand", np.uint32)])        # gs_orf
ORF_TILE = _lib.ORF_TILE


def orf_codon_table(table=11):
    """the 64 letters of translation table 11 or 4, codon index 16 b0 + 4 b1 + b2 with A C G T = 0 1 2 3, `*` = stop (host only)"""
    buf = C.create_string_buffer(64)
    check(_lib.load().gs_orf_codon_table(int(table), buf))
    return buf.raw.decode("ascii")


def _orf_caps(rec_len, min_aa):
    """room that holds every ORF whatever the bases are: a record of L bases has L - 2 codon positions on either strand, a kept ORF min_aa residues or more"""
    cap_aa = 2 * int(np.maximum(np.asarray(rec_len, dtype=np.int64) - 2, 0).sum())
    return cap_aa // max(int(min_aa), 1), cap_aa


def orf_translate_dev(ctx, seq_dev, seq_bytes, rec_start_dev, rec_len_dev, n_rec, cap_orf=0, cap_aa=0, orf_out_dev=None, aa_out_dev=None, aa_start_out_dev=None,
                      aa_len_out_dev=None, rec_orf_off_out_dev=None, min_aa=_lib.ORF_MIN_AA, max_aa=0, table=11):
    """gs_orf_translate_dev: all arrays device memory, the outputs left in flight on the context's stream -> (n_orf, n_aa, n_long), also when the
    capacities are too small (GsError then carries them as .counts). No outputs and zero capacities: count only."""
    prm = _lib.OrfParamsC(int(min_aa), int(max_aa), int(table), 0)
    n = (C.c_uint64 * 3)()
    try:
        check(ctx.L.gs_orf_translate_dev(ctx.h, C.byref(prm), seq_dev, int(seq_bytes), rec_start_dev, rec_len_dev, int(n_rec), int(cap_orf), int(cap_aa), orf_out_dev,
                                         aa_out_dev, aa_start_out_dev, aa_len_out_dev, rec_orf_off_out_dev, n))
    except GsError as e:
        e.counts = (int(n[0]), int(n[1]), int(n[2]))
        raise
    return int(n[0]), int(n[1]), int(n[2])


def orf_translate_packed(seq, rec_start, rec_len, min_aa=_lib.ORF_MIN_AA, max_aa=0, table=11, ctx=None):
    """SPEC 14 on the packed layout of pack_dna_records() (2-bit bases, no invalid base inside a record): the stop-to-stop ORFs of all six frames with
    min_aa <= residues (<= max_aa unless 0), ascending by (record, end, strand) -> dict of `orf` (ORF_DTYPE: begin inside the record in forward
    coordinates, rec, strand), `aa` (upper-case residues back to back), `aa_start`, `aa_len`, `rec_orf_off` (n_rec + 1) and `n_long` (dropped as longer
    than max_aa). This is not a gene caller and the ORF set is not a proteome: it feeds hmmsearch, not the AA sketchers."""
    ctx = ctx or default_context()
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
    rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
    prm = _lib.OrfParamsC(int(min_aa), int(max_aa), int(table), 0)
    cap_orf, cap_aa = _orf_caps(rl, min_aa)
    orf, aa = np.zeros(cap_orf, ORF_DTYPE), np.zeros(cap_aa, np.uint8)
    a_s, a_l, off = np.zeros(cap_orf, np.uint64), np.zeros(cap_orf, np.uint64), np.zeros(len(rs) + 1, np.uint64)
    n = (C.c_uint64 * 3)()
    check(ctx.L.gs_orf_translate(ctx.h, C.byref(prm), _p(seq) if seq.nbytes else None, seq.nbytes, _p(rs) if len(rs) else None, _p(rl) if len(rl) else None, len(rs),
                                 cap_orf, cap_aa, _p(orf), _p(aa), _p(a_s), _p(a_l), _p(off), n))
    return {"orf": orf[:n[0]].copy(), "aa": aa[:n[1]].copy(), "aa_start": a_s[:n[0]].copy(), "aa_len": a_l[:n[0]].copy(), "rec_orf_off": off, "n_long": int(n[2])}


def _orf_segments(contigs):
    """ASCII contigs -> (records, contig of each record, offset of each record in its contig): a contig is split at every byte outside ACGTacgt
    (SPEC 11 segments without qualities), so that no codon holds an invalid base and no frame shifts"""
    recs, rec_contig, rec_off = [], [], []
    for ci, ctg in enumerate(contigs):
        ctg = bytes(ctg)
        for b, l in bigsi_split(ctg):
            recs.append(ctg[b:b + l]); rec_contig.append(ci); rec_off.append(b)
    return recs, np.array(rec_contig, np.int64), np.array(rec_off, np.int64)


def orf_translate(contigs, min_aa=_lib.ORF_MIN_AA, max_aa=0, table=11, ctx=None):
    """ASCII contigs (bytes, no line breaks) -> (per contig the list of (begin, end, strand, protein) in contig coordinates - 0-based, end exclusive,
    strand 0 / 1 = + / -, ascending by (end, strand) -, the flat dict of orf_translate_packed() with `rec_contig` and `rec_offset` of its records).
    Model-free: every maximal run of codons without a stop in any of the six frames, no start-codon rule. Not a gene caller, not a proteome."""
    recs, rc, ro = _orf_segments(contigs)
    seq, rs, rl = pack_dna_records(recs)
    flat = orf_translate_packed(seq, rs, rl, min_aa, max_aa, table, ctx)
    flat["rec_contig"], flat["rec_offset"] = rc, ro
    out = [[] for _ in contigs]
    aa = flat["aa"].tobytes()
    for o, a, n in zip(flat["orf"], flat["aa_start"], flat["aa_len"]):
        b = int(ro[o["rec"]]) + int(o["begin"])
        out[int(rc[o["rec"]])].append((b, b + 3 * int(n), int(o["strand"]), aa[int(a):int(a) + int(n)]))
    return out, flat


def _orf_name(contig_id, begin, end, strand):
    return "%s_%d_%d_%s" % (contig_id, begin + 1, end, "-" if strand else "+")


def write_orf_faa(path, contig_ids, orfs):
    """orfs: per contig the (begin, end, strand, protein) list of orf_translate() -> a protein FASTA with headers `>{contig}_{begin+1}_{end}_{+|-}`
    (FragGeneScan's header convention) and one sequence line per ORF. The file is a set of candidates for hmmsearch, not a proteome."""
    if len(contig_ids) != len(orfs):
        raise ValueError("one id per contig")
    with open(path, "wb") as f:
        for cid, lst in zip(contig_ids, orfs):
            for b, e, s, prot in lst:
                f.write(b">" + _orf_name(cid, b, e, s).encode() + b"\n" + bytes(prot) + b"\n")


def _fna_contigs(path):
    """[(id, bases without line breaks)] of one nucleotide FASTA file, plain or compressed"""
    text = read_fasta_file(path)
    return [(rid, _strip_breaks(text[b:e])) for rid, b, e in fasta_scan(text, skip_capsid=False)]


def _orf_max_aa(fwd, traced):
    """the longest ORF the programs of a translated call take"""
    return min([_lib.HMM_MAX_L] + ([_lib.HMM_FWD_MAX_L] if fwd else []) + ([_lib.HMM_TRACE_MAX_L] if traced else []))


class _DevTargets:
    """The protein targets of hmmsearch(), universal_genes() and universal_sketch() in device memory, in the layout gs_hmm_search_dev reads, and every
    pass over them. A source (_DevOrfs, _DevGenes, _DevProteins) is a constructor that leaves: n targets (n_long: those dropped for their length) with
    residues d_aa, starts d_as and lengths d_al on the device under `mem`; aa_start, aa_len, the host copies of the last two; genome_orf_off
    [n_genomes + 1], the first target of every genome. The host holds the descriptors; whether it holds residues is the source's matter (residues())."""

    def __init__(self, ctx):
        self.ctx, self.mem = ctx, _DevScope(ctx)

    def close(self):
        self.mem.close()

    def __del__(self):
        try:
            if not _exiting[0]:
                self.close()
        except Exception:
            pass

    def names(self):
        """a target cut from a contig is named by its coords() as write_orf_faa() names it (a source of whole proteins keeps their ids instead)"""
        out = []
        for j in range(self.n):
            c, b, e, s = self.coords(j)
            out.append(_orf_name(self.contig_ids[c], b, e, s))
        return out

    def search_dev(self, db, fwd, filter_p, prefilter=False, msv_p=0.02, vf_floor=None):
        """device int32 [n, n_prof] scores of the targets (Forward behind the Viterbi floor when fwd; behind the MSV floor of msv_p when prefilter, SPEC
        13.3; behind the int16 filter at vf_floor when that is given, SPEC 13.7); the caller frees through close()"""
        d_score = self.mem.new(4 * self.n * len(db))
        if self.n == 0:
            return d_score
        with _DevScope(self.ctx) as t:                  # the floors and the Viterbi matrix of a Forward call live as long as the call
            up = lambda a: None if a is None else t.up(a)       # noqa: E731
            if vf_floor is not None:
                d_mfl, d_fl = up(db._floor(msv_p, None, msv=True) if prefilter else None), up(db._floor(filter_p, None) if fwd else None)
                d_vit = t.new(4 * self.n * len(db)) if fwd else d_score
                db.search_staged_dev(self.d_aa, self.d_as, self.d_al, self.n, prefilter, d_mfl, up(np.ascontiguousarray(vf_floor, dtype=np.int32)), d_fl, None, None,
                                     d_vit, d_score if fwd else None)
                self.ctx.sync()
            elif prefilter:
                d_mfl, d_fl = up(db._floor(msv_p, None, msv=True)), up(db._floor(filter_p, None) if fwd else None)
                d_vit = t.new(4 * self.n * len(db)) if fwd else d_score
                db.search_filtered_dev(self.d_aa, self.d_as, self.d_al, self.n, d_mfl, d_fl, None, d_vit, d_score if fwd else None)
                self.ctx.sync()
            elif fwd:
                db.search_forward_dev(self.d_aa, self.d_as, self.d_al, self.n, up(db._floor(filter_p, None)), None, d_score)
                self.ctx.sync()
            else:
                db.search_dev(self.d_aa, self.d_as, self.d_al, self.n, d_score)
        return d_score

    def search(self, db, fwd, filter_p, prefilter=False, msv_p=0.02, vf_floor=None):
        d_score = self.search_dev(db, fwd, filter_p, prefilter, msv_p, vf_floor)
        scores = self.ctx.download(d_score, (self.n, len(db)), np.int32)
        self.mem.free(d_score)
        return scores

    def _over_pairs(self, call, pair_rec, pair_prof, outs):
        """call = db.trace_dev or db.envelopes_dev over the device residues, with room for every item (_all_items). outs(n_pairs, m): (shape, dtype, what a
        call with nothing to do leaves there) of each output at m slots a pair; the last holds the items, the one before it their numbers."""
        pr, pp, _ = _pairs(pair_rec, pair_prof)
        n = len(pr)
        if n == 0 or self.n == 0:
            return tuple(np.full(shape, fill, dt) for shape, dt, fill in outs(n, 8))
        with _DevScope(self.ctx) as d:
            d_pr, d_pp = d.up(pr), d.up(pp)

            def run(m):
                with _DevScope(self.ctx) as o:
                    ptrs = [o.new(int(np.prod(shape)) * np.dtype(dt).itemsize) for shape, dt, _ in outs(n, m)]
                    call(self.d_aa, self.d_as, self.d_al, self.n, d_pr, d_pp, n, m, *ptrs)
                    return tuple(self.ctx.download(ptr, shape, dt) for ptr, (shape, dt, _) in zip(ptrs, outs(n, m)))
            return _all_items(run, len(outs(n, 8)) - 2)

    def trace_all(self, db, pair_rec, pair_prof):
        """what HmmDb.trace_packed() returns, with room for every domain -> (raw, n_dom, dom)"""
        return self._over_pairs(db.trace_dev, pair_rec, pair_prof, lambda n, m: [((n,), np.int32, _lib.HMM_NO_SCORE), ((n,), np.uint32, 0),
                                                                                 ((n, m, _lib.HMM_DOM_WORDS), np.int32, 0)])

    def envelopes_all(self, db, pair_rec, pair_prof):
        """what HmmDb.envelopes_packed() returns, with room for every envelope -> (fwd, bck, n_env, env)"""
        return self._over_pairs(db.envelopes_dev, pair_rec, pair_prof, lambda n, m: [((n,), np.int32, _lib.HMM_NO_SCORE), ((n,), np.int32, _lib.HMM_NO_SCORE),
                                                                                     ((n,), np.uint32, 0), ((n, m, _lib.HMM_ENV_WORDS), np.int32, 0)])

    def bias_all(self, db, pair_rec, pair_prof):
        """envelopes_all() and what HmmDb.null2_packed() returns for them -> (fwd, n_env, env, slots, seq_bias): the envelopes stay on the device between
        the two calls"""
        pr, pp, _ = _pairs(pair_rec, pair_prof)
        n = len(pr)
        if n == 0 or self.n == 0:
            return (np.full(n, _lib.HMM_NO_SCORE, np.int32), np.zeros(n, np.uint32), np.zeros((n, 8, _lib.HMM_ENV_WORDS), np.int32),
                    np.zeros((n, 8, _lib.HMM_N2_WORDS), np.int32), np.zeros(n, np.int32))
        with _DevScope(self.ctx) as d:
            d_pr, d_pp = d.up(pr), d.up(pp)

            def run(m):
                with _DevScope(self.ctx) as o:
                    d_fwd, d_bck, d_ne, d_env = o.new(4 * n), o.new(4 * n), o.new(4 * n), o.new(4 * n * m * _lib.HMM_ENV_WORDS)
                    db.envelopes_dev(self.d_aa, self.d_as, self.d_al, self.n, d_pr, d_pp, n, m, d_fwd, d_bck, d_ne, d_env)
                    ne = self.ctx.download(d_ne, (n,), np.uint32)
                    if len(ne) and int(ne.max()) > m:                           # run again with room for every envelope (_all_items)
                        return None, ne, None
                    d_slot, d_sb = o.new(4 * n * m * _lib.HMM_N2_WORDS), o.new(4 * n)
                    db.null2_dev(self.d_aa, self.d_as, self.d_al, self.n, d_pr, d_pp, n, m, d_ne, d_env, d_slot, d_sb)
                    return (self.ctx.download(d_fwd, (n,), np.int32), ne, self.ctx.download(d_env, (n, m, _lib.HMM_ENV_WORDS), np.int32),
                            self.ctx.download(d_slot, (n, m, _lib.HMM_N2_WORDS), np.int32), self.ctx.download(d_sb, (n,), np.int32))
            got = run(8)
            return got if got[0] is not None else run(int(got[1].max()))

    def align_listed(self, db, pair_rec, pair_prof, n_env, env, columns=True):
        """what HmmDb.align_packed() returns for envelopes as envelopes_all() returned them -> (slots, columns); columns=False: no column is built, slots"""
        pr, pp, _ = _pairs(pair_rec, pair_prof)
        n = len(pr)
        ne, env = np.ascontiguousarray(n_env, dtype=np.uint32), np.ascontiguousarray(env, dtype=np.int32)
        m = env.shape[1]
        if n == 0 or self.n == 0:
            slots = np.zeros((n, m, _lib.HMM_ALI_WORDS), np.int32)
            return (slots, [[] for _ in range(n)]) if columns else slots
        with _DevScope(self.ctx) as d:
            d_slot, d_co, d_col = d.new(4 * n * m * _lib.HMM_ALI_WORDS), None, None
            if columns:
                lens = np.where(pr < self.n, self.aa_len[np.minimum(pr, self.n - 1)], 0)
                M = db.M[pp].astype(np.int64)
                co = _ali_col_off(lens, ne, env, M)
                d_co, d_col = d.up(co), d.new(8 * max(int(co[-1]), 1))
            db.align_dev(self.d_aa, self.d_as, self.d_al, self.n, d.up(pr), d.up(pp), n, m, d.up(ne), d.up(env), d_slot, d_co, d_col)
            slots = self.ctx.download(d_slot, (n, m, _lib.HMM_ALI_WORDS), np.int32)
            if not columns:
                return slots
            cols = self.ctx.download(d_col, (max(int(co[-1]), 1), 2), np.int32)
        return slots, _ali_columns(slots, cols, co, ne, env, M)

    def align_all(self, db, pair_rec, pair_prof, columns=True):
        """envelopes_all() and align_listed() behind it -> (fwd, n_env, env, slots[, columns])"""
        fwd, _, ne, env = self.envelopes_all(db, pair_rec, pair_prof)
        got = self.align_listed(db, pair_rec, pair_prof, ne, env, columns)
        return (fwd, ne, env) + (got if columns else (got,))

    def residues(self, j, a=0, b=None):
        """residues [a, b) of target j, read back from the device"""
        b = int(self.aa_len[j]) if b is None else b
        if b <= a:
            return b""
        return self.ctx.download(self.d_aa + int(self.aa_start[j]) + a, (b - a,), np.uint8).tobytes()


class _DevOrfs(_DevTargets):
    """The stop-to-stop six-frame ORFs of some genomes (each a list of (contig id, bases)), translated on the device (SPEC 14): their residues never
    come to the host. `orf` holds begin, rec and strand of each."""

    def __init__(self, ctx, genomes, min_aa, max_aa, table):
        super().__init__(ctx)
        self.contig_ids = [cid for g in genomes for cid, _ in g]
        contig_genome = [gi for gi, g in enumerate(genomes) for _ in g]
        self.genome_contig0 = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.int64)
        recs, self.rec_contig, self.rec_offset = _orf_segments([c for g in genomes for _, c in g])
        seq, rs, rl = pack_dna_records(recs)
        cap_orf, cap_aa = _orf_caps(rl, min_aa)
        n_rec = len(rs)
        try:
            d_seq, d_rs, d_rl = self.mem.up(seq), self.mem.up(rs), self.mem.up(rl)
            self.d_orf, self.d_aa, self.d_as, self.d_al = self.mem.new(16 * cap_orf), self.mem.new(cap_aa), self.mem.new(8 * cap_orf), self.mem.new(8 * cap_orf)
            d_off = self.mem.new(8 * (n_rec + 1))
            self.n, n_aa, self.n_long = orf_translate_dev(ctx, d_seq, seq.nbytes, d_rs, d_rl, n_rec, cap_orf, cap_aa, self.d_orf, self.d_aa, self.d_as, self.d_al, d_off,
                                                          min_aa, max_aa, table)
            self.orf = ctx.download(self.d_orf, (self.n,), ORF_DTYPE)
            self.aa_start = ctx.download(self.d_as, (self.n,), np.uint64)
            self.aa_len = ctx.download(self.d_al, (self.n,), np.uint64)
            rec_orf_off = ctx.download(d_off, (n_rec + 1,), np.uint64)
            for ptr in (d_seq, d_rs, d_rl, d_off):
                self.mem.free(ptr)
        except Exception:
            self.close()
            raise
        # the first record of every genome -> its first ORF
        rec_genome = np.array([contig_genome[c] for c in self.rec_contig], np.int64)
        first_rec = np.searchsorted(rec_genome, np.arange(len(genomes) + 1))
        self.genome_orf_off = rec_orf_off[first_rec].astype(np.uint64)

    def coords(self, j):
        """(contig index, begin, end, strand) of ORF j in contig coordinates"""
        o = self.orf[j]
        b = int(self.rec_offset[o["rec"]]) + int(o["begin"])
        return int(self.rec_contig[o["rec"]]), b, b + 3 * int(self.aa_len[j]), int(o["strand"])


# ---- genes (SPEC 15): a self-trained gene caller on the device --------------------------------------------------------------------------------
GENE_DTYPE = np.dtype([("begin", np.uint64), ("end", np.uint64), ("score", np.int64), ("rec", np.uint32), ("flags", np.uint32)])      # gs_gene
GENE_INTERVAL_DTYPE = np.dtype([("begin", np.uint64), ("n", np.uint64), ("rec", np.uint32), ("strand", np.uint32)])                   # gs_gene_interval
GENE_START_TYPES = ("ATG", "GTG", "TTG", "edge")


def gene_params(**kw):
    """gs_gene_params: the defaults of SPEC 15 (min_aa 30, table 11, train_min_aa 250, min_train_codons 15000, min_score 5120, max_overlap 60, rounds 2)
    with the given fields replaced"""
    prm = _lib.load().gs_gene_params_default()
    for k, v in kw.items():
        if k not in [f for f, _ in _lib.GeneParamsC._fields_]:
            raise TypeError("no gene parameter %r" % k)
        setattr(prm, k, int(v))
    return prm


def gene_log2_q16(x):
    """floor(65536 log2 x) by the integer recurrence of SPEC 15 (host only)"""
    return int(_lib.load().gs_gene_log2_q16(int(x)))


def _gene_inputs(seq, rec_start, rec_len, genome_rec_off):
    return (np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(rec_start, dtype=np.uint64), np.ascontiguousarray(rec_len, dtype=np.uint64),
            np.ascontiguousarray(genome_rec_off, dtype=np.uint64))


class _DevScope:
    """device buffers of one call or one owner, freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def new(self, nbytes):
        ptr = self.ctx.alloc(max(int(nbytes), 16))
        self.bufs.append(ptr)
        return ptr

    def up(self, arr):
        ptr = self.new(arr.nbytes)
        if arr.nbytes:
            self.ctx.upload(ptr, arr)
        return ptr

    def free(self, ptr):
        self.bufs.remove(ptr)
        self.ctx.free(ptr)

    def close(self):
        while self.bufs:
            self.ctx.free(self.bufs.pop())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def gene_train(seq, rec_start, rec_len, genome_rec_off, intervals, ctx=None, host=False, **params):
    """SPEC 15, counts to tables: the hexamer background of every genome and the in-frame dicodon counts of `intervals` (GENE_INTERVAL_DTYPE, in record
    order) -> (int32 [n_genomes, 4096] score tables, uint64 [n_genomes, 2] = (Nc, trained)). host=True: gs_gene_train_host, the same definitions in
    plain loops without a device; else gs_gene_train_dev."""
    seq, rs, rl, goff = _gene_inputs(seq, rec_start, rec_len, genome_rec_off)
    iv = np.ascontiguousarray(intervals, dtype=GENE_INTERVAL_DTYPE)
    ng = len(goff) - 1
    prm = gene_params(**params)
    tables, info = np.zeros((ng, 4096), np.int32), np.zeros((ng, 2), np.uint64)
    if host:
        check(_lib.load().gs_gene_train_host(C.byref(prm), _p(seq), seq.nbytes, _p(rs), _p(rl), len(rs), _p(goff), ng, _p(iv), len(iv), _p(tables), _p(info)))
        return tables, info
    ctx = ctx or default_context()
    with _DevScope(ctx) as d:
        d_t, d_i = d.new(tables.nbytes), d.new(info.nbytes)
        check(ctx.L.gs_gene_train_dev(ctx.h, C.byref(prm), d.up(seq), seq.nbytes, d.up(rs), d.up(rl), len(rs), d.up(goff), ng, d.up(iv), len(iv), d_t, d_i))
        return ctx.download(d_t, tables.shape, np.int32), ctx.download(d_i, info.shape, np.uint64)


def gene_score(seq, rec_start, rec_len, genome_rec_off, tables, orf, orf_len, ctx=None, host=False, **params):
    """SPEC 15, the best start of every given ORF (ORF_DTYPE descriptors and their codon counts) under the caller's int32 [n_genomes, 4096] tables ->
    (uint64 best j or GENE_NO_START, int64 score, uint32 flags). host=True: gs_gene_score_host, no device; else gs_gene_score_dev."""
    seq, rs, rl, goff = _gene_inputs(seq, rec_start, rec_len, genome_rec_off)
    ng = len(goff) - 1
    tables = np.ascontiguousarray(tables, dtype=np.int32).reshape(ng, 4096)
    orf, ol = np.ascontiguousarray(orf, dtype=ORF_DTYPE), np.ascontiguousarray(orf_len, dtype=np.uint64)
    if len(orf) != len(ol):
        raise ValueError("one length per ORF")
    prm = gene_params(**params)
    n = len(orf)
    bj, sc, fl = np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.uint32)
    if host:
        check(_lib.load().gs_gene_score_host(C.byref(prm), _p(seq), seq.nbytes, _p(rs), _p(rl), len(rs), _p(goff), ng, _p(tables), _p(orf), _p(ol), n, _p(bj), _p(sc), _p(fl)))
        return bj, sc, fl
    ctx = ctx or default_context()
    with _DevScope(ctx) as d:
        d_j, d_s, d_f = d.new(8 * n), d.new(8 * n), d.new(4 * n)
        check(ctx.L.gs_gene_score_dev(ctx.h, C.byref(prm), d.up(seq), seq.nbytes, d.up(rs), d.up(rl), len(rs), d.up(goff), ng, d.up(tables), d.up(orf), d.up(ol), n,
                                      d_j, d_s, d_f))
        return ctx.download(d_j, (n,), np.uint64), ctx.download(d_s, (n,), np.int64), ctx.download(d_f, (n,), np.uint32)


def gene_call_dev(ctx, seq_dev, seq_bytes, rec_start_dev, rec_len_dev, n_rec, genome_rec_off_dev, n_genomes, info_out_dev, cap_gene=0, cap_aa=0, gene_out_dev=None,
                  aa_out_dev=None, aa_start_out_dev=None, aa_len_out_dev=None, rec_gene_off_out_dev=None, tables_out_dev=None, **params):
    """gs_gene_call_dev: all arrays device memory, the outputs left in flight on the context's stream -> (n_gene, n_aa), also when the capacities are too
    small (GsError then carries them as .counts). No gene outputs and zero capacities: count only."""
    prm = gene_params(**params)
    n = (C.c_uint64 * 2)()
    try:
        check(ctx.L.gs_gene_call_dev(ctx.h, C.byref(prm), seq_dev, int(seq_bytes), rec_start_dev, rec_len_dev, int(n_rec), genome_rec_off_dev, int(n_genomes), int(cap_gene),
                                     int(cap_aa), gene_out_dev, aa_out_dev, aa_start_out_dev, aa_len_out_dev, rec_gene_off_out_dev, info_out_dev, tables_out_dev, n))
    except GsError as e:
        e.counts = (int(n[0]), int(n[1]))
        raise
    return int(n[0]), int(n[1])


def gene_call_packed(seq, rec_start, rec_len, genome_rec_off, ctx=None, tables=False, **params):
    """SPEC 15 on the packed layout of pack_dna_records(): every genome (records [genome_rec_off[g], genome_rec_off[g + 1])) trains its own dicodon model
    on its long ORFs and gets the maximal-weight chain of nearly non-overlapping genes of every record -> dict of `gene` (GENE_DTYPE, ascending by
    (record, end, strand), forward coordinates inside the record, stop codon included where there is one), `aa` (residues from the start codon to the
    last sense codon), `aa_start`, `aa_len`, `rec_gene_off` (n_rec + 1), `info` (uint64 [n_genomes, 2] = (Nc, trained)) and, when asked for, `tables`.
    A genome too small to train gets no genes. Not FragGeneScanRs and not its numbers (DESIGN "Known limitations (genes)")."""
    ctx = ctx or default_context()
    seq, rs, rl, goff = _gene_inputs(seq, rec_start, rec_len, genome_rec_off)
    ng = len(goff) - 1
    prm = gene_params(**params)
    cap_gene, cap_aa = _orf_caps(rl, prm.min_aa)
    gene, aa = np.zeros(cap_gene, GENE_DTYPE), np.zeros(cap_aa, np.uint8)
    a_s, a_l, off = np.zeros(cap_gene, np.uint64), np.zeros(cap_gene, np.uint64), np.zeros(len(rs) + 1, np.uint64)
    info, tab = np.zeros((ng, 2), np.uint64), (np.zeros((ng, 4096), np.int32) if tables else None)
    n = (C.c_uint64 * 2)()
    check(ctx.L.gs_gene_call(ctx.h, C.byref(prm), _p(seq) if seq.nbytes else None, seq.nbytes, _p(rs) if len(rs) else None, _p(rl) if len(rl) else None, len(rs), _p(goff),
                             ng, cap_gene, cap_aa, _p(gene), _p(aa), _p(a_s), _p(a_l), _p(off), _p(info), _p(tab), n))
    out = {"gene": gene[:n[0]].copy(), "aa": aa[:n[1]].copy(), "aa_start": a_s[:n[0]].copy(), "aa_len": a_l[:n[0]].copy(), "rec_gene_off": off, "info": info}
    if tables:
        out["tables"] = tab
    return out


def _gene_segments(genomes):
    """genomes (lists of ASCII contigs) -> (records, contig of each record, its offset there, genome_rec_off, first contig of every genome)"""
    contigs = [c for g in genomes for c in g]
    contig0 = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.int64)
    recs, rc, ro = _orf_segments(contigs)
    goff = np.searchsorted(rc, contig0).astype(np.uint64)
    return recs, rc, ro, goff, contig0


def gene_call(genomes, ctx=None, **params):
    """genomes: a list of genomes, each a list of ASCII contigs (bytes, no line breaks) -> (per genome and contig the list of (begin, end, strand, protein,
    score, flags) in contig coordinates - 0-based, end exclusive, the stop codon included where there is one, ascending by (end, strand) -, the flat dict
    of gene_call_packed() with `rec_contig`, `rec_offset` and `genome_rec_off`). A contig is cut at every byte outside ACGTacgt; a gene never spans a cut."""
    recs, rc, ro, goff, contig0 = _gene_segments(genomes)
    seq, rs, rl = pack_dna_records(recs)
    flat = gene_call_packed(seq, rs, rl, goff, ctx, **params)
    flat["rec_contig"], flat["rec_offset"], flat["genome_rec_off"] = rc, ro, goff
    out = [[[] for _ in g] for g in genomes]
    aa = flat["aa"].tobytes()
    for gn, a, n in zip(flat["gene"], flat["aa_start"], flat["aa_len"]):
        ci, off = int(rc[gn["rec"]]), int(ro[gn["rec"]])
        gi = int(np.searchsorted(contig0, ci, side="right")) - 1
        out[gi][ci - int(contig0[gi])].append((off + int(gn["begin"]), off + int(gn["end"]), int(gn["flags"]) & 1, aa[int(a):int(a) + int(n)], int(gn["score"]), int(gn["flags"])))
    return out, flat


def write_gene_faa(path, contig_ids, genes):
    """genes: per contig the tuples of gene_call() -> a protein FASTA with headers `>{contig}_{begin+1}_{end}_{+|-}` (as write_orf_faa), one line per gene"""
    if len(contig_ids) != len(genes):
        raise ValueError("one id per contig")
    with open(path, "wb") as f:
        for cid, lst in zip(contig_ids, genes):
            for g in lst:
                f.write(b">" + _orf_name(cid, g[0], g[1], g[2]).encode() + b"\n" + bytes(g[3]) + b"\n")


_DNA_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def write_gene_ffn(path, contig_ids, contigs, genes):
    """the genes' bases in reading direction (the stop codon included where there is one), upper case, same headers"""
    if len(contig_ids) != len(genes) or len(contigs) != len(genes):
        raise ValueError("one id and one sequence per contig")
    with open(path, "wb") as f:
        for cid, ctg, lst in zip(contig_ids, contigs, genes):
            for g in lst:
                nt = bytes(ctg[g[0]:g[1]])
                if g[2]:
                    nt = nt.translate(_DNA_COMPLEMENT)[::-1]
                f.write(b">" + _orf_name(cid, g[0], g[1], g[2]).encode() + b"\n" + nt.upper() + b"\n")


def write_gene_gff(path, contig_ids, genes):
    """GFF3: one CDS line per gene - 1-based closed coordinates, the score in bits (%.2f of score / 1024), phase 0, attributes ID (the FASTA header),
    start_type (ATG / GTG / TTG / edge) and partial (two digits: 1 = no start codon at the 5' end, 1 = no stop codon at the 3' end)"""
    if len(contig_ids) != len(genes):
        raise ValueError("one id per contig")
    with open(path, "wb") as f:
        f.write(b"##gff-version 3\n")
        for cid, lst in zip(contig_ids, genes):
            for b, e, s, _, score, flags in lst:
                t = (flags >> _lib.GENE_TYPE_SHIFT) & 3
                f.write(("%s\tgsearch_amd\tCDS\t%d\t%d\t%.2f\t%s\t0\tID=%s;start_type=%s;partial=%d%d\n" % (
                    cid, b + 1, e, score / 1024.0, "-" if s else "+", _orf_name(cid, b, e, s), GENE_START_TYPES[t], int(t == _lib.GENE_TYPE_EDGE),
                    int(bool(flags & _lib.GENE_OPEN3)))).encode())


def genecall(fna, prefix, ctx=None, **params):
    """Library counterpart of `FragGeneScanRs -s genome.fna -o prefix -w 1 -t complete` by another method (SPEC 15: self-trained, not FragGeneScan's
    trained model, not its numbers): the genes of one genome file (.fna, also .gz) -> `prefix.faa`, `prefix.ffn`, `prefix.gff`. Returns a dict of
    n_genes, trained and Nc. A genome too small to train (short contigs or plasmids alone) gives empty files and trained = False."""
    recs = _fna_contigs(fna)
    ids, contigs = [r[0] for r in recs], [bytes(r[1]) for r in recs]
    genes, flat = gene_call([contigs], ctx, **params)
    write_gene_faa(prefix + ".faa", ids, genes[0])
    write_gene_ffn(prefix + ".ffn", ids, contigs, genes[0])
    write_gene_gff(prefix + ".gff", ids, genes[0])
    return {"n_genes": len(flat["gene"]), "trained": bool(flat["info"][0, 1] & _lib.GENE_TRAINED), "Nc": int(flat["info"][0, 0])}


class _DevGenes(_DevTargets):
    """The genes of some genomes (SPEC 15) in the place of their ORFs: called on the device, every genome self-trained. `orf` holds begin, rec and
    strand of each gene; `end` its end (the stop codon included where there is one)."""

    def __init__(self, ctx, genomes, min_aa, max_aa, table, gene=None):
        super().__init__(ctx)
        self.contig_ids = [cid for g in genomes for cid, _ in g]
        recs, self.rec_contig, self.rec_offset, goff, contig0 = _gene_segments([[c for _, c in g] for g in genomes])
        self.genome_contig0 = contig0
        seq, rs, rl = pack_dna_records(recs)
        cap_gene, cap_aa = _orf_caps(rl, min_aa)
        n_rec, ng = len(rs), len(genomes)
        try:
            d_seq, d_rs, d_rl, d_goff = self.mem.up(seq), self.mem.up(rs), self.mem.up(rl), self.mem.up(goff)
            d_gene, self.d_aa, self.d_as, self.d_al = self.mem.new(GENE_DTYPE.itemsize * cap_gene), self.mem.new(cap_aa), self.mem.new(8 * cap_gene), self.mem.new(8 * cap_gene)
            d_off, d_info = self.mem.new(8 * (n_rec + 1)), self.mem.new(16 * ng)
            self.n, _ = gene_call_dev(ctx, d_seq, seq.nbytes, d_rs, d_rl, n_rec, d_goff, ng, d_info, cap_gene, cap_aa, d_gene, self.d_aa, self.d_as, self.d_al, d_off,
                                      **dict(gene or {}, min_aa=min_aa, table=table))
            self.n_long = 0
            gene = ctx.download(d_gene, (self.n,), GENE_DTYPE)
            self.aa_start = ctx.download(self.d_as, (self.n,), np.uint64)
            self.aa_len = ctx.download(self.d_al, (self.n,), np.uint64)
            rec_off = ctx.download(d_off, (n_rec + 1,), np.uint64)
            self.info = ctx.download(d_info, (ng, 2), np.uint64)
            for ptr in (d_seq, d_rs, d_rl, d_goff, d_gene, d_off, d_info):
                self.mem.free(ptr)
        except Exception:
            self.close()
            raise
        if max_aa and self.n and int(self.aa_len.max()) > max_aa:
            self.close()
            raise ValueError("a gene of %d residues is longer than the %d the search takes" % (int(self.aa_len.max()), max_aa))
        self.orf = np.zeros(self.n, ORF_DTYPE)
        self.orf["begin"], self.orf["rec"], self.orf["strand"] = gene["begin"], gene["rec"], gene["flags"] & 1
        self.end = gene["end"]
        self.genome_orf_off = rec_off[goff.astype(np.int64)].astype(np.uint64)

    def coords(self, j):
        o = self.orf[j]
        off = int(self.rec_offset[o["rec"]])
        return int(self.rec_contig[o["rec"]]), off + int(o["begin"]), off + int(self.end[j]), int(o["strand"])


class _DevProteins(_DevTargets):
    """The records of some protein FASTA files, one genome a file: filtered as the AA sketchers filter and uploaded once. Target j is record
    j - genome_orf_off[g] of file g. The filtered residues stay on the host too (`aa`), so that reading a hit is no device call."""

    def __init__(self, ctx, faa_files):
        super().__init__(ctx)
        self.ids, seqs, goff = [], [], [0]
        for path in faa_files:
            ids, recs = _faa_records(path)
            self.ids.extend(ids)
            seqs.extend(recs)
            goff.append(len(seqs))
        self.aa, self.aa_start, self.aa_len = filter_aa_records([bytes(s) for s in seqs])
        self.n, self.n_long = len(seqs), 0
        self.genome_orf_off = np.array(goff, np.uint64)
        try:
            self.d_aa, self.d_as, self.d_al = self.mem.up(self.aa), self.mem.up(self.aa_start), self.mem.up(self.aa_len)
        except Exception:
            self.close()
            raise

    def names(self):
        return list(self.ids)

    def residues(self, j, a=0, b=None):
        """residues [a, b) of record j, from the host copy"""
        s = int(self.aa_start[j])
        return self.aa[s + a:s + (int(self.aa_len[j]) if b is None else b)].tobytes()


def _dev_targets(ctx, files, translate, min_aa, max_aa, table, gene=None):
    """the targets of some files, one genome a file: the records of protein FASTA (translate falsy), else of nucleotide FASTA the six-frame ORFs or
    (translate="genes") the called genes. gene: further gene_call parameters (min_aa and table are the call's own)"""
    if not translate:
        return _DevProteins(ctx, files)
    genomes = [_fna_contigs(p) for p in files]
    if translate == "genes":
        return _DevGenes(ctx, genomes, min_aa, max_aa, table, gene)
    return _DevOrfs(ctx, genomes, min_aa, max_aa, table)


# ---- universal-gene sketches (SPEC 13.8, 17 item 11): best hits become sketcher records on the device -------------------------------------------------
def _hit_args(n_item, item, item_words, max_item):
    if (n_item is None) != (item is None):
        raise ValueError("n_item and item go together")
    return int(item_words), int(max_item)


def hit_records_dev(ctx, best_rec_dev, n_genomes, n_prof, aa_dev, rec_start_dev, rec_len_dev, n_rec, cap_rec, cap_aa, out_aa_dev, out_start_dev, out_len_dev,
                    out_genome_off_dev, n_item_dev=None, item_dev=None, item_words=_lib.HMM_DOM_WORDS, max_item=8):
    """gs_hmm_hit_records_dev (SPEC 13.8): all arrays device memory -> (records, residues). When the capacities are too small the GsError carries the true
    counts as .counts and nothing else was written; the other refusals leave .counts None."""
    words, m = _hit_args(n_item_dev, item_dev, item_words, max_item)
    n = (C.c_uint64 * 2)(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
    try:
        check(ctx.L.gs_hmm_hit_records_dev(ctx.h, best_rec_dev, int(n_genomes), int(n_prof), aa_dev, rec_start_dev, rec_len_dev, int(n_rec), n_item_dev, item_dev, words, m,
                                           int(cap_rec), int(cap_aa), out_aa_dev, out_start_dev, out_len_dev, out_genome_off_dev, n))
    except GsError as e:
        e.counts = None if n[0] == 0xFFFFFFFFFFFFFFFF else (int(n[0]), int(n[1]))
        raise
    return int(n[0]), int(n[1])


def hit_records(best_rec, aa, rec_start, rec_len, n_item=None, item=None, cap_rec=None, cap_aa=None, out=None):
    """gs_hmm_hit_records (SPEC 13.8), the host twin of hit_records_dev; no device. best_rec: uint32 [n_genomes, n_prof] as best_hits() gives it over the
    records (aa, rec_start, rec_len); n_item uint32 [n_genomes * n_prof] and item int32 [n_genomes * n_prof, max_item, words]: the spans of trace_packed(),
    envelopes_packed() or align_packed() over the matrix as a pair list. -> (uint8 residues back to back, uint64 start, uint64 len, uint64 genome_off
    [n_genomes + 1]). cap_rec / cap_aa: the room offered (None: enough); out: (aa, start, len, genome_off) arrays to write into instead of new ones. A
    refusal for room carries the true counts as .counts."""
    rec = np.ascontiguousarray(best_rec, dtype=np.uint32)
    if rec.ndim != 2:
        raise ValueError("best_rec: [n_genomes, n_prof]")
    ng, npf = rec.shape
    (aa, rs, rl), recs = _recs(aa, rec_start, rec_len)
    ni = it = None
    words, m = _lib.HMM_DOM_WORDS, 8
    if n_item is not None or item is not None:
        _hit_args(n_item, item, 0, 0)
        ni, it = np.ascontiguousarray(n_item, dtype=np.uint32).reshape(-1), np.ascontiguousarray(item, dtype=np.int32)
        if it.ndim != 3 or it.shape[0] != rec.size or len(ni) != rec.size:
            raise ValueError("n_item and item: one entry per (genome, profile) pair")
        m, words = it.shape[1], it.shape[2]
    named = rec[rec < len(rl)]
    room_rec = rec.size if cap_rec is None else int(cap_rec)
    room_aa = int(rl[named].sum()) if cap_aa is None else int(cap_aa)
    if out is None:
        out = (np.zeros((room_aa + 7) // 8 * 8 + 8, np.uint8), np.zeros(max(room_rec, 1), np.uint64), np.zeros(max(room_rec, 1), np.uint64), np.zeros(ng + 1, np.uint64))
    o_aa, o_s, o_l, o_g = out
    n = (C.c_uint64 * 2)(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
    try:
        check(_lib.load().gs_hmm_hit_records(None, _opt(rec), ng, npf, *recs, _opt(ni), _opt(it), words, m, room_rec, room_aa, _p(o_aa), _p(o_s), _p(o_l), _p(o_g), n))
    except GsError as e:
        e.counts = None if n[0] == 0xFFFFFFFFFFFFFFFF else (int(n[0]), int(n[1]))
        raise
    return o_aa[:int(n[1])], o_s[:int(n[0])], o_l[:int(n[0])], o_g


def _hit_spans_dev(db, dev, d_rec, n_pairs, region, scope):
    """the spans of region over the best-hit matrix as a pair list, left on the device with room for every item (_all_items) ->
    (n_item_dev, item_dev, words of a slot, slots a pair, uint32 n_item)"""
    ctx = db.ctx
    d_pp = scope.up(np.tile(np.arange(len(db), dtype=np.uint32), n_pairs // len(db)))

    def run(m):
        d_a, d_b, d_n = scope.new(4 * n_pairs), scope.new(4 * n_pairs), scope.new(4 * n_pairs)
        if region == "aligned":
            words = _lib.HMM_DOM_WORDS
            d_item = scope.new(4 * n_pairs * m * words)
            db.trace_dev(dev.d_aa, dev.d_as, dev.d_al, dev.n, d_rec, d_pp, n_pairs, m, d_a, d_n, d_item)
        else:
            words = _lib.HMM_ENV_WORDS
            d_item = scope.new(4 * n_pairs * m * words)
            db.envelopes_dev(dev.d_aa, dev.d_as, dev.d_al, dev.n, d_rec, d_pp, n_pairs, m, d_a, d_b, d_n, d_item)
        n_item = ctx.download(d_n, (n_pairs,), np.uint32)
        if len(n_item) and int(n_item.max()) > m:
            for ptr in (d_a, d_b, d_n, d_item):
                scope.free(ptr)
            return None, n_item
        if region == "alignment":
            d_env, words = d_item, _lib.HMM_ALI_WORDS
            d_item = scope.new(4 * n_pairs * m * words)
            db.align_dev(dev.d_aa, dev.d_as, dev.d_al, dev.n, d_rec, d_pp, n_pairs, m, d_n, d_env, d_item)
        return (d_n, d_item, words, m), n_item
    got, n_item = run(8)
    if got is None:
        got, n_item = run(int(n_item.max()))
    return got + (n_item,)


UNIVERSAL_STAGES = ("targets", "search", "best_hits", "spans", "hit_records", "sketch")


def universal_sketch(files, hmm, sketcher, ctx=None, cutoff="ga", score="viterbi", filter_p=1e-3, region="protein", translate=None, min_aa=_lib.ORF_MIN_AA, table=11,
                     prefilter=None, msv_p=0.02, gene=None, genomes_per_call=64, bias=False):
    """SPEC 17 item 11: one universal-gene signature per file - what sketcher.sketch_genomes(universal_genes(files, hmm, ...)[0]) gives, bit for bit, with every
    step between the targets and the signatures on the device: no residue comes back to the host. files: protein FASTA (translate=None), or nucleotide
    FASTA whose candidates are the six-frame ORFs (translate=True, SPEC 14) or the called genes (translate="genes", SPEC 15; gene: further gene_call
    parameters). cutoff, score, filter_p, region, min_aa, table, prefilter and msv_p as universal_genes() takes them; bias=True (host-side best hits) is
    not offered: ValueError. A round takes genomes_per_call files: their targets (_dev_targets), the staged
    search universal_genes() would choose, best_hits_dev, for region != "protein" the trace / envelopes / alignments of the best-hit matrix as a pair list,
    gs_hmm_hit_records_dev, gs_sketch_batch_dev. Per round the signatures, the genome offsets, the hit lengths, best_rec and the item counts come back.
    -> (signatures [n_files, m] - zeros for a file without a hit -, uint64 hits per file, uint64 residues sketched per file, uint32 [n_files, n_prof]
    record numbers inside each file as universal_genes() returns them, stats: seconds per stage of UNIVERSAL_STAGES under "stage_s", "wall_s", "rounds")"""
    import os
    import time
    if score not in ("viterbi", "forward"):
        raise ValueError("score: 'viterbi' or 'forward'")
    if region not in ("protein", "aligned", "envelope", "alignment"):
        raise ValueError("region: 'protein', 'aligned', 'envelope' or 'alignment'")
    if bias:
        raise ValueError("bias=True takes its best hits on the host: universal_genes() offers it, universal_sketch() does not")
    if translate not in (None, False, True, "genes"):
        raise ValueError("translate: None, True or 'genes'")
    if sketcher.params.c.data_t != DATA["aa"]:
        raise ValueError("universal genes are proteins: an amino-acid sketcher")
    per = int(genomes_per_call)
    if per < 1:
        raise ValueError("genomes_per_call: at least 1")
    pre_msv, pre_vit16 = _check_prefilter(prefilter)
    ctx = ctx or sketcher.ctx
    db = _as_hmm_db(hmm, ctx)
    ctx = db.ctx
    fwd = score == "forward"
    vf_floor = db.vf_floor(fwd, filter_p, cutoff) if pre_vit16 else None
    thr = db.thresholds(cutoff)
    files = [os.fsdecode(f) for f in files]
    n, npf, m = len(files), len(db), sketcher.params.c.sketch_size
    sig = np.zeros((n, m), sketcher.sig_dtype())
    nrec, nsym = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    local = np.full((n, npf), _lib.HMM_NO_HIT, np.uint32)
    stage = dict.fromkeys(UNIVERSAL_STAGES, 0.0)
    t_all = t = time.perf_counter()

    def lap(name):
        nonlocal t
        now = time.perf_counter()
        stage[name] += now - t
        t = now
    rounds = 0
    for f0 in range(0, n, per) if npf else ():
        chunk = files[f0:f0 + per]
        ng = len(chunk)
        rounds += 1
        t = time.perf_counter()
        dev = _dev_targets(ctx, chunk, translate, min_aa, _orf_max_aa(fwd or region in ("envelope", "alignment"), region == "aligned"), table, gene)
        lap("targets")
        with _DevScope(ctx) as out:
            try:
                if dev.n == 0:
                    continue
                d_score = dev.search_dev(db, fwd, filter_p, pre_msv, msv_p, vf_floor)
                lap("search")
                d_rec = dev.mem.new(4 * ng * npf)
                db.best_hits_dev(d_score, dev.n, dev.mem.up(dev.genome_orf_off), ng, dev.mem.up(thr), d_rec, dev.mem.new(4 * ng * npf))
                rec = ctx.download(d_rec, (ng, npf), np.uint32)
                lap("best_hits")
                hit = rec != _lib.HMM_NO_HIT
                if not hit.any():
                    continue
                spans = (None, None, _lib.HMM_DOM_WORDS, 8)
                if region != "protein":
                    spans = _hit_spans_dev(db, dev, d_rec, ng * npf, region, dev.mem)[:4]
                    lap("spans")
                cap_rec, cap_aa = int(hit.sum()), int(dev.aa_len[rec[hit]].sum())
                aa_bytes = (cap_aa + 7) // 8 * 8 + 8
                d_aa, d_os, d_ol, d_goff = out.new(aa_bytes), out.new(8 * cap_rec), out.new(8 * cap_rec), out.new(8 * (ng + 1))
                n_hit, n_aa = hit_records_dev(ctx, d_rec, ng, npf, dev.d_aa, dev.d_as, dev.d_al, dev.n, cap_rec, cap_aa, d_aa, d_os, d_ol, d_goff, *spans)
                base = dev.genome_orf_off[:-1].astype(np.uint32)[:, None]
            finally:
                dev.close()                                 # the targets are not needed any more: the sketcher reads the compacted copy
            lap("hit_records")
            d_sig = out.new(ng * m * sig.dtype.itemsize)
            check(ctx.L.gs_sketch_batch_dev(ctx.h, C.byref(sketcher.params.c), d_aa, aa_bytes, d_os, d_ol, n_hit, d_goff, ng, d_sig))
            got = ctx.download(d_sig, (ng, m), sig.dtype)
            goff = ctx.download(d_goff, (ng + 1,), np.uint64).astype(np.int64)
            csum = np.concatenate([[0], np.cumsum(ctx.download(d_ol, (n_hit,), np.uint64).astype(np.int64))])
            lap("sketch")
        has = goff[1:] > goff[:-1]
        sig[f0:f0 + ng][has] = got[has]
        nrec[f0:f0 + ng] = goff[1:] - goff[:-1]
        nsym[f0:f0 + ng] = csum[goff[1:]] - csum[goff[:-1]]
        local[f0:f0 + ng] = np.where(hit, rec - base, rec)
    return sig, nrec, nsym, local, {"stage_s": stage, "wall_s": time.perf_counter() - t_all, "rounds": rounds}


# ---- bigsig (binaux/src/bin/bigsig.rs; SPEC 11) -----------------------------------------------------------------------------------------
def _text_records(groups, quals=None):
    """groups: a list of lists of records (ASCII bytes) -> (text, qual or None, rec_begin, rec_end, group_rec_off) for the host forms"""
    recs = [r for g in groups for r in g]
    text = np.frombuffer(b"".join(recs), dtype=np.uint8) if recs else np.zeros(0, np.uint8)
    qual = None
    if quals is not None:
        qrecs = [q for g in quals for q in g]
        if [len(q) for q in qrecs] != [len(r) for r in recs]:
            raise ValueError("every record needs as many quality bytes as it has text bytes")
        qual = np.frombuffer(b"".join(qrecs), dtype=np.uint8) if qrecs else np.zeros(0, np.uint8)
    end = np.cumsum([len(r) for r in recs], dtype=np.uint64) if recs else np.zeros(0, np.uint64)
    begin = np.concatenate([np.zeros(1, np.uint64), end[:-1]]) if recs else np.zeros(0, np.uint64)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum([len(g) for g in groups], dtype=np.uint64)]).astype(np.uint64)
    return text, qual, begin, end, off


def bigsi_positions(v, num_hash, bloom_size):
    """SPEC 11: the num_hash rows of the k-mer value v (host arithmetic)"""
    out = np.zeros(int(num_hash), np.uint64)
    check(_lib.load().gs_bigsi_positions(int(v), int(num_hash), int(bloom_size), _p(out)))
    return out


def bigsi_split(text, qual=None, min_phred=15, min_len=1):
    """SPEC 11: the segments of a text, list of (offset of the first base, bases); a non-ACGT byte or a base below min_phred ends a segment"""
    L = _lib.load()
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    q = None if qual is None else np.frombuffer(bytes(qual), dtype=np.uint8)
    n = C.c_uint64()
    check(L.gs_bigsi_split(_p(t) if len(t) else None, _p(q) if q is not None and len(q) else None, len(t), int(min_phred), int(min_len), 0, None, None, C.byref(n)))
    b, l = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
    check(L.gs_bigsi_split(_p(t) if len(t) else None, _p(q) if q is not None and len(q) else None, len(t), int(min_phred), int(min_len), n.value, _p(b), _p(l), C.byref(n)))
    return [(int(x), int(y)) for x, y in zip(b, l)]


def bigsi_tail(t_c, bloom_size, num_hash, n_kmers, best_hits):
    """SPEC 11: P(X >= best_hits), X ~ Binomial(n_kmers, (t_c / bloom_size)^num_hash) (host arithmetic)"""
    return _lib.load().gs_bigsi_tail(int(t_c), int(bloom_size), int(num_hash), int(n_kmers), int(best_hits))


BIGSI_MINI_TILE = 63        # GS_BIGSI_MINI_TILE of gsearch_amd.h: the windows a wavefront of the minimizer kernel takes at a time


def bigsi_minimizers(text, k, m, qual=None, min_phred=15, data_t="dna"):
    """SPEC 11.1: the minimizer occurrences of one text (window k, minimizer m) in order -> (values u64, offsets in text of each m-mer's first base u64);
    host arithmetic"""
    L = _lib.load()
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    q = None if qual is None else np.frombuffer(bytes(qual), dtype=np.uint8)
    if q is not None and len(q) != len(t):
        raise ValueError("the text needs as many quality bytes as it has bytes")
    dt = DATA[data_t] if isinstance(data_t, str) else int(data_t)
    tp, qp = _p(t) if len(t) else None, _p(q) if q is not None and len(q) else None
    n = C.c_uint64()
    check(L.gs_bigsi_minimizers(tp, qp, len(t), int(min_phred), int(k), int(m), dt, 0, None, None, C.byref(n)))
    v, pos = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
    check(L.gs_bigsi_minimizers(tp, qp, len(t), int(min_phred), int(k), int(m), dt, n.value, _p(v), _p(pos), C.byref(n)))
    return v, pos


def bigsig_write_reads(prefix, accessions, read_ids, best_colour, best_hits, n_kmers, accept):
    """`{prefix}_reads.txt` and `{prefix}_counts.txt` (SPEC 11)"""
    acc = (C.c_char_p * max(len(accessions), 1))(*[a.encode() for a in accessions])
    ids = (C.c_char_p * max(len(read_ids), 1))(*[r.encode() for r in read_ids])
    bc, bh, nk = (np.ascontiguousarray(x, dtype=np.uint32) for x in (best_colour, best_hits, n_kmers))
    ac = np.ascontiguousarray(accept, dtype=np.uint8)
    check(_lib.load().gs_bigsig_write_reads(str(prefix).encode(), acc, len(accessions), ids, len(read_ids), _p(bc), _p(bh), _p(nk), _p(ac)))


BIGSI_VERDICTS = ("too_short", "no_hits", "no_significant_hits", "unique", "tied")      # GS_BIGSI_TOO_SHORT .. GS_BIGSI_TIED of gsearch_amd.h (SPEC 11.2)


def bigsi_verdict_code(n_kmers, best_hits, n_tied, tail, fp_correct):
    """SPEC 11.2: the verdict table alone (host arithmetic) -> an index into BIGSI_VERDICTS"""
    return int(_lib.load().gs_bigsi_verdict_code(int(n_kmers), int(best_hits), int(n_tied), float(tail), float(fp_correct)))


def bigsig_write_report(prefix, accessions, read_ids, n_kmers, best_hits, n_tied, tied, verdict):
    """the six-field `{prefix}_reads.txt` and `{prefix}_counts.txt` (SPEC 11.2); tied: (n_reads, max_ties) u32"""
    acc = (C.c_char_p * max(len(accessions), 1))(*[a.encode() for a in accessions])
    ids = (C.c_char_p * max(len(read_ids), 1))(*[r.encode() for r in read_ids])
    nk, bh, nt = (np.ascontiguousarray(x, dtype=np.uint32) for x in (n_kmers, best_hits, n_tied))
    td = np.ascontiguousarray(tied, dtype=np.uint32)
    if td.ndim != 2 or td.shape[0] != len(read_ids):
        raise ValueError("tied is (n_reads, max_ties)")
    vd = np.ascontiguousarray(verdict, dtype=np.uint8)
    check(_lib.load().gs_bigsig_write_report(str(prefix).encode(), acc, len(accessions), ids, len(read_ids), td.shape[1], _p(nk), _p(bh), _p(nt), _p(td), _p(vd)))


class Bigsi:
    """A bit-sliced Bloom index of genomes (bigsig): bloom_size rows, one column ("colour") per genome in the order added; the matrix lives on the device."""

    def __init__(self, k, num_hash, bloom_size, capacity, data_t="dna", ctx=None, minimizer=0, coverage_filter=0, minimizer_len=0, _handle=None):
        """minimizer_len = m > 0: a minimizer index (SPEC 11.1) of window length k. minimizer / coverage_filter are the two struct fields that must stay 0."""
        self.ctx = ctx or default_context()
        self.L = self.ctx.L
        if _handle is not None:
            self.h = _handle
            return
        prm = _lib.BigsiParamsC(int(k), int(num_hash), int(bloom_size), DATA[data_t] if isinstance(data_t, str) else int(data_t), int(minimizer),
                                int(coverage_filter))
        h = C.c_void_p()
        if minimizer_len:
            check(self.L.gs_bigsi_create_mini(self.ctx.h, C.byref(prm), int(minimizer_len), int(capacity), C.byref(h)))
        else:
            check(self.L.gs_bigsi_create(self.ctx.h, C.byref(prm), int(capacity), C.byref(h)))
        self.h = h

    @classmethod
    def new(cls, k, num_hash, bloom_size, capacity, **kw):
        return cls(k, num_hash, bloom_size, capacity, **kw)

    def close(self):
        if getattr(self, "h", None):
            self.L.gs_bigsi_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if not _exiting[0]:
                self.close()
        except Exception:
            pass

    def info(self):
        d = _lib.BigsiDescC()
        check(self.L.gs_bigsi_info(self.h, C.byref(d)))
        return {"k": d.prm.k, "num_hash": d.prm.num_hash, "bloom_size": d.prm.bloom_size, "data_t": d.prm.data_t, "n_colours": d.n_colours,
                "colour_capacity": d.colour_capacity, "row_words": d.row_words, "minimizer_len": self.L.gs_bigsi_minimizer_len(self.h)}

    def add_genomes(self, genomes, accessions=None, quals=None, min_phred=15, min_count=1):
        """genomes: a list of lists of records (ASCII bytes), one new colour each; quals: the same shape, quality bytes; min_count >= 2: the coverage
        filter (SPEC 11.1) - within each colour only values that occur that often are inserted"""
        text, qual, b, e, off = _text_records(genomes, quals)
        names = None if accessions is None else self.accessions() + list(accessions)
        tp, qp = _p(text) if len(text) else None, _p(qual) if qual is not None and len(qual) else None
        if int(min_count) > 1:
            check(self.L.gs_bigsi_add_batch_min_count(self.h, tp, qp, int(min_phred), _p(b), _p(e), len(b), _p(off), len(genomes), int(min_count)))
        else:
            check(self.L.gs_bigsi_add_batch(self.h, tp, qp, int(min_phred), _p(b), _p(e), len(b), _p(off), len(genomes)))
        if names is not None:
            self.set_accessions(names)

    def add_genomes_dev(self, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_genome_rec_off, n_genomes, min_count=1):
        """the packed layout of gs_sketch_batch_dev, every pointer device memory; queued on the context's stream (with min_count >= 2 the host waits once
        per colour for the size of its value list)"""
        if int(min_count) > 1:
            check(self.L.gs_bigsi_add_batch_min_count_dev(self.h, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_genome_rec_off, n_genomes, int(min_count)))
        else:
            check(self.L.gs_bigsi_add_batch_dev(self.h, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_genome_rec_off, n_genomes))

    def add_files(self, paths, accessions=None, quality=15, min_count=1):
        """one colour per FASTA / FASTQ file (plain, gz, bz2, xz), every record of the file; FASTQ bases below `quality` end a segment"""
        genomes, quals, any_q = [], [], False
        for p in paths:
            recs, qs = _read_seq_records(read_fasta_file(p))
            genomes.append([r for _, r in recs])
            quals.append(qs if qs is not None else [b"~" * len(r) for _, r in recs])
            any_q = any_q or qs is not None
        self.add_genomes(genomes, accessions=accessions, quals=quals if any_q else None, min_phred=quality, min_count=min_count)

    def set_accessions(self, names):
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        check(self.L.gs_bigsi_set_accessions(self.h, arr, len(names)))

    def accessions(self):
        nb = C.c_uint64()
        check(self.L.gs_bigsi_accessions(self.h, None, 0, C.byref(nb)))
        buf = C.create_string_buffer(max(nb.value, 1))
        check(self.L.gs_bigsi_accessions(self.h, buf, nb.value, C.byref(nb)))
        return [x.decode() for x in buf.raw[:nb.value].split(b"\0")[:-1]]

    def bits_set(self, return_kmers=False):
        """t_c of every colour (and, on request, the k-mer occurrences fed)"""
        n = self.info()["n_colours"]
        t, q = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        check(self.L.gs_bigsi_bits_set(self.h, 0, n, _p(t), _p(q)))
        return (t, q) if return_kmers else t

    def rows(self, rows):
        """the named rows as (len(rows), row_words) u64"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros((len(r), self.info()["row_words"]), np.uint64)
        check(self.L.gs_bigsi_rows(self.h, _p(r), len(r), _p(out)))
        return out

    def query(self, reads, quals=None, min_phred=15, down_sample=1, dense=False):
        """reads: a list of lists of records (the mates of a pair: two records) -> (n_kmers, best_colour, best_hits[, counts (n_reads, n_colours)])"""
        text, qual, b, e, off = _text_records(reads, quals)
        n = len(reads)
        nk, bc, bh = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        cnt = np.zeros((n, self.info()["n_colours"]), np.uint32) if dense else None
        check(self.L.gs_bigsi_query(self.h, _p(text) if len(text) else None, _p(qual) if qual is not None and len(qual) else None, int(min_phred), _p(b), _p(e),
                                    len(b), _p(off), n, int(down_sample), _p(nk), _p(bc), _p(bh), _p(cnt)))
        return (nk, bc, bh, cnt) if dense else (nk, bc, bh)

    def query_dev(self, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_read_rec_off, n_reads, d_n_kmers, d_best_colour, d_best_hits, d_counts=None,
                  down_sample=1):
        check(self.L.gs_bigsi_query_dev(self.h, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_read_rec_off, n_reads, int(down_sample), d_n_kmers,
                                        d_best_colour, d_best_hits, d_counts))

    def classify_dev(self, n_reads, d_n_kmers, d_best_colour, d_best_hits, fp_correct, d_tail, d_accept):
        check(self.L.gs_bigsi_classify_dev(self.h, n_reads, d_n_kmers, d_best_colour, d_best_hits, float(fp_correct), d_tail, d_accept))

    def classify(self, n_kmers, best_colour, best_hits, fp_correct):
        """(tail f64, accept bool) of every read; fp_correct is the threshold itself (bigsig passes 10^-p)"""
        n = len(n_kmers)
        if n == 0:
            return np.zeros(0, np.float64), np.zeros(0, bool)
        c = self.ctx
        ptrs = [c.alloc(4 * n) for _ in range(3)] + [c.alloc(8 * n), c.alloc(n)]
        try:
            for ptr, a in zip(ptrs, (n_kmers, best_colour, best_hits)):
                c.upload(ptr, np.ascontiguousarray(a, dtype=np.uint32))
            self.classify_dev(n, ptrs[0], ptrs[1], ptrs[2], fp_correct, ptrs[3], ptrs[4])
            return c.download(ptrs[3], n, np.float64), c.download(ptrs[4], n, np.uint8).astype(bool)
        finally:
            for ptr in ptrs:
                c.free(ptr)

    def query_ties(self, reads, quals=None, min_phred=15, down_sample=1, max_ties=16):
        """SPEC 11.2: reads as in query -> (n_kmers, best_hits, n_tied, tied (n_reads, max_ties), sig_colour): every colour that reaches best_hits is counted,
        the max_ties smallest are listed (UINT32_MAX behind them), sig_colour is the tied colour with the fewest bits set"""
        text, qual, b, e, off = _text_records(reads, quals)
        n, mt = len(reads), int(max_ties)
        nk, bh, nt, sc = (np.zeros(n, np.uint32) for _ in range(4))
        td = np.zeros((n, mt if 1 <= mt <= 1024 else 1), np.uint32)
        check(self.L.gs_bigsi_query_ties(self.h, _p(text) if len(text) else None, _p(qual) if qual is not None and len(qual) else None, int(min_phred), _p(b), _p(e),
                                         len(b), _p(off), n, int(down_sample), mt, _p(nk), _p(bh), _p(nt), _p(td), _p(sc)))
        return nk, bh, nt, td, sc

    def query_ties_dev(self, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_read_rec_off, n_reads, d_n_kmers, d_best_hits, d_n_tied, d_tied, d_sig_colour,
                       down_sample=1, max_ties=16):
        """d_tied: n_reads x max_ties u32; queued on the context's stream"""
        check(self.L.gs_bigsi_query_ties_dev(self.h, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_read_rec_off, n_reads, int(down_sample), int(max_ties),
                                             d_n_kmers, d_best_hits, d_n_tied, d_tied, d_sig_colour))

    def verdict_dev(self, n_reads, d_n_kmers, d_best_hits, d_n_tied, d_sig_colour, fp_correct, d_tail, d_verdict):
        check(self.L.gs_bigsi_verdict_dev(self.h, n_reads, d_n_kmers, d_best_hits, d_n_tied, d_sig_colour, float(fp_correct), d_tail, d_verdict))

    def verdict(self, n_kmers, best_hits, n_tied, sig_colour, fp_correct):
        """(tail f64 of sig_colour, verdict u8 - an index into BIGSI_VERDICTS) of every read; fp_correct is the threshold itself"""
        n = len(n_kmers)
        if n == 0:
            return np.zeros(0, np.float64), np.zeros(0, np.uint8)
        c = self.ctx
        ptrs = [c.alloc(4 * n) for _ in range(4)] + [c.alloc(8 * n), c.alloc(n)]
        try:
            for ptr, a in zip(ptrs, (n_kmers, best_hits, n_tied, sig_colour)):
                c.upload(ptr, np.ascontiguousarray(a, dtype=np.uint32))
            self.verdict_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], fp_correct, ptrs[4], ptrs[5])
            return c.download(ptrs[4], n, np.float64), c.download(ptrs[5], n, np.uint8)
        finally:
            for ptr in ptrs:
                c.free(ptr)

    def save(self, path):
        check(self.L.gs_bigsi_save(self.h, str(path).encode()))

    @staticmethod
    def describe(path):
        """the fixed header of a .gsbx file as it stands there (host only, no context; SPEC 16.2); has_accessions and digest are filled by verify"""
        d = _lib.BigsiFileDescriptionC()
        check(_lib.load().gs_bigsi_describe(str(path).encode(), C.byref(d)))
        return {name: int(getattr(d, name)) for name, _ in d._fields_}

    @staticmethod
    def verify(path):
        """everything load checks before it asks the device for memory, with load's codes (host only, no context; SPEC 16.2): the header, whether any accession is
        non-empty, and the FNV-1a digest of every byte behind the header (SPEC 16.3)"""
        d = _lib.BigsiFileDescriptionC()
        check(_lib.load().gs_bigsi_verify(str(path).encode(), C.byref(d)))
        return {name: int(getattr(d, name)) for name, _ in d._fields_}

    @classmethod
    def load(cls, path, ctx=None, capacity=0):
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(ctx.L.gs_bigsi_load(ctx.h, str(path).encode(), int(capacity), C.byref(h)))
        return cls(0, 0, 0, 0, ctx=ctx, _handle=h)


def _hnswrs_description(d):
    out = {name: int(getattr(d, name)) for name, _ in d._fields_ if name not in ("distance", "t_name")}
    out["distance"], out["t_name"] = d.distance.decode("utf-8", "replace"), d.t_name.decode("utf-8", "replace")
    return out


def hnswrs_describe(basename):
    """the description at the head of <basename>.hnsw.graph as it stands there - dump mode, M, layers, ef, nb_point, dimension, distance and T names, kind or -1
    (the reference's get_hnsw_type, reloadhnsw.rs:13-38). Host only, no context; the verify-only fields are 0."""
    d = _lib.HnswrsDescriptionC()
    check(_lib.load().gs_hnswrs_describe(str(basename).encode(), C.byref(d)))
    return _hnswrs_description(d)


def hnswrs_verify(basename):
    """everything Hnsw.load_hnswrs checks before it touches the device, with its codes (SPEC 16.1). Host only, no context. The description plus what a load would
    build: n_upper, entry, ids_are_nodes and the FNV-1a digest of graph, vectors and ids (SPEC 16.3)."""
    d = _lib.HnswrsDescriptionC()
    check(_lib.load().gs_hnswrs_verify(str(basename).encode(), C.byref(d)))
    return _hnswrs_description(d)


def _strip_breaks(b):
    return b.replace(b"\n", b"").replace(b"\r", b"")


def _read_seq_records(text):
    """FASTA or FASTQ (by the first non-blank byte) -> ([(id, sequence without line breaks)], [quality strings] or None)"""
    if text.lstrip()[:1] == b"@":
        recs, quals = [], []
        for rid, sb, se in fastq_scan(text):
            seq = _strip_breaks(text[sb:se])
            pos = text.index(b"\n", text.index(b"+", se)) + 1             # the quality text follows the '+' line
            q = bytearray()
            while len(q) < len(seq):
                nl = text.find(b"\n", pos)
                nl = len(text) if nl < 0 else nl
                q += text[pos:nl].rstrip(b"\r")
                pos = nl + 1
            recs.append((rid, seq))
            quals.append(bytes(q[:len(seq)]))
        return recs, quals
    return [(rid, _strip_breaks(text[sb:se])) for rid, sb, se in fasta_scan(text, skip_capsid=False)], None


def read_ref_list(path):
    """bigsig's reference list: `accession\tpath` per line -> [(accession, path)]; an accession listed twice is GS_ERR_INVALID"""
    out, seen = [], set()
    for line in read_path_list(path):
        acc, _, fpath = line.partition("\t")
        if not fpath or acc in seen:
            raise GsError(_lib.GS_ERR_INVALID, "reference list %s: %s" % (path, "accession %r listed twice" % acc if fpath else "line %r has no tab" % line))
        seen.add(acc)
        out.append((acc, fpath.strip()))
    return out


def bigsig_construct(ref_list, out_base, k, num_hash, bloom_size, quality=15, threads=0, ctx=None, batch=64, minimizer=False, value=21, filter=0):
    """bigsig construct: one colour per line of ref_list, the index written to `{out_base}.gsbx` (`{out_base}.gsmx` with minimizer=True) and returned.
    minimizer (-m): a minimizer index of window k and minimizer length `value` (-v, default 21), k > value. filter (-f): the coverage filter, values seen
    fewer than `filter` times in a colour are left out; <= 1: none (upstream's automatic -f -1 is not built). threads: accepted, unused (files are read
    one after the other on the host)"""
    if minimizer and int(k) <= int(value):
        raise GsError(_lib.GS_ERR_INVALID, "bigsig construct: the window k = %d must be longer than the minimizer value = %d" % (k, value))
    refs = read_ref_list(ref_list)
    bx = Bigsi(k, num_hash, bloom_size, max(len(refs), 1), ctx=ctx, minimizer_len=int(value) if minimizer else 0)
    for i in range(0, len(refs), batch):
        part = refs[i:i + batch]
        bx.add_files([p for _, p in part], accessions=[a for a, _ in part], quality=quality, min_count=max(int(filter), 1))
    bx.save(str(out_base) + (".gsmx" if minimizer else ".gsbx"))
    return bx


def bigsig_identify(index, queries, prefix, down_sample=1, fp_correct=3.0, quality=15, batch=50000, ctx=None, report="best", max_ties=16):
    """bigsig identify: every read of the query file(s) against the index (a Bigsi or the path of a saved one); two query paths are the mates of pairs.
    fp_correct is bigsig's -p: the threshold is 10^-fp_correct. Writes `{prefix}_reads.txt` / `{prefix}_counts.txt`, returns the per-read arrays.
    report="best": five fields, the smallest colour with the most hits (SPEC 11). report="ties": the six fields of upstream's README - every tied
    top colour, up to max_ties of them listed, and a tied read rejected (SPEC 11.2)."""
    if report not in ("best", "ties"):
        raise GsError(_lib.GS_ERR_INVALID, "bigsig identify: report is 'best' or 'ties'")
    bx = index if isinstance(index, Bigsi) else Bigsi.load(index, ctx=ctx)
    queries = [queries] if isinstance(queries, (str, bytes)) or hasattr(queries, "__fspath__") else list(queries)
    if len(queries) not in (1, 2):
        raise GsError(_lib.GS_ERR_INVALID, "one query file, or two for pairs")
    files = [_read_seq_records(read_fasta_file(q)) for q in queries]
    n = len(files[0][0])
    if any(len(f[0]) != n for f in files):
        raise GsError(_lib.GS_ERR_INVALID, "the two query files hold different numbers of reads")
    any_q = any(f[1] is not None for f in files)
    ids = [rid for rid, _ in files[0][0]]
    ties = report == "ties"
    outs = [[] for _ in range(7 if ties else 4)]
    thr = 10.0 ** (-float(fp_correct))
    for i in range(0, n, max(int(batch), 1)):
        j = min(n, i + max(int(batch), 1))
        reads = [[f[0][r][1] for f in files] for r in range(i, j)]
        quals = [[(f[1][r] if f[1] is not None else b"~" * len(f[0][r][1])) for f in files] for r in range(i, j)] if any_q else None
        if ties:
            nk, bh, nt, td, sc = bx.query_ties(reads, quals=quals, min_phred=quality, down_sample=down_sample, max_ties=max_ties)
            tl, vd = bx.verdict(nk, bh, nt, sc, thr)
            for o, a in zip(outs, (nk, bh, nt, td, sc, tl, vd)):
                o.append(a)
            continue
        nk, bc, bh = bx.query(reads, quals=quals, min_phred=quality, down_sample=down_sample)
        _, acc = bx.classify(nk, bc, bh, thr)
        for o, a in zip(outs, (nk, bc, bh, acc)):
            o.append(a)
    if ties:
        empty = (np.zeros(0, np.uint32),) * 3 + (np.zeros((0, int(max_ties)), np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float64), np.zeros(0, np.uint8))
        nk, bh, nt, td, sc, tl, vd = (np.concatenate(o) if o else z for o, z in zip(outs, empty))
        bigsig_write_report(prefix, bx.accessions(), ids, nk, bh, nt, td, vd)
        return {"ids": ids, "n_kmers": nk, "best_hits": bh, "n_tied": nt, "tied": td, "sig_colour": sc, "tail": tl, "verdict": vd}
    nk, bc, bh, acc = (np.concatenate(o) if o else np.zeros(0, np.uint32) for o in outs)
    bigsig_write_reads(prefix, bx.accessions(), ids, bc, bh, nk, acc)
    return {"ids": ids, "n_kmers": nk, "best_colour": bc, "best_hits": bh, "accept": acc.astype(bool)}


# ----------------------------------------------------------------------------------------------------------
class DistHamming:
    """anndists::dist::DistHamming — eval(a, b) = count(a[i] != b[i]) / len, f32."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()

    def eval(self, va, vb):
        va = np.ascontiguousarray(va)
        vb = np.ascontiguousarray(vb, dtype=va.dtype)
        return float(self.eval_qxc(va[None, :], vb[None, :])[0, 0])

    def eval_qxc(self, Q, Cm):
        Q = np.ascontiguousarray(Q)
        Cm = np.ascontiguousarray(Cm, dtype=Q.dtype)
        if Q.shape[1] != Cm.shape[1]:
            raise GsError(_lib.GS_ERR_INVALID, "signature lengths differ")
        out = np.zeros((Q.shape[0], Cm.shape[0]), dtype=np.float32)
        check(self.ctx.L.gs_hamming_qxc(self.ctx.h, DTYPE_KIND[Q.dtype], Q.shape[1], _p(Q), Q.shape[0], _p(Cm), Cm.shape[0], _p(out)))
        return out

    def eval_pairs(self, A, B, ia, ib):
        A = np.ascontiguousarray(A)
        B = np.ascontiguousarray(B, dtype=A.dtype)
        ia = np.ascontiguousarray(ia, dtype=np.uint64)
        ib = np.ascontiguousarray(ib, dtype=np.uint64)
        out = np.zeros(len(ia), dtype=np.float32)
        check(self.ctx.L.gs_hamming_pairs(self.ctx.h, DTYPE_KIND[A.dtype], A.shape[1], _p(A), A.shape[0], _p(B), B.shape[0],
                                          _p(ia), _p(ib), len(ia), _p(out)))
        return out


def ani(distance, kmer_size, model=1):
    """reformat.rs:80-86 calculate_ani."""
    return _lib.load().gs_ani(float(distance), int(kmer_size), int(model))


def bindash_sketch_params(kmer_size, sketch_size, dens=0):
    """The sketcher bindash-rs builds for (kmer_size, dens): OptDens (dens = 0) or RevOptDens (dens = 1) over f32 (bindash.rs:182-226), with the
    k-mer closure of its three branches - k <= 14: the forward window, NOT canonical (bindash.rs:346-354); k = 16 and 17..32: canonical
    (bindash.rs:366-377, 388-397)."""
    if dens not in (0, 1):
        raise ValueError("Only densification = 0 or 1 are supported!")          # bindash.rs:227-229
    return SeqSketcherParams(kmer_size, sketch_size, "optdens" if dens == 0 else "revoptdens", "dna_fwd" if kmer_size <= 14 else "dna")


def bindash_distance(hamming_distance, kmer_size):
    """bindash.rs:93-99 compute_distance: j = 1 - d ; 1 - (2j/(1+j))^(1/k), with the f32 powf the reference uses."""
    j = np.float32(1.0) - np.float32(hamming_distance)
    frac = np.float32(2.0) * j / (np.float32(1.0) + j)
    return float(1.0 - float(np.power(frac, np.float32(1.0) / np.float32(kmer_size), dtype=np.float32)))


class ReqAnswer:
    """src/answer.rs:18-76 — text record of one request; only neighbours with distance < threshold are written
    (out_threshold = 0.99, dnarequest.rs:83). `seqdict` = list of (path, fasta_id, length) indexed by d_id."""

    def __init__(self, rank, req_item, neighbours):
        self.rank, self.req_item, self.neighbours = rank, req_item, neighbours

    def dump(self, seqdict, threshold, out):
        if not any(n.distance <= threshold for n in self.neighbours):
            return 0
        path, fasta_id, length = self.req_item
        out.write("\n%d\t%s\tfasta_id:\t%s\tlength:\t%d" % (self.rank, path, fasta_id, length))
        nb_match = 0
        for n in self.neighbours:
            if n.distance < threshold:
                nb_match += 1
                dpath, dfid, dlen = seqdict[n.d_id]
                out.write("\nquery_id:\t%s\tdistance:\t%s\tanswer_fasta_path\t%s\t%s \t answer_seq_len:\t %d"
                          % (path, _rust_5e(n.distance), dpath, dfid, dlen))
        return nb_match


# ---- ann (embed.rs; SPEC 8): k-NN graph statistics and a UMAP-like embedding ----------------------------------------------------------
GS_EMBED_KNBN = 8          # embed.rs:19 kgraph_from_hnsw_all(hnsw, 8)


class EmbedParams:
    """gs_embed_params: dim, epochs (E), neg_samples (S), neg_rate (r), lr, seed; the defaults come from the library (gs_embed_params_default)"""
    FIELDS = ("dim", "epochs", "neg_samples", "neg_rate", "lr", "seed")

    def __init__(self, **kw):
        d = _lib.load().gs_embed_params_default()
        for f in self.FIELDS:
            setattr(self, f, kw.pop(f, getattr(d, f)))
        if kw:
            raise TypeError("unknown embedding parameters: %s" % ", ".join(sorted(kw)))

    def c(self):
        return _lib.EmbedParamsC(int(self.dim), int(self.epochs), int(self.neg_samples), float(self.neg_rate), float(self.lr), int(self.seed))

    def __repr__(self):
        return "EmbedParams(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in self.FIELDS)


def _embed_init(init, n, dim):
    if init is None:
        return None
    init = np.ascontiguousarray(init, dtype=np.float32)
    if init.shape != (n, dim):
        raise GsError(_lib.GS_ERR_INVALID, "initial positions must be (%d, %d)" % (n, dim))
    return init


def _graph_arrays(ids, dist, cnt):
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    if ids.ndim != 2 or dist.shape != ids.shape or cnt.shape != (ids.shape[0],):
        raise GsError(_lib.GS_ERR_INVALID, "a graph is ids (n, knbn), dist (n, knbn) and cnt (n,)")
    return ids, dist, cnt


def embed_knn_graph(ids, dist, cnt, params=None, init=None, return_memb=False, ctx=None):
    """SPEC 8 embedding of any k-NN graph in node numbers (e.g. Hnsw.knn_graph of an index without caller ids, or the layer-0 lists of
    export_graph) -> (n, dim) float32 positions; return_memb: also the (n, knbn) calibrated memberships"""
    ctx = ctx or default_context()
    ids, dist, cnt = _graph_arrays(ids, dist, cnt)
    n, knbn = ids.shape
    prm = params or EmbedParams()
    init = _embed_init(init, n, prm.dim)
    out = np.zeros((n, prm.dim), np.float32)
    memb = np.zeros((n, knbn), np.float32) if return_memb else None
    check(ctx.L.gs_embed_knn_graph(ctx.h, n, knbn, _p(ids), _p(dist), _p(cnt), C.byref(prm.c()), _p(init), _p(out), _p(memb)))
    return (out, memb) if return_memb else out


def embed_knn_graph_dev(ctx, n, knbn, ids_dev, dist_dev, cnt_dev, pos_out_dev, params=None, init_dev=None, memb_out_dev=None):
    """gs_embed_knn_graph_dev: every *_dev is a device pointer (int)"""
    prm = params or EmbedParams()
    check(ctx.L.gs_embed_knn_graph_dev(ctx.h, int(n), int(knbn), ids_dev, dist_dev, cnt_dev, C.byref(prm.c()), init_dev, pos_out_dev, memb_out_dev))


def _stats_dict(st, occ, hist):
    nh = min(int(st.n), 16)
    return dict(n=int(st.n), knbn=int(st.knbn), n_edges=int(st.n_edges), n_empty=int(st.n_empty), max_occ=int(st.max_occ),
                occ_mean=float(st.occ_mean), occ_std=float(st.occ_std), occ_skew=float(st.occ_skew),
                hubs=[(int(st.hub_ids[h]), int(st.hub_occ[h])) for h in range(nh)],
                quantiles=list(_lib.EMBED_QUANTILES), q_first=np.array(st.q_first[:], np.float32), q_last=np.array(st.q_last[:], np.float32),
                occ=occ, hist=hist)


def knn_graph_stats(ids, dist, cnt, ctx=None):
    """SPEC 8 statistics of a k-NN graph in node numbers -> dict: n, knbn, n_edges, n_empty, max_occ, occ_mean / occ_std / occ_skew (k-occurrence
    moments, occ_skew = hubness), hubs [(node, occ)] (16 largest, ties by node number), q_first / q_last (quantiles of the first / last kept
    distance), occ (n,), hist (occ 0..63, then >= 64)"""
    ctx = ctx or default_context()
    ids, dist, cnt = _graph_arrays(ids, dist, cnt)
    n, knbn = ids.shape
    st, occ, hist = _lib.KnnStatsC(), np.zeros(n, np.uint32), np.zeros(_lib.EMBED_HIST_BINS + 1, np.uint64)
    check(ctx.L.gs_knn_graph_stats(ctx.h, n, knbn, _p(ids), _p(dist), _p(cnt), C.byref(st), _p(occ), _p(hist)))
    return _stats_dict(st, occ, hist)


GS_EMBQ_KQ = 200           # embed.rs:69 get_quality_estimate_from_edge_length(200)
EMBQ_TILE_Q = 256          # GS_EMBQ_TILE_Q of gsearch_amd.h: the rows of a workgroup of the counting kernel
EMBQ_TILE_P = 1024         # GS_EMBQ_TILE_P of gsearch_amd.h: the points of one LDS tile of the counting kernel


def _quality_pos(pos, n):
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[0] != n:
        raise GsError(_lib.GS_ERR_INVALID, "positions must be (%d, dim)" % n)
    return pos


def _quality_dict(s, kq, hist, arrays):
    d = dict(n=int(s.n), knbn=int(s.knbn), kq=int(kq), kq_eff=int(s.kq_eff), n_rows=int(s.n_rows), n_edges=int(s.n_edges), n_conserved=int(s.n_conserved),
             n_nomatch=int(s.n_nomatch), mean_conserved=float(s.mean_conserved), frac_conserved=float(s.frac_conserved), hist_conserved=hist,
             quantiles=list(_lib.EMBED_QUANTILES), q_edge=np.array(s.q_edge[:], np.float64), q_radius=np.array(s.q_radius[:], np.float64),
             q_ratio=np.array(s.q_ratio[:], np.float64))
    if arrays is not None:
        d["rank"], d["e2"], d["rad2"] = arrays
    return d


def _quality_outputs(n, knbn, return_arrays):
    hist = np.zeros(knbn + 1, np.uint64)
    arrays = (np.zeros((n, knbn), np.uint32), np.zeros((n, knbn), np.float32), np.zeros(n, np.float32)) if return_arrays else None
    return hist, arrays, ([_p(a) for a in arrays] if return_arrays else [None] * 3)


def embed_quality(ids, dist, cnt, pos, kq=GS_EMBQ_KQ, ctx=None, return_arrays=False):
    """SPEC 8.1: how much of every row of a k-NN graph in node numbers lies among the kq nearest points of its node at the positions `pos`
    (n, dim) -> dict: n, knbn, kq, kq_eff, n_rows, n_edges, n_conserved, n_nomatch, mean_conserved, frac_conserved, hist_conserved (knbn + 1,),
    quantiles and q_edge / q_radius / q_ratio (float64); return_arrays: also rank (n, knbn) uint32, e2 (n, knbn) and rad2 (n,) float32"""
    ctx = ctx or default_context()
    ids, dist, cnt = _graph_arrays(ids, dist, cnt)
    n, knbn = ids.shape
    pos = _quality_pos(pos, n)
    s = _lib.EmbedQualityC()
    hist, arrays, ptrs = _quality_outputs(n, knbn, return_arrays)
    check(ctx.L.gs_embed_quality(ctx.h, n, knbn, _p(ids), _p(dist), _p(cnt), _p(pos), pos.shape[1], int(kq), C.byref(s), _p(hist), *ptrs))
    return _quality_dict(s, kq, hist, arrays)


def embed_quality_dev(ctx, n, knbn, ids_dev, dist_dev, cnt_dev, pos_dev, dim, kq=GS_EMBQ_KQ, rank_out_dev=None, e2_out_dev=None, rad2_out_dev=None):
    """gs_embed_quality_dev: every *_dev is a device pointer (int); an output that is None is not computed"""
    check(ctx.L.gs_embed_quality_dev(ctx.h, int(n), int(knbn), ids_dev, dist_dev, cnt_dev, pos_dev, int(dim), int(kq), rank_out_dev, e2_out_dev, rad2_out_dev))


def embed_quality_last_ms(ctx=None):
    """milliseconds of the stages of the context's last quality call -> dict: edge, rank, radius (list, one per pass), finish, summary"""
    ctx = ctx or default_context()
    ms = np.zeros(_lib.EMBQ_TIMES, np.float64)
    check(ctx.L.gs_embed_quality_last_ms(ctx.h, _p(ms)))
    return dict(edge=float(ms[0]), rank=float(ms[1]), radius=[float(x) for x in ms[2:-2]], finish=float(ms[-2]), summary=float(ms[-1]))


def embed_quality_text(summary):
    """the fixed lines of the quality report (SPEC 8.1), as ann(out=) prints them"""
    s = summary

    def row(name, v):
        return "%s quantiles: %s\n" % (name, " ".join("%g:%.6g" % (q, x) for q, x in zip(s["quantiles"], v)))
    return ("embedding quality of %d nodes, knbn %d: %d rows with neighbours, %d edges, kq %d\n" % (s["n"], s["knbn"], s["n_rows"], s["n_edges"], s["kq_eff"])
            + "neighbourhoods without a match: %d\n" % s["n_nomatch"]
            + "neighbours conserved per matched row: mean %.6g\n" % s["mean_conserved"]
            + "edges conserved: %d, fraction %.6g\n" % (s["n_conserved"], s["frac_conserved"])
            + row("embedded edge length", s["q_edge"]) + row("embedded radius", s["q_radius"]) + row("edge / radius", s["q_ratio"]))


def write_embedding_csv(path, xy):
    """database_embedded.csv: no header, one row per node in node order (= DataId order in gsearch), the coordinates comma-separated as the
    shortest text that reads back to the same float32 ([CHOICE], SPEC 8)"""
    xy = np.asarray(xy, dtype=np.float32)
    with open(path, "w") as f:
        for row in xy:
            f.write(",".join(np.format_float_positional(v, unique=True, trim="-") for v in row) + "\n")
    return len(xy)


def ann(hnsw, stats=True, embed=False, params=None, csv_path="database_embedded.csv", knbn=GS_EMBED_KNBN, out=None, quality=None):
    """get_graph_stats_embed (embed.rs:15-70): --stats prints the k-NN graph statistics, --embed writes csv_path. Returns
    {"stats": dict or None, "embedding": (n, dim) array or None}. quality = kq (upstream: 200) with embed: the embedding just written is measured
    (SPEC 8.1), the report goes to `out` and the result gains the key "quality"; None: nothing of that"""
    res = {"stats": None, "embedding": None}
    if stats:
        st = res["stats"] = hnsw.knn_graph_stats(knbn)
        if out is not None:
            out.write("k-NN graph of %d nodes, knbn %d: %d edges, %d empty rows\n" % (st["n"], st["knbn"], st["n_edges"], st["n_empty"]))
            out.write("first neighbour distance quantiles: %s\n" % " ".join("%g:%g" % (q, v) for q, v in zip(st["quantiles"], st["q_first"])))
            out.write("last neighbour distance quantiles: %s\n" % " ".join("%g:%g" % (q, v) for q, v in zip(st["quantiles"], st["q_last"])))
            out.write("k-occurrence mean %.6g std %.6g, hubness (standardised third moment) %.6g, max %d\n" % (st["occ_mean"], st["occ_std"],
                                                                                                           st["occ_skew"], st["max_occ"]))
            out.write("largest hubs: %s\n" % " ".join("%d:%d" % h for h in st["hubs"]))
    if embed:
        xy = res["embedding"] = hnsw.embed(knbn, params)
        if csv_path:
            write_embedding_csv(csv_path, xy)
        if quality is not None:
            res["quality"] = hnsw.embed_quality(xy, knbn, quality)
            if out is not None:
                out.write(embed_quality_text(res["quality"]))
    return res


def dump_knn_graph(seqdict, node_ids, ids, dist, cnt, out):
    """hnsw2knn's neighbour-list text: one line per node, `path:` then per neighbour, in order, a tab, `path:` and the distance with six
    decimals. node_ids[i] = the caller id of row i (Hnsw.get_ids), ids / dist / cnt = Hnsw.knn_graph's answer; `seqdict` = list of
    (path, fasta_id, length) indexed by the caller id, as in ReqAnswer.dump. Returns the number of lines written."""
    for i, nid in enumerate(node_ids):
        out.write("%s:" % seqdict[int(nid)][0])
        for j in range(int(cnt[i])):
            out.write("\t%s:%.6f" % (seqdict[int(ids[i, j])][0], float(dist[i, j])))
        out.write("\n")
    return len(node_ids)


ClusterResult = namedtuple("ClusterResult", ["centre_node", "centre_id", "centre_count", "medoids", "medoid_ids", "sizes", "n_core", "iterations",
                                             "converged", "cost_core", "cost_all", "core_nodes", "core_weight"])
ClusterResult.__doc__ = """Hnsw.cluster's answer (SPEC 10). Per node, in node order: centre_node (node number of its centre), centre_id (the centre's caller
id), centre_count (mismatch count to it). medoids / medoid_ids / sizes: the k centres by ascending node number (empty for n_cluster = 0, where the
centres are the coreset points). core_nodes / core_weight: the coreset, None unless asked for."""

ComponentsResult = namedtuple("ComponentsResult", ["label_node", "label_id", "n_clusters", "n_singletons", "largest", "c_max"])
DerepResult = namedtuple("DerepResult", ["rep_node", "rep_id", "rep_count", "reps", "sizes", "n_clusters", "n_singletons", "largest", "c_max"])
DerepResult.__doc__ = """Hnsw.derep's answer (SPEC 18). Per node, in node order: rep_node (node number of its representative, itself for a representative),
rep_id (that node's caller id), rep_count (mismatch count to it). reps: the representatives' node numbers in rank order; sizes: the nodes each
received, itself included; n_clusters, n_singletons, largest, c_max: gs_derep_info."""


def ani_cut(ani_value, kmer, model, m):
    """an ANI threshold (percent) as a cut of the derep entry points -> (c_max, max_dist): c_max = the largest mismatch count c of m whose ANI by the
    forward transform ani((f32)c / (f32)m, kmer, model) is >= ani_value, max_dist = (f32)c_max / (f32)m. Found by bisection over the counts (the
    transform falls as c grows); no inverse formula is evaluated, so nothing rounds at the boundary. No count passes: GS_ERR_INVALID."""
    m, model = int(m), int(model)
    if model not in (1, 2) or not 1 <= m <= 65535 or not float(ani_value) == float(ani_value):
        raise GsError(_lib.GS_ERR_INVALID, "ani_cut: model 1 or 2, m in 1..65535, ani a number")

    def ok(c):
        return ani(float(np.float32(c) / np.float32(m)), kmer, model) >= float(ani_value)
    if not ok(0):
        raise GsError(_lib.GS_ERR_INVALID, "ani_cut: not even equal signatures reach an ANI of %r" % (ani_value,))
    lo, hi = 0, m + 1                                        # ok(lo), not ok(hi) (hi = m + 1 stands for "none")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo, float(np.float32(lo) / np.float32(m))


HNSWCORE_TYPES = {"u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "f32": np.float32}
HNSWCORE_REFUSED = ("f64", "i32", "i64")            # hnswcore.rs:163-170 also names these: no sketcher produces them (SPEC 10)


def write_cluster_csv(path, ids, centre_ids):
    """hnswcore's membership file (hnswcore.rs:13-25): one line `{data_id},{centre_data_id}` per node, in node order (SPEC 10; the upstream writer is
    not vendored, the exact layout is unverified). Returns the number of lines."""
    ids, centre_ids = np.asarray(ids, np.uint64), np.asarray(centre_ids, np.uint64)
    if ids.shape != centre_ids.shape:
        raise GsError(_lib.GS_ERR_INVALID, "one centre per id")
    with open(path, "w") as f:
        f.write("".join("%d,%d\n" % (a, b) for a, b in zip(ids.tolist(), centre_ids.tolist())))
    return len(ids)


def hnswcore(dir, fname, typename, cluster=0, fraction=0.1, out_dir=".", max_iter=15, seed=None, ctx=None):
    """hnswcore --dir dir --fname fname --typename typename [clustercore --cluster k --fraction f] (binaux/src/bin/hnswcore.rs): reloads the hnsw_rs dump
    dir/fname.hnsw.{graph,data}, clusters it (Hnsw.cluster) and writes out_dir/clustercoreset.csv (coreset.csv when cluster = 0).
    Returns (csv path, ClusterResult)."""
    import os
    if typename in HNSWCORE_REFUSED:
        raise GsError(_lib.GS_ERR_UNSUPPORTED, "hnswcore: element type %s is not a signature type of this library (served: %s)" % (typename, ", ".join(sorted(HNSWCORE_TYPES))))
    if typename not in HNSWCORE_TYPES:
        raise GsError(_lib.GS_ERR_INVALID, "hnswcore: unknown type name %r (served: %s)" % (typename, ", ".join(sorted(HNSWCORE_TYPES))))
    hn = Hnsw.load_hnswrs(os.path.join(str(dir), fname), ctx=ctx)
    try:
        if hn.dtype != np.dtype(HNSWCORE_TYPES[typename]):
            raise GsError(_lib.GS_ERR_INVALID, "hnswcore: the dump holds %s, not %s" % (hn.dtype.name, typename))
        res = hn.cluster(cluster, fraction, max_iter, seed)
        path = os.path.join(str(out_dir), "clustercoreset.csv" if cluster else "coreset.csv")
        write_cluster_csv(path, hn.get_ids(), res.centre_id)
    finally:
        hn.close()
    return path, res


def _rust_e(x, digits):
    """Rust's {:.<digits>E}: mantissa with that many decimals, exponent without padding or plus sign (6.07500E-1, 5.400E-1); `inf` and `NaN` as
    Rust's Display writes them"""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    mant, exp = ("%.*E" % (int(digits), x)).split("E")
    return "%sE%d" % (mant, int(exp))


def _rust_5e(x):
    """Rust's {:.5E} (answer.rs:58-64)"""
    return _rust_e(x, 5)


# ----------------------------------------------------------------------------------------------------------
class Hnsw:
    """hnsw_rs::Hnsw<Sig, DistHamming> as gsearch uses it."""

    def __init__(self, max_nb_connection, max_elements, max_layer, ef_construction, dist_f=None, dtype=np.float32,
                 sketch_size=None, seed=0, insert_batch=0, ctx=None):
        self.ctx = ctx or (dist_f.ctx if dist_f is not None else default_context())
        self.prm = IndexParams(DTYPE_KIND[np.dtype(dtype)], int(sketch_size or 0), int(max_nb_connection), int(max_elements),
                               int(max_layer), int(ef_construction), 1.0, 0, 0, int(seed), int(insert_batch))
        self.dtype = np.dtype(dtype)
        self.h = None

    @classmethod
    def new(cls, max_nb_connection, max_elements, max_layer, ef_construction, dist_f=None, **kw):
        return cls(max_nb_connection, max_elements, max_layer, ef_construction, dist_f, **kw)

    # setters are only legal before the first point, like the reference's use (dnasketch.rs:141,159-160)
    def modify_level_scale(self, scale_modification):
        self._frozen_check()
        self.prm.scale_modify = float(scale_modification)

    def set_extend_candidates(self, flag):
        self._frozen_check()
        self.prm.extend_candidates = int(bool(flag))

    def set_keeping_pruned(self, flag):
        self._frozen_check()
        self.prm.keep_pruned = int(bool(flag))

    def _frozen_check(self):
        if self.h is not None:
            raise GsError(_lib.GS_ERR_STATE, "index parameters are frozen once the index holds points")

    def _ensure(self, m):
        if self.h is None:
            if self.prm.m == 0:
                self.prm.m = int(m)
            h = C.c_void_p()
            check(self.ctx.L.gs_index_create(self.ctx.h, C.byref(self.prm), C.byref(h)))
            self.h = h
        if int(m) != self.prm.m:
            raise GsError(_lib.GS_ERR_INVALID, "signature length %d != index length %d" % (m, self.prm.m))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.gs_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if not _exiting[0]:
                self.close()
        except Exception:
            pass

    def get_nb_point(self):
        return 0 if self.h is None else self.ctx.L.gs_index_nb_point(self.h)

    def parallel_insert(self, datas, ids=None):
        """datas: (n, m) array (ids: optional DataIds, default nb_point..), or a list of (vector, id) pairs like the reference's
        parallel_insert(&[(&Vec<Sig>, usize)]) (dnasketch.rs:426-435); searches return the ids as d_id"""
        if isinstance(datas, (list, tuple)) and len(datas) and isinstance(datas[0], tuple):
            ids = [did for _, did in datas]
            datas = np.stack([d for d, _ in datas])
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        self._ensure(datas.shape[1])
        if ids is None:
            check(self.ctx.L.gs_index_parallel_insert(self.h, _p(datas), datas.shape[0]))
        else:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            if len(ids) != datas.shape[0]:
                raise GsError(_lib.GS_ERR_INVALID, "one id per vector")
            check(self.ctx.L.gs_index_parallel_insert_ids(self.h, _p(datas), _p(ids), datas.shape[0]))

    def set_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        check(self.ctx.L.gs_index_set_ids(self.h, _p(ids), len(ids)))

    def get_ids(self, first=0, n=None):
        n = self.get_nb_point() - first if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        check(self.ctx.L.gs_index_get_ids(self.h, first, n, _p(out)))
        return out

    def search_arrays_pid(self, datas, knbn, ef):
        """search_arrays plus hnsw_rs' PointId of every neighbour: (ids, dist, cnt, evals, pid_layer, pid_rank)"""
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "search on an empty index")
        nq = datas.shape[0]
        ids, dist = np.zeros((nq, knbn), np.uint64), np.zeros((nq, knbn), np.float32)
        cnt, ev = np.zeros(nq, np.uint32), np.zeros(nq, np.uint64)
        pl, pr = np.zeros((nq, knbn), np.uint8), np.zeros((nq, knbn), np.int32)
        check(self.ctx.L.gs_index_parallel_search_pid(self.h, _p(datas), nq, knbn, ef, _p(ids), _p(dist), _p(cnt), _p(ev), _p(pl), _p(pr)))
        return ids, dist, cnt, ev, pl, pr

    def search_arrays(self, datas, knbn, ef):
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "search on an empty index")
        nq = datas.shape[0]
        ids = np.zeros((nq, knbn), dtype=np.uint64)
        dist = np.zeros((nq, knbn), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        ev = np.zeros(nq, dtype=np.uint64)
        check(self.ctx.L.gs_index_parallel_search(self.h, _p(datas), nq, knbn, ef, _p(ids), _p(dist), _p(cnt), _p(ev)))
        return ids, dist, cnt, ev

    def search_dev(self, d_queries, nq, knbn, ef, d_ids, d_dist, d_count=None, d_evals=None):
        """gs_index_parallel_search_dev: every d_* is a device pointer (int)"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "search on an empty index")
        check(self.ctx.L.gs_index_parallel_search_dev(self.h, d_queries, int(nq), int(knbn), int(ef), d_ids, d_dist, d_count, d_evals))

    def search_merge_dev(self, d_queries, nq, knbn, ef, d_run_ids, d_run_dist, d_run_count, d_run_evals=None, d_rows=None, nr=0, id_offset=0):
        """this index as one piece of a split database (gs_index_search_merge_dev): the listed query rows (d_rows: nr ascending uint32 rows on the
        device, None: all nq) are searched and the answers, id_offset added, merged in place into their running lists under (distance, id).
        Every d_* is a device pointer (int); topk_reset_dev makes the empty lists."""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "search on an empty index")
        check(self.ctx.L.gs_index_search_merge_dev(self.h, d_queries, int(nq), d_rows, int(nr), int(knbn), int(ef), int(id_offset), d_run_ids, d_run_dist,
                                                   d_run_count, d_run_evals))

    def search_merge(self, datas, knbn, ef, run_ids, run_dist, run_count, run_evals=None, rows=None, id_offset=0):
        """the host-pointer twin (gs_index_search_merge): datas (nq, m); run_ids (nq, knbn) uint64, run_dist (nq, knbn) float32, run_count (nq,)
        uint32 and run_evals (nq,) uint64 are C-contiguous arrays updated in place; rows: ascending row numbers, None = every query"""
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "search on an empty index")
        nq = datas.shape[0]
        want = [(run_ids, np.uint64, (nq, knbn)), (run_dist, np.float32, (nq, knbn)), (run_count, np.uint32, (nq,))]
        if run_evals is not None:
            want.append((run_evals, np.uint64, (nq,)))
        for a, dt, shape in want:
            if not (isinstance(a, np.ndarray) and a.dtype == dt and a.shape == shape and a.flags.c_contiguous and a.flags.writeable):
                raise GsError(_lib.GS_ERR_INVALID, "the running lists are writable C-contiguous arrays: ids (nq, knbn) uint64, dist (nq, knbn) float32, count (nq,) uint32, evals (nq,) uint64")
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.size and (rows.min() < 0 or rows.max() > 0xFFFFFFFF):
                raise GsError(_lib.GS_ERR_INVALID, "a row number is a uint32")
            rows = rows.astype(np.uint32)
            if rows.size == 0:
                return
        check(self.ctx.L.gs_index_search_merge(self.h, _p(datas), nq, _p(rows), 0 if rows is None else len(rows), int(knbn), int(ef), int(id_offset),
                                               _p(run_ids), _p(run_dist), _p(run_count), _p(run_evals)))

    def parallel_search(self, datas, knbn, ef):
        """-> Vec<Vec<Neighbour>>, ascending distance (dnarequest.rs:353)."""
        ids, dist, cnt, _, pl, pr = self.search_arrays_pid(datas, knbn, ef)
        return [[Neighbour(int(ids[i, j]), float(dist[i, j]), (int(pl[i, j]), int(pr[i, j]))) for j in range(int(cnt[i]))] for i in range(len(ids))]

    def count_matrix(self, datas):
        """mismatch counts of every query against every node (nq x nb_point, uint16) from the dense producer the search would use"""
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        out = np.zeros((datas.shape[0], self.get_nb_point()), dtype=np.uint16)
        check(self.ctx.L.gs_index_count_matrix(self.h, _p(datas), datas.shape[0], _p(out)))
        return out

    def nearest_of(self, nodes):
        """for every node, the position in `nodes` (node numbers) that minimises (mismatch count, position), and that count (gs_index_nearest_of)
        -> (arg uint32, count uint16), one entry per node"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "nearest_of on an empty index")
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        n = self.get_nb_point()
        arg, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint16)
        check(self.ctx.L.gs_index_nearest_of(self.h, _p(nodes), len(nodes), _p(arg), _p(cnt)))
        return arg, cnt

    def cluster(self, n_cluster=0, fraction=0.1, max_iter=15, seed=None, return_coreset=False):
        """hnswcore (SPEC 10): a coreset of about fraction x nb_point nodes, n_cluster medoids on it (0: the coreset points are the centres), every
        node to its nearest centre (gs_index_cluster) -> ClusterResult. seed None: the library's default."""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "clustering of an empty index")
        prm = _lib.load().gs_cluster_params_default()
        prm.n_cluster, prm.fraction, prm.max_iter = int(n_cluster), float(fraction), int(max_iter)
        if seed is not None:
            prm.seed = int(seed)
        n, k = self.get_nb_point(), int(n_cluster)
        cen, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint16)
        med, sizes = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        info = _lib.ClusterInfoC()
        core = wgt = None
        if return_coreset:
            core, wgt = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        check(self.ctx.L.gs_index_cluster(self.h, C.byref(prm), _p(cen), _p(cnt), _p(med), _p(sizes), _p(core), _p(wgt), n if return_coreset else 0, C.byref(info)))
        ids = self.get_ids()
        p = int(info.n_core)
        return ClusterResult(cen, ids[cen.astype(np.int64)], cnt, med, ids[med.astype(np.int64)], sizes, p, int(info.iterations), int(info.converged),
                             int(info.cost_core), int(info.cost_all), core[:p] if return_coreset else None, wgt[:p] if return_coreset else None)

    def components(self, max_dist):
        """single linkage at a cut (SPEC 18, gs_index_components): nodes whose mismatch count is <= c_max (max_dist as in exact_search_arrays) are
        linked -> ComponentsResult: per node, in node order, label_node (the smallest node number of its connected component) and label_id (that
        node's caller id); the info fields n_clusters, n_singletons, largest, c_max"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "components of an empty index")
        n = self.get_nb_point()
        lab, info = np.zeros(n, np.uint64), _lib.DerepInfoC()
        check(self.ctx.L.gs_index_components(self.h, float(max_dist), _p(lab), C.byref(info)))
        return ComponentsResult(lab, self.get_ids()[lab.astype(np.int64)], int(info.n_clusters), int(info.n_singletons), int(info.largest), int(info.c_max))

    def derep(self, max_dist, priority=None):
        """greedy representatives at a cut (SPEC 18, gs_index_derep; CD-HIT's incremental clustering in its -g 1 form) -> DerepResult. priority: one
        uint64 per node, higher is better, None = all equal; ties go by node number."""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "derep of an empty index")
        n = self.get_nb_point()
        if priority is not None:
            priority = np.ascontiguousarray(priority, dtype=np.uint64)
            if priority.shape != (n,):
                raise GsError(_lib.GS_ERR_INVALID, "one priority per node")
        rep, cnt, info = np.zeros(n, np.uint64), np.zeros(n, np.uint16), _lib.DerepInfoC()
        check(self.ctx.L.gs_index_derep(self.h, float(max_dist), _p(priority), _p(rep), _p(cnt), C.byref(info)))
        is_rep = rep == np.arange(n, dtype=np.uint64)
        key = np.zeros(n, np.uint64) if priority is None else priority
        order = np.lexsort((np.arange(n), np.iinfo(np.uint64).max - key))           # priority descending, node number ascending
        reps = order[is_rep[order]].astype(np.uint64)
        sizes = np.bincount(rep.astype(np.int64), minlength=n)[reps.astype(np.int64)].astype(np.uint64)
        return DerepResult(rep, self.get_ids()[rep.astype(np.int64)], cnt, reps, sizes, int(info.n_clusters), int(info.n_singletons), int(info.largest),
                           int(info.c_max))

    def sketch_and_search_dev(self, params, d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_genome_rec_off, n_genomes, knbn, ef, d_ids, d_dist, d_count=None,
                              d_evals=None, d_sig=None):
        """sketch_and_request on device-resident genomes (gs_index_sketch_and_search_dev): every d_* is a device pointer (int)"""
        check(self.ctx.L.gs_index_sketch_and_search_dev(self.h, C.byref(params.c), d_seq, seq_bytes, d_rec_start, d_rec_len, n_rec, d_genome_rec_off, n_genomes, d_sig,
                                                        knbn, ef, d_ids, d_dist, d_count, d_evals))

    def bruteforce_search(self, datas, knbn):
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        ids = np.zeros((datas.shape[0], knbn), dtype=np.uint64)
        dist = np.zeros((datas.shape[0], knbn), dtype=np.float32)
        check(self.ctx.L.gs_index_bruteforce_search(self.h, _p(datas), datas.shape[0], knbn, _p(ids), _p(dist)))
        return ids, dist

    def exact_search_arrays(self, datas, knbn, max_dist=1.0):
        """exact knbn nearest nodes of every query by exhaustive DistHamming (gs_index_exact_search), keeping distances <= max_dist:
        (ids, dist, cnt) in the layout of search_arrays"""
        datas = np.ascontiguousarray(datas, dtype=self.dtype)
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "exact search on an empty index")
        nq = datas.shape[0]
        ids, dist, cnt = np.zeros((nq, knbn), np.uint64), np.zeros((nq, knbn), np.float32), np.zeros(nq, np.uint32)
        check(self.ctx.L.gs_index_exact_search(self.h, _p(datas), nq, knbn, float(max_dist), _p(ids), _p(dist), _p(cnt)))
        return ids, dist, cnt

    def exact_search_dev(self, d_queries, nq, knbn, d_ids, d_dist, d_count, max_dist=1.0):
        """gs_index_exact_search_dev: every d_* is a device pointer (int)"""
        check(self.ctx.L.gs_index_exact_search_dev(self.h, d_queries, nq, knbn, float(max_dist), d_ids, d_dist, d_count))

    def knn_graph(self, knbn, max_dist=1.0, first=0, n=None):
        """the database's own exact k-NN graph (hnsw2knn): for nodes first..first+n in insertion order, their knbn nearest OTHER nodes
        (gs_index_knn_graph) -> (ids, dist, cnt) in the layout of search_arrays"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "k-NN graph of an empty index")
        n = self.get_nb_point() - first if n is None else n
        ids, dist, cnt = np.zeros((n, knbn), np.uint64), np.zeros((n, knbn), np.float32), np.zeros(n, np.uint32)
        check(self.ctx.L.gs_index_knn_graph(self.h, knbn, float(max_dist), first, n, _p(ids), _p(dist), _p(cnt)))
        return ids, dist, cnt

    def knn_graph_dev(self, knbn, first, n, d_ids, d_dist, d_count, max_dist=1.0):
        """gs_index_knn_graph_dev: every d_* is a device pointer (int)"""
        check(self.ctx.L.gs_index_knn_graph_dev(self.h, knbn, float(max_dist), first, n, d_ids, d_dist, d_count))

    def embed(self, knbn=GS_EMBED_KNBN, params=None, init=None, max_dist=1.0):
        """ann --embed (embed.rs:34-64): the exact self graph of knbn neighbours (kept on the device) embedded by SPEC 8 -> (n, dim) float32,
        one row per node in node (insertion) order, also when the index holds caller ids (map rows with get_ids)"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "embedding of an empty index")
        prm = params or EmbedParams()
        n = self.get_nb_point()
        init = _embed_init(init, n, prm.dim)
        out = np.zeros((n, prm.dim), np.float32)
        check(self.ctx.L.gs_index_embed(self.h, int(knbn), float(max_dist), C.byref(prm.c()), _p(init), _p(out)))
        return out

    def embed_quality(self, pos, knbn=GS_EMBED_KNBN, kq=GS_EMBQ_KQ, max_dist=1.0, return_arrays=False):
        """the quality of the positions `pos` (n, dim; node order, as embed() returns them) against the exact self graph of knbn neighbours
        (SPEC 8.1; dict, see embed_quality)"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "embedding quality of an empty index")
        n = self.get_nb_point()
        pos = _quality_pos(pos, n)
        s = _lib.EmbedQualityC()
        hist, arrays, ptrs = _quality_outputs(n, int(knbn), return_arrays)
        check(self.ctx.L.gs_index_embed_quality(self.h, int(knbn), float(max_dist), _p(pos), pos.shape[1], int(kq), C.byref(s), _p(hist), *ptrs))
        return _quality_dict(s, kq, hist, arrays)

    def knn_graph_stats(self, knbn=GS_EMBED_KNBN, max_dist=1.0):
        """ann --stats (embed.rs:26-33): statistics of the exact self graph of knbn neighbours (dict, see knn_graph_stats; hubs are node numbers)"""
        if self.h is None:
            raise GsError(_lib.GS_ERR_STATE, "statistics of an empty index")
        st, occ, hist = _lib.KnnStatsC(), np.zeros(self.get_nb_point(), np.uint32), np.zeros(_lib.EMBED_HIST_BINS + 1, np.uint64)
        check(self.ctx.L.gs_index_knn_graph_stats(self.h, int(knbn), float(max_dist), C.byref(st), _p(occ), _p(hist)))
        return _stats_dict(st, occ, hist)

    # graph import/export in the library's dense layout (role of HnswIo::load_hnsw / file_dump)
    def import_graph(self, sigs, g):
        sigs = np.ascontiguousarray(sigs, dtype=self.dtype)
        self._ensure(sigs.shape[1])
        a = {k: np.ascontiguousarray(v) for k, v in g.items() if isinstance(v, np.ndarray)}
        U = int(g["n_upper"])
        check(self.ctx.L.gs_index_import(self.h, _p(sigs), sigs.shape[0], _p(a["levels"]), int(g["entry"]), _p(a["deg0"]),
                                         _p(a["nbr0"]), _p(a["cnt0"]), _p(a["upidx"]), U,
                                         _p(a["degU"]) if U else None, _p(a["nbrU"]) if U else None, _p(a["cntU"]) if U else None))

    def export_graph(self):
        n = self.get_nb_point()
        M, ML = self.prm.max_nb_conn, self.prm.max_layer
        levels = np.zeros(n, np.uint8)
        entry = np.zeros(1, np.int64)
        nup = np.zeros(1, np.uint64)
        check(self.ctx.L.gs_index_export(self.h, None, _p(entry), None, None, None, None, _p(nup), None, None, None))
        U = int(nup[0])
        deg0, nbr0, cnt0 = np.zeros(n, np.uint32), np.zeros((n, 2 * M), np.uint32), np.zeros((n, 2 * M), np.uint32)
        upidx = np.zeros(n, np.int32)
        degU, nbrU, cntU = np.zeros((max(U, 1), ML), np.uint32), np.zeros((max(U, 1), ML, M), np.uint32), np.zeros((max(U, 1), ML, M), np.uint32)
        check(self.ctx.L.gs_index_export(self.h, _p(levels), _p(entry), _p(deg0), _p(nbr0), _p(cnt0), _p(upidx), _p(nup),
                                         _p(degU), _p(nbrU), _p(cntU)))
        return dict(levels=levels, entry=int(entry[0]), deg0=deg0, nbr0=nbr0, cnt0=cnt0, upidx=upidx, n_upper=U,
                    degU=degU[:U], nbrU=nbrU[:U], cntU=cntU[:U])

    def get_data(self, first=0, n=None):
        n = self.get_nb_point() - first if n is None else n
        out = np.zeros((n, self.prm.m), dtype=self.dtype)
        check(self.ctx.L.gs_index_get_data(self.h, first, n, _p(out)))
        return out

    def file_dump(self, path):
        """Hnsw::file_dump counterpart (own format, dumpload.rs:31)"""
        check(self.ctx.L.gs_index_save(self.h, str(path).encode()))

    @classmethod
    def load(cls, path, ctx=None):
        """HnswIo::load_hnsw counterpart (reloadhnsw.rs:41-51)"""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(ctx.L.gs_index_load(ctx.h, str(path).encode(), C.byref(h)))
        self = cls.__new__(cls)
        self.ctx, self.h = ctx, h
        self.prm = IndexParams()
        check(ctx.L.gs_index_get_params(h, C.byref(self.prm)))
        self.dtype = KIND_DTYPE[self.prm.kind]
        return self

    def search_stats(self, reset=False):
        """device-side work counters since the last reset (include/gsearch_amd.h gs_index_search_stats)"""
        if self.h is None:
            return {}
        out = np.zeros(8, dtype=np.uint64)
        check(self.ctx.L.gs_index_search_stats(self.h, _p(out), int(reset)))
        pops = int(out[1])
        return {"join_atomics": int(out[0]), "pops": pops, "accepting_pops": int(out[2]), "wg_in_flight": int(out[3]),
                "adj_bytes": pops * int(out[4]), "pops_phase1": int(out[5]), "pops_phase2": int(out[6]), "join_shared_expansions": int(out[7])}

    def file_dump_hnswrs(self, basename, truncate_255=False):
        """Hnsw::file_dump(dir, "hnswdump") in hnsw_rs' own format: <basename>.hnsw.graph + <basename>.hnsw.data (dumpload.rs:26-31).
        truncate_255: the format keeps neighbour counts in one byte; cut longer layer-0 lists to their 255 closest entries instead of refusing"""
        check(self.ctx.L.gs_index_dump_hnswrs_ex(self.h, str(basename).encode(), 1 if truncate_255 else 0))

    @classmethod
    def load_hnswrs(cls, basename, hint=None, ctx=None):
        """HnswIo::load_hnsw counterpart for hnsw_rs dumps (reloadhnsw.rs:41-51); `hint`: an Hnsw whose parameters (capacity, level scale,
        flags, seed, insert batch) later insertions should use"""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(ctx.L.gs_index_load_hnswrs(ctx.h, str(basename).encode(), C.byref(hint.prm) if hint is not None else None, C.byref(h)))
        self = cls.__new__(cls)
        self.ctx, self.h = ctx, h
        self.prm = IndexParams()
        check(ctx.L.gs_index_get_params(h, C.byref(self.prm)))
        self.dtype = KIND_DTYPE[self.prm.kind]
        return self

    def insert_evals(self):
        return 0 if self.h is None else self.ctx.L.gs_index_insert_evals(self.h)

    def debug_fill_scratch(self, byte):
        """debugging, not for production use: fill the per-call scratch buffers of the index with `byte` (gs_index_debug_fill_scratch)"""
        if self.h is not None:
            check(self.ctx.L.gs_index_debug_fill_scratch(self.h, int(byte)))
