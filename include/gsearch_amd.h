/*
 * gsearch_amd.h — C ABI of the MI355X-native sketch-and-query hot path of gsearch.
 *
 * The reference (Rust, /root/reference) has no FFI of its own for this path: the extension points are
 * generic traits resolved at compile time. Each entry point below replaces one *batch-level* call the
 * reference makes into those traits (paths relative to /root/reference); INTEGRATION.md shows the
 * `extern "C"` block a Rust maintainer would add to bind them.
 *
 * Conventions: every function returns 0 on success and a negative GS_ERR_* code on failure; nothing
 * throws or aborts across the boundary; gs_last_error() gives a thread-local message. All pointers
 * are HOST pointers unless the name ends in `_dev`. Plain C types only.
 * Arithmetic is normative in SPEC.md.
 */
#ifndef GSEARCH_AMD_H
#define GSEARCH_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------- */
enum {
    GS_OK = 0,
    GS_ERR_INVALID = -1,      /* bad argument / unsupported parameter combination */
    GS_ERR_HIP = -2,          /* HIP runtime error (no device, OOM, launch failure) */
    GS_ERR_UNSUPPORTED = -3,  /* valid in the reference but not implemented on the device yet */
    GS_ERR_STATE = -4,        /* object used in the wrong state (e.g. search on an empty index) */
    GS_ERR_IO = -5
};
/* kmerutils::sketcharg::SketchAlgo / DataType as parsed at src/bin/gsearch.rs:181-196,258-263 */
enum { GS_ALGO_PROB3A = 0, GS_ALGO_SUPER = 1, GS_ALGO_SUPER2 = 2, GS_ALGO_HLL = 3, GS_ALGO_OPTDENS = 4, GS_ALGO_REVOPTDENS = 5,
       GS_ALGO_HMH = 6 /* HyperMinHash of hypermash (src/bin/hypermash.rs): sketch_size 16384, canonical DNA, k 1..32 (15 accepted), u16 (SPEC 7) */ };
enum { GS_HMH_REGISTERS = 16384 };
/* GS_DATA_DNA_FWD: DNA whose k-mer value is the forward window itself, WITHOUT the reverse-complement minimum - the closure bindash-rs passes
 * for k <= 14 (`kmer.get_compressed_value() & mask`, src/bin/bindash.rs:346-354; its k = 16 and k > 16 closures, :366-377,:388-397, and every
 * closure of gsearch itself, dnasketch.rs:164-169, are canonical = GS_DATA_DNA). Accepted for every k and algo; same (k -> Kmer::Val, Sig) table as DNA. */
enum { GS_DATA_DNA = 0, GS_DATA_AA = 1, GS_DATA_DNA_FWD = 2 };
/* signature element type (table SURVEY 2.2; src/dna/dnasketch.rs:499-642, src/aa/aasketch.rs:455-550) */
enum { GS_KIND_U16 = 0, GS_KIND_U32 = 1, GS_KIND_U64 = 2, GS_KIND_F32 = 3 };

const char *gs_last_error(void);
const char *gs_version(void);

/* ---------------------------------------------------------------------------------------------- */
/* Context: one per (process, GPU). Owns a HIP stream; every call on a context is enqueued on it.   */
/* Every entry point that takes a context (or an index made on one) may be called concurrently from */
/* several host threads. The synchronous host-pointer calls gs_sketch_batch, gs_hamming_qxc and      */
/* gs_hamming_pairs run side by side: every calling thread but the first gets a worker stream +      */
/* scratch of its own on the same device (GS_THREAD_CONTEXTS=0: off). Everything else - the `_dev`   */
/* calls, whose ordering on the context's stream the caller relies on, and the calls on an index -   */
/* queues on the context's one stream and scratch pool behind its lock.                              */
/* `stream` may be NULL (the context creates its own) or an existing hipStream_t to adopt.          */
typedef struct gs_ctx gs_ctx;
int   gs_ctx_create(gs_ctx **out, int device_id, void *stream);
void  gs_ctx_destroy(gs_ctx *);
int   gs_ctx_sync(gs_ctx *);
int   gs_ctx_release_scratch(gs_ctx *);   /* free the device scratch the context keeps between calls (it grows on demand) */
void *gs_ctx_stream(gs_ctx *);                         /* the hipStream_t kernels are launched on */
int   gs_ctx_device_info(gs_ctx *, int *n_cu, uint64_t *hbm_bytes, char *name, size_t name_cap);
/* HIP-event stopwatch on the context's stream (bench.py measures kernels with it) */
int   gs_ctx_timer_start(gs_ctx *);
int   gs_ctx_timer_stop(gs_ctx *, float *elapsed_ms);
/* duration (ms) and launch count of the kernels of one family since the last reset, measured with
 * HIP events around every launch when profiling is enabled (gs_ctx_profile(ctx,1)).
 * family: 0 = sketch main kernel, 1 = hamming q x c, 2 = index search kernel, 3 = index insert kernels */
int   gs_ctx_profile(gs_ctx *, int enable);
int   gs_ctx_profile_read(gs_ctx *, int family, double *total_ms, uint64_t *launches, int reset);

/* which form of the slot-min sketch kernel (optdens / revoptdens / super / super2 level 0) the LAST sketch call on this context launched:
 * out[0] = 1 when the early-rejection ("filtered") emitter ran, out[1] = 1 when the slot table lived in LDS, out[2] = workgroups per
 * genome, out[3] = launches; GS_ALGO_HMH reports {0, 1, workgroups per genome, launches}. Tests use it to prove that a parity case exercised the instantiation the bench times. */
int   gs_ctx_last_sketch_info(gs_ctx *, uint32_t out[4]);

/* plain device-memory helpers so that hosts without a HIP binding can keep data resident in HBM */
int   gs_dev_alloc(gs_ctx *, size_t bytes, void **dev_ptr);
int   gs_dev_free(gs_ctx *, void *dev_ptr);
int   gs_dev_upload(gs_ctx *, void *dst_dev, const void *src_host, size_t bytes);
int   gs_dev_download(gs_ctx *, void *dst_host, const void *src_dev, size_t bytes);
int   gs_dev_memset(gs_ctx *, void *dst_dev, int byte, size_t bytes);

/* ---------------------------------------------------------------------------------------------- */
/* Sketching: replaces SeqSketcherT::sketch_compressedkmer_seqs / sketch_compressedkmer            */
/*   call sites: src/dna/dnasketch.rs:336,357  src/dna/dnarequest.rs:272,287                        */
/*               src/aa/aasketch.rs:313,329    src/aa/aarequest.rs:268,283  src/bin/bindash.rs:81   */
/* mirrors kmerutils::sketcharg::SeqSketcherParams{kmer_size, sketch_size, algo, data_t}            */
typedef struct { uint32_t k, sketch_size, algo, data_t; } gs_sketch_params;

int    gs_check_params(const gs_sketch_params *);       /* k=15, k>32 (DNA) / k>12 (AA) -> error; hmh: see GS_ALGO_HMH */
int    gs_sig_kind(const gs_sketch_params *);           /* GS_KIND_* */
size_t gs_sig_elem_bytes(const gs_sketch_params *);
int    gs_value_bits(const gs_sketch_params *);         /* width of Kmer::Val: 32 or 64 */

/*
 * One signature per genome, in input order (asserts at dnasketch.rs:338,359).
 *   seq        DNA: 2-bit packed, base i in byte i>>2 at bits [6-2(i&3), 7-2(i&3)] (SPEC 1.1);
 *              AA : one ASCII letter per residue, already alphabet-filtered (aafiles.rs:11-28).
 *   seq_bytes  size of seq; for the _dev variant the allocation must extend to a multiple of 8 bytes.
 *   record r   = bases/residues [rec_start[r], rec_start[r]+rec_len[r]); k-mers never span records.
 *   genome g   = records [genome_rec_off[g], genome_rec_off[g+1]).  `--block` mode = one record/genome.
 *   sig_out    n_genomes x sketch_size elements of gs_sig_kind(), caller owned.
 * Thread-safe: callable concurrently from many host threads on ONE context, like the reference's &self sketcher cloned into
 * --nbthreads workers (dnasketch.rs:252,305,322): gs_sketch_batch calls of different threads overlap on the device (worker streams; 16 threads
 * x 4 genomes of 2 Mbp per call: 34.7 k genomes/s against 19.2 k queued, profiles/r04_thread_contexts.log); gs_sketch_batch_dev queues on the context's stream.
 */
int gs_sketch_batch(gs_ctx *, const gs_sketch_params *, const void *seq, uint64_t seq_bytes,
                    const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                    const uint64_t *genome_rec_off, uint64_t n_genomes, void *sig_out);
/* same, every pointer in device memory, asynchronous on the context's stream */
int gs_sketch_batch_dev(gs_ctx *, const gs_sketch_params *, const void *seq_dev, uint64_t seq_bytes,
                        const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                        const uint64_t *genome_rec_off_dev, uint64_t n_genomes, void *sig_out_dev);
/* ---- FASTA ingest: the reader side of src/dna/dnafiles.rs:43-193 for already-decompressed text ---- */
/* host: record boundaries. Record r = sequence text bytes [seq_begin[r], seq_end[r]) (newlines included) and the header's first
 * word [id_begin[r], +id_len[r]). Records whose header LINE (needletail id(): description included) contains "capsid" are skipped
 * when skip_capsid != 0 (dnafiles.rs:62-67).
 * Arrays may be NULL / cap 0 to count only; *n_rec_out = number of records kept. */
int gs_fasta_scan(const char *buf, uint64_t n, int skip_capsid, uint64_t cap, uint64_t *seq_begin, uint64_t *seq_end,
                  uint64_t *id_begin, uint32_t *id_len, uint64_t *n_rec_out);
/* device: filter + case-fold + 2-bit pack the text of n_rec records (Sequence::encode_and_add, dnafiles.rs:70-71,148-149; every
 * non-ACGT byte, newlines included, is dropped). text_dev: raw text; seq_begin/seq_end: HOST offsets from gs_fasta_scan;
 * packed_dev: ZEROED device buffer >= n_bytes/4 + 8*n_rec + 64 bytes; rec_start_out/rec_len_out: HOST, ready for gs_sketch_batch_dev. */
int gs_pack_fasta_dev(gs_ctx *, const void *text_dev, uint64_t n_bytes, const uint64_t *seq_begin, const uint64_t *seq_end,
                      uint64_t n_rec, void *packed_dev, uint64_t *rec_start_out, uint64_t *rec_len_out);
/* amino acids: drop everything outside the 20-letter alphabet (filter_out_non_aa, src/aa/aafiles.rs:11-28; newlines of the raw text go
 * with it) from the text of n_rec records; kept letters come out in upper case, as from gs_filter_aa. out_dev: >= n_bytes bytes;
 * rec_start_out / rec_len_out: HOST, residue coordinates. */
int gs_filter_aa_dev(gs_ctx *, const void *text_dev, uint64_t n_bytes, const uint64_t *seq_begin, const uint64_t *seq_end,
                     uint64_t n_rec, void *out_dev, uint64_t *rec_start_out, uint64_t *rec_len_out);
/* ---- files: the reader side of sketchandstore_dir_compressedkmer, src/dna/dnasketch.rs:240-300 ---- */
/* src/utils/files.rs:117-146: 1 when the name carries a FASTA suffix gsearch accepts for data_t (fna fa fasta / faa, also .gz .xz .bz2) */
int  gs_is_fasta_file(const char *path, int data_t);
/* whole file in memory, gzip (multi-member) / bzip2 / xz decompressed by magic bytes like needletail (files.rs:220-250); release the
 * malloc-ed *text_out with gs_host_free */
int  gs_read_fasta_file(const char *path, void **text_out, uint64_t *n_out);
void gs_host_free(void *);
/* files.rs:148-215,345-455: accepted files under dir, recursively, name order. paths_buf NULL to size (*n_out files, *bytes_out bytes),
 * then a buffer that receives the NUL-terminated paths back to back */
int  gs_list_fasta_files(const char *dir, int data_t, char *paths_buf, uint64_t cap_bytes, uint64_t *n_out, uint64_t *bytes_out);
/* One signature per file, input order. Groups of `pio` files (--pio, files.rs:258-341; 0 -> 32) are read + decompressed + scanned by
 * n_threads host threads (0 -> the CPUs the process may use: affinity mask and cgroup quota) while the previous group crosses PCIe from pinned memory on a copy stream and the one before is
 * filtered / 2-bit packed / sketched on the context's stream. block_mode 0: k-mers never span records (process_file_by_sequence,
 * dnafiles.rs:43-107); 1: --block, records concatenated (process_file_in_one_block, dnafiles.rs:200-262); `capsid` records skipped.
 * sig_out: HOST n_files x sketch_size. Optional per-file n_records_out / n_symbols_out (HOST) and stats_out[4] = {host read+decode+scan
 * seconds summed over threads, seconds waited for PCIe, seconds in device pack + sketch, wall seconds}. */
int  gs_sketch_files(gs_ctx *, const gs_sketch_params *, const char *const *paths, uint64_t n_files, int block_mode, uint32_t pio,
                     uint32_t n_threads, void *sig_out, uint64_t *n_records_out, uint64_t *n_symbols_out, double *stats_out);
/* the same call with a SIZED statistics array: the first min(stats_cap, GS_SKETCH_FILES_STATS) entries of {the four above, .gz members inflated by
 * the device kernel (counted per file: a single-member file, or a bgzip file all of whose members the kernel inflated and found good; not the members
 * that stayed with the host decoders or were handed back), members the device path handed back to the host decoders (multi-member files, a trailer /
 * CRC-32 that does not check, no room)} are written - a later library may know more entries, a caller never receives more than it made room for. */
enum { GS_SKETCH_FILES_STATS = 6 };
int  gs_sketch_files_ex(gs_ctx *, const gs_sketch_params *, const char *const *paths, uint64_t n_files, int block_mode, uint32_t pio,
                        uint32_t n_threads, void *sig_out, uint64_t *n_records_out, uint64_t *n_symbols_out, double *stats_out, uint32_t stats_cap);
/* gzip members inflated ON the device (gs_inflate.hip; the .gz path of gs_sketch_files, exposed for parity tests against zlib - the
 * reference reads .gz through needletail's flate2 reader, files.rs:258-341). in[i]/in_len[i]: HOST bytes of one single-member gzip file;
 * out[i]/out_cap[i]: HOST buffers for the text; out_len[i]: bytes produced; status[i]: 0 = ok (deflate data, ISIZE and CRC-32 all
 * check), 1..8 = malformed deflate data, 100 = header not taken (not gzip, reserved flags), 101 = bytes after the member (multi-member
 * file: host path), 102 = ISIZE mismatch, 103 = CRC mismatch, 104 = out_cap below the member's ISIZE. */
int  gs_gunzip_batch(gs_ctx *, const uint8_t *const *in, const uint64_t *in_len, uint64_t n, uint8_t *const *out, const uint64_t *out_cap,
                     uint64_t *out_len, int *status);
/* ASCII helpers for hosts that do not pack themselves (Sequence::encode_and_add, dnafiles.rs:70-71) */
uint64_t gs_pack_dna(const uint8_t *ascii, uint64_t n, uint8_t *packed_zeroed, uint64_t base_off);
uint64_t gs_filter_aa(const uint8_t *ascii, uint64_t n, uint8_t *out);

/* ---------------------------------------------------------------------------------------------- */
/* DistHamming::eval, batched (anndists; bound at dnasketch.rs:72,139; direct use bindash.rs:93-99) */
/* dist = (f32)count(a[i] != b[i]) / (f32)m                                                         */
int gs_hamming_qxc(gs_ctx *, int kind, uint32_t m, const void *Q, uint64_t nq, const void *C, uint64_t nc,
                   float *dist_out /* nq x nc */);
int gs_hamming_qxc_dev(gs_ctx *, int kind, uint32_t m, const void *Q_dev, uint64_t nq, const void *C_dev,
                       uint64_t nc, float *dist_out_dev);
int gs_hamming_pairs(gs_ctx *, int kind, uint32_t m, const void *A, uint64_t na, const void *B, uint64_t nb,
                     const uint64_t *ia, const uint64_t *ib, uint64_t npairs, float *dist_out);
/* reformat.rs:80-86 calculate_ani (model 1 Poisson, 2 binomial), host arithmetic in f64 */
double gs_ani(double distance, int kmer_size, int model);

/* ---------------------------------------------------------------------------------------------- */
/* hypermash (src/bin/hypermash.rs; the `hyperminhash` crate): HyperMinHash sketches of 16384 u16 registers (gs_sketch_batch with   */
/* GS_ALGO_HMH) and the similarity / distance of every query x reference pair. Arithmetic: SPEC 7.                                   */
/* cardinality of each of n sketches (n x 16384 u16) -> card_out[n] (u64), bit-exact to SPEC 7 */
int gs_hmh_cardinality(gs_ctx *, const uint16_t *sigs, uint64_t n, uint64_t *card_out);
int gs_hmh_cardinality_dev(gs_ctx *, const uint16_t *sigs_dev, uint64_t n, uint64_t *card_out_dev);
/* similarity of every (query, reference) pair -> sim_out[nq x nr] (f64, query-major). The _dev form queues on the context's stream but waits for it
 * once, to learn which sketches take the small-set branch; rows must be 16-byte aligned. nr < 65535 x 128. */
int gs_hmh_similarity_qxc(gs_ctx *, const uint16_t *Q, uint64_t nq, const uint16_t *R, uint64_t nr, double *sim_out);
int gs_hmh_similarity_qxc_dev(gs_ctx *, const uint16_t *Q_dev, uint64_t nq, const uint16_t *R_dev, uint64_t nr, double *sim_out_dev);
/* hypermash.rs:261-263: 1 - (2 sim / (1 + sim))^(1/k), host arithmetic in f64 */
double gs_hmh_distance(double sim, int kmer_size);
/* FASTQ records of a text: an '@' header line, sequence lines up to a '+' line, then as many quality bytes (line breaks not counted) as
 * the sequence has. Multi-line records and CRLF are accepted; a truncated or malformed record is GS_ERR_IO. Record r: sequence text =
 * bytes [seq_begin[r], seq_end[r]) (line breaks included), id = the header's first word. Arrays may be NULL / cap 0 to count only. */
int gs_fastq_scan(const char *buf, uint64_t n, uint64_t cap, uint64_t *seq_begin, uint64_t *seq_end, uint64_t *id_begin, uint32_t *id_len,
                  uint64_t *n_rec_out);
/* One HyperMinHash sketch (16384 u16) per file, input order, with hypermash's reader rules: FASTA or FASTQ (by the first non-blank byte),
 * plain / gz / bz2 / xz (a zstd file is GS_ERR_UNSUPPORTED), no capsid filter, records of <= k bases (line breaks not counted) skipped,
 * k-mers never span records. The pipeline of gs_sketch_files (host threads read / decode / scan, PCIe copies, device pack + sketch).
 * n_records_out / n_bases_out: optional per-file (records kept, bases sketched); stats_out: optional, the first four doubles of gs_sketch_files. */
int gs_hmh_sketch_files(gs_ctx *, uint32_t k, const char *const *paths, uint64_t n_files, uint32_t n_threads, uint16_t *sig_out,
                        uint64_t *n_records_out, uint64_t *n_bases_out, double *stats_out);

/* ---------------------------------------------------------------------------------------------- */
/* superaai (binaux/src/bin/superaai.rs): FracMinHash / bottom-k sketches of proteomes (MurmurHash3_x64_128 h1, seed 42, of every k-byte
 * window of a record) and the AAI of every query x reference pair. Arithmetic: SPEC 9. 1 <= k <= 32 (larger k: GS_ERR_UNSUPPORTED);
 * scaled = 0: no threshold; num = 0: no bound on the sketch size. A sketch is the num smallest distinct hashes <= gs_frac_max_hash(scaled), ascending. */
/* sourmash max_hash_for_scaled: 0 -> 0, 1 -> 2^64-1, else (u64)((f64)(2^64-1) / scaled) */
uint64_t gs_frac_max_hash(uint32_t scaled);
/* host text in, library-allocated host CSR out: record r = bytes [rec_begin[r], rec_end[r]) of text, '\n' and '\r' dropped, every other byte kept;
 * genome g = records [genome_rec_off[g], genome_rec_off[g+1]). *hash_out (release with gs_host_free): the sketches end to end, genome g's at
 * [off_out[g], off_out[g+1]); off_out: n_genomes + 1 entries. */
int gs_frac_sketch_batch(gs_ctx *, uint32_t k, uint32_t scaled, uint32_t num, const void *text, uint64_t n_bytes, const uint64_t *rec_begin,
                         const uint64_t *rec_end, uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, uint64_t **hash_out, uint64_t *off_out);
/* device form: residues (no line breaks) on the device, record r = [rec_start[r], rec_start[r] + rec_len[r]) of seq_dev, all arrays device memory.
 * Genome g's sketch goes to hash_out_dev[g * cap ...], its true size to count_out_dev[g]; a sketch longer than cap is cut at cap and the call
 * returns GS_ERR_INVALID (the counts are written first). */
int gs_frac_sketch_batch_dev(gs_ctx *, uint32_t k, uint32_t scaled, uint32_t num, const void *seq_dev, uint64_t n_bytes, const uint64_t *rec_start_dev,
                             const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint32_t cap,
                             uint64_t *hash_out_dev, uint32_t *count_out_dev);
/* sourmash similarity (jaccard with the union bounded to num) of every (query, reference) pair of ascending, distinct sketches in CSR form
 * (Q[q_off[i] .. q_off[i+1]), R likewise) -> sim_out[nq x nr] (f64, query-major); common_out / union_out (optional, u32): |A n B n U| and |U|.
 * The _dev form queues on the context's stream (it reads q_off_dev back once) and does not check that the sketches are ascending. */
int gs_frac_similarity_qxc(gs_ctx *, uint32_t num, const uint64_t *Q, const uint64_t *q_off, uint64_t nq, const uint64_t *R, const uint64_t *r_off,
                           uint64_t nr, double *sim_out, uint32_t *common_out, uint32_t *union_out);
int gs_frac_similarity_qxc_dev(gs_ctx *, uint32_t num, const uint64_t *Q_dev, const uint64_t *q_off_dev, uint64_t nq, const uint64_t *R_dev,
                               const uint64_t *r_off_dev, uint64_t nr, double *sim_out_dev, uint32_t *common_out_dev, uint32_t *union_out_dev);
/* One sketch per file, input order, with superaai's reader rules: FASTA or FASTQ (by the first non-blank byte), plain / gz / bz2 / xz (zstd:
 * GS_ERR_UNSUPPORTED), no capsid filter, no length filter; all records of a file feed its sketch, k-mers never span records. Output as
 * gs_frac_sketch_batch (off_out: n_files + 1). n_records_out / n_bytes_out: optional per-file records and residues; stats_out: optional,
 * the first four doubles of gs_sketch_files. */
int gs_frac_sketch_files(gs_ctx *, uint32_t k, uint32_t scaled, uint32_t num, const char *const *paths, uint64_t n_files, uint32_t n_threads,
                         uint64_t **hash_out, uint64_t *off_out, uint64_t *n_records_out, uint64_t *n_bytes_out, double *stats_out);
/* superaai.rs:159: 1 + ln(2 sim / (1 + sim)) / k, f64, C library log; sim = 0 -> -inf */
double gs_aai(double sim, uint32_t k);
/* superaai.rs:160,165: writes `q\tr\t{sim}\t{aai}` for every pair, query-major, lines joined by '\n' (no trailing newline, no header), f64 as
 * Rust's Display (shortest round-trip digits, never an exponent); sim: nq x nr. GS_ERR_IO when the file cannot be written. */
int gs_superaai_write(const char *out_path, const char *const *q_paths, uint64_t nq, const char *const *r_paths, uint64_t nr, const double *sim, uint32_t k);

/* ---------------------------------------------------------------------------------------------- */
/* superani (binaux/src/bin/superani.rs): seed-chaining ANI of genome pairs. Arithmetic: SPEC 12 - FracMinHash seeds of the canonical k-mers
 * (8 <= k <= 16, one in about c kept), the anchors of a pair, colinear chaining over the 64 anchors in front, and per side the seeds matched
 * and covered by the kept chains. A seed is four u32: {value, contig, pos, fwd}; contig = the record's index inside its genome, pos = the
 * window's first base inside the record, fwd = 1 when the canonical value is the forward window. Seeds are in position order. */
/* input as gs_sketch_batch (2-bit packed DNA, records, genomes); library-allocated host CSR out: *seeds_out (release with gs_host_free) holds
 * 4 u32 per seed, genome g's seeds are [off_out[g], off_out[g+1]); off_out: n_genomes + 1 entries. */
int gs_ani_sketch_batch(gs_ctx *, uint32_t k, uint32_t c, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len,
                        uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t **seeds_out, uint64_t *off_out);
/* device form: all arrays device memory, seq_dev as for gs_sketch_batch_dev. Genome g's seeds go to seeds_out_dev[4 * g * cap ...], its true
 * count to count_out_dev[g]; a genome with more than cap seeds is cut at cap and the call returns GS_ERR_INVALID (the counts are written first). */
int gs_ani_sketch_batch_dev(gs_ctx *, uint32_t k, uint32_t c, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                            const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint32_t cap,
                            uint32_t *seeds_out_dev, uint32_t *count_out_dev);
/* pair p = (query pair_q[p], reference pair_r[p]) of two seed CSRs (as gs_ani_sketch_batch returns them, both made with the same k and c) ->
 * out[8 p ...] = {n_anchors, n_chains_kept, M_q, C_q, A_q, M_r, C_r, A_r} (SPEC 12). A pair may be listed more than once. Pairs are worked
 * through in blocks of at most max_block_anchors anchors (0: the default, 2^24; a pair with more is a block of its own); no result depends on it.
 * A pair with more than 2^26 anchors: GS_ERR_UNSUPPORTED. The _dev form reads the offsets and the pair lists back once. */
int gs_ani_pairs(gs_ctx *, uint32_t k, const uint32_t *q_seeds, const uint64_t *q_off, uint64_t nq, const uint32_t *r_seeds, const uint64_t *r_off,
                 uint64_t nr, const uint32_t *pair_q, const uint32_t *pair_r, uint64_t n_pairs, uint64_t *out, uint64_t max_block_anchors);
int gs_ani_pairs_dev(gs_ctx *, uint32_t k, const uint32_t *q_seeds_dev, const uint64_t *q_off_dev, uint64_t nq, const uint32_t *r_seeds_dev,
                     const uint64_t *r_off_dev, uint64_t nr, const uint32_t *pair_q_dev, const uint32_t *pair_r_dev, uint64_t n_pairs, uint64_t *out_dev,
                     uint64_t max_block_anchors);
/* the chaining step alone, for hosts that bring their own anchors: pair p's anchors are [off_dev[p], off_dev[p+1]) of the five arrays, in order
 * of (r contig, r position) inside a pair (anything else: GS_ERR_INVALID). f_out_dev (i32), pred_out_dev and root_out_dev (u32, counted from
 * the pair's first anchor; pred = 0xFFFFFFFF: the anchor starts a chain) as SPEC 12 defines them. */
int gs_ani_chain_dev(gs_ctx *, const uint32_t *rcontig_dev, const uint32_t *rpos_dev, const uint32_t *qcontig_dev, const uint32_t *qpos_dev,
                     const uint32_t *strand_dev, const uint64_t *off_dev, uint64_t n_pairs, int32_t *f_out_dev, uint32_t *pred_out_dev, uint32_t *root_out_dev);
/* host only, SPEC 12 closed form: counts = 8 u64 per pair as gs_ani_pairs writes them, bases_q / bases_r = the kept bases of the pair's genomes
 * -> out[3 p ...] = {ani, af_q, af_r} as f32 (ani is a fraction; 0 when neither aligned fraction reaches 0.10). */
int gs_ani_estimate(const uint64_t *counts, const uint64_t *bases_q, const uint64_t *bases_r, uint64_t n_pairs, uint32_t k, float *out);

/* ---------------------------------------------------------------------------------------------- */
/* hmmsearch (`hmmsearch_rs -f proteome.faa -m profile.HMM`, the universal-gene level): the local multihit Viterbi score of every protein
 * against every profile of a set of HMMER3 profiles, the Forward score of the pairs that pass a Viterbi floor (further down, SPEC 13.1), and
 * the best protein per genome and profile. Arithmetic: SPEC 13 - int32 in units of
 * 2^-10 bit, no floating point in the scored path. A record is residues as gs_filter_aa leaves them (the 20 letters, either case). */
#define GS_HMM_MAX_M 1280u            /* nodes of a profile at most (20 per lane of a wavefront); the reference's longest has 1238 */
#define GS_HMM_MAX_L (1u << 18)       /* residues of a record at most: L * 6608 + 151000 < 2^31 (SPEC 13) */
#define GS_HMM_NO_SCORE INT32_MIN     /* score of an empty record (or of one with a byte that is no residue) */
#define GS_HMM_NO_HIT 0xFFFFFFFFu
#define GS_HMM_TABLE_ROWS 27u         /* rows of a profile's table: 20 match rows (ACDEFGHIKLMNPQRSTVWY), then m->m m->i m->d i->m i->i d->m d->d */
#define GS_HMM_HAS_GA 1u
#define GS_HMM_HAS_TC 2u
#define GS_HMM_HAS_NC 4u
#define GS_HMM_HAS_STATS 8u
typedef struct gs_hmm_db gs_hmm_db;
typedef struct {
    char name[64], acc[32];           /* NAME and ACC (empty when the file has none), cut to fit, NUL-terminated */
    uint32_t M, flags;                /* nodes; GS_HMM_HAS_* */
    double ga[2], tc[2], nc[2];       /* cutoffs in bits as the file gives them */
    double mu, lambda;                /* STATS LOCAL VITERBI */
    int32_t ga_units, tbm;            /* GA1 in units (rounded half up); the entry score units(ln(2 / (M (M + 1)))) */
} gs_hmm_info;
/* host only: model number `model` of a HMMER3 ASCII text that holds *n_models_out models (either dialect of the reference's sets, with or
 * without a COMPO line). info_out and tables_out are optional; tables_out: int32 [27][M + 1], row a < 20 = match score of residue a at node
 * k = 1..M (column 0 is 0), rows 20..26 = the transition scores of node k = 0..M; cap_words >= 27 (M + 1) or GS_ERR_INVALID. Anything
 * malformed (truncated, no `//`, a node number out of order, more than 5 decimals, ALPH other than amino): GS_ERR_INVALID; M > GS_HMM_MAX_M:
 * GS_ERR_UNSUPPORTED. */
int gs_hmm_parse_mem(const void *text, uint64_t n_bytes, uint32_t model, gs_hmm_info *info_out, int32_t *tables_out, uint64_t cap_words,
                     uint32_t *n_models_out);
/* host only: out = {tloop, tmove, null, tBM, nloop, nmove} of a target of L = n_residues (1 <= L <= GS_HMM_MAX_L) and a profile of M = n_nodes
 * (1 <= M <= GS_HMM_MAX_M), null = L * nloop + nmove; larger: GS_ERR_UNSUPPORTED */
int gs_hmm_specials(uint64_t n_residues, uint32_t n_nodes, int32_t out[6]);
/* a set of profiles in device memory, in the order of the files and of the models inside each; release with gs_hmm_db_free */
int gs_hmm_db_load(gs_ctx *ctx, const char *const *paths, uint64_t n_paths, gs_hmm_db **out);
int gs_hmm_db_load_mem(gs_ctx *ctx, const void *const *texts, const uint64_t *n_bytes, uint64_t n_texts, gs_hmm_db **out);
void gs_hmm_db_free(gs_hmm_db *db);
/* *n_prof_out = the number of profiles; info_out (optional): the first min(cap, n_prof) of them */
int gs_hmm_db_info(gs_hmm_db *db, uint64_t *n_prof_out, gs_hmm_info *info_out, uint64_t cap);
/* the table of profile p as gs_hmm_parse_mem writes it, nodes 1..M read back from the device copy the kernel uses */
int gs_hmm_db_tables(gs_hmm_db *db, uint64_t p, int32_t *tables_out, uint64_t cap_words);
/* host only: out[k - 1] = the consensus letter of node k = 1 .. M of profile p, upper case, no terminator: the residue whose match score plus background
 * log-odds (SPEC 13) is largest, the first in the order ACDEFGHIKLMNPQRSTVWY on a tie; cap < M: GS_ERR_INVALID */
int gs_hmm_db_consensus(gs_hmm_db *db, uint64_t p, char *out, uint64_t cap);
/* score_out[r * n_prof + p] = raw score of record r = aa[rec_start[r] .. + rec_len[r]) against profile p. Device form: all arrays device
 * memory; the lengths are read back once. A record longer than GS_HMM_MAX_L, or 2^32 records or more: GS_ERR_UNSUPPORTED, nothing written. */
int gs_hmm_search_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                      int32_t *score_out_dev);
int gs_hmm_search(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int32_t *score_out);
/* segmented argmax: genome g = records [genome_rec_off[g], genome_rec_off[g+1]) of an n_rec x n_prof score matrix;
 * best_rec_out[g * n_prof + p] = the record with the largest score >= thr[p], the lowest such record on a tie, GS_HMM_NO_HIT when none;
 * best_score_out = its score or GS_HMM_NO_SCORE. thr_dev = NULL: every profile's GA1 (a profile without GA: GS_ERR_INVALID). All device memory. */
int gs_hmm_best_hits_dev(gs_ctx *ctx, gs_hmm_db *db, const int32_t *score_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes,
                         const int32_t *thr_dev, uint32_t *best_rec_out, int32_t *best_score_out);
/* host only, double: raw / 1024, and E = n_targets * P with P = -expm1(-exp(-lambda (bits - mu))) (the Gumbel tail of STATS LOCAL VITERBI) */
double gs_hmm_bits(int32_t raw);
double gs_hmm_evalue(double bits, double mu, double lambda, double n_targets);

/* Forward scores (SPEC 13.1): the same model, tables and units, every max that joins alternatives replaced by lse(a, b) = hi + T[min((hi - lo + 1) >> 1,
 * 5903)] in a fixed blocked order, so fwd >= vit holds on the integers. HMMER's own order: the Viterbi score of every pair first, Forward only for the
 * pairs at or above a per-profile Viterbi floor. The files' GA / TC / NC cutoffs were gathered on this score. */
#define GS_HMM_FWD_MAX_L 65536u       /* residues of a record at most for Forward: L * 21353 < 2^31 with 7.4e8 to spare (SPEC 13.1) */
#define GS_HMM_LSE_N 5903u            /* entries of T: T[j] = floor(1024 log2(1 + 2^(-2 j / 1024)) + 1/2), T[0] = 1024, T[5902] = 1; beyond: 0 */
/* host only: out[0 .. GS_HMM_LSE_N) = T; cap < GS_HMM_LSE_N: GS_ERR_INVALID */
int gs_hmm_logsum_table(uint16_t *out, uint64_t cap);
/* host only: out = {msv mu, lambda, viterbi mu, lambda, forward tau, lambda} of the STATS LOCAL lines of model number `model` of a text (0 where a
 * line is missing); *has_out bit 0 / 1 / 2 = the MSV / VITERBI / FORWARD line was there. Errors as gs_hmm_parse_mem. */
int gs_hmm_parse_stats_mem(const void *text, uint64_t n_bytes, uint32_t model, double out[6], uint32_t *has_out);
/* host only, SPEC 13.1: the Viterbi score in units whose Gumbel tail mass is p, floor((mu - ln(-ln(1 - p)) / lambda) * 1024 + 1/2), kept inside
 * [INT32_MIN + 1, INT32_MAX]; lambda <= 0 or p outside (0, 1): GS_ERR_INVALID */
int gs_hmm_viterbi_floor(double mu, double lambda, double p, int32_t *floor_out);
/* vit_out[r * n_prof + p] = what gs_hmm_search writes (optional); fwd_out[r * n_prof + p] = the Forward raw score of the pairs with vit != GS_HMM_NO_SCORE
 * and vit >= vit_floor[p], GS_HMM_NO_SCORE for the others. vit_floor: n_prof words, NULL = every pair that has a Viterbi score. Device form: all arrays
 * device memory; the lengths are read back once. A record longer than GS_HMM_FWD_MAX_L, or 2^32 records or more: GS_ERR_UNSUPPORTED, nothing written to
 * either output; a set of another context: GS_ERR_INVALID. */
int gs_hmm_search_forward_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                              const int32_t *vit_floor_dev, int32_t *vit_out_dev, int32_t *fwd_out_dev);
int gs_hmm_search_forward(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                          const int32_t *vit_floor, int32_t *vit_out, int32_t *fwd_out);
/* host only, double: E = n_targets * P with P = 1 for bits < tau, exp(-lambda (bits - tau)) otherwise (the exponential tail of STATS LOCAL FORWARD) */
double gs_hmm_forward_evalue(double bits, double tau, double lambda, double n_targets);

/* MSV prefilter (SPEC 13.3): the model of SPEC 13 without insert and delete states and with m->m taken as 0 - ungapped diagonals, any number of them -
 * in the same units, all int32. It is neither a lower nor an upper bound of the Viterbi score. HMMER's own order puts it in front of Viterbi: the full
 * dynamic program runs only for the pairs at or above a per-profile MSV floor, gs_hmm_viterbi_floor(mu, lambda, P) of the STATS LOCAL MSV line with
 * P = 0.02. A pair whose gapped alignment is good and whose ungapped diagonals are weak is lost: the stated cost of the filter.
 * msv_out[r * n_prof + p] = the MSV raw score, GS_HMM_NO_SCORE for an empty record or one with a byte that is no residue. Arguments and refusals are
 * those of gs_hmm_search(_dev). */
int gs_hmm_search_msv_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                          int32_t *msv_out_dev);
int gs_hmm_search_msv(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int32_t *msv_out);
/* msv_out (optional) as above; vit_out[r * n_prof + p] = what gs_hmm_search writes for the pairs with msv != GS_HMM_NO_SCORE and msv >= msv_floor[p],
 * GS_HMM_NO_SCORE for the others; fwd_out (optional, NULL = no Forward pass) = what gs_hmm_search_forward writes behind that Viterbi matrix and
 * vit_floor. msv_floor, vit_floor: n_prof words each, NULL = every pair that has the score in front (vit_floor is read only with fwd_out). Device form:
 * all arrays device memory; the lengths are read back once. A record longer than GS_HMM_MAX_L - with fwd_out: than GS_HMM_FWD_MAX_L - or 2^32 records or
 * more: GS_ERR_UNSUPPORTED before anything is queued, nothing written; a set of another context: GS_ERR_INVALID. */
int gs_hmm_search_filtered_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                               const int32_t *msv_floor_dev, const int32_t *vit_floor_dev, int32_t *msv_out_dev, int32_t *vit_out_dev, int32_t *fwd_out_dev);
int gs_hmm_search_filtered(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                           const int32_t *msv_floor, const int32_t *vit_floor, int32_t *msv_out, int32_t *vit_out, int32_t *fwd_out);

/* The packed int16 Viterbi filter (SPEC 13.7), opt-in: no other call changes. vf is the Viterbi program of SPEC 13 with int16 cells in half units - every
 * table word x becomes h(x) = max(-32768, (x + 1) >> 1), every cell operation saturates to [-32768, 32767] - and the specials of SPEC 13 in int32 with
 * E[i] = 2 * max_k M16[i][k]. Every int16 input is at least half its int32 counterpart and max and the saturating add are monotone, so vf >= vit for every
 * pair that has both; a record whose E16 reaches 32767 in some row gets GS_HMM_VF_OVER, which is above every floor. So the pairs with vf >= f contain the
 * pairs with vit >= f: a filter that loses no hit.
 * vf_out[r * n_prof + p] = vf, GS_HMM_NO_SCORE for an empty record or one with a byte that is no residue (that goes before an overflow). Arguments and
 * refusals are those of gs_hmm_search(_dev). */
#define GS_HMM_VF_OVER INT32_MAX
int gs_hmm_search_vit16_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                            int32_t *vf_out_dev);
int gs_hmm_search_vit16(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int32_t *vf_out);
/* the int16 table of profile p: [GS_HMM_TABLE_ROWS][M + 1] as gs_hmm_db_tables lays it out, every word h() of the int32 word, nodes 1..M read back
 * from the device copy k_hmm_vit16 uses */
int gs_hmm_db_tables16(gs_hmm_db *db, uint64_t p, int16_t *tables_out, uint64_t cap_words);
/* The staged search: use_msv != 0: msv_out (optional) = the MSV score of every pair as gs_hmm_search_msv writes it, and vf runs for the pairs with msv !=
 * GS_HMM_NO_SCORE and msv >= msv_floor[p]; use_msv == 0: vf runs for every pair (msv_floor and msv_out are not read). vf_out (optional) = vf of the pairs
 * it ran for, GS_HMM_NO_SCORE for the others; vit_out[r * n_prof + p] = what gs_hmm_search writes for the pairs with vf != GS_HMM_NO_SCORE and vf >=
 * vf_floor[p] (the kernels of gs_hmm_search_filtered over those lists), GS_HMM_NO_SCORE for the others; fwd_out (optional, NULL = no Forward pass) as
 * in gs_hmm_search_filtered. A floor of NULL: every pair that has the score in front. With vf_floor[p] <= f the words of vit_out that are >= f are those of
 * gs_hmm_search (use_msv == 0) or of gs_hmm_search_filtered (use_msv != 0, the same msv_floor), word for word. Refusals as gs_hmm_search_filtered. */
int gs_hmm_search_staged_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                             int use_msv, const int32_t *msv_floor_dev, const int32_t *vf_floor_dev, const int32_t *vit_floor_dev, int32_t *msv_out_dev,
                             int32_t *vf_out_dev, int32_t *vit_out_dev, int32_t *fwd_out_dev);
int gs_hmm_search_staged(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int use_msv,
                         const int32_t *msv_floor, const int32_t *vf_floor, const int32_t *vit_floor, int32_t *msv_out, int32_t *vf_out, int32_t *vit_out,
                         int32_t *fwd_out);

/* Trace-back (SPEC 13.2): the domains of the Viterbi path of a list of (record, profile) pairs - the segments of the path between a B -> M entry and the
 * M -> E exit that follows it. The dynamic program (with back-pointers) and the walk back both run on the device. A domain is GS_HMM_DOM_WORDS int32:
 * i_from, i_to, k_from, k_to (1-based, inclusive), seg = M[i_to][k_to] - B[i_from - 1], n_match, n_ins, n_del. Pairs in any order, repeats allowed.
 * raw_out[j] = what gs_hmm_search writes for pair j; n_dom_out[j] = the true number of domains; dom_out[j][0 .. min(n_dom, max_dom)) = the first domains
 * in sequence order, the other slots of the pair zeros (max_dom = 0 with dom_out = NULL is allowed). A pair with pair_rec = GS_HMM_NO_HIT, an empty
 * record or a record with a byte that is no residue: raw = GS_HMM_NO_SCORE, n_dom = 0, zeroed slots - the [n_genomes][n_prof] output of
 * gs_hmm_best_hits_dev is a pair list as it lies, with pair_prof = index % n_prof. Any other pair_rec >= n_rec, or a pair_prof >= n_prof: GS_ERR_INVALID; a
 * named record longer than GS_HMM_TRACE_MAX_L: GS_ERR_UNSUPPORTED; both before anything is queued, nothing written (records that no pair names may be
 * any length). max_block_cells bounds the cells (sum of L * 64 Q over the pairs of a block, Q the nodes per lane of the profile's class) whose
 * back-pointers are alive at once; 0 = 2^27; a block always holds at least one pair. Device form: every array device memory; the lengths and the pair
 * list are read back once. */
#define GS_HMM_TRACE_MAX_L 65536u
#define GS_HMM_DOM_WORDS 8u
int gs_hmm_trace(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                 const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_dom, uint64_t max_block_cells, int32_t *raw_out, uint32_t *n_dom_out, int32_t *dom_out);
int gs_hmm_trace_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                     const uint32_t *pair_rec_dev, const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_dom, uint64_t max_block_cells,
                     int32_t *raw_out_dev, uint32_t *n_dom_out_dev, int32_t *dom_out_dev);

/* Backward scores and posterior envelopes (SPEC 13.4): where on the record the probability mass of the model sits, from the Forward and the Backward
 * pass of a list of (record, profile) pairs, and what each such stretch scores on its own - integers only, both passes and the rule on the device.
 * With out[i] = log2 P(x_i is emitted outside the core model) and cont[i] = log2 P(x_i outside, or a domain ends at row i), in units: a row is in iff
 * out[i] <= -156 (occupancy >= 0.10); a run is a maximal stretch of in-rows in which every row but the last has cont[i] <= -156; a run is an envelope
 * iff some row of it has out[i] <= -425 (occupancy >= 0.25). An envelope is GS_HMM_ENV_WORDS int32: i_from, i_to (1-based, inclusive), env_raw = the
 * Forward raw score of the rows i_from .. i_to alone under the length model of the whole record, peak = the smallest out[i] of the envelope.
 * No stochastic clustering (a run is one envelope); the alignment of an envelope is gs_hmm_align (SPEC 13.6); env_raw is uncorrected (the null2 correction is gs_hmm_null2). Pairs in any order, repeats allowed.
 * fwd_out[j] = what gs_hmm_search_forward writes for pair j; bck_out[j] = bN[0] - null, the same probability summed from the other end (it differs
 * from fwd_out[j] by rounding alone); n_env_out[j] = the true number of envelopes; env_out[j][0 .. min(n_env, max_env)) = the first envelopes in
 * sequence order, the other slots of the pair zeros (max_env = 0 with env_out = NULL is allowed). row_off (n_pairs + 1 words, optional, with out_rows
 * and cont_rows): out[1 .. L] and cont[1 .. L] of pair j are written to out_rows / cont_rows from word row_off[j] on; row_off[j + 1] - row_off[j] >= L,
 * else GS_ERR_INVALID; the words of a pair that gets no envelopes below are not written. A pair with pair_rec = GS_HMM_NO_HIT, an empty record or a
 * record with a byte that is no residue: fwd = bck = GS_HMM_NO_SCORE, n_env = 0, zeroed slots. Any other pair_rec >= n_rec, or a pair_prof >= n_prof:
 * GS_ERR_INVALID; a named record longer than GS_HMM_FWD_MAX_L: GS_ERR_UNSUPPORTED; both before anything is queued, nothing written (records that no
 * pair names may be any length); a set of another context: GS_ERR_INVALID. max_block_rows bounds the kept rows (sum of L + 1 over the pairs of a
 * block, 24 bytes each) alive at once; 0 = 2^25; a block always holds at least one pair; no output depends on it. Device form: every array device
 * memory; the lengths, the pair list and row_off are read back once. */
#define GS_HMM_ENV_WORDS 4u
int gs_hmm_envelopes(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                     const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_rows, int32_t *fwd_out, int32_t *bck_out, uint32_t *n_env_out,
                     int32_t *env_out, const uint64_t *row_off, int32_t *out_rows, int32_t *cont_rows);
int gs_hmm_envelopes_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                         const uint32_t *pair_rec_dev, const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_rows,
                         int32_t *fwd_out_dev, int32_t *bck_out_dev, uint32_t *n_env_out_dev, int32_t *env_out_dev, const uint64_t *row_off_dev,
                         int32_t *out_rows_dev, int32_t *cont_rows_dev);

/* null2 bias correction (SPEC 13.5): what a model of the segment's own composition would have scored, taken off the envelope and sequence scores -
 * HMMER3's null2 by expectation, restated in the integer units and lse of SPEC 13 / 13.1. Opt-in: no other call changes. For every listed envelope
 * a .. b of a pair (a slot, Ld = b - a + 1) Forward and Backward run over x_a .. x_b under the length model of the whole record, both on the device;
 * their products give the expected usage of every emitting state, from it the 20 log-odds n2[a] of the segment's null model, and
 * corr = sum of n2[x_i] over the segment (64 bits, kept inside +-2^30), dom_bias = lse(0, -8192 + corr), seq_bias = lse(0, -8192 + the sum of corr over
 * the pair's listed envelopes). Both biases are >= 0; the corrected scores are env_raw - dom_bias and fwd - seq_bias.
 * Arguments and refusals are those of gs_hmm_envelopes; n_env and env are inputs, as that call wrote them for the same pairs and max_env. Envelope e
 * of pair j is listed iff e < min(n_env[j], max_env): when n_env > max_env the sequence bias counts the listed envelopes only. An envelope with
 * i_from > i_to or a bound outside 1 .. L: GS_ERR_INVALID, nothing written.
 * slot_out[j][e] = GS_HMM_N2_WORDS int32: corr, dom_bias, seg_raw (== env_raw of the envelope, on the integers), mass (the summed usage over Ld, a
 * check word: 0 in exact arithmetic); the other slots of the pair zeros. seq_bias_out[j]. n2_out (optional): [n_pairs][max_env][20]. occ_off
 * (n_pairs + 1 words, optional, with occm_out and occi_out): the rows occM[1 .. M] and occI[1 .. M] (log2 of the expected number of residues M_k and
 * I_k emit; occI[M] = GS_HMM_NEG) of slot e of pair j are written from word occ_off[j] + e * M on; occ_off[j + 1] - occ_off[j] >= min(n_env, max_env) *
 * M, else GS_ERR_INVALID. A pair with pair_rec = GS_HMM_NO_HIT, an empty record or a record with a byte that is no residue: zeroed slots, seq_bias = 0,
 * no rows. max_block_cells bounds the cells (sum of 64 Q * Ld over the slots of a block, 8 bytes each) whose Forward M and I are alive at once; 0 = 2^26;
 * a block always holds at least one slot; no output depends on it. Device form: every array device memory; the lengths, the pair list, n_env, env and
 * occ_off are read back once. */
#define GS_HMM_N2_WORDS 4u
int gs_hmm_null2(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                 const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env, int32_t *slot_out,
                 int32_t *seq_bias_out, int32_t *n2_out, const uint64_t *occ_off, int32_t *occm_out, int32_t *occi_out);
int gs_hmm_null2_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                     const uint32_t *pair_rec_dev, const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env_dev,
                     const int32_t *env_dev, int32_t *slot_out_dev, int32_t *seq_bias_out_dev, int32_t *n2_out_dev, const uint64_t *occ_off_dev, int32_t *occm_out_dev,
                     int32_t *occi_out_dev);

/* Optimal-accuracy alignment (SPEC 13.6): which residue of a listed envelope sits on which node, and how sure the model is of each column - HMMER3's
 * maximum-expected-accuracy alignment restated in the integer units and lse of SPEC 13 / 13.1, all on the device. Opt-in: no other call changes.
 * Forward and Backward over the envelope are gs_hmm_null2's; their sums minus the segment's total are the posteriors pM, pI, pX in units (<= 0), a
 * posterior counts w(p) = EXP2[-p & 1023] >> (-p >> 10) in Q16 (0 .. 65536), and the alignment is the one path N.. B M/I/D.. E C.. through the
 * segment - exactly one domain, only transitions the profile allows (table word > GS_HMM_STAR) - whose emitting cells' weights sum highest; ties go
 * to the first alternative of SPEC 13.6, so the path is unique. Arguments and refusals are those of gs_hmm_null2 (n_env and env are inputs); beyond
 * them a listed envelope of more than GS_HMM_ALI_MAX_LD residues: GS_ERR_UNSUPPORTED, nothing written.
 * slot_out[j][e] = GS_HMM_ALI_WORDS int32: i_from, i_to (record coordinates, 1-based, inclusive), k_from, k_to, oa (the path's summed weight plus
 * w(pX) of the segment's rows outside i_from .. i_to; expected accuracy = oa / (65536 Ld)), n_match, n_ins, n_del; the other slots of the pair
 * zeros. n_match + n_ins = i_to - i_from + 1 and n_match + n_del = k_to - k_from + 1.
 * col_off (n_pairs + 1 words, optional, with col_out): the columns of slot e of pair j, in order from (i_from, k_from) to (i_to, k_to), two int32
 * each, start at column col_off[j] + the sum over e' < e of Ld_e' + M; word 0 = state << 28 | k << 16 | (i - 1) with state 0 M, 1 I, 2 D and i the
 * record row of the cell (for D the row it sits in), word 1 = pM or pI of the cell in units, 0 for D; n_match + n_ins + n_del of them are written.
 * col_off[j + 1] - col_off[j] must hold that sum over all listed slots of the pair, else GS_ERR_INVALID. A pair with pair_rec = GS_HMM_NO_HIT, an
 * empty record or a record with a byte that is no residue: zeroed slots, no columns. max_block_cells as for gs_hmm_null2; no output depends on it.
 * Device form: every array device memory; the lengths, the pair list, n_env, env and col_off are read back once. */
#define GS_HMM_ALI_WORDS 8u
#define GS_HMM_ALI_MAX_LD 8192u
#define GS_HMM_EXP2_N 1024u           /* entries of EXP2: EXP2[f] = floor(65536 * 2^(-f / 1024) + 1/2), EXP2[0] = 65536 */
/* host only: out[0 .. GS_HMM_EXP2_N) = EXP2; cap < GS_HMM_EXP2_N: GS_ERR_INVALID */
int gs_hmm_exp2_table(uint32_t *out, uint64_t cap);
int gs_hmm_align(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                 const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env, int32_t *slot_out,
                 const uint64_t *col_off, int32_t *col_out);
int gs_hmm_align_dev(gs_ctx *ctx, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                     const uint32_t *pair_rec_dev, const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env_dev,
                     const int32_t *env_dev, int32_t *slot_out_dev, const uint64_t *col_off_dev, int32_t *col_out_dev);

/* Best hits become sketcher records (SPEC 13.8): the [n_genomes][n_prof] matrix best_rec as gs_hmm_best_hits_dev leaves it (GS_HMM_NO_HIT = none) over
 * the searched records (aa, rec_start, rec_len, n_rec) -> the chosen residues back to back in out_aa and their descriptors, what gs_sketch_batch_dev
 * reads. Output record j is the j-th hit of the matrix in (genome, profile) order; out_start[j] / out_len[j] address out_aa; the hits of genome g are
 * records [out_genome_off[g], out_genome_off[g + 1]), an empty range for a genome without one. A record that two profiles chose appears twice.
 * Spans (n_item and item both given, or both NULL): item is [n_genomes * n_prof][max_item][item_words] int32 with i_from in word 0 and i_to in word 1 of
 * a slot, 1-based and inclusive - the layout the GS_HMM_DOM_WORDS, GS_HMM_ENV_WORDS and GS_HMM_ALI_WORDS slots share. Hit h = g * n_prof + p with
 * n_item[h] >= 1 contributes residues [i_from of item 0 - 1, i_to of item n_item[h] - 1) of its record, a hit with n_item[h] = 0 and every hit of a
 * call without spans the whole record. The items of a pair that is no hit are not read.
 * n_out (HOST) = {records, residues}. GS_ERR_INVALID, nothing written (n_out neither): a best_rec that is neither GS_HMM_NO_HIT nor < n_rec; a hit with
 * n_item[h] > max_item (run the spans again with room); a span outside its record (i_from < 1, i_to > the record's length or i_to < i_from - 1); spans
 * with item_words < 2 or max_item = 0. More than cap_rec records or cap_aa residues: GS_ERR_INVALID with n_out filled and nothing else written.
 * No byte of out_aa at or past n_out[1] and no descriptor at or past n_out[0] is written. 2^32 pairs or records and more: GS_ERR_UNSUPPORTED.
 * Device form: every array but n_out device memory; one wait for the counts, one at the end. The host form computes on the host (ctx may be NULL). */
int gs_hmm_hit_records_dev(gs_ctx *ctx, const uint32_t *best_rec_dev, uint64_t n_genomes, uint64_t n_prof, const uint8_t *aa_dev, const uint64_t *rec_start_dev,
                           const uint64_t *rec_len_dev, uint64_t n_rec, const uint32_t *n_item_dev, const int32_t *item_dev, uint32_t item_words, uint32_t max_item,
                           uint64_t cap_rec, uint64_t cap_aa, uint8_t *out_aa_dev, uint64_t *out_start_dev, uint64_t *out_len_dev, uint64_t *out_genome_off_dev,
                           uint64_t n_out[2]);
int gs_hmm_hit_records(gs_ctx *ctx, const uint32_t *best_rec, uint64_t n_genomes, uint64_t n_prof, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len,
                       uint64_t n_rec, const uint32_t *n_item, const int32_t *item, uint32_t item_words, uint32_t max_item, uint64_t cap_rec, uint64_t cap_aa,
                       uint8_t *out_aa, uint64_t *out_start, uint64_t *out_len, uint64_t *out_genome_off, uint64_t n_out[2]);

/* ---------------------------------------------------------------------------------------------- */
/* orfs (SPEC 14): stop-to-stop six-frame translation of packed nucleotide records on the device - the model-free way to feed hmmsearch from genomes.
 * It is NOT a gene caller and does not replace FragGeneScanRs: the ORF set is not a proteome and must not be given to the AA sketchers or superaai.
 * Input: the packed layout of gs_sketch_batch_dev (2-bit bases, record r = bases [rec_start[r], rec_start[r] + rec_len[r]), no invalid base inside a
 * record, records inside seq_bytes and not overlapping). An ORF is a maximal run of codons without a stop in one of the six (strand, class mod 3)
 * frames; `begin` is its lowest base, n its codons, end = begin + 3 n, all in forward coordinates. Kept: min_aa <= n, and n <= max_aa unless max_aa = 0;
 * longer ones are dropped and counted. Order: ascending (record, end, strand). */
typedef struct { uint32_t min_aa, max_aa, table, flags; } gs_orf_params;      /* table 11 or 4; flags = 0 */
typedef struct { uint64_t begin; uint32_t rec, strand; } gs_orf;              /* begin: offset inside the record, forward coordinates; strand 0 = forward */
#define GS_ORF_TILE 192u            /* bases one wavefront takes at a time (a codon of each class per lane); no result depends on it */
/* host only: the 64 letters of a translation table, codon index 16 b0 + 4 b1 + b2 (A C G T = 0 1 2 3), `*` = stop; another table: GS_ERR_UNSUPPORTED */
int gs_orf_codon_table(uint32_t table, char out[64]);
/* n_out (HOST) = {kept ORFs, their residues, ORFs dropped as longer than max_aa}. All five output pointers NULL with zero caps: count only. With
 * outputs: a cap below the count is GS_ERR_INVALID with n_out filled and nothing written; a partial set of pointers is GS_ERR_INVALID. aa_out: the
 * upper-case residues of the kept ORFs back to back in ORF order; aa_start_out / aa_len_out: what gs_hmm_search_dev takes as rec_start / rec_len;
 * rec_orf_off_out (n_rec + 1): the ORFs of record r are [off[r], off[r + 1]). min_aa = 0 or 0 < max_aa < min_aa: GS_ERR_INVALID; flags != 0, another
 * table, 2^32 records or more, seq_bytes / 48 + n_rec >= 2^26: GS_ERR_UNSUPPORTED; a record outside seq_bytes, or records whose bases add up to more
 * than seq holds: GS_ERR_INVALID. The device form waits for the
 * stream once (the counts) and leaves the outputs in flight on it. */
int gs_orf_translate_dev(gs_ctx *ctx, const gs_orf_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                         const uint64_t *rec_len_dev, uint64_t n_rec, uint64_t cap_orf, uint64_t cap_aa, gs_orf *orf_out_dev, uint8_t *aa_out_dev,
                         uint64_t *aa_start_out_dev, uint64_t *aa_len_out_dev, uint64_t *rec_orf_off_out_dev, uint64_t n_out[3]);
int gs_orf_translate(gs_ctx *ctx, const gs_orf_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len,
                     uint64_t n_rec, uint64_t cap_orf, uint64_t cap_aa, gs_orf *orf_out, uint8_t *aa_out, uint64_t *aa_start_out, uint64_t *aa_len_out,
                     uint64_t *rec_orf_off_out, uint64_t n_out[3]);

/* ---------------------------------------------------------------------------------------------- */
/* genes (SPEC 15): a self-trained gene caller for complete prokaryotic genomes on the device - the way from genomes to the proteomes that the AA
 * sketchers, superaai and hmmsearch read. Every genome learns in-frame dicodon statistics from its own long ORFs, every ORF's candidate starts are scored
 * with them, and a maximal-weight chain of nearly non-overlapping genes is chosen per record on both strands. It is the self-trained kind of Prodigal and
 * GeneMarkS, NOT FragGeneScanRs (whose trained models the reference does not hold) and it does not give that program's numbers: no ribosome-binding-site
 * model, no error or frameshift model (complete genomes, not reads), no pre-trained model (a genome too small to train gets no genes), tables 11 and 4.
 * Input: the packed layout of gs_orf_translate_dev, genome g = records [genome_rec_off[g], genome_rec_off[g + 1]) with genome_rec_off[0] = 0 and
 * genome_rec_off[n_genomes] = n_rec. All integer arithmetic: every result is a function of the input alone. */
typedef struct {
    uint32_t min_aa, table;                 /* as gs_orf_params; default 30, 11 */
    uint32_t train_min_aa;                  /* round 1 trains on the whole ORFs of this many codons and more; default 250 */
    uint32_t min_train_codons;              /* a genome with fewer training dicodons is untrained and gets no genes; default 15000 */
    int32_t min_score;                      /* a gene's least score, 1024 = 1 bit; default 5120 */
    uint32_t max_overlap;                   /* bases two chosen genes may share; below 3 * min_aa; default 60 */
    uint32_t rounds;                        /* training rounds, >= 1; default 2 */
    uint32_t flags;                         /* 0 */
} gs_gene_params;
/* a training interval: n codons at bases [begin, begin + 3 n) of record rec (forward coordinates), read on strand 0 / 1 */
typedef struct { uint64_t begin, n; uint32_t rec, strand; } gs_gene_interval;
/* a gene: bases [begin, end) of record rec in forward coordinates, the stop codon included where there is one */
typedef struct { uint64_t begin, end; int64_t score; uint32_t rec, flags; } gs_gene;
#define GS_GENE_STRAND 1u                   /* flags: bit 0 the strand */
#define GS_GENE_TYPE_SHIFT 1                /*        bits 1-2 the start: 0 ATG, 1 GTG, 2 TTG, 3 the record's edge */
#define GS_GENE_TYPE_EDGE 3u
#define GS_GENE_OPEN3 8u                    /*        no stop ends it: it runs into the record's edge */
#define GS_GENE_HAS_START 16u               /*        (gs_gene_score*) the ORF has a candidate start */
#define GS_GENE_CANDIDATE 32u               /*        (gs_gene_score*) and its score is min_score or more */
#define GS_GENE_OPEN5 64u                   /*        (gs_gene_score*) no stop precedes the ORF */
#define GS_GENE_NO_START 0xFFFFFFFFFFFFFFFFull
#define GS_GENE_TRAINED 1u                  /* info[2 g + 1] */
/* host only: the defaults above */
gs_gene_params gs_gene_params_default(void);
/* host only: floor(65536 log2 x) of SPEC 15 (x >= 1; 0 for x = 0), the logarithm behind the score tables */
uint32_t gs_gene_log2_q16(uint64_t x);
/* Stage 1, counts to tables. tables_out: [n_genomes][4096] scores S[64 c + c'] of codon c followed in frame by c', 1024 = 1 bit; info_out:
 * [n_genomes][2] = {Nc, GS_GENE_TRAINED or 0}. The intervals are ordered by record. GS_ERR_INVALID: bad parameters (max_overlap >= 3 * min_aa among them),
 * a record outside seq_bytes, genome_rec_off not ascending from 0 to n_rec, an interval outside its record, out of record order or with strand > 1;
 * GS_ERR_UNSUPPORTED: a genome of more than 2^30 hexamer positions or 2^32 - 4096 training dicodons, an interval of 2^24 codons or more. Waits for the
 * stream once (the error word). */
int gs_gene_train_dev(gs_ctx *ctx, const gs_gene_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                      const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes,
                      const gs_gene_interval *iv_dev, uint64_t n_iv, int32_t *tables_out_dev, uint64_t *info_out_dev);
/* the same on the host, host memory throughout, no device */
int gs_gene_train_host(const gs_gene_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                       const uint64_t *genome_rec_off, uint64_t n_genomes, const gs_gene_interval *iv, uint64_t n_iv, int32_t *tables_out,
                       uint64_t *info_out);
/* Stage 2, the best start of every given ORF (gs_orf + its codons orf_len) under the caller's tables: best_j_out = the codon the gene starts at or
 * GS_GENE_NO_START, score_out its score (0 without a start), flags_out the strand, start type, GS_GENE_OPEN3 / OPEN5 / HAS_START / CANDIDATE.
 * GS_ERR_INVALID also for an ORF outside its record or without codons and for a table entry outside +-32768. Waits for the stream once. */
int gs_gene_score_dev(gs_ctx *ctx, const gs_gene_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                      const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, const int32_t *tables_dev,
                      const gs_orf *orf_dev, const uint64_t *orf_len_dev, uint64_t n_orf, uint64_t *best_j_out_dev, int64_t *score_out_dev,
                      uint32_t *flags_out_dev);
int gs_gene_score_host(const gs_gene_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                       const uint64_t *genome_rec_off, uint64_t n_genomes, const int32_t *tables, const gs_orf *orf, const uint64_t *orf_len,
                       uint64_t n_orf, uint64_t *best_j_out, int64_t *score_out, uint32_t *flags_out);
/* The whole pipeline. n_out (HOST) = {genes, their residues}. gene_out in (record, end, strand) order; aa_out the residues from the start codon to the
 * last sense codon back to back, the first one M unless the start is the record's edge; aa_start_out / aa_len_out / rec_gene_off_out (n_rec + 1) in
 * the layout of gs_orf_translate_dev, so gs_hmm_search_dev takes them unchanged. info_out: [n_genomes][2] as above, of the last round. tables_out
 * (optional): the last round's tables. The five gene outputs all NULL with zero caps: count only (info_out and tables_out are still written); a cap
 * below the count is GS_ERR_INVALID with n_out filled; a partial set of pointers is GS_ERR_INVALID. An untrained genome is no error. */
int gs_gene_call_dev(gs_ctx *ctx, const gs_gene_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                     const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint64_t cap_gene,
                     uint64_t cap_aa, gs_gene *gene_out_dev, uint8_t *aa_out_dev, uint64_t *aa_start_out_dev, uint64_t *aa_len_out_dev,
                     uint64_t *rec_gene_off_out_dev, uint64_t *info_out_dev, int32_t *tables_out_dev, uint64_t n_out[2]);
int gs_gene_call(gs_ctx *ctx, const gs_gene_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len,
                 uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, uint64_t cap_gene, uint64_t cap_aa, gs_gene *gene_out,
                 uint8_t *aa_out, uint64_t *aa_start_out, uint64_t *aa_len_out, uint64_t *rec_gene_off_out, uint64_t *info_out, int32_t *tables_out,
                 uint64_t n_out[2]);

/* ---------------------------------------------------------------------------------------------- */
/* Hnsw<Sig, DistHamming> (hnsw_rs) as gsearch drives it:                                           */
/*   new/modify_level_scale/set_extend_candidates/set_keeping_pruned  dnasketch.rs:139-141,159-160  */
/*   parallel_insert dnasketch.rs:435, aasketch.rs:407;  parallel_search dnarequest.rs:353, aarequest.rs:344 */
typedef struct gs_index gs_index;
typedef struct {
    int      kind;               /* GS_KIND_* of Sig */
    uint32_t m;                  /* signature length */
    uint32_t max_nb_conn;        /* M <= 255 (gsearch.rs:268) */
    uint64_t capacity;           /* hnsw_params.capacity, 1_500_000 in gsearch (gsearch.rs:269); rows are pre-allocated */
    uint32_t max_layer;          /* 16 (dnasketch.rs:139) */
    uint32_t ef_construction;
    double   scale_modify;       /* modify_level_scale factor (dnasketch.rs:141) */
    int      extend_candidates;  /* true in gsearch (dnasketch.rs:159) */
    int      keep_pruned;        /* false in gsearch (dnasketch.rs:160) */
    uint64_t seed;               /* level generator seed (SPEC 5; upstream uses OS entropy) */
    uint32_t insert_batch;       /* B of SPEC 5 parallel_insert; 0 -> default */
} gs_index_params;

int      gs_index_create(gs_ctx *, const gs_index_params *, gs_index **out);
void     gs_index_destroy(gs_index *);
uint64_t gs_index_nb_point(const gs_index *);
int      gs_index_get_params(const gs_index *, gs_index_params *out);
/* parallel_insert(&[(&Vec<Sig>, usize)]) for ids that continue nb_point.. in input order, gsearch's own case (dnasketch.rs:429-433) */
int      gs_index_parallel_insert(gs_index *, const void *sigs, uint64_t n);
int      gs_index_parallel_insert_dev(gs_index *, const void *sigs_dev, uint64_t n);
/* parallel_insert(&[(&Vec<Sig>, usize)]) with the caller's DataIds (HOST array in both forms; hnsw_rs takes any usize, dnasketch.rs:426-435): searches
 * return them as d_id, both dump formats store them, and gs_index_set_ids / gs_index_get_ids carry them across gs_index_import / _export.
 * Inside the library nodes are numbered in insertion order; that number breaks distance ties in answers ((distance, insertion order) ascending)
 * and is the id whenever no ids were given. */
int      gs_index_parallel_insert_ids(gs_index *, const void *sigs, const uint64_t *ids, uint64_t n);
int      gs_index_parallel_insert_ids_dev(gs_index *, const void *sigs_dev, const uint64_t *ids, uint64_t n);
int      gs_index_set_ids(gs_index *, const uint64_t *ids, uint64_t n /* == nb_point */);
int      gs_index_get_ids(gs_index *, uint64_t first, uint64_t n, uint64_t *ids_out);
/* parallel_search(&[Vec<Sig>], knbn, ef) -> per query min(knbn, found) Neighbour{d_id, distance}, ascending by (distance, node number): the
 * node number is the insertion order, which IS d_id unless the caller gave its own ids (gs_index_parallel_insert_ids / gs_index_set_ids) - ties
 * are then still broken by insertion order, not by the caller's id - or the index came from gs_index_load_hnswrs of a dump with ids other than
 * 0..n-1, whose nodes are renumbered in data-file order (layer-major). Unused tail slots: id = UINT64_MAX, distance = +inf.
 * evals_out (optional): number of DistHamming evaluations spent per query.
 * ef: gsearch asks for 5000 (gsearch.rs:893). Up to ~6700 (at max_nb_conn <= 128) either traversal serves; beyond that, up to 65535, the call takes the
 * dense strategy (count matrix + look-up traversal) whatever the cost model says, and is GS_ERR_UNSUPPORTED where that is not possible
 * (m > 65535, GS_DIST_MODE=gather). */
int      gs_index_parallel_search(gs_index *, const void *queries, uint64_t nq, uint32_t knbn, uint32_t ef,
                                  uint64_t *ids_out, float *dist_out, uint32_t *count_out, uint64_t *evals_out);
int      gs_index_parallel_search_dev(gs_index *, const void *queries_dev, uint64_t nq, uint32_t knbn, uint32_t ef,
                                      uint64_t *ids_out_dev, float *dist_out_dev, uint32_t *count_out_dev,
                                      uint64_t *evals_out_dev);
/* the same search, also returning hnsw_rs' PointId of every neighbour (Neighbour.p_id, answer.rs:42): pid_layer_out[nq x knbn] = the layer the
 * point is filed under (its level), pid_rank_out[nq x knbn] = its rank among the points of that layer in insertion order; 0xFF / -1 in unused slots */
int      gs_index_parallel_search_pid(gs_index *, const void *queries, uint64_t nq, uint32_t knbn, uint32_t ef, uint64_t *ids_out, float *dist_out,
                                      uint32_t *count_out, uint64_t *evals_out, uint8_t *pid_layer_out, int32_t *pid_rank_out);
int      gs_index_parallel_search_pid_dev(gs_index *, const void *queries_dev, uint64_t nq, uint32_t knbn, uint32_t ef, uint64_t *ids_out_dev,
                                          float *dist_out_dev, uint32_t *count_out_dev, uint64_t *evals_out_dev, uint8_t *pid_layer_out_dev,
                                          int32_t *pid_rank_out_dev);
/* sketch_and_request (sketch the request genomes, then ONE parallel_search: sketch_and_request_dir_compressedkmer, dnarequest.rs:240-360) as one call on
 * device-resident genomes (layout of gs_sketch_batch_dev). Same answers as gs_sketch_batch_dev + gs_index_parallel_search_dev; with the dense strategy the
 * sketch of the next <= 3276 genomes runs on a second stream beside the count matrix of the previous ones. sig_out_dev (optional): the n_genomes signatures. */
int      gs_index_sketch_and_search_dev(gs_index *, const gs_sketch_params *, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                                        const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, void *sig_out_dev,
                                        uint32_t knbn, uint32_t ef, uint64_t *ids_out_dev, float *dist_out_dev, uint32_t *count_out_dev, uint64_t *evals_out_dev);
/* exact top-k by exhaustive DistHamming (recall ground truth; also what bindash.rs:120-157 computes) */
int      gs_index_bruteforce_search(gs_index *, const void *queries, uint64_t nq, uint32_t knbn,
                                    uint64_t *ids_out, float *dist_out);
/* the dense producer on its own: DistHamming of every query against EVERY node as 16-bit mismatch counts (count / m = the distance), the
 * matrix the dense traversal looks its distances up in - match-join (with heavy blocks through the compare tile kernel) or compare tile kernel
 * as the search would choose. counts_out: HOST nq x nb_point, row-major. Needs m <= 65535. (bindash.rs:120-157 computes the same all-pairs) */
int      gs_index_count_matrix(gs_index *, const void *queries, uint64_t nq, uint16_t *counts_out);
/* exact k nearest nodes of each query by exhaustive DistHamming (count matrix + device top-k select); keeps neighbours with
 * (float)count / (float)m <= max_dist (1.0f: no cut-off); 1 <= knbn <= 1024; needs m <= 65535 (GS_ERR_UNSUPPORTED otherwise).
 * Same answer layout as gs_index_parallel_search: nq x knbn ids / distances ascending by (distance, node number), the caller's ids, unused slots
 * UINT64_MAX / +inf, count_out[q] = neighbours kept. SPEC.md "Exact k-NN". */
int      gs_index_exact_search(gs_index *, const void *queries, uint64_t nq, uint32_t knbn, float max_dist,
                               uint64_t *ids_out, float *dist_out, uint32_t *count_out);
int      gs_index_exact_search_dev(gs_index *, const void *queries_dev, uint64_t nq, uint32_t knbn, float max_dist,
                                   uint64_t *ids_out_dev, float *dist_out_dev, uint32_t *count_out_dev);
/* the database against itself (hnsw2knn.rs; exact instead of the layer-0 lists): for nodes [first, first + n_rows) in insertion order,
 * their knbn nearest OTHER nodes. Only the node itself is excluded (by node number); duplicates of it at distance 0 stay. */
int      gs_index_knn_graph(gs_index *, uint32_t knbn, float max_dist, uint64_t first, uint64_t n_rows,
                            uint64_t *ids_out, float *dist_out, uint32_t *count_out);
int      gs_index_knn_graph_dev(gs_index *, uint32_t knbn, float max_dist, uint64_t first, uint64_t n_rows,
                                uint64_t *ids_out_dev, float *dist_out_dev, uint32_t *count_out_dev);
/* ann (embed.rs): statistics and a UMAP-like embedding of a k-NN graph, bit-exact and reproducible (SPEC.md 8). A graph is n rows of knbn
 * entries in the layout of gs_index_knn_graph, but in NODE NUMBERS: ids < n, count[i] kept entries ascending by distance, no self, no repeat,
 * distances >= 0 and not NaN (GS_ERR_INVALID otherwise). n x knbn < 2^31, knbn <= 1024. */
typedef struct {
    uint32_t dim;            /* output dimension, 1..4 (2) */
    uint32_t epochs;         /* E (0: the initial positions) */
    uint32_t neg_samples;    /* S negative samples per node and epoch, 1..65535 */
    float    neg_rate;       /* r: repulsion weight r * W_i / S per sample */
    float    lr;             /* learning rate at epoch 0, decaying linearly */
    uint64_t seed;           /* initial positions (when none are given) and negative samples */
} gs_embed_params;
gs_embed_params gs_embed_params_default(void);
/* positions (n x dim f32, row-major) after E epochs; prm NULL: defaults; init (n x dim, optional): the initial positions instead of the seeded
 * draw; memb_out (n x knbn f32, optional): the calibrated memberships p_it (0 in unused slots) */
int      gs_embed_knn_graph(gs_ctx *, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *count,
                            const gs_embed_params *prm, const float *init, float *pos_out, float *memb_out);
int      gs_embed_knn_graph_dev(gs_ctx *, uint64_t n, uint32_t knbn, const uint64_t *ids_dev, const float *dist_dev, const uint32_t *count_dev,
                                const gs_embed_params *prm, const float *init_dev, float *pos_out_dev, float *memb_out_dev);
/* the index's own exact k-NN graph (gs_index_knn_graph, never leaving the device) embedded; rows in node (insertion) order, also with caller ids.
 * init / pos_out: HOST. Empty index: GS_ERR_STATE; m > 65535: GS_ERR_UNSUPPORTED. */
int      gs_index_embed(gs_index *, uint32_t knbn, float max_dist, const gs_embed_params *prm, const float *init, float *pos_out);
typedef struct {
    uint64_t n, n_edges, n_empty;   /* rows, kept entries (sum of counts), rows with count 0 */
    uint32_t knbn, max_occ;
    double   occ_mean, occ_std, occ_skew;   /* k-occurrence moments; occ_skew = hubness (standardised third moment) */
    uint64_t hub_ids[16];           /* the 16 largest k-occurrences, ties by node number (node numbers; UINT64_MAX when n < 16) */
    uint32_t hub_occ[16];
    float    q_first[7], q_last[7]; /* quantiles 0.01 0.05 0.25 0.5 0.75 0.95 0.99 of the first / last kept distance (rows with count >= 1) */
} gs_knn_stats;
/* occ_out (n u32, optional): k-occurrence of every node; hist_out (65 u64, optional): nodes with occ 0..63, then >= 64. HOST arrays. */
int      gs_knn_graph_stats(gs_ctx *, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *count,
                            gs_knn_stats *stats_out, uint32_t *occ_out, uint64_t *hist_out);
int      gs_index_knn_graph_stats(gs_index *, uint32_t knbn, float max_dist, gs_knn_stats *stats_out, uint32_t *occ_out, uint64_t *hist_out);
/* quality of an embedding by neighbourhood conservation (embed.rs:68-70, get_quality_estimate_from_edge_length(200); SPEC.md 8.1): how much of
 * every row of the graph lies among the kq nearest points of its node in the EMBEDDED space, exactly, over all n x n pairs of positions. pos: n x dim
 * f32 (1 <= dim <= 4), finite. d2 = squared Euclidean distance in f32; kq_eff = min(kq, n - 1); rad2[i] = the kq_eff-th smallest d2 of node i to
 * another node; e2[i][t] = d2 of i to its t-th neighbour (+0 in unused slots); rank[i][t] = the number of OTHER nodes strictly nearer than that
 * neighbour (0xFFFFFFFF in unused slots). An edge is conserved when rank < kq_eff (the same as e2 <= rad2). n < 2, kq = 0, a coordinate that is not
 * finite and everything the graph rules above refuse: GS_ERR_INVALID. */
#define GS_EMBQ_TILE_Q 256u         /* rows of a workgroup of the counting kernel, one per thread; no result depends on it */
#define GS_EMBQ_TILE_P 1024u        /* points of one LDS tile of the counting kernel; no result depends on it */
#define GS_EMBQ_TIMES 20u           /* gs_embed_quality_last_ms: edge pass, rank pass, 16 radius passes, rank finish, summary on the host */
typedef struct {
    uint64_t n, n_rows, n_edges;        /* nodes, rows with count >= 1, kept entries */
    uint64_t n_conserved, n_nomatch;    /* conserved edges; rows with count >= 1 and no conserved edge */
    uint32_t knbn, kq_eff;
    double   mean_conserved;            /* n_conserved / (n_rows - n_nomatch), 0 when no row has a match */
    double   frac_conserved;            /* n_conserved / n_edges, NaN without edges */
    /* quantiles 0.01 0.05 0.25 0.5 0.75 0.95 0.99 over the rows with count >= 1 of: the longest embedded edge sqrt(max_t e2), the embedded
     * radius sqrt(rad2), and their ratio sqrt(max_t e2 / rad2) with 0/0 = 1, x/0 = +inf, inf/inf = 1 (all in f64; NaN when there is no such row) */
    double   q_edge[7], q_radius[7], q_ratio[7];
} gs_embed_quality_summary;
/* HOST arrays. hist_out (knbn + 1 u64, optional): rows with count >= 1 by their number of conserved edges. rank_out (n x knbn u32), e2_out
 * (n x knbn f32), rad2_out (n f32): optional. */
int      gs_embed_quality(gs_ctx *, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *count, const float *pos,
                          uint32_t dim, uint32_t kq, gs_embed_quality_summary *summary_out, uint64_t *hist_out, uint32_t *rank_out, float *e2_out,
                          float *rad2_out);
/* DEVICE arrays; the per-node arrays stay on the device (each optional; an array nobody asks for is not computed) */
int      gs_embed_quality_dev(gs_ctx *, uint64_t n, uint32_t knbn, const uint64_t *ids_dev, const float *dist_dev, const uint32_t *count_dev,
                              const float *pos_dev, uint32_t dim, uint32_t kq, uint32_t *rank_out_dev, float *e2_out_dev, float *rad2_out_dev);
/* the index's own exact k-NN graph (as gs_index_embed builds it: node numbers, never leaving the device) against HOST positions in node order.
 * Empty index: GS_ERR_STATE; m > 65535: GS_ERR_UNSUPPORTED. */
int      gs_index_embed_quality(gs_index *, uint32_t knbn, float max_dist, const float *pos, uint32_t dim, uint32_t kq,
                                gs_embed_quality_summary *summary_out, uint64_t *hist_out, uint32_t *rank_out, float *e2_out, float *rad2_out);
/* milliseconds of the stages of the context's last quality call (ms_out: GS_EMBQ_TIMES doubles; device stages by stream events; a stage that
 * did not run: 0) */
int      gs_embed_quality_last_ms(gs_ctx *, double *ms_out);
/* hnswcore (binaux/src/bin/hnswcore.rs): a coreset of the database, an optional k-medoid pass on it, and the dispatch of every node to its nearest
 * centre. All-integer and reproducible bit for bit (SPEC.md 10); Bmor's beta / gamma have no counterpart. */
typedef struct {
    uint32_t n_cluster;      /* k medoids; 0 = coreset only, the centres are the coreset points (hnswcore without --cluster) */
    double   fraction;       /* coreset size aimed at, as a fraction of the database, in (0, 1] (0.1, hnswcore.rs:328) */
    uint32_t max_iter;       /* k-medoid iterations at most, >= 1 (15, hnswcore.rs:272) */
    uint64_t seed;           /* sampling */
} gs_cluster_params;
gs_cluster_params gs_cluster_params_default(void);
typedef struct {
    uint64_t n_core;         /* p: points of the coreset */
    uint32_t iterations;     /* k-medoid iterations run */
    uint32_t converged;      /* 1: the last iteration moved no medoid */
    uint64_t cost_core;      /* sum over the coreset of weight x count to the medoid, at the last assign step */
    uint64_t cost_all;       /* sum over all nodes of the count to their centre */
} gs_cluster_info;
/* for every node, the position in cand_nodes (node numbers < nb_point, nc >= 1; the same node may be listed twice) that minimises
 * (mismatch count, position), and that count. arg_out / count_out: HOST, nb_point entries. Needs m <= 65535. */
int      gs_index_nearest_of(gs_index *, const uint64_t *cand_nodes, uint64_t nc, uint32_t *arg_out, uint16_t *count_out);
/* prm NULL: defaults. HOST outputs: centre_node_out[nb_point] = the NODE NUMBER of each node's centre (gs_index_get_ids maps it to the caller's id),
 * centre_count_out[nb_point] = the mismatch count to it, medoids_out[k] = the medoids' node numbers, ascending, sizes_out[k] = nodes dispatched to
 * each. Optional: core_nodes_out / core_weight_out (room for core_cap entries each): the coreset in node order and its weights; info_out->n_core is
 * written in any case, and a core_cap below it is GS_ERR_INVALID. Empty index: GS_ERR_STATE; m > 65535 or nb_point x m >= 2^40: GS_ERR_UNSUPPORTED. */
int      gs_index_cluster(gs_index *, const gs_cluster_params *prm, uint64_t *centre_node_out, uint16_t *centre_count_out, uint64_t *medoids_out,
                          uint64_t *sizes_out, uint64_t *core_nodes_out, uint64_t *core_weight_out, uint64_t core_cap, gs_cluster_info *info_out);
/* derep (SPEC.md 18): clusters of the database at a distance cut, exact, with no limit on a node's degree, in one pass over the count matrix.
 * Nodes u != v are LINKED iff their mismatch count is <= c_max, the largest count c with (float)c / (float)m <= max_dist (as in gs_index_exact_search);
 * equal signatures are linked. Every output is a function of the counts (and, for gs_index_derep, the priorities) alone. */
typedef struct {
    uint64_t n_clusters;     /* components / representatives */
    uint64_t n_singletons;   /* clusters of one node */
    uint64_t largest;        /* nodes of the largest cluster */
    uint32_t c_max;          /* the cut as a count */
    uint32_t reserved;       /* 0 */
} gs_derep_info;
/* single linkage: label_out[nb_point] (HOST) = the smallest NODE NUMBER of the node's connected component of the link graph.
 * max_dist NaN or negative, null outputs: GS_ERR_INVALID; empty index: GS_ERR_STATE; m > 65535: GS_ERR_UNSUPPORTED (also for gs_index_derep). */
int      gs_index_components(gs_index *, float max_dist, uint64_t *label_out, gs_derep_info *info_out);
/* greedy representatives (CD-HIT's incremental clustering in its -g 1 form). priority: nb_point HOST values, higher is better, NULL = all equal; the
 * rank of a node is its position under (priority descending, node number ascending). A node is a representative iff no representative of earlier
 * rank is linked to it. HOST outputs, nb_point entries: rep_node_out[v] = v and rep_count_out[v] = 0 for a representative, otherwise the NODE NUMBER
 * of the representative of earlier rank linked to v that minimises (mismatch count, rank), and that count. */
int      gs_index_derep(gs_index *, float max_dist, const uint64_t *priority, uint64_t *rep_node_out, uint16_t *rep_count_out, gs_derep_info *info_out);
/* Graph import / export (the role of hnswio::HnswIo::load_hnsw / Hnsw::file_dump, reloadhnsw.rs:41-51,
 * dumpload.rs:31, in this library's own dense layout): levels[n], entry id, layer 0: deg0[n], nbr0[n*2M],
 * cnt0[n*2M] (mismatch counts to the owner); upper layers: upidx[n] (-1 for level-0 nodes) and for the
 * n_upper nodes of level >= 1: degU[U*max_layer], nbrU[U*max_layer*M], cntU[...] (row l-1 = layer l). */
int      gs_index_import(gs_index *, const void *sigs, uint64_t n, const uint8_t *levels, int64_t entry,
                         const uint32_t *deg0, const uint32_t *nbr0, const uint32_t *cnt0, const int32_t *upidx,
                         uint64_t n_upper, const uint32_t *degU, const uint32_t *nbrU, const uint32_t *cntU);
int      gs_index_export(gs_index *, uint8_t *levels, int64_t *entry, uint32_t *deg0, uint32_t *nbr0,
                         uint32_t *cnt0, int32_t *upidx, uint64_t *n_upper, uint32_t *degU, uint32_t *nbrU,
                         uint32_t *cntU);
int      gs_index_get_data(gs_index *, uint64_t first, uint64_t n, void *sigs_out);
int      gs_index_save(gs_index *, const char *path);
int      gs_index_load(gs_ctx *, const char *path, gs_index **out);
/* hnsw_rs' own dump (Hnsw::file_dump / HnswIo::load_hnsw: dumpload.rs:26-31, reloadhnsw.rs:13-51): <basename>.hnsw.graph and
 * <basename>.hnsw.data, format 3. The byte layout is restated from the un-vendored crate as recalled (gs_hnswio.hip header lists every
 * recalled constant). dump needs max_layer = 16 and lists of at most 255 neighbours; load takes capacity / scale_modify / flags / seed /
 * insert_batch for later insertions from `hint` (may be NULL) - the dump itself holds only max_nb_connection, ef and the element type. */
int      gs_index_dump_hnswrs(gs_index *, const char *basename);
/* flags = GS_DUMP_TRUNCATE_255: neighbour counts are ONE byte in this format while layer 0 holds up to 2 * max_nb_conn = 256..510 ids; lists
 * longer than 255 are cut to their 255 closest entries (lossy for those nodes; without the flag such an index is refused - gs_index_save is lossless) */
enum { GS_DUMP_TRUNCATE_255 = 1 };
int      gs_index_dump_hnswrs_ex(gs_index *, const char *basename, uint32_t flags);
int      gs_index_load_hnswrs(gs_ctx *, const char *basename, const gs_index_params *hint, gs_index **out);
/* Host only, no context. Both files of a dump come from another program and are untrusted: SPEC.md 16.1 lists what is refused, in which order and
 * with which code; no size named by a file is allocated before it was held against the sizes of the files.
 * gs_hnswrs_describe: the description at the head of <basename>.hnsw.graph as it stands there (the reference's get_hnsw_type, reloadhnsw.rs:13-38),
 * nothing judged but its magic and that it is whole; the verify-only fields are 0.
 * gs_hnswrs_verify: everything gs_index_load_hnswrs checks before it touches the device, with the same codes and messages; out may be NULL. */
typedef struct {
    uint32_t dump_mode;          /* 1 = full, 0 = light (graph only) */
    uint32_t max_nb_conn;
    uint32_t nb_layer;
    int32_t  kind;               /* GS_KIND_* of t_name, -1: not a signature type of gsearch */
    uint64_t ef, nb_point, dimension;
    char     distance[128];      /* type names, NUL-terminated, cut to fit */
    char     t_name[32];
    /* filled by gs_hnswrs_verify only: what a load would build */
    uint64_t n_upper;            /* points above layer 0 */
    uint64_t entry;              /* node number of the entry point */
    uint64_t ids_are_nodes;      /* 1: the DataIds are 0..n-1 and are the node numbers; 0: nodes in data-file order, DataIds kept as caller ids */
    uint64_t digest;             /* FNV-1a of the loaded graph, vectors and ids (SPEC.md 16.3) */
} gs_hnswrs_description;
int      gs_hnswrs_describe(const char *basename, gs_hnswrs_description *out);
int      gs_hnswrs_verify(const char *basename, gs_hnswrs_description *out);
uint64_t gs_index_insert_evals(const gs_index *);      /* DistHamming evaluations spent by inserts so far */
/* after the last parallel_insert of a build (the replicas of a multi-GPU request, a server that only answers): gives the insert-time pair cache back - up to 55 % of
 * the device, 90 GB at 300 k nodes - and keeps everything a search needs. Later inserts still work (bit-identical graph): pairs among the nodes inserted before the
 * call are evaluated from their rows instead of looked up. */
int      gs_index_release_build_scratch(gs_index *);
/* device-side work counters of the searches and dense-mode inserts since the last reset (bench.py prices kernels with them):
 * out[0] memory-side atomics sent by the match-join, out[1] candidates popped by the dense traversal, out[2] pops that accepted
 * at least one neighbour, out[3] traversal workgroups in flight (last launch), out[4] bytes of adjacency a pop loads, out[5] / out[6] pops before / after the traversal
 * became order-free, out[7] chance matches on shared table entries the match-join expanded over a cluster's members (heavy blocks) */
int      gs_index_search_stats(gs_index *, uint64_t out[8], int reset);

/* ---------------------------------------------------------------------------------------------- */
/* bigsig (binaux/src/bin/bigsig.rs): a bit-sliced Bloom index (BIGSI) of reference genomes - bloom_size rows, one column ("colour") per genome in
 * the order added - and the genome each sequencing read comes from. Arithmetic: SPEC.md 11. A k-mer never contains a non-ACGT base (or, with
 * quality bytes, a base below min_phred): such a base ends a segment. The fields minimizer / coverage_filter of gs_bigsi_params other than 0 are
 * GS_ERR_UNSUPPORTED: bigsig's -m is a property of the index and comes in through gs_bigsi_create_mini, its -f is an argument of one build call,
 * gs_bigsi_add_batch_min_count[_dev] (SPEC.md 11.1). */
typedef struct gs_bigsi gs_bigsi;
typedef struct {
    uint32_t k;                  /* 1..32 (15 accepted) */
    uint32_t num_hash;           /* 1..16 rows per k-mer */
    uint64_t bloom_size;         /* rows, 1 <= bloom_size < 2^40, any value */
    uint32_t data_t;             /* GS_DATA_DNA (canonical k-mers) or GS_DATA_DNA_FWD */
    uint32_t minimizer;          /* 0 (anything else: GS_ERR_UNSUPPORTED; a minimizer index is made by gs_bigsi_create_mini) */
    uint32_t coverage_filter;    /* 0 (anything else: GS_ERR_UNSUPPORTED; the filter is the min_count of gs_bigsi_add_batch_min_count) */
} gs_bigsi_params;
typedef struct {
    gs_bigsi_params prm;
    uint64_t n_colours, colour_capacity;
    uint64_t row_words;          /* u64 words of a row = ceil(colour_capacity / 64); colour c is bit c & 63 of word c >> 6 */
} gs_bigsi_desc;
int    gs_bigsi_check_params(const gs_bigsi_params *prm);
/* the matrix (bloom_size x row_words u64, zeroed) is allocated here: the colour capacity is fixed */
int    gs_bigsi_create(gs_ctx *ctx, const gs_bigsi_params *prm, uint64_t colour_capacity, gs_bigsi **out);
/* A minimizer index (SPEC 11.1): prm->k is the window length, minimizer_len = m the length of the m-mers that are inserted and looked up, one per run of
 * windows that share their minimizer. m = 0 or m >= k: GS_ERR_INVALID. Every call below works on it as it is: the index knows its m. */
int    gs_bigsi_create_mini(gs_ctx *ctx, const gs_bigsi_params *prm, uint32_t minimizer_len, uint64_t colour_capacity, gs_bigsi **out);
uint32_t gs_bigsi_minimizer_len(gs_bigsi *bx);      /* 0: a plain index */
#define GS_BIGSI_MINI_TILE 63u      /* windows a wavefront of the minimizer kernel takes at a time; no result depends on it */
void   gs_bigsi_free(gs_bigsi *bx);
int    gs_bigsi_info(gs_bigsi *bx, gs_bigsi_desc *out);
/* n_genomes new colours, in input order; the layout of gs_sketch_batch_dev (2-bit packed, every record free of invalid bases). Past the capacity: GS_ERR_STATE */
int    gs_bigsi_add_batch_dev(gs_bigsi *bx, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                              const uint64_t *genome_rec_off_dev, uint64_t n_genomes);
/* host text: record r = bytes [rec_begin[r], rec_end[r]) of text (line breaks skipped), genome g = records [genome_rec_off[g], genome_rec_off[g+1]).
 * qual (optional): quality byte of text[i] at qual[i]; a base with qual[i] - 33 < min_phred counts as non-ACGT. The library splits and packs (a host loop). */
int    gs_bigsi_add_batch(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end,
                          uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes);
/* The same with a coverage filter (SPEC 11.1): within each new colour only values that occur at least min_count times are inserted, and nk_c counts their
 * occurrences; min_count <= 1: no filter, the calls above bit for bit. A colour whose every value is filtered keeps its number with t_c = 0. One colour holds
 * fewer than 2^32 occurrences here (GS_ERR_UNSUPPORTED beyond); its value list is sorted on the device, one colour at a time. */
int    gs_bigsi_add_batch_min_count_dev(gs_bigsi *bx, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev,
                                        uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint32_t min_count);
int    gs_bigsi_add_batch_min_count(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end,
                                    uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t min_count);
/* colours [first, first + n): bits set in the column (t_c) and k-mer occurrences fed (nk_c); either output may be NULL */
int    gs_bigsi_bits_set(gs_bigsi *bx, uint64_t first, uint64_t n, uint64_t *t_out, uint64_t *nk_out);
/* the named rows -> words_out[n x row_words] (HOST) */
int    gs_bigsi_rows(gs_bigsi *bx, const uint64_t *rows, uint64_t n, uint64_t *words_out);
/* read r = records [read_rec_off[r], read_rec_off[r+1]) (the mates of a pair: the records of one read). Of a read's k-mer occurrences in order, those
 * with running index j, j mod down_sample == 0, are used: n_kmers[r] of them. best_hits[r] = the largest number of used occurrences whose num_hash
 * rows all hold one colour's bit, best_colour[r] = the smallest colour reaching it (0 when best_hits is 0). counts (optional): n_reads x n_colours u32,
 * every colour's hits. down_sample = 0: GS_ERR_INVALID; no colour: GS_ERR_STATE. The _dev form queues on the context's stream. */
int    gs_bigsi_query_dev(gs_bigsi *bx, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                          const uint64_t *read_rec_off_dev, uint64_t n_reads, uint32_t down_sample, uint32_t *n_kmers_dev, uint32_t *best_colour_dev,
                          uint32_t *best_hits_dev, uint32_t *counts_dev);
int    gs_bigsi_query(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end, uint64_t n_rec,
                      const uint64_t *read_rec_off, uint64_t n_reads, uint32_t down_sample, uint32_t *n_kmers, uint32_t *best_colour, uint32_t *best_hits,
                      uint32_t *counts);
/* tail[r] = P(X >= best_hits), X ~ Binomial(n_kmers, (t_c / bloom_size)^num_hash) for c = best_colour (SPEC 11); accept[r] = best_hits > 0 and tail < fp_correct */
int    gs_bigsi_classify_dev(gs_bigsi *bx, uint64_t n_reads, const uint32_t *n_kmers_dev, const uint32_t *best_colour_dev, const uint32_t *best_hits_dev,
                             double fp_correct, double *tail_dev, uint8_t *accept_dev);
/* the accessions of the colours (n == n_colours); read back NUL-terminated, back to back: buf NULL to size (*bytes_out) */
int    gs_bigsi_set_accessions(gs_bigsi *bx, const char *const *names, uint64_t n);
int    gs_bigsi_accessions(gs_bigsi *bx, char *buf, uint64_t cap_bytes, uint64_t *bytes_out);
/* own little-endian file (SPEC 11; upstream's .bxi is a bincode of crate types): version 1 for a plain index, version 2 (it holds m) for a minimizer
 * index; load takes both. load: colour_capacity 0 = the file's n_colours */
int    gs_bigsi_save(gs_bigsi *bx, const char *path);
int    gs_bigsi_load(gs_ctx *ctx, const char *path, uint64_t colour_capacity, gs_bigsi **out);
/* Host only, no context; the file is untrusted (SPEC.md 16.2: what is refused, in which order, with which code - the size of the file is held against
 * bloom_size x ceil(n_colours / 64) words before the device is asked for anything). gs_bigsi_describe: the fixed header as it stands in the file, nothing
 * judged but magic and version; gs_bigsi_verify: everything gs_bigsi_load checks before it allocates, same codes and messages; out may be NULL. */
typedef struct {
    uint32_t version;            /* 1: a plain index, 2: a minimizer index */
    uint32_t k, num_hash, data_t;
    uint32_t minimizer_len;      /* 0 in version 1 */
    uint32_t has_accessions;     /* verify only: some accession is not empty */
    uint64_t bloom_size, n_colours;
    uint64_t row_words;          /* ceil(n_colours / 64): u64 words of a row IN THE FILE */
    uint64_t digest;             /* verify only: FNV-1a of every byte behind the fixed header (SPEC.md 16.3) */
} gs_bigsi_file_description;
int    gs_bigsi_describe(const char *path, gs_bigsi_file_description *out);
int    gs_bigsi_verify(const char *path, gs_bigsi_file_description *out);
/* host arithmetic of SPEC 11, no device: the num_hash rows of k-mer value v; the segments of a text (begin = offset of the first base, len in bases,
 * segments shorter than min_len dropped; arrays may be NULL / cap 0 to count only); the tail */
int    gs_bigsi_positions(uint64_t v, uint32_t num_hash, uint64_t bloom_size, uint64_t *pos_out);
int    gs_bigsi_split(const void *text, const void *qual, uint64_t n, uint32_t min_phred, uint64_t min_len, uint64_t cap, uint64_t *seg_begin,
                      uint64_t *seg_len, uint64_t *n_out);
double gs_bigsi_tail(uint64_t t_c, uint64_t bloom_size, uint32_t num_hash, uint32_t n_kmers, uint32_t best_hits);
/* host arithmetic of SPEC 11.1, no device: the minimizer occurrences of one text (window k, minimizer m, 1 <= m < k <= 32) in order - value_out = the m-mer value,
 * pos_out = the offset in text of its first base. *n_out = their number; the arrays are filled up to cap entries and may be NULL to count only. */
int    gs_bigsi_minimizers(const void *text, const void *qual, uint64_t n, uint32_t min_phred, uint32_t k, uint32_t m, uint32_t data_t, uint64_t cap,
                           uint64_t *value_out, uint64_t *pos_out, uint64_t *n_out);
/* `{prefix}_reads.txt`: read_id, accession | no_hits, best_hits, n_kmers, accept | reject, tab-separated, one line per read; `{prefix}_counts.txt`:
 * accession, reads over the accepted reads (descending by count, then by accession), then a `reject` and a `no_hits` line. Host only. */
int    gs_bigsig_write_reads(const char *prefix, const char *const *accessions, uint64_t n_colours, const char *const *read_ids, uint64_t n_reads,
                             const uint32_t *best_colour, const uint32_t *best_hits, const uint32_t *n_kmers, const uint8_t *accept);
/* Tied top hits and the six-field report (SPEC.md 11.2). The query with ties: n_kmers and best_hits as gs_bigsi_query; n_tied[r] = the number of colours
 * that reach best_hits (0 when best_hits is 0), exact; tied[r x max_ties ..] = the min(n_tied, max_ties) smallest of them, ascending, UINT32_MAX in the
 * slots behind them (written by the call: the buffer may hold anything); sig_colour[r] = the tied colour with the fewest bits set, the smallest of equal
 * ones (UINT32_MAX when best_hits is 0), taken over all tied colours. tied[r x max_ties] is gs_bigsi_query's best_colour wherever best_hits > 0.
 * max_ties outside 1 .. GS_BIGSI_MAX_TIES: GS_ERR_INVALID; the other codes are gs_bigsi_query's. The _dev form queues on the context's stream. */
#define GS_BIGSI_MAX_TIES 1024u
#define GS_BIGSI_DEFAULT_TIES 16u
int    gs_bigsi_query_ties_dev(gs_bigsi *bx, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                               const uint64_t *read_rec_off_dev, uint64_t n_reads, uint32_t down_sample, uint32_t max_ties, uint32_t *n_kmers_dev,
                               uint32_t *best_hits_dev, uint32_t *n_tied_dev, uint32_t *tied_dev, uint32_t *sig_colour_dev);
int    gs_bigsi_query_ties(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end,
                           uint64_t n_rec, const uint64_t *read_rec_off, uint64_t n_reads, uint32_t down_sample, uint32_t max_ties, uint32_t *n_kmers,
                           uint32_t *best_hits, uint32_t *n_tied, uint32_t *tied, uint32_t *sig_colour);
/* the verdict of a read, the first row that holds: no occurrence used; no hit; the tail of sig_colour not below fp_correct; one top colour; several */
enum { GS_BIGSI_TOO_SHORT = 0, GS_BIGSI_NO_HITS = 1, GS_BIGSI_NOT_SIGNIFICANT = 2, GS_BIGSI_UNIQUE = 3, GS_BIGSI_TIED = 4 };
/* tail[r] = gs_bigsi_tail for c = sig_colour (1.0 where best_hits is 0); verdict[r] = gs_bigsi_verdict_code of the read */
int    gs_bigsi_verdict_dev(gs_bigsi *bx, uint64_t n_reads, const uint32_t *n_kmers_dev, const uint32_t *best_hits_dev, const uint32_t *n_tied_dev,
                            const uint32_t *sig_colour_dev, double fp_correct, double *tail_dev, uint8_t *verdict_dev);
/* host arithmetic, no device: the verdict table alone */
uint32_t gs_bigsi_verdict_code(uint32_t n_kmers, uint32_t best_hits, uint32_t n_tied, double tail, double fp_correct);
/* `{prefix}_reads.txt`: read_id, status, hits, n_kmers, accept | reject, ties - tab-separated, one line per read. status: too_short | no_hits |
 * no_significant_hits | the accession | the listed accessions joined by `,` (then `,...` when n_tied > max_ties); hits and ties are 0 in the first three.
 * `{prefix}_counts.txt`: accession, reads over the GS_BIGSI_UNIQUE reads (descending by count, then by accession), then a `reject` (not significant + tied),
 * a `no_hits` and a `too_short` line. A verdict above GS_BIGSI_TIED, max_ties outside 1 .. GS_BIGSI_MAX_TIES, and on a UNIQUE or TIED read n_tied = 0 or a
 * listed colour >= n_colours: GS_ERR_INVALID, before anything is written. Host only. */
int    gs_bigsig_write_report(const char *prefix, const char *const *accessions, uint64_t n_colours, const char *const *read_ids, uint64_t n_reads,
                              uint32_t max_ties, const uint32_t *n_kmers, const uint32_t *best_hits, const uint32_t *n_tied, const uint32_t *tied,
                              const uint8_t *verdict);

/* ---------------------------------------------------------------------------------------------- */
/* Multi-GPU: one process per GPU, query batches sharded, DB + graph replicated. The path has ONE exchange step - the
 * all-gather of the per-rank top-k blocks - and this is it, over RCCL / xGMI, for hosts that are not Python (the reference's host is
 * Rust; conceptual ancestor: the per-shard loop of scripts/multiple_search.sh:71-107). Bootstrap like NCCL: one rank calls
 * gs_comm_unique_id and hands the 128 bytes to the others by its own means (file, socket, MPI); every rank then calls gs_comm_create. */
typedef struct gs_comm gs_comm;
int  gs_comm_unique_id(void *id_out_128);
int  gs_comm_create(gs_ctx *, int n_ranks, int rank, const void *id_128, gs_comm **out);
void gs_comm_destroy(gs_comm *);
int  gs_comm_rank(const gs_comm *);
int  gs_comm_size(const gs_comm *);
/* ids_dev / dist_dev: this rank's nq_local x knbn block (device memory); all_*_dev: n_ranks x nq_local x knbn, rank order.
 * One ncclAllGather of the packed block (12 bytes per neighbour). Same nq_local and knbn on every rank. */
int  gs_comm_allgather_topk_dev(gs_comm *, const uint64_t *ids_dev, const float *dist_dev, uint64_t nq_local, uint32_t knbn,
                                uint64_t *all_ids_dev, float *all_dist_dev);
/* the same exchange for UNEQUAL shards (a contiguous sharding of a batch hands out blocks that differ by one query; a rank may hold none): every rank
 * passes its own nq_local and the same nq_max >= all of them; all_*_dev (room for n_ranks x nq_max rows) receive the COMPACT concatenation in rank order,
 * counts_out (HOST, n_ranks, optional) every rank's count. Still ONE ncclAllGather - of fixed-size blocks, gs_topk_block_bytes() each. */
int  gs_comm_allgatherv_topk_dev(gs_comm *, const uint64_t *ids_dev, const float *dist_dev, uint64_t nq_local, uint64_t nq_max, uint32_t knbn,
                                 uint64_t *all_ids_dev, float *all_dist_dev, uint64_t *counts_out);
/* the same exchange WITHOUT the host round trip: the pack kernel, the ncclAllGather and the unpack kernel are queued on the context's stream and the call returns;
 * work queued afterwards on that stream (the next step's sketch, gs_topk_merge_dev) sees the gathered answers in order. counts_dev (DEVICE, n_ranks + 1 words,
 * optional): every rank's count, then a word that is non-zero when a rank sent a block of another shape. gs_comm_wait: waits for the stream, fails with
 * GS_ERR_INVALID on such a block, hands the counts of the LAST exchange to the host (counts_out: HOST, n_ranks, optional). */
int  gs_comm_allgatherv_topk_async_dev(gs_comm *, const uint64_t *ids_dev, const float *dist_dev, uint64_t nq_local, uint64_t nq_max, uint32_t knbn,
                                       uint64_t *all_ids_dev, float *all_dist_dev, uint64_t *counts_dev);
int  gs_comm_wait(gs_comm *, uint64_t *counts_out);
/* the block layout itself, on the HOST (no device needed), for hosts that move the blocks by their own means (MPI, sockets): header {u64 nq_local, u32 knbn,
 * u32 magic}, nq_max x knbn ids, nq_max x knbn distances. unpack: n_ranks blocks back to back -> compact rows in rank order + counts. */
uint64_t gs_topk_block_bytes(uint64_t nq_max, uint32_t knbn);
int  gs_topk_pack(const uint64_t *ids, const float *dist, uint64_t nq_local, uint64_t nq_max, uint32_t knbn, void *block_out);
int  gs_topk_unpack(const void *blocks, int n_ranks, uint64_t nq_max, uint32_t knbn, uint64_t *all_ids, float *all_dist, uint64_t *counts_out);
/* DB-sharded alternative (the per-shard loop + merge of scripts/multiple_search.sh:71-107: the database split over the GPUs, every rank answers ALL queries
 * on its shard, the gathered answers are merged): ids_dev / dist_dev = n_shards x nq x knbn_in (shard-major, as gathered), id_offset (HOST, optional) is
 * added to the ids of each shard; out_*_dev: nq x knbn_out, the best under (distance, id). */
int  gs_topk_merge_dev(gs_ctx *, const uint64_t *ids_dev, const float *dist_dev, uint32_t n_shards, uint64_t nq, uint32_t knbn_in, const uint64_t *id_offset,
                       uint32_t knbn_out, uint64_t *out_ids_dev, float *out_dist_dev);
/* Split databases on ONE device (the loop of scripts/multiple_search.sh with the queries sketched once, SPEC.md 17 items 12-18): the queries and their
 * running answers stay on the device while the pieces of the database are loaded, searched and closed one after the other.
 * gs_topk_reset_dev: nq empty running lists - run_ids UINT64_MAX, run_dist +inf, run_count 0, run_evals (optional) 0.
 * gs_index_search_merge_dev: for every listed row q = rows_dev[r] (rows_dev NULL: every query, nr is ignored) the answers A of
 * gs_index_parallel_search_dev(piece, queries[q], knbn, ef), id_offset added to every id, are merged into run[q] in place: run[q] becomes the first
 * knbn of run[q] and A ascending by (distance as its bit pattern, id) - the rule of gs_topk_merge_dev -, the running entry first on a full tie;
 * run_count[q] = min(knbn, run_count[q] + count), run_evals[q] (optional) += evals, unused tail slots UINT64_MAX / +inf. Only the first run_count[q]
 * entries of run[q] are read, and they are ascending under that order (what a reset and earlier merges leave). A row that is not listed is not written.
 * queries_dev: nq rows of the index's signature type, back to back. rows_dev: strictly ascending and below nq, checked on the device before the search
 * starts (GS_ERR_INVALID, nothing written). knbn <= 1024 (GS_ERR_UNSUPPORTED beyond); nq < 2^31. The refusals of gs_index_parallel_search_dev apply.
 * gs_index_search_merge: the same with every pointer in HOST memory. */
int  gs_topk_reset_dev(gs_ctx *, uint64_t nq, uint32_t knbn, uint64_t *run_ids_dev, float *run_dist_dev, uint32_t *run_count_dev, uint64_t *run_evals_dev);
int  gs_index_search_merge_dev(gs_index *piece, const void *queries_dev, uint64_t nq, const uint32_t *rows_dev, uint64_t nr, uint32_t knbn, uint32_t ef,
                               uint64_t id_offset, uint64_t *run_ids_dev, float *run_dist_dev, uint32_t *run_count_dev, uint64_t *run_evals_dev);
int  gs_index_search_merge(gs_index *piece, const void *queries, uint64_t nq, const uint32_t *rows, uint64_t nr, uint32_t knbn, uint32_t ef,
                           uint64_t id_offset, uint64_t *run_ids, float *run_dist, uint32_t *run_count, uint64_t *run_evals);

/* ---------------------------------------------------------------------------------------------- */
/* Synthetic inputs generated in HBM (bench / tests): counter-based, reproducible on the host.      */
/* DNA genome g of length L: packed word w (32 bases, 8 bytes little endian as stored) =             */
/*   splitmix64 finaliser of (seed*0x9e3779b97f4a7c15 + g*0xbf58476d1ce4e5b9 + w)  (see gs_synth.hip) */
int gs_synth_dna_dev(gs_ctx *, uint64_t seed, uint64_t first_genome, uint64_t n_genomes, uint64_t len_bases,
                     void *seq_dev /* n_genomes * ceil(len/32)*8 bytes */);
/* proteome g of length L (residues of the 20-letter alphabet, one byte each; ceil(L/8)*8 bytes per proteome, back to back): residue j of
 * word w = "ACDEFGHIKLMNPQRSTVWY"[byte j of the synth word of (seed ^ 0xAA5EED, g, w) mod 20] */
int gs_synth_aa_dev(gs_ctx *, uint64_t seed, uint64_t first_proteome, uint64_t n_proteomes, uint64_t len_residues, void *seq_dev);
/* related genomes: genome g = root genome number hash(seed,g) mod n_roots with iid substitutions at rate
 * mu(g) ~ U[mu_lo, mu_hi] (Jaccard to the root ~ p/(2-p), p=(1-mu)^k). Same layout as gs_synth_dna_dev. */
int gs_synth_dna_family_dev(gs_ctx *, uint64_t seed, uint64_t first_genome, uint64_t n_genomes, uint64_t len_bases,
                            uint64_t n_roots, double mu_lo, double mu_hi, void *seq_dev);
/* sketch-level database: n_roots random root signatures; row r belongs to root hash(seed,r) mod n_roots
 * and keeps each root slot with probability J(r) ~ U[j_lo, j_hi], else draws its own value. */
int gs_synth_sigs_dev(gs_ctx *, int kind, uint32_t m, uint64_t seed, uint64_t first_row, uint64_t n_rows,
                      uint64_t n_roots, double j_lo, double j_hi, void *sigs_dev /* n_rows x m */);
/* the same two generators with SKEWED family sizes (the regime of NCBI / GTDB prokaryotes, /root/reference/README.md:134: a few species with 10^4 genomes,
 * a long tail of singletons): member g belongs to root floor(n_roots * u(g)^alpha), u uniform in [0,1) - root 0 holds a fraction n_roots^(-1/alpha) of
 * everything (alpha = 3.5, n_roots = 3000: 10 %), the sizes fall off as a power law. alpha = 1 is uniform. */
int gs_synth_dna_family_skew_dev(gs_ctx *, uint64_t seed, uint64_t first_genome, uint64_t n_genomes, uint64_t len_bases,
                                 uint64_t n_roots, double mu_lo, double mu_hi, double alpha, void *seq_dev);
int gs_synth_sigs_skew_dev(gs_ctx *, int kind, uint32_t m, uint64_t seed, uint64_t first_row, uint64_t n_rows,
                           uint64_t n_roots, double j_lo, double j_hi, double alpha, void *sigs_dev /* n_rows x m */);

/* ---------------------------------------------------------------------------------------------- */
/* Debugging (tests only, not for production use): device temporaries are never cleared between uses, and these two calls fill them with a chosen
 * byte so that a kernel which reads what nothing wrote shows in a comparison (tests/test_gpu_stale_scratch.py).
 * gs_debug_mem_fill: process-wide; byte 0..255 = on, -1 = off (the default), anything else GS_ERR_INVALID. While on, every device allocation the
 * library makes (gs_dev_alloc included) and every scratch slot at the moment a call takes it is filled, whole, with the byte. Each fill
 * synchronises the whole device. Off costs one relaxed atomic load per allocation.
 * gs_index_debug_fill_scratch: fills the buffers an index keeps as per-call scratch (not its data, graph, caches or counters), synchronously. */
int gs_debug_mem_fill(int byte);
int gs_index_debug_fill_scratch(gs_index *, int byte);
/* Debugging (tests only, not for production use): the three device primitives of gs_radix.hip, on which the sorted ProbMinHash form, FracMinHash sketches,
 * the seed order of superani, the coverage filter of bigsig, the adjacency of the embedding and the candidate order of the gene caller stand, exposed for
 * parity tests against numpy (tests/test_gpu_radix.py). All pointers are HOST pointers: each call stages to the device, runs the primitive on the
 * context's stream, waits, and copies back.
 * gs_debug_radix_sort_u64: out[0..n) = keys[0..n) in ascending, stable order on bits [0, 8 * ceil(endbit / 8)) - the passes take whole 8-bit digits, so
 *   an endbit that is no multiple of 8 is only the order on bits [0, endbit) when every key is zero from endbit upwards. endbit outside 1..64:
 *   GS_ERR_INVALID. n = 0 writes nothing, n = 1 returns the key.
 * gs_debug_run_lengths_u64: the r runs of equal neighbours of sorted[0..n): uniq[0..r) their keys, len[0..r) their lengths, *n_runs_out = r; nothing is
 *   written from r on. n = 0: GS_ERR_UNSUPPORTED (the primitive's own refusal), as is n >= 2^32.
 * gs_debug_scan_u32: out[0..n) = the exclusive prefix sums of in[0..n) modulo 2^32, *total_out = the sum. n = 0: *total_out = 0, out is not written. */
int gs_debug_radix_sort_u64(gs_ctx *c, const uint64_t *keys, uint64_t n, int endbit, uint64_t *out);
int gs_debug_run_lengths_u64(gs_ctx *c, const uint64_t *sorted, uint64_t n, uint64_t *uniq, uint32_t *len, uint64_t *n_runs_out);
int gs_debug_scan_u32(gs_ctx *c, const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *total_out);
/* Debugging (tests only, not for production use): the two host drivers of the DistHamming compare kernels (gs_hamming.hip), which produce every distance
 * of the library and are otherwise reached only through the index, exposed for parity tests against numpy (tests/test_gpu_hamming.py). All pointers are
 * HOST pointers: each call stages to the device, runs the driver on the context's stream exactly as its callers do, waits, and copies back. kind is
 * GS_KIND_F32, GS_KIND_U32 or GS_KIND_U64 (anything else: GS_ERR_UNSUPPORTED); row strides are in bytes, hold at least a row of m elements and are
 * multiples of 4; the bytes of a row beyond its m elements may hold anything. A null context, operand or parts_out, m = 0 or a bad stride:
 * GS_ERR_INVALID; a row count, list length or output pitch of 2^24 or more, a row stride of 2^32
 * bytes or more, or an operand of more than 2^32 bytes (rows x stride): GS_ERR_UNSUPPORTED. *parts_out = the number of parts the row words were split into over the grid's third dimension (1 = no split).
 * gs_debug_hamming_strided: the dense form. Q: nq rows at strideQ_bytes, C: nc rows at strideC_bytes (buffers of nq * strideQ_bytes and
 *   nc * strideC_bytes bytes). shift_bytes (a multiple of the element size, below 256, else GS_ERR_INVALID): both device copies start that many bytes
 *   behind a 256-byte boundary. form 0: out[q * ld_out + e] = (float)count / (float)m (f32), form 1: the mismatch count as u32, form 2: as u16
 *   (m <= 65535); another form, or ld_out < nc: GS_ERR_INVALID. out holds nq * ld_out elements of the form's type; it is uploaded before the call and
 *   downloaded after it, so the cells with a column from nc on come back as the caller set them. nq = 0 or nc = 0: GS_OK, *parts_out = 1, nothing
 *   else is written.
 * gs_debug_hamming_blocks: the work-list form. items: n_items x {first entry in qlist, query rows, first entry in clist, candidate rows} (u32); item i
 *   writes out16[qlist[a] * ld_out + clist[b]] = the mismatch count of query row qlist[a] and candidate row clist[b] for every a, b of its two
 *   ranges; no two items may name the same cell. The first n_thin items go to the thin kernel where it applies. out16: nq_rows x ld_out u16, uploaded
 *   and downloaded like `out` above: every cell that no item names comes back as the caller set it. What the driver takes on trust is checked
 *   here, GS_ERR_INVALID otherwise: item ranges inside the lists, list entries below nq_rows / nc_rows, 1..128 rows on each side of an item, at
 *   most 16 query rows in each of the first n_thin items, n_thin <= n_items, m <= 65535, ld_out >= nc_rows. n_items = 0: GS_OK, *parts_out = 1,
 *   nothing else is written. */
int gs_debug_hamming_strided(gs_ctx *c, int kind, uint32_t m, const void *Q, uint64_t nq, uint64_t strideQ_bytes, const void *C, uint64_t nc,
                             uint64_t strideC_bytes, uint32_t shift_bytes, int form, void *out, uint64_t ld_out, uint32_t *parts_out);
int gs_debug_hamming_blocks(gs_ctx *c, int kind, uint32_t m, const void *Q, uint64_t nq_rows, uint64_t strideQ_bytes, const void *C, uint64_t nc_rows,
                            uint64_t strideC_bytes, const uint32_t *items, uint32_t n_items, const uint32_t *qlist, uint64_t n_qlist, const uint32_t *clist,
                            uint64_t n_clist, uint32_t n_thin, uint16_t *out16, uint64_t ld_out, uint32_t *parts_out);

#ifdef __cplusplus
}
#endif
#endif
