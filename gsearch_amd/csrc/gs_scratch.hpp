// gs_scratch.hpp — the names of the per-context scratch slots and the bookkeeping of who holds one. Plain C++ (no HIP): tests/test_scratch_leases.py
// compiles it with the host compiler alone. gs_internal.hpp puts the device memory behind it (ScratchPool, PoolBuf, PinnedPool).
#pragma once
#include <stdint.h>
#include <memory>
#include "../../include/gsearch_amd.h"

namespace gs {

void set_error(const char *fmt, ...);       // gs_ctx.hip: the text behind gs_last_error()

// One enumerator per buffer role, grouped by owner: this list is the map of the pool. To add a buffer, add an enumerator. A slot is one grow-only
// device allocation per context, so two buffers that can be alive at the same time need two enumerators; the lease check below reports the ones that do not.
#define GS_SCRATCH_SLOT_LIST(X)                                                                                                                       \
    /* sketch_dev_impl, every algorithm: unit prefix of the records, units of the genomes */                                                          \
    X(SK_REC_UNITS) X(SK_GENOME_UNITS)                                                                                                                \
    /* OPH (optdens / revoptdens) */                                                                                                                  \
    X(OPH_TABLE) X(OPH_WIN)                                                                                                                           \
    /* SuperMinHash (run_smh): slot table, then the cold walk */                                                                                      \
    X(SMH_TABLE) X(SMH_COLD_FLAGS) X(SMH_COLD_LIST) X(SMH_COLD_Q) X(SMH_COLD_P) X(SMH_COLD_CNT)                                                       \
    /* ProbMinHash driver (run_prob): alive around whichever form runs */                                                                             \
    X(PROB_REC_UNITS) X(PROB_GENOME_UNITS) X(PROB_REC_KMERS) X(PROB_GENOME_KMERS)                                                                     \
    /* ProbMinHash, bucketed and tiered forms (the sorted form's names for the same memory follow the enum) */                                        \
    X(PROB_INFO) X(PROB_BOFF) X(PROB_VBASE) X(PROB_HIST) X(PROB_BST) X(PROB_BSZ) X(PROB_BGN) X(PROB_CTR) X(PROB_VALS) X(PROB_Q) X(PROB_QPREV)         \
    X(PROB_SIG) X(PROB_SIGPASS) X(PROB_THR) X(PROB_WMAX) X(PROB_QMAX) X(PROB_CAND_V) X(PROB_CAND_H) X(PROB_CAND_GB) X(PROB_AKEY) X(PROB_SEGN)         \
    X(PROB_TMPV) X(PROB_COARSE)                                                                                                                       \
    /* ProbMinHash, sorted form: what it does not share with the other two */                                                                         \
    X(PROBS_GENOME_UNITS) X(PROBS_REC_KMERS) X(PROBS_GENOME_KMERS) X(PROBS_POS)                                                                       \
    /* HLL (run_hll): global register tables, survivor lists of pass A */                                                                             \
    X(HLL_GTAB) X(HLL_SURVIVORS)                                                                                                                      \
    /* HyperMinHash sketch (run_hmh): merge table of a genome split over workgroups */                                                                \
    X(HMH_GTAB)                                                                                                                                       \
    /* gs_sketch_batch: staging of a host-pointer call */                                                                                             \
    X(SKB_SEQ) X(SKB_REC_START) X(SKB_REC_LEN) X(SKB_GENOME_OFF) X(SKB_SIG)                                                                           \
    /* ingest (ingest_records_dev) */                                                                                                                 \
    X(INGEST_BEGIN) X(INGEST_END) X(INGEST_COUNT) X(INGEST_BASE)                                                                                      \
    /* inflate: stream descriptors / results, CRC-32 chunks, FASTA scan, staging of gs_gunzip_batch */                                                \
    X(INFL_STREAMS) X(INFL_RESULTS) X(CRC_CHUNKS) X(CRC_POWERS) X(CRC_OUT) X(SCAN_CHUNKS) X(SCAN_STARTS) X(SCAN_COUNT) X(SCAN_FILE_END)               \
    X(SCAN_HEADER_END) X(SCAN_CAPSID) X(GUNZIP_COMP) X(GUNZIP_TEXT)                                                                                   \
    /* index: staging of search requests and of user rows */                                                                                          \
    X(IX_QUERIES) X(IX_IDS) X(IX_DIST) X(IX_COUNT) X(IX_EVALS) X(IX_PAIR_L) X(IX_PAIR_R) X(IX_ROW_STAGE) X(IX_SKETCH_SIG)                             \
    /* index: the database's own k-NN graph (self_graph_dev) */                                                                                       \
    X(IXG_IDS) X(IXG_DIST) X(IXG_COUNT)                                                                                                               \
    /* hamming: widened u16 rows of the device forms, staging of gs_hamming_qxc / gs_hamming_pairs */                                                 \
    X(HAM_WIDE_Q) X(HAM_WIDE_C) X(HAM_Q) X(HAM_C) X(HAM_OUT) X(HAMP_A) X(HAMP_B) X(HAMP_IA) X(HAMP_IB) X(HAMP_OUT) X(HAMP_WIDE_A) X(HAMP_WIDE_B)      \
    /* hypermash (gs_hmh.hip) */                                                                                                                      \
    X(HMH_CARD_Q) X(HMH_CARD_R) X(HMH_NB) X(HMH_PACK_Q) X(HMH_PACK_R) X(HMH_LIST) X(HMH_LIST_REL) X(HMHC_SIGS) X(HMHC_CARD)                           \
    X(HMHS_Q) X(HMHS_R) X(HMHS_SIM)                                                                                                                   \
    /* ann / embed (gs_embed.hip) */                                                                                                                  \
    X(EMB_FLAG) X(EMB_PM) X(EMB_KEYS) X(EMB_ALT) X(EMB_RADIX) X(EMB_RANGE) X(EMB_DEG) X(EMB_OFF) X(EMB_ADJ) X(EMB_W) X(EMB_WSUM) X(EMB_HEAVY)         \
    X(EMB_Y0) X(EMB_Y1) X(KST_OCC) X(KST_ENDS) X(EMBIN_IDS) X(EMBIN_DIST) X(EMBIN_COUNT) X(EMB_INIT) X(EMB_POS) X(EMB_MEMB)                           \
    /* superaai (gs_frac.hip) */                                                                                                                      \
    X(FRAC_CAND) X(FRAC_THR) X(FRAC_OFF) X(FRAC_CAP) X(FRAC_CNT) X(FRAC_TASK) X(FRAC_SEL) X(FRAC_DIST) X(FRAC_ALT) X(FRAC_LEN) X(FRAC_POS)            \
    X(FRAC_RADIX) X(FRAC_NRUNS) X(FRAC_COPY_SRC) X(FRAC_COPY_DST) X(FRAC_COPY_N) X(FRAC_HOST_ROWS) X(FRACB_TEXT) X(FRACB_RESIDUES)                    \
    X(FRACS_Q) X(FRACS_QOFF) X(FRACS_R) X(FRACS_ROFF) X(FRACS_SIM) X(FRACS_COMMON) X(FRACS_UNION)                                                     \
    /* hnswcore (gs_cluster.hip): gathered rows of a block, candidate list, running (count, position) pairs, sampling, then the k-medoid state */         \
    X(CL_ROWS) X(CL_NODES) X(CL_BEST) X(CL_IN0) X(CL_BLOCKS) X(CL_CORE) X(CL_WEIGHT) X(CL_LABEL) X(CL_P) X(CL_TOT) X(CL_MED) X(CL_DMIN) X(CL_ACC)    \
    X(CL_OUT_NODE) X(CL_OUT_COUNT) X(CL_OUT_ARG)                                                                                                       \
    /* derep (gs_derep.hip): the nodes in rank order; per node its parent (components) or its rank once it is a representative (greedy); per row of a   \
       block its cover and its mask of earlier block members; the block's representatives; per node its representative and the count; counters */      \
    X(DR_ORDER) X(DR_STATE) X(DR_COVER) X(DR_MASK) X(DR_BREP) X(DR_OUT_NODE) X(DR_OUT_COUNT) X(DR_ACC)                                                 \
    /* bigsig (gs_bigsi.hip): unit prefix of a build, the colour block's bitmaps, staging of the host forms and of gs_bigsi_rows */                   \
    X(BIGSI_REC_UNITS) X(BIGSI_GENOME_UNITS) X(BIGSI_BITMAP) X(BIGSI_SEQ) X(BIGSI_REC_START) X(BIGSI_REC_LEN) X(BIGSI_GROUP_OFF) X(BIGSI_OUT_N)       \
    X(BIGSI_OUT_COLOUR) X(BIGSI_OUT_HITS) X(BIGSI_OUT_COUNTS) X(BIGSI_ROW_LIST) X(BIGSI_ROW_WORDS)                                                    \
    /* bigsig, minimizer indexes and the coverage filter: tile prefix of a build, per-genome window counts, the ordered per-read lists of a query */ \
    X(BIGSI_REC_TILES) X(BIGSI_GENOME_TILES) X(BIGSI_GENOME_WINDOWS) X(BIGSI_Q_OFF) X(BIGSI_Q_CNT) X(BIGSI_Q_VALS)                                    \
    /* bigsig, sort-count-filter build of one colour: value list and its second buffer, run lengths, head positions, radix counts, cursor + runs */  \
    X(BIGSI_LIST_VALS) X(BIGSI_LIST_ALT) X(BIGSI_LIST_LEN) X(BIGSI_LIST_POS) X(BIGSI_LIST_RADIX) X(BIGSI_LIST_CTR)                                    \
    /* bigsig, the query with ties (host form): per read the number of tied colours, the listed ones, the most significant one */                      \
    X(BIGSI_OUT_NTIED) X(BIGSI_OUT_TIED) X(BIGSI_OUT_SIG)                                                                                              \
    /* superani (gs_ani.hip), seeds: staging of the host form, unit prefix and per-unit counts of a block of genomes, the seeds of a block */           \
    X(ANIB_SEQ) X(ANIB_REC_START) X(ANIB_REC_LEN) X(ANIB_GOFF) X(ANI_UPRE) X(ANI_GUNIT) X(ANI_UCNT) X(ANI_GBASE) X(ANI_SEEDS)                         \
    /* superani, pairs: staging of the host form, value-ordered keys of both sides, slices of a block of pairs and its offsets */                      \
    X(ANIP_Q) X(ANIP_QOFF) X(ANIP_R) X(ANIP_ROFF) X(ANIP_PQ) X(ANIP_PR) X(ANIP_OUT) X(ANI_QKEYS) X(ANI_RKEYS) X(ANI_KEYS_ALT) X(ANI_RADIX)            \
    X(ANI_SLICES) X(ANI_SLICE_CNT) X(ANI_SLICE_BASE) X(ANI_AOFF) X(ANI_SOFF)                                                                          \
    /* superani, a block's anchors, its segments, the chaining result, chain ends and the per-seed marks of both sides */                              \
    X(ANI_A_RCTG) X(ANI_A_RPOS) X(ANI_A_QCTG) X(ANI_A_QPOS) X(ANI_A_STRAND) X(ANI_A_RIDX) X(ANI_A_QIDX) X(ANI_A_PAIR) X(ANI_SEG_TILES)                \
    X(ANI_SEG_START) X(ANI_SEG_N) X(ANI_F) X(ANI_PRED) X(ANI_ROOT) X(ANI_BEST) X(ANI_NCHAIN) X(ANI_MATCHED) X(ANI_DIFF)                               \
    /* hmmsearch (gs_hmm.hip). What a host form stages of its inputs - the forms of one context cannot nest, so they share these: the records, the     \
       profiles of a list of pairs, the Viterbi and MSV floors, the row offsets of the envelopes */                                                    \
    X(HMMB_AA) X(HMMB_REC_START) X(HMMB_REC_LEN) X(HMMB_PAIR_PROF) X(HMMB_FLOOR) X(HMMB_MSV_FLOOR) X(HMMB_ROW_OFF)                                     \
    /* hmmsearch, the score matrices of a call where they are not the caller's device memory: a host form's staging, or the matrix nobody asked for;   \
       the records of a call, longest first; per profile the records that a floor selects and their number */                                          \
    X(HMM_VIT) X(HMM_MSV) X(HMM_FWD) X(HMM_ORDER) X(HMM_SEL) X(HMM_SEL_COUNT)                                                                          \
    /* hmmsearch, the int16 filter (SPEC 13.7): the vf matrix of a call like the matrices above, a host form's staging of the vf floors */              \
    X(HMM_VF) X(HMMB_VF_FLOOR)                                                                                                                         \
    /* hmmsearch over a list of pairs (trace-back, envelopes): a block's pairs and their profiles' lists; a host form's staging of per-pair outputs: \
       the score, the Backward score, the number of domains or envelopes, those, and the two row arrays of the envelopes */                            \
    X(HMMP_PAIRS) X(HMMP_PROFS) X(HMMB_PAIR_SCORE) X(HMMB_PAIR_BCK) X(HMMB_PAIR_COUNT) X(HMMB_PAIR_ITEMS) X(HMMB_OUT_ROWS) X(HMMB_CONT_ROWS)           \
    /* hmmsearch, a block's scratch: back-pointers and row specials of the trace-back, Forward and Backward rows of the envelopes */                   \
    X(HMMT_PTR) X(HMMT_ROWS) X(HMME_FROWS) X(HMME_BROWS)                                                                                               \
    /* hmmsearch, null2: the pairs and the listed envelope slots of a call, which pairs have a score, a block's kept M and I rows of Forward (its       \
       special rows lie in HMME_FROWS: the forms of one context cannot nest); a host form's staging of the n2 vectors */                               \
    X(HMMN_PAIRS) X(HMMN_SLOTS) X(HMMN_OK) X(HMMN_KEEP) X(HMMB_PAIR_N2)                                                                                \
    /* hmmsearch, alignment: per listed slot where its nibbles and columns start, the place of the seg_raw words null2's Forward writes and nobody      \
       reads (everything else lies in null2's, the trace's and the envelopes' slots: the forms of one context cannot nest); a host form's columns */    \
    X(HMMA_SLOTS) X(HMMA_SEG) X(HMMB_PAIR_COLS)                                                                                                         \
    /* hmmsearch, best hits to sketcher records (gs_hmm_hits.hip): per (genome, profile) pair whether it is a hit, its residues and where they start    \
       in the source; the prefix sums of the first two; the two totals and the error word */                                                            \
    X(HMMH_FLAG) X(HMMH_LEN) X(HMMH_SRC) X(HMMH_POS) X(HMMH_OFF) X(HMMH_META)                                                                          \
    /* orfs (gs_orf.hip): tile prefix of the records and the call's counters; per tile the last stop of each (strand, class) pair, then its kept ORFs,      \
       residues and long drops (each scanned in place); the partial results of those scans; staging of the host form */                                 \
    X(ORF_REC_TILES) X(ORF_META) X(ORF_STOPS) X(ORF_COUNTS) X(ORF_PARTIALS) X(ORFB_SEQ) X(ORFB_REC_START) X(ORFB_REC_LEN) X(ORFB_ORF) X(ORFB_AA)         \
    X(ORFB_AA_START) X(ORFB_AA_LEN) X(ORFB_REC_OFF)                                                                                                    \
    /* genes (gs_gene.hip): per genome the hexamer counts of both strands and the in-frame dicodon counts of the training intervals; the call's error word */ \
    X(GENE_BG) X(GENE_COD) X(GENE_META)                                                                                                                \
    /* genes, a call: the ORF descriptors, the tables, one training interval per ORF, every ORF's best start; two columns and their prefix sums; the     \
       candidates' keys, sorted, and the candidates in (record, end, strand) order; per record their range, per candidate k(i), the running maximum of   \
       the chain and who reaches it, the predecessor, the choice; staging of the host form */                                                            \
    X(GENE_ORF) X(GENE_ORF_LEN) X(GENE_ORF_START) X(GENE_ORF_OFF) X(GENE_TABLES) X(GENE_IV) X(GENE_BEST_J) X(GENE_SCORE) X(GENE_FLAGS) X(GENE_COL0)     \
    X(GENE_COL1) X(GENE_SCAN0) X(GENE_SCAN1) X(GENE_KEYS) X(GENE_KEYS_ALT) X(GENE_RADIX) X(GENE_CAND_ORF) X(GENE_CAND) X(GENE_REC_CAND) X(GENE_K)      \
    X(GENE_PMAX) X(GENE_PARG) X(GENE_PRED) X(GENE_CHOSEN) X(GENEB_SEQ) X(GENEB_REC_START) X(GENEB_REC_LEN) X(GENEB_GOFF) X(GENEB_INFO) X(GENEB_TABLES) \
    X(GENEB_GENE) X(GENEB_AA) X(GENEB_AA_START) X(GENEB_AA_LEN) X(GENEB_REC_OFF) X(GENE_SCAN_SUMS) X(GENE_SCAN_OFFS)                                                                      \
    /* comm (gs_topk_merge_dev) */                                                                                                                    \
    X(COMM_ID_OFFSET)                                                                                                                                 \
    /* gs_radix.hip behind host pointers (gs_debug_radix_sort_u64, gs_debug_run_lengths_u64, gs_debug_scan_u32; the suite only): the keys, their second \
       buffer and the radix counts of a sort; the sorted keys, runs, lengths, head positions, head counts and run counter; the values and their sum */  \
    X(DBG_SORT_KEYS) X(DBG_SORT_ALT) X(DBG_SORT_RADIX) X(DBG_RLE_SORTED) X(DBG_RLE_UNIQ) X(DBG_RLE_LEN) X(DBG_RLE_POS) X(DBG_RLE_RADIX) X(DBG_RLE_NRUNS) \
    X(DBG_SCAN_VALS) X(DBG_SCAN_TOTAL)                                                                                                                 \
    /* gs_hamming.hip behind host pointers (gs_debug_hamming_strided, gs_debug_hamming_blocks; the suite only): both operands and the output of the     \
       dense form; both operands, the items, the two row lists and the output of the work-list form */                                                  \
    X(DBG_HAM_Q) X(DBG_HAM_C) X(DBG_HAM_OUT) X(DBG_HAMB_Q) X(DBG_HAMB_C) X(DBG_HAMB_ITEMS) X(DBG_HAMB_QLIST) X(DBG_HAMB_CLIST) X(DBG_HAMB_OUT)              \
    /* split databases (gs_split.hip): the flag of the row check, the gathered query rows, a piece's answers to them (ids, distances, counts,         \
       evaluations); the host twin's staging of the queries and of the listed rows' running lists */                                                  \
    X(SPLIT_FLAG) X(SPLIT_QROWS) X(SPLIT_IDS) X(SPLIT_DIST) X(SPLIT_COUNT) X(SPLIT_EVALS) X(SPLITB_QUERIES) X(SPLITB_RUN_IDS) X(SPLITB_RUN_DIST)      \
    X(SPLITB_RUN_COUNT) X(SPLITB_RUN_EVALS)

enum ScratchSlot : int {
#define X(name) SL_##name,
    GS_SCRATCH_SLOT_LIST(X)
#undef X
    SCRATCH_SLOTS        // the number of slots
};
inline const char *scratch_slot_name(ScratchSlot s)
{
    static const char *const names[] = {
#define X(name) #name,
        GS_SCRATCH_SLOT_LIST(X)
#undef X
    };
    return (int)s >= 0 && s < SCRATCH_SLOTS ? names[s] : "?";
}

// Second names for memory that sibling forms share ON PURPOSE, because some of these buffers run to gigabytes. A second name is only sound where the two
// users can never be alive together - the reason stands at each group, and the lease check holds it to that.
//
// sketch_dev_impl runs ONE algorithm per call and run_smh / run_hll / run_prob never call one another: the workspaces of HLL and of the ProbMinHash forms
// lie in SuperMinHash's (the cold-walk scratch of either is 8 m bytes per lane, the ProbMinHash generator states 0.5 GB).
constexpr ScratchSlot SL_HLL_CUT = SL_SMH_TABLE, SL_HLL_COLD_FLAGS = SL_SMH_COLD_FLAGS, SL_HLL_COLD_LIST = SL_SMH_COLD_LIST, SL_HLL_COLD_Q = SL_SMH_COLD_Q,
                      SL_HLL_COLD_P = SL_SMH_COLD_P, SL_HLL_CNT = SL_SMH_COLD_CNT;
constexpr ScratchSlot SL_PROB_AGL = SL_SMH_TABLE, SL_PROB_ACNT = SL_SMH_COLD_FLAGS, SL_PROB_ASTATE = SL_SMH_COLD_LIST, SL_PROB_PH = SL_SMH_COLD_Q,
                      SL_PROB_PB = SL_SMH_COLD_P, SL_PROB_OVF = SL_SMH_COLD_CNT;
// The tiered form is the bucketed form with other bucket descriptors; run_prob calls the two one after the other, never one from the other.
constexpr ScratchSlot SL_PROBT_DESC = SL_PROB_BST, SL_PROBT_BIG = SL_PROB_BSZ, SL_PROBT_KEPT = SL_PROB_TMPV;
// The sorted form takes what the other two flag or do not suit, after they have returned (run_prob, old_range): its k-mer keys and their sorted copy
// (8 bytes per k-mer each) lie in the memory of the bucketed values and registers.
constexpr ScratchSlot SL_PROBS_BASE = SL_PROB_INFO, SL_PROBS_Q = SL_PROB_BOFF, SL_PROBS_QPREV = SL_PROB_VBASE, SL_PROBS_SIG = SL_PROB_HIST,
                      SL_PROBS_SIGPASS = SL_PROB_BST, SL_PROBS_WMAX = SL_PROB_BSZ, SL_PROBS_QMAX = SL_PROB_BGN, SL_PROBS_NACT = SL_PROB_CTR,
                      SL_PROBS_VALS = SL_PROB_VALS, SL_PROBS_SORTED = SL_PROB_Q, SL_PROBS_UCNT = SL_PROB_SIG, SL_PROBS_NRUNS = SL_PROB_SIGPASS,
                      SL_PROBS_RADIX = SL_PROB_THR, SL_PROBS_CAND_H = SL_PROB_WMAX, SL_PROBS_CAND_B = SL_PROB_QMAX, SL_PROBS_AKEY = SL_PROB_CAND_V,
                      SL_PROBS_ACNT = SL_PROB_CAND_H, SL_PROBS_ASTATE = SL_PROB_CAND_GB, SL_PROBS_NLIST = SL_PROB_AKEY, SL_PROBS_REC_UNITS = SL_PROB_SEGN;

// Who holds which slot of ONE pool. A lease describes host scopes only: kernels still queued when a scope ends are protected by stream order (a slot is
// only handed out again by a later call on the same context, i.e. behind them on its stream).
struct SlotLeases {
    uint8_t held[SCRATCH_SLOTS] = {};
    bool take(ScratchSlot s) { if (held[s]) return false; held[s] = 1; return true; }
    void give(ScratchSlot s) { held[s] = 0; }
};
// One lease. It keeps the table it took the slot from alive and gives back to that table only: a pool that was deleted in between (gs_ctx_release_scratch,
// on_worker_failed) has dropped its reference, the pool made after it has a table of its own, and neither is touched.
struct SlotLease {
    std::shared_ptr<SlotLeases> from; ScratchSlot slot;
    explicit SlotLease(ScratchSlot s) : slot(s) {}
    SlotLease(const SlotLease &) = delete;
    SlotLease &operator=(const SlotLease &) = delete;
    ~SlotLease() { give(); }
    // GS_OK: the slot of `table` is ours (or already was: allocating again through the same object is allowed). An error: another lease holds it.
    // *fresh (optional): this call is the one that took the lease - the slot's content is whatever its last holder left (gs_debug_mem_fill poisons it
    // then); false when the object held it already, and the caller may count on what it wrote there
    int take(const std::shared_ptr<SlotLeases> &table, bool *fresh = nullptr)
    {
        if (fresh) *fresh = false;
        if (from == table) return GS_OK;
        give();
        if (!table->take(slot)) {
            set_error("scratch slot %s is already in use further up this call: two buffers that are alive at once need two slots (gs_scratch.hpp)", scratch_slot_name(slot));
            return GS_ERR_STATE;
        }
        from = table;
        if (fresh) *fresh = true;
        return GS_OK;
    }
    void give() { if (from) { from->give(slot); from.reset(); } }
};

// Pinned host staging (PinnedPool): one range of slots per role.
enum : int {
    PIN_TEXT = 0, PIN_TEXT_N = 16,                            // gs_sketch_files: the texts of the groups in flight
    PIN_COMP = PIN_TEXT + PIN_TEXT_N, PIN_COMP_N = 16,        //                  their compressed members for the device inflate
    PIN_INFLATE = PIN_COMP + PIN_COMP_N, PIN_INFLATE_N = 2,   //                  inflate descriptors / results, one per parity
    PIN_JOIN = PIN_INFLATE + PIN_INFLATE_N,                   // match_join_counts: its host-side lists
    PINNED_SLOTS = PIN_JOIN + 1
};
static_assert(PIN_TEXT == 0 && PIN_TEXT + PIN_TEXT_N <= PIN_COMP && PIN_COMP + PIN_COMP_N <= PIN_INFLATE && PIN_INFLATE + PIN_INFLATE_N <= PIN_JOIN &&
                  PIN_JOIN < PINNED_SLOTS,
              "the ranges of the pinned pool are disjoint and fit");

}  // namespace gs
