// gs_orf.hpp - what gs_gene.hip shares with gs_orf.hip: the tile passes of SPEC 14 up to the counts and the emission of the descriptors.
#pragma once
#include "gs_internal.hpp"

namespace gs {

struct OrfArgs {
    const uint8_t *seq; const uint64_t *rec_start, *rec_len, *rtoff, *meta;
    uint64_t n_rec, cap_tiles;
    uint64_t *stops;                       // [6][cap_tiles], pair q = 2 class + strand
    uint64_t *counts;                      // [3][cap_tiles]: kept ORFs, residues, long drops
    uint64_t stop_mask; uint32_t min_aa, max_aa, table_ix;
    gs_orf *orf; uint8_t *aa; uint64_t *aa_start, *aa_len;
};
struct OrfWork {
    PoolBuf rtoff, meta, stops, counts, partials;
    OrfArgs a{};
    explicit OrfWork(gs_ctx *c) : rtoff(c, SL_ORF_REC_TILES), meta(c, SL_ORF_META), stops(c, SL_ORF_STOPS), counts(c, SL_ORF_COUNTS), partials(c, SL_ORF_PARTIALS) {}
};

// the passes up to the counts: n_out filled, the scanned per-tile state left in w for orf_emit. Waits for the stream once.
int orf_count(gs_ctx *c, const gs_orf_params *prm, const uint8_t *seq, uint64_t seq_bytes, const uint64_t *rs, const uint64_t *rl, uint64_t n_rec, OrfWork &w,
              uint64_t n_out[3]);
// queued on c's stream behind orf_count; nothing is waited for. aa = nullptr: descriptors, aa_start, aa_len and rec_orf_off without the residues
int orf_emit(gs_ctx *c, uint64_t n_rec, OrfWork &w, gs_orf *orf, uint8_t *aa, uint64_t *aa_start, uint64_t *aa_len, uint64_t *rec_orf_off);

}  // namespace gs
