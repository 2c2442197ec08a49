// gs_bigsi.hip — bigsig (binaux/src/bin/bigsig.rs): a bit-sliced Bloom index of genomes and the genome each read comes from. Arithmetic: SPEC.md 11,
// constants in gs_spec.hpp; layout and what binds each kernel: DESIGN.md 3.15.
//
//  The matrix M is row-major: row r = W = ceil(capacity / 64) u64 words at M + r * W, colour c = bit c & 63 of word c >> 6. All offsets are 64-bit.
//
//  build, a block of <= 512 colours at a time:
//  * k_bigsi_fill      : walk_genome per genome (`parts` workgroups each), every k-mer ORs its num_hash bits into the genome's private bitmap
//                        of bloom_size bits in scratch (atomicOr: a few MB per genome, re-hit while it is walked).
//  * k_bigsi_popcount  : t_c of every genome of the block from its bitmap.
//  * k_bigsi_transpose : 512 rows x the block's colours per workgroup. Each colour's 64 bytes (512 rows) are staged in LDS, 64 colours x 32 rows
//                        become 32 row words by __ballot, the words of 256 rows are staged again and leave as runs of 8 words = 64 bytes per row.
//  query:
//  * k_bigsi_query     : one wavefront per read, lanes = colour words. 64 k-mers are hashed at once (one per lane), then taken in turn: num_hash
//                        nontemporal row loads, an AND, and a ripple add of the 64-bit vector into bit-plane counters in registers.
//  * k_bigsi_classify  : one lane per read, the binomial tail of SPEC 11.
//  * k_bigsi_query<.., TIES = true> (SPEC 11.2): every colour that reaches the largest count instead of the smallest one - their number, the first max_ties
//                        in ascending order (popcount + a wave prefix sum place each lane's colours), the one with the fewest bits set.
//  * k_bigsi_verdict   : one lane per read, the tail of that colour and the verdict table of SPEC 11.2.
//  minimizer indexes and the coverage filter (SPEC 11.1):
//  * k_bigsi_minimizers: one wavefront per tile of MZ_TILE windows of one record. Every lane windows and hashes the m-mer at its position, keys and
//                        (value, h1, step) of the tile and its halo go to LDS, every lane picks the minimizer of its window (minimizer_pick, gs_spec.hpp)
//                        and compares it with its left neighbour's. Three consumers: bits of a genome's bitmap (build), an unordered value list of one
//                        colour (build with a filter), an ordered list per read (query; one wavefront per read, ballot + popcount compaction).
//  * k_bigsi_query<.., LIST = true> takes its values from that list instead of windowing the sequence; everything after the hash is the same kernel.
//  * filter            : per colour the value list -> radix_sort_u64 -> run_length_encode_u64 -> k_bigsi_fill_runs (runs of at least min_count) ->
//                        the bitmap, then popcount and transpose as ever. A plain index lists its k-mers with walk_genome (k_bigsi_list).
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"
#include "gs_bigsi_file.hpp"
#include "gs_walk.hpp"

struct gs_bigsi {
    gs_ctx *c = nullptr;
    gs_bigsi_params prm{};
    uint64_t cap = 0, W = 0, n = 0;
    uint32_t m = 0;                        // minimizer length, 0 = a plain index
    gs::DevBuf M, tc, nk;                  // the matrix; t_c and nk_c of every colour
    std::vector<std::string> names;        // accessions (empty until set)
};

namespace gs {

constexpr uint32_t BX_BLOCK = 512;         // colours of a build block: 8 words = one 64-byte sector of every row
constexpr uint32_t TR_ROWS = 512;          // rows of a transpose tile: 64 bytes of every colour's bitmap
constexpr uint32_t TR_IN_PITCH = 17;       // u32 per colour in LDS (16 + 1: lanes = colours read one column without bank conflicts)
constexpr uint32_t TR_OUT_PITCH = 9;       // u64 per row in LDS (8 + 1)

static inline uint32_t bigsi_kq(const gs_bigsi_params &p) { return p.k | (p.data_t == GS_DATA_DNA_FWD ? (uint32_t)KQ_FWD : 0u); }
// u32 words of one genome's bitmap: whole transpose tiles
static inline uint64_t bitmap_pitch(uint64_t B) { return round_up(B, TR_ROWS) / 32; }

struct BitEmit {
    uint32_t *bm; uint64_t B; uint32_t h;
    __device__ __forceinline__ void bits(uint64_t h1, uint64_t st) const
    {
        for (uint32_t i = 0; i < h; i++) {
            const uint64_t pos = bigsi_pos(h1, st, i, B);
            atomicOr(&bm[pos >> 5], 1u << (pos & 31));
        }
    }
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const
    {
        uint64_t h1, st;
        bigsi_hash(v, h1, st);
        bits(h1, st);
    }
};
// the values themselves, unordered, for the sort-count-filter build of one colour of a plain index (cap: the list's size; the count is exact, so nothing is cut)
struct ListEmit {
    uint64_t *vals; unsigned long long *cursor; uint64_t cap;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const
    {
        const uint64_t i = atomicAdd(cursor, 1ull);
        if (i < cap) vals[i] = v;
    }
};
__global__ __launch_bounds__(SK_THREADS) void k_bigsi_fill(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                           const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off,
                                                           const uint64_t *__restrict__ gen_units, uint32_t kq, uint64_t B, uint32_t h, uint32_t *__restrict__ bm,
                                                           uint64_t pitch)
{
    const uint64_t g = blockIdx.y;
    BitEmit emit{bm + g * pitch, B, h};
    walk_genome<false, BitEmit>(seq, rec_start, rec_len, rec_upre, genome_rec_off[g], genome_rec_off[g + 1], gen_units[g], kq, blockIdx.x, gridDim.x, emit);
}
__global__ __launch_bounds__(SK_THREADS) void k_bigsi_list(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                           const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off,
                                                           const uint64_t *__restrict__ gen_units, uint32_t kq, uint64_t *__restrict__ vals,
                                                           unsigned long long *__restrict__ cursor, uint64_t cap)
{
    ListEmit emit{vals, cursor, cap};
    walk_genome<false, ListEmit>(seq, rec_start, rec_len, rec_upre, genome_rec_off[0], genome_rec_off[1], gen_units[0], kq, blockIdx.x, gridDim.x, emit);
}
// tc[g] += bits of genome g's bitmap (grid: x = slices, y = genomes); nk[g] = k-mer occurrences of its records (slice 0; nk NULL: the caller counts them itself)
__global__ __launch_bounds__(256) void k_bigsi_popcount(const uint32_t *__restrict__ bm, uint64_t pitch, const uint64_t *__restrict__ rec_len,
                                                        const uint64_t *__restrict__ genome_rec_off, uint32_t k, unsigned long long *__restrict__ tc,
                                                        unsigned long long *__restrict__ nk)
{
    const uint64_t g = blockIdx.y;
    const uint32_t *b = bm + g * pitch;
    unsigned long long s = 0, q = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < pitch; i += (uint64_t)gridDim.x * 256) s += __popc(b[i]);
    if (blockIdx.x == 0 && nk)
        for (uint64_t r = genome_rec_off[g] + threadIdx.x; r < genome_rec_off[g + 1]; r += 256) { const uint64_t l = rec_len[r]; if (l >= k) q += l - k + 1; }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o); q += __shfl_down(q, o); }
    if ((threadIdx.x & 63) == 0) { if (s) atomicAdd(&tc[g], s); if (q) atomicAdd(&nk[g], q); }
}
// Colour slot sc of the block = bit sc & 63 of word w0 + (sc >> 6); slot sc holds genome sc - cshift of the block (cshift = first colour & 63), none
// outside [0, ng). The first word is OR-ed into the matrix when earlier colours share it (or_first); every other word of the block is new.
__global__ __launch_bounds__(256) void k_bigsi_transpose(const uint32_t *__restrict__ bm, uint64_t pitch, uint32_t ng, uint32_t cshift, uint64_t B,
                                                         uint64_t *__restrict__ M, uint64_t W, uint64_t w0, uint32_t nw, int or_first)
{
    __shared__ uint32_t s_in[BX_BLOCK * TR_IN_PITCH];
    __shared__ uint64_t s_out[256 * TR_OUT_PITCH];
    const uint64_t r0 = (uint64_t)blockIdx.x * TR_ROWS;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 16 lanes read the 64 contiguous bytes of one colour
    for (uint32_t idx = tid; idx < nw * 64 * 16; idx += 256) {
        const uint32_t sc = idx >> 4, j = idx & 15;
        const int gi = (int)sc - (int)cshift;
        s_in[sc * TR_IN_PITCH + j] = (gi >= 0 && gi < (int)ng) ? bm[(uint64_t)gi * pitch + (r0 >> 5) + j] : 0u;
    }
    __syncthreads();
    for (uint32_t half = 0; half < 2; half++) {
        for (uint32_t wi = wave; wi < nw; wi += 4) {
            for (uint32_t jj = 0; jj < 8; jj++) {
                const uint32_t v = s_in[(wi * 64 + lane) * TR_IN_PITCH + half * 8 + jj];
                uint64_t keep = 0;
#pragma unroll
                for (uint32_t b = 0; b < 32; b++) {
                    const uint64_t word = __ballot((v >> b) & 1u);
                    if (lane == b) keep = word;
                }
                if (lane < 32) s_out[(jj * 32 + lane) * TR_OUT_PITCH + wi] = keep;
            }
        }
        __syncthreads();
        // 8 lanes write the 64 contiguous bytes of one row
        for (uint32_t idx = tid; idx < 256 * 8; idx += 256) {
            const uint32_t row = idx >> 3, w = idx & 7;
            const uint64_t r = r0 + half * 256 + row;
            if (w < nw && r < B) {
                const uint64_t val = s_out[row * TR_OUT_PITCH + w];
                uint64_t *p = M + r * W + w0 + w;
                if (or_first && w == 0) { if (val) *p |= val; }
                else *p = val;
            }
        }
        __syncthreads();
    }
}

__global__ void k_bigsi_gather_rows(const uint64_t *__restrict__ M, uint64_t W, const uint64_t *__restrict__ rows, uint64_t n, uint64_t *__restrict__ out)
{
    const uint64_t total = n * W;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / W, w = t - i * W;
        out[t] = M[rows[i] * W + w];
    }
}

// ---- query -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl64(uint64_t x, uint32_t src)
{
    return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)src) << 32) | (uint32_t)__shfl((int)(uint32_t)x, (int)src);
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, uint32_t m)
{
    return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), (int)m) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)x, (int)m);
}
__device__ __forceinline__ uint64_t readlane64(uint64_t x, uint32_t lane_uniform)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)lane_uniform) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)lane_uniform);
}
// the k-mer value (SPEC 1.1) of the k bases from base s of the packed sequence; every base of it lies inside one record
__device__ __forceinline__ uint64_t kmer_at(const uint64_t *__restrict__ w64, uint64_t s, uint32_t k, uint64_t mask, bool fwd_only)
{
    const uint64_t u = s >> 5;
    const uint32_t o = (uint32_t)(s & 31);
    uint64_t left = __builtin_bswap64(w64[u]) << (2 * o);
    if (o + k > 32) left |= __builtin_bswap64(w64[u + 1]) >> (64 - 2 * o);          // o >= 1 here
    left &= ~(uint64_t)0 << (64 - 2 * k);
    const uint64_t fwd = left >> (64 - 2 * k);
    if (fwd_only) return fwd;
    const uint64_t rc = rc64(left) & mask;                                          // the 32 - k padding bases end up above the mask
    return fwd < rc ? fwd : rc;
}
// Counts are u32. A read of fewer than 2^BX_PLANES_SHORT k-mers (every sequencing read) keeps 12 planes; the same kernel with 32 planes takes the others
// (a contig given as a read) in a second launch: each launch leaves the other's reads alone.
enum { BX_PLANES_SHORT = 12, BX_PLANES_LONG = 32 };
// planes += a 1-bit vector, from plane p up; leaves as soon as no lane of the wavefront carries (nested ifs: the planes keep constant indices, i.e. registers)
template <int p, int BX_PLANES> __device__ __forceinline__ void ripple_add(uint64_t (&P)[BX_PLANES], uint64_t carry)
{
    if constexpr (p < BX_PLANES) {
        if (__ballot(carry != 0) == 0) return;
        const uint64_t t = P[p] & carry;
        P[p] ^= carry;
        ripple_add<p + 1, BX_PLANES>(P, t);
    }
}
// HB: row loads in flight per k-mer (num_hash when it is <= 4, else 4; a short last group repeats its last row: AND is idempotent)
// LIST (a minimizer index): the values come from the ordered per-read lists k_bigsi_minimizers wrote - seq64 = the values, rec_start[read] = where the
// read's list begins, rec_len[read] = its entries, read_rec_off unused. A list is walked as ONE record whose windows are its entries (its "length" is
// entries + k - 1), so the running index, down_sample and n are the arithmetic of the plain form.
// TIES (SPEC 11.2): instead of the smallest colour that reaches the largest count, all of them - their number, the first max_ties in ascending order, and
// the one with the fewest bits set (the smallest tail). The plain form carries an empty BxTies and none of the code below that names it.
template <bool TIES> struct BxTies {};
template <> struct BxTies<true> {
    const uint64_t *tc;                    // t_c of every colour
    uint32_t *n_tied, *tied, *sig;         // per read: |T_r|, its first max_ties members (UINT32_MAX behind them), argmin (t_c, c) over T_r
    uint32_t max_ties;
};
__device__ __forceinline__ uint32_t wave_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// One chunk's cand (the colours of word wi that hold the largest count so far; lanes in ascending word order) appended to the read's list, which holds n_tied
// colours already: an exclusive prefix sum of the lanes' popcounts places each lane's colours, every lane walks its set bits. (sig_t, sig_c): the smallest
// (t_c, c) so far; earlier chunks hold smaller colours, so a later one replaces it with fewer bits only. Everything returned is wave-uniform.
__device__ __forceinline__ void bigsi_take_ties(const BxTies<true> &ties, uint64_t read, uint32_t lane, uint64_t wi, uint64_t cand, uint32_t &n_tied, uint64_t &sig_t,
                                                uint32_t &sig_c)
{
    const uint32_t cnt = (uint32_t)__popcll(cand);
    uint32_t x = cnt;
    for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, o); if (lane >= o) x += y; }
    const uint32_t total = (uint32_t)__shfl((int)x, 63);
    uint64_t at = (uint64_t)n_tied + (x - cnt), bt = ~(uint64_t)0;
    uint32_t bc = UINT32_MAX;
    uint32_t *row = ties.tied + read * ties.max_ties;
    for (uint64_t m = cand; m; m &= m - 1) {
        const uint32_t col = (uint32_t)(wi * 64) + (uint32_t)__builtin_ctzll(m);
        if (at < ties.max_ties) row[at] = col;
        at++;
        const uint64_t t = ties.tc[col];
        if (t < bt) { bt = t; bc = col; }                // ascending colours: the first of equal t_c stays
    }
    for (uint32_t o = 32; o > 0; o >>= 1) {
        const uint64_t ot = shfl_xor64(bt, o);
        const uint32_t oc = (uint32_t)__shfl_xor((int)bc, (int)o);
        if (ot < bt || (ot == bt && oc < bc)) { bt = ot; bc = oc; }
    }
    if (bt < sig_t) { sig_t = readlane64(bt, 0); sig_c = wave_u32(bc); }
    n_tied = wave_u32(n_tied + total);
}
template <int HB, int BX_PLANES, bool LIST = false, bool TIES = false>
__global__ __launch_bounds__(256) void k_bigsi_query(const uint64_t *__restrict__ seq64, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                     const uint64_t *__restrict__ read_rec_off, uint64_t n_reads, uint32_t kq, uint32_t d, uint64_t B, uint32_t h,
                                                     const uint64_t *__restrict__ M, uint64_t W, uint64_t nc, uint32_t *__restrict__ out_n,
                                                     uint32_t *__restrict__ out_col, uint32_t *__restrict__ out_hits, uint32_t *__restrict__ dense,
                                                     const BxTies<TIES> ties)
{
    const uint32_t wave_u = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t read = (uint64_t)blockIdx.x * 4 + wave_u;
    if (read >= n_reads) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = kq_k(kq);
    const bool fwd_only = (kq & KQ_FWD) != 0;
    const uint64_t mask = kmer_mask(false, k);
    const uint64_t ra = LIST ? read : read_rec_off[read], rb = LIST ? read + 1 : read_rec_off[read + 1];
    // n: the occurrences used
    uint64_t n64 = 0, jb = 0;
    for (uint64_t r = ra; r < rb; r++) {
        const uint64_t len = rec_len[r] + (LIST ? k - 1 : 0);
        if (len < k) continue;
        const uint64_t cnt = len - k + 1, first = (jb + d - 1) / d * d;
        if (first < jb + cnt) n64 += (jb + cnt - 1 - first) / d + 1;
        jb += cnt;
    }
    const uint32_t n = (uint32_t)n64;
    if ((n >> BX_PLANES_SHORT) != 0 ? BX_PLANES == BX_PLANES_SHORT : BX_PLANES != BX_PLANES_SHORT) return;      // the other launch's read
    const uint32_t np = n ? 32 - (uint32_t)__builtin_clz(n) : 0;                    // planes that can hold a count <= n
    uint32_t Wp = 64;
    if (W < 64) { Wp = 1; while (Wp < W) Wp <<= 1; }
    const uint32_t G = 64 / Wp, grp = lane / Wp, wl = lane & (Wp - 1);
    uint32_t best_h = 0, best_c = 0;
    uint32_t n_tied = 0, sig_c = UINT32_MAX;                                        // TIES: wave-uniform, carried across the chunks
    uint64_t sig_t = ~(uint64_t)0;
    (void)best_c; (void)n_tied; (void)sig_c; (void)sig_t;
    for (uint64_t wc = 0; wc < W; wc += 64) {
        const uint64_t wi = wc + wl;
        const bool active = wi < W;
        uint64_t P[BX_PLANES];
#pragma unroll
        for (int p = 0; p < BX_PLANES; p++) P[p] = 0;
        jb = 0;
        for (uint64_t r = ra; r < rb; r++) {
            const uint64_t len = rec_len[r] + (LIST ? k - 1 : 0);
            if (len < k) continue;
            const uint64_t rs = rec_start[r], cnt = len - k + 1, first = (jb + d - 1) / d * d;
            if (first < jb + cnt) {
                const uint64_t nu = (jb + cnt - 1 - first) / d + 1, off0 = first - jb;
                for (uint64_t c0 = 0; c0 < nu; c0 += 64) {
                    uint64_t h1 = 0, st = 0;
                    if (c0 + lane < nu) {
                        const uint64_t at = rs + off0 + (c0 + lane) * d;
                        bigsi_hash(LIST ? seq64[at] : kmer_at(seq64, at, k, mask, fwd_only), h1, st);
                    }
                    const uint32_t m = (uint32_t)(nu - c0 < 64 ? nu - c0 : 64);
                    for (uint32_t t = 0; t < m; t += G) {
                        const uint32_t src = t + grp;
                        const bool kv = active && src < m;
                        uint64_t a1, as;
                        if (G == 1) { a1 = readlane64(h1, t); as = readlane64(st, t); }      // wave-uniform: the positions are scalar arithmetic
                        else { a1 = shfl64(h1, src & 63); as = shfl64(st, src & 63); }
                        uint64_t acc = kv ? ~(uint64_t)0 : 0;
                        for (uint32_t i0 = 0; i0 < h; i0 += HB) {
                            uint64_t w[HB];
#pragma unroll
                            for (int j = 0; j < HB; j++) {
                                const uint32_t i = i0 + j < h ? i0 + j : h - 1;
                                const uint64_t pos = bigsi_pos(a1, as, i, B);
                                w[j] = kv ? __builtin_nontemporal_load(M + pos * W + wi) : 0;
                            }
#pragma unroll
                            for (int j = 0; j < HB; j++) acc &= w[j];
                        }
                        // ripple add of the 1-bit vector into the planes; leaves as soon as no lane carries
                        ripple_add<0, BX_PLANES>(P, acc);
                    }
                }
            }
            jb += cnt;
        }
        // the k-mer groups of a narrow matrix hold partial counts of the same words: add them plane by plane (full adder), every lane ends with the sum
        for (uint32_t off = Wp; off < 64; off <<= 1) {
            uint64_t carry = 0;
#pragma unroll
            for (int p = 0; p < BX_PLANES; p++) {
                if ((uint32_t)p < np) {
                    const uint64_t a = P[p], b = shfl_xor64(a, off), x = a ^ b;
                    P[p] = x ^ carry;
                    carry = (a & b) | (carry & x);
                }
            }
        }
        // the largest count, from the top plane down: keep the colours that have the bit whenever any has it
        uint64_t cand = 0;
        if (grp == 0 && active) cand = wi * 64 + 64 <= nc ? ~(uint64_t)0 : (wi * 64 >= nc ? 0 : (((uint64_t)1 << (nc - wi * 64)) - 1));
        uint32_t bh = 0;
#pragma unroll
        for (int p = BX_PLANES - 1; p >= 0; p--) {
            if ((uint32_t)p < np) {
                const uint64_t tt = cand & P[p];
                if (__ballot(tt != 0) != 0) { cand = tt; bh |= 1u << p; }
            }
        }
        if constexpr (TIES) {
            // a chunk with more hits starts the list again, one with as many adds to it, one with fewer is left alone. Counted from cand, never from the
            // planes: on a narrow matrix every k-mer group holds the full sums, and cand is seeded in group 0 alone
            if (bh > best_h) { n_tied = 0; sig_t = ~(uint64_t)0; sig_c = UINT32_MAX; best_h = bh; }
            if (bh > 0 && bh == best_h) bigsi_take_ties(ties, read, lane, wi, cand, n_tied, sig_t, sig_c);
        } else if (bh > best_h) {          // (a later chunk holds larger colours: it only wins with more hits)
            const uint64_t bal = __ballot(cand != 0);
            const uint32_t fl = (uint32_t)__builtin_ctzll(bal);
            const uint32_t mine = cand ? (uint32_t)(wi * 64) + (uint32_t)__builtin_ctzll(cand) : 0u;
            best_c = (uint32_t)__shfl((int)mine, (int)fl);
            best_h = bh;
        }
        if (!TIES && dense && grp == 0 && active) {
            for (uint32_t b = 0; b < 64; b++) {
                const uint64_t col = wi * 64 + b;
                if (col >= nc) break;
                uint32_t cnt = 0;
#pragma unroll
                for (int p = 0; p < BX_PLANES; p++)
                    if ((uint32_t)p < np) cnt |= (uint32_t)((P[p] >> b) & 1u) << p;
                dense[read * nc + col] = cnt;
            }
        }
    }
    if constexpr (TIES) {
        // the slots behind the list are written here: the caller's buffer may hold anything
        uint32_t *row = ties.tied + read * ties.max_ties;
        for (uint64_t i = (uint64_t)(n_tied < ties.max_ties ? n_tied : ties.max_ties) + lane; i < ties.max_ties; i += 64) row[i] = UINT32_MAX;
        if (lane == 0) { out_n[read] = n; out_hits[read] = best_h; ties.n_tied[read] = n_tied; ties.sig[read] = sig_c; }
    } else {
        if (lane == 0) { out_n[read] = n; out_col[read] = best_c; out_hits[read] = best_h; }
    }
}

// ---- minimizer occurrences (SPEC 11.1) ---------------------------------------------------------------------------------------------------------
constexpr uint32_t MZ_TILE = GS_BIGSI_MINI_TILE;       // new windows per tile: lane 0 of a tile repeats the last window of the tile before, so a_{s-1} is one shuffle away
constexpr uint32_t MZ_POS = 64 + GS_BIGSI_KMAX;        // positions of a tile in LDS: 64 windows + the w - 1 <= 31 to their right (rounded up)
__host__ __device__ static inline uint64_t mz_tiles(uint64_t windows) { return (windows + MZ_TILE - 1) / MZ_TILE; }

// Per record the tiles in front of it inside its genome (rec_tpre), per genome its tiles and its windows (an upper bound of its occurrences; on a plain
// index the k-mer occurrences themselves). One wavefront per genome.
__global__ __launch_bounds__(256) void k_bigsi_tile_prefix(const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ genome_rec_off, uint64_t n_genomes,
                                                           uint32_t k, uint64_t *__restrict__ rec_tpre, uint64_t *__restrict__ gen_tiles,
                                                           uint64_t *__restrict__ gen_windows)
{
    const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1];
    unsigned long long run = 0, wins = 0;
    for (uint64_t base = r0; base < r1; base += 64) {
        const uint64_t r = base + lane;
        unsigned long long t = 0, wn = 0;
        if (r < r1) { const uint64_t l = rec_len[r]; if (l >= k) { wn = l - k + 1; t = (wn + MZ_TILE - 1) / MZ_TILE; } }
        unsigned long long x = t;
        for (uint32_t o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(x, o); if (lane >= o) x += y; }
        if (r < r1) rec_tpre[r] = run + x - t;
        run += __shfl(x, 63);
        for (int o = 32; o > 0; o >>= 1) wn += __shfl_down(wn, o);
        wins += __shfl(wn, 0);
    }
    if (lane == 0) { gen_tiles[g] = run; gen_windows[g] = wins; }
}
// off[r] = the windows of the reads in front of read r (an upper bound of their occurrences: where the read's list begins), off[n_reads] = all of them.
// ONE workgroup, lanes take contiguous stretches of reads (as k_scan_u32, gs_radix.hip)
__global__ __launch_bounds__(1024) void k_bigsi_window_prefix(const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ read_rec_off, uint64_t n_reads, uint32_t k,
                                                              uint64_t *__restrict__ off)
{
    __shared__ uint64_t part[1024];
    const uint64_t per = (n_reads + 1023) / 1024, b0 = (uint64_t)threadIdx.x * per, b = b0 < n_reads ? b0 : n_reads, e = b + per < n_reads ? b + per : n_reads;
    uint64_t s = 0;
    for (uint64_t r = b; r < e; r++)
        for (uint64_t q = read_rec_off[r]; q < read_rec_off[r + 1]; q++) { const uint64_t l = rec_len[q]; if (l >= k) s += l - k + 1; }
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t r = b; r < e; r++) {
        off[r] = run;
        for (uint64_t q = read_rec_off[r]; q < read_rec_off[r + 1]; q++) { const uint64_t l = rec_len[q]; if (l >= k) run += l - k + 1; }
    }
    if (threadIdx.x == 1023) off[n_reads] = part[1023];
}

struct MzLds { uint64_t h1[MZ_POS], st[MZ_POS], v[MZ_POS]; };
// Tile j of the record of L >= k bases that starts at base rs: lane l holds window s = j * MZ_TILE + l. true: the window's minimizer is an occurrence
// (window 0's, or another one than the window's before); v, h1, st: its value and hash. The workgroup is ONE wavefront; the answer of a window depends
// on the record alone - on the tile only in which lane computes it.
__device__ __forceinline__ bool mz_tile(const uint64_t *__restrict__ seq64, uint64_t rs, uint64_t L, uint64_t j, uint32_t k, uint32_t m, uint64_t mask_m, bool fwd_only,
                                        MzLds &lds, uint64_t &v, uint64_t &h1, uint64_t &st)
{
    const uint32_t lane = threadIdx.x, w = k - m + 1;
    const uint64_t p0 = j * MZ_TILE, np = L - m + 1;           // the tile's first position = its first window; the positions of the record
    for (uint32_t i = lane; i < 64 + w - 1; i += 64) {         // (i < 95 < MZ_POS)
        const uint64_t p = p0 + i;
        uint64_t vv = 0, a = ~(uint64_t)0, b = 0;
        if (p < np) { vv = kmer_at(seq64, rs + p, m, mask_m, fwd_only); bigsi_hash(vv, a, b); }     // (a position past the record: read by no valid window)
        lds.v[i] = vv; lds.h1[i] = a; lds.st[i] = b;
    }
    __syncthreads();
    const uint64_t s = p0 + lane;
    const uint32_t a = lane + minimizer_pick(lds.h1 + lane, w);                                      // lane + w - 1 <= 63 + w - 1: written above
    const uint32_t prev = (uint32_t)__shfl_up((int)a, 1);
    const bool emit = s + k <= L && (s == 0 || (lane > 0 && a != prev));
    v = lds.v[a]; h1 = lds.h1[a]; st = lds.st[a];
    __syncthreads();                                           // the next tile overwrites
    return emit;
}
struct MzArgs {
    const uint64_t *seq64, *rec_start, *rec_len, *group_rec_off;      // the packed layout; a group = a genome (build) or a read (query)
    const uint64_t *rec_tpre, *gen_tiles;                             // build: k_bigsi_tile_prefix
    uint32_t kq, m;
    uint32_t *bm; uint64_t pitch, B; uint32_t h; unsigned long long *nk;                           // MZ_BITS: the block's bitmaps, nk_c of its colours
    uint64_t *vals; unsigned long long *cursor; uint64_t cap;                                      // MZ_LIST: one colour's value list
    const uint64_t *voff; uint64_t *vcnt;                                                          // MZ_QUERY: where each read's list begins; its entries
};
enum { MZ_BITS = 0, MZ_LIST = 1, MZ_QUERY = 2 };
// MZ_BITS / MZ_LIST: grid x = wavefronts that share a genome's tiles, y = genomes. MZ_QUERY: one wavefront per read, its records and tiles in order.
template <int MODE> __global__ __launch_bounds__(64) void k_bigsi_minimizers(const MzArgs a)
{
    __shared__ MzLds lds;
    const uint32_t lane = threadIdx.x, k = kq_k(a.kq), m = a.m;
    const bool fwd_only = (a.kq & KQ_FWD) != 0;
    const uint64_t mask_m = kmer_mask(false, m), lt = ((uint64_t)1 << lane) - 1;
    uint64_t v, h1, st;
    if constexpr (MODE == MZ_QUERY) {
        const uint64_t read = blockIdx.x, base = a.voff[read], end = a.voff[read + 1];
        uint64_t cnt = 0;
        for (uint64_t r = a.group_rec_off[read]; r < a.group_rec_off[read + 1]; r++) {
            const uint64_t L = a.rec_len[r];
            if (L < k) continue;
            const uint64_t rs = a.rec_start[r], nt = mz_tiles(L - k + 1);
            for (uint64_t j = 0; j < nt; j++) {
                const bool emit = mz_tile(a.seq64, rs, L, j, k, m, mask_m, fwd_only, lds, v, h1, st);
                const uint64_t bal = __ballot(emit);
                const uint64_t at = base + cnt + (uint64_t)__popcll(bal & lt);
                if (emit && at < end) a.vals[at] = v;            // (occurrences never exceed windows: `end` is never reached)
                cnt += (uint64_t)__popcll(bal);
            }
        }
        if (lane == 0) a.vcnt[read] = cnt;
    } else {
        const uint64_t g = blockIdx.y, r0 = a.group_rec_off[g], r1 = a.group_rec_off[g + 1], nt = a.gen_tiles[g];
        BitEmit be{a.bm + g * a.pitch, a.B, a.h};
        unsigned long long fed = 0;
        for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
            uint64_t lo = r0, hi = r1;                           // the record that owns tile t: the last r with rec_tpre[r] <= t
            while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.rec_tpre[mid] <= t) lo = mid; else hi = mid; }
            const bool emit = mz_tile(a.seq64, a.rec_start[lo], a.rec_len[lo], t - a.rec_tpre[lo], k, m, mask_m, fwd_only, lds, v, h1, st);
            const uint64_t bal = __ballot(emit);
            if (bal == 0) continue;
            if constexpr (MODE == MZ_BITS) {
                if (emit) be.bits(h1, st);
                fed += (unsigned long long)__popcll(bal);
            } else {
                unsigned long long at = 0;
                if (lane == 0) at = atomicAdd(a.cursor, (unsigned long long)__popcll(bal));
                at = shfl64(at, 0) + (unsigned long long)__popcll(bal & lt);
                if (emit && at < a.cap) a.vals[at] = v;
            }
        }
        if (MODE == MZ_BITS && lane == 0 && fed) atomicAdd(&a.nk[g], fed);
    }
}
// the runs of one colour's sorted value list that the coverage filter keeps: their bits into the colour's bitmap, their lengths into nk_c
__global__ __launch_bounds__(256) void k_bigsi_fill_runs(const uint64_t *__restrict__ uniq, const uint32_t *__restrict__ len, const uint32_t *__restrict__ nruns,
                                                         uint32_t min_count, uint32_t *__restrict__ bm, uint64_t B, uint32_t h, unsigned long long *__restrict__ nk)
{
    const uint32_t nr = *nruns;
    BitEmit be{bm, B, h};
    unsigned long long fed = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < nr; r += (uint64_t)gridDim.x * 256) {
        const uint32_t l = len[r];
        if (l >= min_count) { be(uniq[r], 0, 0); fed += l; }
    }
    for (int o = 32; o > 0; o >>= 1) fed += __shfl_down(fed, o);
    if ((threadIdx.x & 63) == 0 && fed) atomicAdd(nk, fed);
}

__global__ void k_bigsi_classify(uint64_t n_reads, const uint32_t *__restrict__ nk, const uint32_t *__restrict__ col, const uint32_t *__restrict__ hits,
                                 const uint64_t *__restrict__ tc, uint64_t nc, uint64_t B, uint32_t h, double fp, double *__restrict__ tail,
                                 uint8_t *__restrict__ accept)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t c = col[r], x0 = hits[r];
    const double t = bigsi_tail(c < nc ? tc[c] : 0, B, h, nk[r], x0);
    tail[r] = t;
    accept[r] = (x0 > 0 && t < fp) ? 1 : 0;
}

// SPEC 11.2: the tail of the most significant tied colour and the verdict of the read
static_assert(GS_BIGSI_TOO_SHORT == 0 && GS_BIGSI_NO_HITS == 1 && GS_BIGSI_NOT_SIGNIFICANT == 2 && GS_BIGSI_UNIQUE == 3 && GS_BIGSI_TIED == 4, "bigsi_verdict (gs_spec.hpp)");
__global__ void k_bigsi_verdict(uint64_t n_reads, const uint32_t *__restrict__ nk, const uint32_t *__restrict__ hits, const uint32_t *__restrict__ n_tied,
                                const uint32_t *__restrict__ sig, const uint64_t *__restrict__ tc, uint64_t nc, uint64_t B, uint32_t h, double fp,
                                double *__restrict__ tail, uint8_t *__restrict__ verdict)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t c = sig[r], x0 = hits[r], n = nk[r];
    const double t = x0 > 0 ? bigsi_tail(c < nc ? tc[c] : 0, B, h, n, x0) : 1.0;
    tail[r] = t;
    verdict[r] = bigsi_verdict(n, x0, n_tied[r], t, fp);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
static inline int base_code(uint8_t ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
    }
}
// the segments of text bytes [b, e): f(begin offset, bases) for every maximal run of valid bases; line breaks are skipped, and `code` receives every valid base
template <class Seg, class Base>
static void split_text(const uint8_t *text, const uint8_t *qual, uint64_t b, uint64_t e, uint32_t min_phred, const Seg &seg, const Base &base)
{
    uint64_t begin = 0, len = 0;
    for (uint64_t i = b; i < e; i++) {
        const uint8_t ch = text[i];
        if (ch == '\n' || ch == '\r') continue;
        const int code = base_code(ch);
        const bool ok = code >= 0 && (!qual || (int)qual[i] - 33 >= (int)min_phred);
        if (ok) { if (len == 0) begin = i; len++; base(code); }
        else if (len) { seg(begin, len); len = 0; }
    }
    if (len) seg(begin, len);
}
// host text -> packed segments (each at least k bases) on the device, grouped as the caller grouped its records
struct Staged {
    PoolBuf seq, rs, rl, go;
    uint64_t seq_bytes = 0, n_seg = 0;
    explicit Staged(gs_ctx *c) : seq(c, SL_BIGSI_SEQ), rs(c, SL_BIGSI_REC_START), rl(c, SL_BIGSI_REC_LEN), go(c, SL_BIGSI_GROUP_OFF) {}
};
static int stage_text(gs_ctx *c, uint32_t k, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end,
                      uint64_t n_rec, const uint64_t *group_off, uint64_t n_groups, Staged &s)
{
    GS_REQUIRE(group_off[n_groups] <= n_rec, GS_ERR_INVALID, "the record offsets exceed n_rec");
    const uint8_t *tx = (const uint8_t *)text, *ql = (const uint8_t *)qual;
    std::vector<uint8_t> packed;
    std::vector<uint64_t> start, len, goff(n_groups + 1);
    uint64_t nb = 0;                       // bases packed so far
    for (uint64_t g = 0; g < n_groups; g++) {
        goff[g] = start.size();
        GS_REQUIRE(group_off[g] <= group_off[g + 1], GS_ERR_INVALID, "the record offsets do not ascend");
        for (uint64_t r = group_off[g]; r < group_off[g + 1]; r++) {
            GS_REQUIRE(rec_begin[r] <= rec_end[r], GS_ERR_INVALID, "record %llu ends before it begins", (unsigned long long)r);
            uint64_t seg0 = nb;
            split_text(tx, ql, rec_begin[r], rec_end[r], min_phred,
                       [&](uint64_t, uint64_t l) {
                           if (l >= k) { start.push_back(seg0); len.push_back(l); seg0 = nb; }
                           else { nb = seg0; packed.resize((nb + 3) / 4); if (nb & 3) packed.back() &= (uint8_t)(0xFF00u >> (2 * (nb & 3))); }   // too short: take it back
                       },
                       [&](int code) {
                           if ((nb & 3) == 0) packed.push_back(0);
                           packed[nb >> 2] |= (uint8_t)(code << (6 - 2 * (nb & 3)));
                           nb++;
                       });
        }
    }
    goff[n_groups] = start.size();
    s.n_seg = start.size();
    s.seq_bytes = round_up(packed.size(), 8) + 8;
    packed.resize(s.seq_bytes, 0);
    int rc;
    if ((rc = s.seq.alloc(s.seq_bytes)) || (rc = s.rs.alloc(8 * (s.n_seg + 1))) || (rc = s.rl.alloc(8 * (s.n_seg + 1))) || (rc = s.go.alloc(8 * (n_groups + 1)))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(s.seq.p, packed.data(), s.seq_bytes, hipMemcpyHostToDevice, c->stream));
    if (s.n_seg) {
        GS_HIP_CHECK(hipMemcpyAsync(s.rs.p, start.data(), 8 * s.n_seg, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(s.rl.p, len.data(), 8 * s.n_seg, hipMemcpyHostToDevice, c->stream));
    }
    GS_HIP_CHECK(hipMemcpyAsync(s.go.p, goff.data(), 8 * (n_groups + 1), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));      // the vectors go out of scope
    return GS_OK;
}

static int bigsi_alloc(gs_ctx *c, const gs_bigsi_params *prm, uint64_t cap, gs_bigsi **out)
{
    int rc = gs_bigsi_check_params(prm);
    if (rc) return rc;
    GS_REQUIRE(c && out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(cap >= 1 && cap < ((uint64_t)1 << 32), GS_ERR_INVALID, "colour capacity %llu out of range", (unsigned long long)cap);
    GS_CTX_LOCK(c);
    gs_bigsi *bx = new gs_bigsi();
    bx->c = c; bx->prm = *prm; bx->cap = cap; bx->W = (cap + 63) / 64;
    const uint64_t words = prm->bloom_size * bx->W;
    if (words >= ((uint64_t)1 << 58) || (rc = bx->M.alloc(words * 8)) || (rc = bx->tc.alloc(cap * 8)) || (rc = bx->nk.alloc(cap * 8))) {
        if (!rc) { set_error("a matrix of %llu rows x %llu words does not fit", (unsigned long long)prm->bloom_size, (unsigned long long)bx->W); rc = GS_ERR_HIP; }
        delete bx;
        return rc;
    }
    hipError_t e = hipMemsetAsync(bx->M.p, 0, words * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(bx->tc.p, 0, cap * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(bx->nk.p, 0, cap * 8, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { set_error("zeroing the matrix failed: %s", hipGetErrorString(e)); delete bx; return GS_ERR_HIP; }
    *out = bx;
    return GS_OK;
}

static int write_all(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n ? 0 : -1; }
static int read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n ? 0 : -1; }

}  // namespace gs

extern "C" {

int gs_bigsi_create(gs_ctx *c, const gs_bigsi_params *prm, uint64_t colour_capacity, gs_bigsi **out) { return gs::bigsi_alloc(c, prm, colour_capacity, out); }

int gs_bigsi_create_mini(gs_ctx *c, const gs_bigsi_params *prm, uint32_t minimizer_len, uint64_t colour_capacity, gs_bigsi **out)
{
    int rc = gs_bigsi_check_params(prm);
    if (rc) return rc;
    GS_REQUIRE(minimizer_len >= 1 && minimizer_len < prm->k, GS_ERR_INVALID, "bigsig: minimizer length %u outside 1..k-1 (k = %u)", minimizer_len, prm->k);
    if ((rc = gs::bigsi_alloc(c, prm, colour_capacity, out))) return rc;
    (*out)->m = minimizer_len;
    return GS_OK;
}

uint32_t gs_bigsi_minimizer_len(gs_bigsi *bx) { return bx ? bx->m : 0; }

void gs_bigsi_free(gs_bigsi *bx)
{
    if (!bx) return;
    { GS_CTX_LOCK(bx->c); (void)hipStreamSynchronize(bx->c->stream); }
    delete bx;
}

int gs_bigsi_info(gs_bigsi *bx, gs_bigsi_desc *out)
{
    GS_REQUIRE(bx && out, GS_ERR_INVALID, "null argument");
    out->prm = bx->prm; out->n_colours = bx->n; out->colour_capacity = bx->cap; out->row_words = bx->W;
    return GS_OK;
}

// One colour of the block under a coverage filter (SPEC 11.1): its occurrence values -> sorted -> runs -> the runs of at least min_count into its bitmap.
// `windows`: the colour's windows (host copy) - the k-mer occurrences of a plain index, an upper bound of a minimizer index's.
static int bigsi_filter_colour(gs_bigsi *bx, const void *seq, const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *rec_upre, const uint64_t *rec_tpre,
                               const uint64_t *genome_rec_off, const uint64_t *gen_units, const uint64_t *gen_tiles, uint64_t windows, uint32_t min_count,
                               uint32_t *bm, unsigned long long *nk)
{
    using namespace gs;
    gs_ctx *c = bx->c;
    if (windows == 0) return GS_OK;
    const bool mini = bx->m != 0;
    const uint64_t B = bx->prm.bloom_size;
    GS_REQUIRE(mini || windows < ((uint64_t)1 << 32), GS_ERR_UNSUPPORTED,
               "bigsig: %llu occurrences in one colour; the coverage filter sorts fewer than 2^32 per colour", (unsigned long long)windows);
    PoolBuf vals(c, SL_BIGSI_LIST_VALS), alt(c, SL_BIGSI_LIST_ALT), len(c, SL_BIGSI_LIST_LEN), pos(c, SL_BIGSI_LIST_POS), radix(c, SL_BIGSI_LIST_RADIX),
        ctr(c, SL_BIGSI_LIST_CTR);
    int rc;
    if ((rc = vals.alloc(8 * windows)) || (rc = ctr.alloc(16))) return rc;
    unsigned long long *cursor = ctr.as<unsigned long long>();
    uint32_t *nruns = ctr.as<uint32_t>() + 2;
    GS_HIP_CHECK(hipMemsetAsync(ctr.p, 0, 16, c->stream));
    const uint64_t nt = mz_tiles(windows) + 1;                  // at least the tiles of the colour when it is one record; more records: more, shorter tiles
    const uint32_t parts = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(nt / 4, 1), (uint64_t)c->n_cu * 32);
    // (with gs_ctx_profile on, the three steps are timed as families: emit = FAM_SKETCH, sort and run lengths = FAM_HAMMING, fill = FAM_INSERT)
    if (mini) {
        MzArgs a{};
        a.seq64 = (const uint64_t *)seq; a.rec_start = rec_start; a.rec_len = rec_len; a.group_rec_off = genome_rec_off; a.rec_tpre = rec_tpre; a.gen_tiles = gen_tiles;
        a.kq = bigsi_kq(bx->prm); a.m = bx->m; a.vals = vals.as<uint64_t>(); a.cursor = cursor; a.cap = windows;
        ProfScope ps(c, FAM_SKETCH);
        hipLaunchKernelGGL(k_bigsi_minimizers<MZ_LIST>, dim3(parts, 1), dim3(64), 0, c->stream, a);
    } else {
        ProfScope ps(c, FAM_SKETCH);
        const uint32_t lp = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(windows / 32 / SK_THREADS, 1), (uint64_t)c->n_cu * 4);
        hipLaunchKernelGGL(k_bigsi_list, dim3(lp), dim3(SK_THREADS), 0, c->stream, (const uint8_t *)seq, rec_start, rec_len, rec_upre, genome_rec_off, gen_units,
                           bigsi_kq(bx->prm), vals.as<uint64_t>(), cursor, windows);
    }
    GS_HIP_CHECK(hipGetLastError());
    unsigned long long n = 0;
    GS_HIP_CHECK(hipMemcpyAsync(&n, cursor, 8, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    GS_REQUIRE(n <= windows, GS_ERR_STATE, "bigsig: %llu occurrences listed for %llu windows", n, (unsigned long long)windows);
    GS_REQUIRE(n < ((uint64_t)1 << 32), GS_ERR_UNSUPPORTED, "bigsig: %llu occurrences in one colour; the coverage filter sorts fewer than 2^32 per colour", n);
    if (n == 0) return GS_OK;
    if ((rc = alt.alloc(8 * n)) || (rc = len.alloc(4 * n)) || (rc = pos.alloc(4 * n)) || (rc = radix.alloc(radix_scratch_bytes(n)))) return rc;
    uint64_t *sorted = nullptr, *uniq = nullptr;
    {
        ProfScope ps(c, FAM_HAMMING);
        if ((rc = radix_sort_u64(c, vals.as<uint64_t>(), alt.as<uint64_t>(), n, (int)(2 * (mini ? bx->m : bx->prm.k)), radix.p, &sorted))) return rc;
        uniq = sorted == vals.as<uint64_t>() ? alt.as<uint64_t>() : vals.as<uint64_t>();
        if ((rc = run_length_encode_u64(c, sorted, n, uniq, len.as<uint32_t>(), nruns, pos.as<uint32_t>(), radix.p))) return rc;
    }
    ProfScope ps(c, FAM_INSERT);
    hipLaunchKernelGGL(k_bigsi_fill_runs, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->n_cu * 8)), dim3(256), 0, c->stream, uniq, len.as<uint32_t>(), nruns,
                       min_count, bm, B, bx->prm.num_hash, nk);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

// min_count <= 1: no filter
static int bigsi_add_dev(gs_bigsi *bx, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                         const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t min_count)
{
    using namespace gs;
    GS_REQUIRE(bx && (n_genomes == 0 || (seq && rec_start && rec_len && genome_rec_off)), GS_ERR_INVALID, "null argument");
    if (n_genomes == 0) return GS_OK;
    GS_REQUIRE(bx->n + n_genomes <= bx->cap, GS_ERR_STATE, "bigsig: %llu more genomes do not fit the colour capacity %llu (%llu used)",
               (unsigned long long)n_genomes, (unsigned long long)bx->cap, (unsigned long long)bx->n);
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    const uint64_t B = bx->prm.bloom_size, pitch = bitmap_pitch(B);
    const uint32_t kq = bigsi_kq(bx->prm);
    GS_REQUIRE((B + TR_ROWS - 1) / TR_ROWS < ((uint64_t)1 << 31), GS_ERR_UNSUPPORTED, "bigsig: bloom_size too large for the transpose grid");
    const bool mini = bx->m != 0, filt = min_count >= 2;
    PoolBuf upre(c, SL_BIGSI_REC_UNITS), gunits(c, SL_BIGSI_GENOME_UNITS), bmb(c, SL_BIGSI_BITMAP);
    PoolBuf tpre(c, SL_BIGSI_REC_TILES), gtiles(c, SL_BIGSI_GENOME_TILES), gwin(c, SL_BIGSI_GENOME_WINDOWS);
    int rc;
    if (!mini) {
        if ((rc = upre.alloc(8 * (n_rec + 1))) || (rc = gunits.alloc(8 * n_genomes))) return rc;
        hipLaunchKernelGGL(k_unit_prefix, dim3((uint32_t)((n_genomes + 3) / 4)), dim3(256), 0, c->stream, rec_start, rec_len, genome_rec_off, n_genomes, bx->prm.k,
                           upre.as<uint64_t>(), gunits.as<uint64_t>());
        GS_HIP_CHECK(hipGetLastError());
    }
    std::vector<uint64_t> windows;                                                  // per genome, on the host: the filter sizes each colour's list by it
    if (mini || filt) {
        if ((rc = tpre.alloc(8 * (n_rec + 1))) || (rc = gtiles.alloc(8 * n_genomes)) || (rc = gwin.alloc(8 * n_genomes))) return rc;
        hipLaunchKernelGGL(k_bigsi_tile_prefix, dim3((uint32_t)((n_genomes + 3) / 4)), dim3(256), 0, c->stream, rec_len, genome_rec_off, n_genomes, bx->prm.k,
                           tpre.as<uint64_t>(), gtiles.as<uint64_t>(), gwin.as<uint64_t>());
        GS_HIP_CHECK(hipGetLastError());
        if (filt) {
            windows.resize(n_genomes);
            GS_HIP_CHECK(hipMemcpyAsync(windows.data(), gwin.p, 8 * n_genomes, hipMemcpyDeviceToHost, c->stream));
            GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        }
    }
    // colours of a block: whole words of 64 up to BX_BLOCK, fewer when the bitmaps (bloom_size bits each) would take more than a quarter of the free memory
    size_t fr = 0, tot = 0;
    GS_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    uint64_t fit = std::max<uint64_t>((fr / 4 + bmb.bytes) / (pitch * 4), 1);
    {   // what the slot already holds counts as free
        ScratchPool *pool = (ScratchPool *)c->scratch_pool;
        if (pool) fit = std::max<uint64_t>(fit, pool->b[SL_BIGSI_BITMAP].bytes / (pitch * 4));
    }
    const uint64_t blk = fit >= BX_BLOCK ? BX_BLOCK : (fit >= 64 ? fit / 64 * 64 : fit);
    const uint64_t avg_units = seq_bytes / 8 / n_genomes + 1;
    c->last_sketch[0] = 0; c->last_sketch[1] = 0; c->last_sketch[2] = 0; c->last_sketch[3] = 0;
    for (uint64_t g0 = 0; g0 < n_genomes;) {
        const uint64_t c0 = bx->n + g0;                                             // first colour of the block
        const uint64_t cend = blk >= 64 ? c0 / 64 * 64 + blk : std::min(c0 + blk, c0 / 64 * 64 + 64);
        const uint64_t ng = std::min(n_genomes - g0, cend - c0);
        if ((rc = bmb.alloc(ng * pitch * 4))) return rc;
        GS_HIP_CHECK(hipMemsetAsync(bmb.p, 0, ng * pitch * 4, c->stream));
        // few genomes: several workgroups each, as the sketchers do (min_geom, gs_sketch.hip)
        uint32_t parts = (uint32_t)((2 * (uint64_t)c->n_cu + ng - 1) / ng);
        const uint64_t maxp = (avg_units + SK_THREADS - 1) / SK_THREADS;
        if (parts > maxp) parts = (uint32_t)maxp;
        if (parts < 1) parts = 1;
        c->last_sketch[2] = parts; c->last_sketch[3]++;
        unsigned long long *nk0 = bx->nk.as<unsigned long long>() + c0;
        if (!mini && !filt) {
            hipLaunchKernelGGL(k_bigsi_fill, dim3(parts, (uint32_t)ng), dim3(SK_THREADS), 0, c->stream, (const uint8_t *)seq, rec_start, rec_len, upre.as<uint64_t>(),
                               genome_rec_off + g0, gunits.as<uint64_t>() + g0, kq, B, bx->prm.num_hash, bmb.as<uint32_t>(), pitch);
            GS_HIP_CHECK(hipGetLastError());
        } else {
            GS_HIP_CHECK(hipMemsetAsync(nk0, 0, 8 * ng, c->stream));                 // counted by the kernels below, not from the record lengths
            if (!filt) {
                // a wavefront per MZ_TILE windows; as many as the tiles of an average genome, and no more than fill the device eight times over
                const uint64_t avg_tiles = seq_bytes * 4 / MZ_TILE / n_genomes + 1;
                const uint32_t mp = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((8 * 32 * (uint64_t)c->n_cu + ng - 1) / ng, 1), avg_tiles);
                c->last_sketch[2] = mp;
                MzArgs a{};
                a.seq64 = (const uint64_t *)seq; a.rec_start = rec_start; a.rec_len = rec_len; a.group_rec_off = genome_rec_off + g0; a.rec_tpre = tpre.as<uint64_t>();
                a.gen_tiles = gtiles.as<uint64_t>() + g0; a.kq = kq; a.m = bx->m; a.bm = bmb.as<uint32_t>(); a.pitch = pitch; a.B = B; a.h = bx->prm.num_hash; a.nk = nk0;
                hipLaunchKernelGGL(k_bigsi_minimizers<MZ_BITS>, dim3(mp, (uint32_t)ng), dim3(64), 0, c->stream, a);
                GS_HIP_CHECK(hipGetLastError());
            } else {
                for (uint64_t g = 0; g < ng; g++)                                   // filtered colours are read sets, few and large: one at a time
                    if ((rc = bigsi_filter_colour(bx, seq, rec_start, rec_len, upre.as<uint64_t>(), tpre.as<uint64_t>(), genome_rec_off + g0 + g,
                                                  mini ? nullptr : gunits.as<uint64_t>() + g0 + g, gtiles.as<uint64_t>() + g0 + g, windows[g0 + g], min_count,
                                                  bmb.as<uint32_t>() + g * pitch, nk0 + g)))
                        return rc;
            }
        }
        const uint32_t slices = (uint32_t)std::min<uint64_t>((pitch + 256 * 16 - 1) / (256 * 16), 1024);
        hipLaunchKernelGGL(k_bigsi_popcount, dim3(slices, (uint32_t)ng), dim3(256), 0, c->stream, bmb.as<uint32_t>(), pitch, rec_len, genome_rec_off + g0, bx->prm.k,
                           bx->tc.as<unsigned long long>() + c0, (mini || filt) ? (unsigned long long *)nullptr : nk0);
        GS_HIP_CHECK(hipGetLastError());
        const uint64_t w0 = c0 / 64;
        const uint32_t cshift = (uint32_t)(c0 & 63), nw = (uint32_t)((cshift + ng + 63) / 64);
        hipLaunchKernelGGL(k_bigsi_transpose, dim3((uint32_t)((B + TR_ROWS - 1) / TR_ROWS)), dim3(256), 0, c->stream, bmb.as<uint32_t>(), pitch, (uint32_t)ng, cshift, B,
                           bx->M.as<uint64_t>(), bx->W, w0, nw, cshift != 0 ? 1 : 0);
        GS_HIP_CHECK(hipGetLastError());
        g0 += ng;
    }
    bx->n += n_genomes;
    if (!bx->names.empty()) bx->names.resize(bx->n);
    return GS_OK;
}

int gs_bigsi_add_batch_dev(gs_bigsi *bx, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                           const uint64_t *genome_rec_off, uint64_t n_genomes)
{
    return bigsi_add_dev(bx, seq, seq_bytes, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, 1);
}
int gs_bigsi_add_batch_min_count_dev(gs_bigsi *bx, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                                     const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t min_count)
{
    return bigsi_add_dev(bx, seq, seq_bytes, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, min_count);
}

int gs_bigsi_add_batch(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end, uint64_t n_rec,
                       const uint64_t *genome_rec_off, uint64_t n_genomes)
{
    return gs_bigsi_add_batch_min_count(bx, text, qual, min_phred, rec_begin, rec_end, n_rec, genome_rec_off, n_genomes, 1);
}
int gs_bigsi_add_batch_min_count(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end, uint64_t n_rec,
                                 const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t min_count)
{
    using namespace gs;
    GS_REQUIRE(bx && (n_genomes == 0 || ((text || n_rec == 0) && genome_rec_off && (n_rec == 0 || (rec_begin && rec_end)))), GS_ERR_INVALID, "null argument");
    if (n_genomes == 0) return GS_OK;
    GS_REQUIRE(bx->n + n_genomes <= bx->cap, GS_ERR_STATE, "bigsig: %llu more genomes do not fit the colour capacity %llu (%llu used)",
               (unsigned long long)n_genomes, (unsigned long long)bx->cap, (unsigned long long)bx->n);
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    Staged s(c);
    int rc = stage_text(c, bx->prm.k, text, qual, min_phred, rec_begin, rec_end, n_rec, genome_rec_off, n_genomes, s);
    if (rc) return rc;
    rc = bigsi_add_dev(bx, s.seq.p, s.seq_bytes, s.rs.as<uint64_t>(), s.rl.as<uint64_t>(), s.n_seg, s.go.as<uint64_t>(), n_genomes, min_count);
    if (rc) return rc;
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_bigsi_bits_set(gs_bigsi *bx, uint64_t first, uint64_t n, uint64_t *t_out, uint64_t *nk_out)
{
    GS_REQUIRE(bx, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(first + n <= bx->n, GS_ERR_INVALID, "colours [%llu, %llu) exceed the %llu added", (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)bx->n);
    if (n == 0) return GS_OK;
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    if (t_out) GS_HIP_CHECK(hipMemcpyAsync(t_out, bx->tc.as<uint64_t>() + first, 8 * n, hipMemcpyDeviceToHost, c->stream));
    if (nk_out) GS_HIP_CHECK(hipMemcpyAsync(nk_out, bx->nk.as<uint64_t>() + first, 8 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_bigsi_rows(gs_bigsi *bx, const uint64_t *rows, uint64_t n, uint64_t *words_out)
{
    using namespace gs;
    GS_REQUIRE(bx && (n == 0 || (rows && words_out)), GS_ERR_INVALID, "null argument");
    if (n == 0) return GS_OK;
    for (uint64_t i = 0; i < n; i++) GS_REQUIRE(rows[i] < bx->prm.bloom_size, GS_ERR_INVALID, "row %llu outside the matrix", (unsigned long long)rows[i]);
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    PoolBuf dl(c, SL_BIGSI_ROW_LIST), dw(c, SL_BIGSI_ROW_WORDS);
    int rc;
    if ((rc = dl.alloc(8 * n)) || (rc = dw.alloc(8 * n * bx->W))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dl.p, rows, 8 * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bigsi_gather_rows, dim3((uint32_t)std::min<uint64_t>((n * bx->W + 255) / 256, 65536)), dim3(256), 0, c->stream, bx->M.as<uint64_t>(), bx->W,
                       dl.as<uint64_t>(), n, dw.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    GS_HIP_CHECK(hipMemcpyAsync(words_out, dw.p, 8 * n * bx->W, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

extern "C++" {
// the launches of both forms of the query (arguments checked by the callers): TIES = false writes best_colour (and counts), TIES = true what `ties` names
template <bool TIES>
static int bigsi_query_launch(gs_bigsi *bx, const void *seq, const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *read_rec_off, uint64_t n_reads,
                              uint32_t down_sample, uint32_t *n_kmers, uint32_t *best_colour, uint32_t *best_hits, uint32_t *counts, const gs::BxTies<TIES> ties)
{
    using namespace gs;
    GS_REQUIRE(n_reads < ((uint64_t)1 << 33), GS_ERR_INVALID, "too many reads in one batch");
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    const uint32_t h = bx->prm.num_hash, hb = h < 4 ? h : 4;
    const dim3 grid((uint32_t)((n_reads + 3) / 4)), block(256);
    if (bx->m) {
        // a minimizer index: the ordered occurrence list of every read first (where a list begins: the windows in front of it), then the list form
        GS_REQUIRE(n_reads < ((uint64_t)1 << 31), GS_ERR_INVALID, "too many reads in one batch");
        PoolBuf qoff(c, SL_BIGSI_Q_OFF), qcnt(c, SL_BIGSI_Q_CNT), qv(c, SL_BIGSI_Q_VALS);
        int rc;
        if ((rc = qoff.alloc(8 * (n_reads + 1))) || (rc = qcnt.alloc(8 * n_reads))) return rc;
        hipLaunchKernelGGL(k_bigsi_window_prefix, dim3(1), dim3(1024), 0, c->stream, rec_len, read_rec_off, n_reads, bx->prm.k, qoff.as<uint64_t>());
        GS_HIP_CHECK(hipGetLastError());
        uint64_t total = 0;
        GS_HIP_CHECK(hipMemcpyAsync(&total, qoff.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));                               // the lists are sized by it
        if ((rc = qv.alloc(8 * std::max<uint64_t>(total, 1)))) return rc;
        MzArgs a{};
        a.seq64 = (const uint64_t *)seq; a.rec_start = rec_start; a.rec_len = rec_len; a.group_rec_off = read_rec_off; a.kq = bigsi_kq(bx->prm); a.m = bx->m;
        a.vals = qv.as<uint64_t>(); a.voff = qoff.as<uint64_t>(); a.vcnt = qcnt.as<uint64_t>();
        {   // (with gs_ctx_profile on: the pre-pass is FAM_SKETCH, the look-ups FAM_SEARCH)
            ProfScope ps(c, FAM_SKETCH);
            hipLaunchKernelGGL(k_bigsi_minimizers<MZ_QUERY>, dim3((uint32_t)n_reads), dim3(64), 0, c->stream, a);
        }
        GS_HIP_CHECK(hipGetLastError());
        ProfScope ps(c, FAM_SEARCH);
#define GS_BX_LAUNCH_LIST(HB)                                                                                                                                \
    do {                                                                                                                                                     \
        hipLaunchKernelGGL((k_bigsi_query<HB, BX_PLANES_SHORT, true, TIES>), grid, block, 0, c->stream, qv.as<uint64_t>(), qoff.as<uint64_t>(), qcnt.as<uint64_t>(), \
                           (const uint64_t *)nullptr, n_reads, bigsi_kq(bx->prm), down_sample, bx->prm.bloom_size, h, bx->M.as<uint64_t>(), bx->W, bx->n,     \
                           n_kmers, best_colour, best_hits, counts, ties);                                                                                         \
        hipLaunchKernelGGL((k_bigsi_query<HB, BX_PLANES_LONG, true, TIES>), grid, block, 0, c->stream, qv.as<uint64_t>(), qoff.as<uint64_t>(), qcnt.as<uint64_t>(),  \
                           (const uint64_t *)nullptr, n_reads, bigsi_kq(bx->prm), down_sample, bx->prm.bloom_size, h, bx->M.as<uint64_t>(), bx->W, bx->n,     \
                           n_kmers, best_colour, best_hits, counts, ties);                                                                                         \
    } while (0)
        if (hb == 1) GS_BX_LAUNCH_LIST(1);
        else if (hb == 2) GS_BX_LAUNCH_LIST(2);
        else if (hb == 3) GS_BX_LAUNCH_LIST(3);
        else GS_BX_LAUNCH_LIST(4);
#undef GS_BX_LAUNCH_LIST
        GS_HIP_CHECK(hipGetLastError());
        return GS_OK;
    }
#define GS_BX_LAUNCH(HB)                                                                                                                                     \
    do {                                                                                                                                                     \
        hipLaunchKernelGGL((k_bigsi_query<HB, BX_PLANES_SHORT, false, TIES>), grid, block, 0, c->stream, (const uint64_t *)seq, rec_start, rec_len, read_rec_off, n_reads, \
                           bigsi_kq(bx->prm), down_sample, bx->prm.bloom_size, h, bx->M.as<uint64_t>(), bx->W, bx->n, n_kmers, best_colour, best_hits, counts, ties); \
        hipLaunchKernelGGL((k_bigsi_query<HB, BX_PLANES_LONG, false, TIES>), grid, block, 0, c->stream, (const uint64_t *)seq, rec_start, rec_len, read_rec_off, n_reads, \
                           bigsi_kq(bx->prm), down_sample, bx->prm.bloom_size, h, bx->M.as<uint64_t>(), bx->W, bx->n, n_kmers, best_colour, best_hits, counts, ties); \
    } while (0)
    if (hb == 1) GS_BX_LAUNCH(1);
    else if (hb == 2) GS_BX_LAUNCH(2);
    else if (hb == 3) GS_BX_LAUNCH(3);
    else GS_BX_LAUNCH(4);
#undef GS_BX_LAUNCH
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}
}  // extern "C++"

int gs_bigsi_query_dev(gs_bigsi *bx, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                       const uint64_t *read_rec_off, uint64_t n_reads, uint32_t down_sample, uint32_t *n_kmers, uint32_t *best_colour, uint32_t *best_hits,
                       uint32_t *counts)
{
    (void)seq_bytes; (void)n_rec;
    GS_REQUIRE(bx, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(down_sample >= 1, GS_ERR_INVALID, "bigsig: down_sample = 0");
    GS_REQUIRE(bx->n >= 1, GS_ERR_STATE, "bigsig: the index holds no genome");
    GS_REQUIRE(n_reads == 0 || (seq && rec_start && rec_len && read_rec_off && n_kmers && best_colour && best_hits), GS_ERR_INVALID, "null argument");
    if (n_reads == 0) return GS_OK;
    return bigsi_query_launch<false>(bx, seq, rec_start, rec_len, read_rec_off, n_reads, down_sample, n_kmers, best_colour, best_hits, counts, gs::BxTies<false>{});
}

int gs_bigsi_query_ties_dev(gs_bigsi *bx, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                            const uint64_t *read_rec_off, uint64_t n_reads, uint32_t down_sample, uint32_t max_ties, uint32_t *n_kmers, uint32_t *best_hits,
                            uint32_t *n_tied, uint32_t *tied, uint32_t *sig_colour)
{
    (void)seq_bytes; (void)n_rec;
    GS_REQUIRE(bx, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(down_sample >= 1, GS_ERR_INVALID, "bigsig: down_sample = 0");
    GS_REQUIRE(max_ties >= 1 && max_ties <= GS_BIGSI_MAX_TIES, GS_ERR_INVALID, "bigsig: max_ties %u outside 1..%u", max_ties, GS_BIGSI_MAX_TIES);
    GS_REQUIRE(bx->n >= 1, GS_ERR_STATE, "bigsig: the index holds no genome");
    GS_REQUIRE(n_reads == 0 || (seq && rec_start && rec_len && read_rec_off && n_kmers && best_hits && n_tied && tied && sig_colour), GS_ERR_INVALID, "null argument");
    if (n_reads == 0) return GS_OK;
    gs::BxTies<true> ties;
    ties.tc = bx->tc.as<uint64_t>(); ties.n_tied = n_tied; ties.tied = tied; ties.sig = sig_colour; ties.max_ties = max_ties;
    return bigsi_query_launch<true>(bx, seq, rec_start, rec_len, read_rec_off, n_reads, down_sample, n_kmers, nullptr, best_hits, nullptr, ties);
}

int gs_bigsi_query(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end, uint64_t n_rec,
                   const uint64_t *read_rec_off, uint64_t n_reads, uint32_t down_sample, uint32_t *n_kmers, uint32_t *best_colour, uint32_t *best_hits,
                   uint32_t *counts)
{
    using namespace gs;
    GS_REQUIRE(bx, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(down_sample >= 1, GS_ERR_INVALID, "bigsig: down_sample = 0");
    GS_REQUIRE(bx->n >= 1, GS_ERR_STATE, "bigsig: the index holds no genome");
    GS_REQUIRE(n_reads == 0 || ((text || n_rec == 0) && read_rec_off && (n_rec == 0 || (rec_begin && rec_end)) && n_kmers && best_colour && best_hits), GS_ERR_INVALID,
               "null argument");
    if (n_reads == 0) return GS_OK;
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    Staged s(c);
    int rc = stage_text(c, bx->prm.k, text, qual, min_phred, rec_begin, rec_end, n_rec, read_rec_off, n_reads, s);
    if (rc) return rc;
    PoolBuf dn(c, SL_BIGSI_OUT_N), dc(c, SL_BIGSI_OUT_COLOUR), dh(c, SL_BIGSI_OUT_HITS), dd(c, SL_BIGSI_OUT_COUNTS);
    if ((rc = dn.alloc(4 * n_reads)) || (rc = dc.alloc(4 * n_reads)) || (rc = dh.alloc(4 * n_reads))) return rc;
    if (counts && (rc = dd.alloc(4 * n_reads * bx->n))) return rc;
    rc = gs_bigsi_query_dev(bx, s.seq.p, s.seq_bytes, s.rs.as<uint64_t>(), s.rl.as<uint64_t>(), s.n_seg, s.go.as<uint64_t>(), n_reads, down_sample, dn.as<uint32_t>(),
                            dc.as<uint32_t>(), dh.as<uint32_t>(), counts ? dd.as<uint32_t>() : nullptr);
    if (rc) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(n_kmers, dn.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(best_colour, dc.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(best_hits, dh.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    if (counts) GS_HIP_CHECK(hipMemcpyAsync(counts, dd.p, 4 * n_reads * bx->n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_bigsi_query_ties(gs_bigsi *bx, const void *text, const void *qual, uint32_t min_phred, const uint64_t *rec_begin, const uint64_t *rec_end, uint64_t n_rec,
                        const uint64_t *read_rec_off, uint64_t n_reads, uint32_t down_sample, uint32_t max_ties, uint32_t *n_kmers, uint32_t *best_hits,
                        uint32_t *n_tied, uint32_t *tied, uint32_t *sig_colour)
{
    using namespace gs;
    GS_REQUIRE(bx, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(down_sample >= 1, GS_ERR_INVALID, "bigsig: down_sample = 0");
    GS_REQUIRE(max_ties >= 1 && max_ties <= GS_BIGSI_MAX_TIES, GS_ERR_INVALID, "bigsig: max_ties %u outside 1..%u", max_ties, GS_BIGSI_MAX_TIES);
    GS_REQUIRE(bx->n >= 1, GS_ERR_STATE, "bigsig: the index holds no genome");
    GS_REQUIRE(n_reads == 0 || ((text || n_rec == 0) && read_rec_off && (n_rec == 0 || (rec_begin && rec_end)) && n_kmers && best_hits && n_tied && tied && sig_colour),
               GS_ERR_INVALID, "null argument");
    if (n_reads == 0) return GS_OK;
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    Staged s(c);
    int rc = stage_text(c, bx->prm.k, text, qual, min_phred, rec_begin, rec_end, n_rec, read_rec_off, n_reads, s);
    if (rc) return rc;
    PoolBuf dn(c, SL_BIGSI_OUT_N), dh(c, SL_BIGSI_OUT_HITS), dt(c, SL_BIGSI_OUT_NTIED), dl(c, SL_BIGSI_OUT_TIED), ds(c, SL_BIGSI_OUT_SIG);
    if ((rc = dn.alloc(4 * n_reads)) || (rc = dh.alloc(4 * n_reads)) || (rc = dt.alloc(4 * n_reads)) || (rc = dl.alloc(4 * n_reads * max_ties)) || (rc = ds.alloc(4 * n_reads)))
        return rc;
    rc = gs_bigsi_query_ties_dev(bx, s.seq.p, s.seq_bytes, s.rs.as<uint64_t>(), s.rl.as<uint64_t>(), s.n_seg, s.go.as<uint64_t>(), n_reads, down_sample, max_ties,
                                 dn.as<uint32_t>(), dh.as<uint32_t>(), dt.as<uint32_t>(), dl.as<uint32_t>(), ds.as<uint32_t>());
    if (rc) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(n_kmers, dn.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(best_hits, dh.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(n_tied, dt.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(tied, dl.p, 4 * n_reads * max_ties, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(sig_colour, ds.p, 4 * n_reads, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_bigsi_verdict_dev(gs_bigsi *bx, uint64_t n_reads, const uint32_t *n_kmers, const uint32_t *best_hits, const uint32_t *n_tied, const uint32_t *sig_colour,
                         double fp_correct, double *tail, uint8_t *verdict)
{
    using namespace gs;
    GS_REQUIRE(bx && (n_reads == 0 || (n_kmers && best_hits && n_tied && sig_colour && tail && verdict)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(bx->n >= 1, GS_ERR_STATE, "bigsig: the index holds no genome");
    if (n_reads == 0) return GS_OK;
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    hipLaunchKernelGGL(k_bigsi_verdict, dim3((uint32_t)((n_reads + 63) / 64)), dim3(64), 0, c->stream, n_reads, n_kmers, best_hits, n_tied, sig_colour,
                       bx->tc.as<uint64_t>(), bx->n, bx->prm.bloom_size, bx->prm.num_hash, fp_correct, tail, verdict);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

uint32_t gs_bigsi_verdict_code(uint32_t n_kmers, uint32_t best_hits, uint32_t n_tied, double tail, double fp_correct)
{
    return gs::bigsi_verdict(n_kmers, best_hits, n_tied, tail, fp_correct);
}

int gs_bigsi_classify_dev(gs_bigsi *bx, uint64_t n_reads, const uint32_t *n_kmers, const uint32_t *best_colour, const uint32_t *best_hits, double fp_correct,
                          double *tail, uint8_t *accept)
{
    using namespace gs;
    GS_REQUIRE(bx && (n_reads == 0 || (n_kmers && best_colour && best_hits && tail && accept)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(bx->n >= 1, GS_ERR_STATE, "bigsig: the index holds no genome");
    if (n_reads == 0) return GS_OK;
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    hipLaunchKernelGGL(k_bigsi_classify, dim3((uint32_t)((n_reads + 63) / 64)), dim3(64), 0, c->stream, n_reads, n_kmers, best_colour, best_hits, bx->tc.as<uint64_t>(),
                       bx->n, bx->prm.bloom_size, bx->prm.num_hash, fp_correct, tail, accept);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

int gs_bigsi_set_accessions(gs_bigsi *bx, const char *const *names, uint64_t n)
{
    GS_REQUIRE(bx && (n == 0 || names), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n == bx->n, GS_ERR_INVALID, "%llu accessions for %llu colours", (unsigned long long)n, (unsigned long long)bx->n);
    std::vector<std::string> v(n);
    for (uint64_t i = 0; i < n; i++) { GS_REQUIRE(names[i], GS_ERR_INVALID, "null accession"); v[i] = names[i]; }
    bx->names.swap(v);
    return GS_OK;
}

int gs_bigsi_accessions(gs_bigsi *bx, char *buf, uint64_t cap_bytes, uint64_t *bytes_out)
{
    GS_REQUIRE(bx && bytes_out, GS_ERR_INVALID, "null argument");
    uint64_t need = 0;
    for (uint64_t i = 0; i < bx->n; i++) need += (i < bx->names.size() ? bx->names[i].size() : 0) + 1;
    *bytes_out = need;
    if (!buf) return GS_OK;
    GS_REQUIRE(cap_bytes >= need, GS_ERR_INVALID, "the buffer holds %llu of %llu bytes", (unsigned long long)cap_bytes, (unsigned long long)need);
    char *o = buf;
    for (uint64_t i = 0; i < bx->n; i++) {
        if (i < bx->names.size()) { memcpy(o, bx->names[i].data(), bx->names[i].size()); o += bx->names[i].size(); }
        *o++ = 0;
    }
    return GS_OK;
}

// magic, version, k, num_hash, data_t (u32 each; a minimizer index: version 2 and one more u32, m), bloom_size, n_colours (u64), per colour: u32 length + accession bytes, t_c[n], nk_c[n] (u64), then
// bloom_size rows of ceil(n_colours / 64) u64 words
int gs_bigsi_save(gs_bigsi *bx, const char *path)
{
    using namespace gs;
    GS_REQUIRE(bx && path, GS_ERR_INVALID, "null argument");
    gs_ctx *c = bx->c;
    GS_CTX_LOCK(c);
    FILE *f = fopen(path, "wb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot write %s: %s", path, strerror(errno));
    const uint64_t n = bx->n, B = bx->prm.bloom_size, wu = (n + 63) / 64;
    const uint32_t head[5] = {bx->m ? BX_VERSION_MINI : BX_VERSION, bx->prm.k, bx->prm.num_hash, bx->prm.data_t, bx->m};
    int bad = write_all(f, BX_MAGIC, 8) | write_all(f, head, bx->m ? 20 : 16) | write_all(f, &B, 8) | write_all(f, &n, 8);
    for (uint64_t i = 0; i < n && !bad; i++) {
        const std::string nm = i < bx->names.size() ? bx->names[i] : std::string();
        const uint32_t l = (uint32_t)nm.size();
        bad |= write_all(f, &l, 4) | write_all(f, nm.data(), l);
    }
    std::vector<uint64_t> t(n), q(n);
    int rc = n ? gs_bigsi_bits_set(bx, 0, n, t.data(), q.data()) : GS_OK;
    if (!rc) bad |= write_all(f, t.data(), 8 * n) | write_all(f, q.data(), 8 * n);
    const uint64_t chunk = std::max<uint64_t>(((uint64_t)64 << 20) / (8 * std::max<uint64_t>(wu, 1)), 1);
    std::vector<uint64_t> buf(wu ? chunk * wu : 0);
    for (uint64_t r = 0; r < B && wu && !bad && !rc; r += chunk) {
        const uint64_t nr = std::min(chunk, B - r);
        if (hipMemcpy2D(buf.data(), wu * 8, bx->M.as<uint64_t>() + r * bx->W, bx->W * 8, wu * 8, nr, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("reading the matrix back failed"); rc = GS_ERR_HIP;
        }
        else bad |= write_all(f, buf.data(), nr * wu * 8);
    }
    if (fclose(f) != 0) bad = 1;
    if (rc) return rc;
    GS_REQUIRE(!bad, GS_ERR_IO, "writing %s failed", path);
    return GS_OK;
}

int gs_bigsi_load(gs_ctx *c, const char *path, uint64_t colour_capacity, gs_bigsi **out)
{
    using namespace gs;
    GS_REQUIRE(c && path && out, GS_ERR_INVALID, "null argument");
    // the host half (gs_bigsi_file.cpp, SPEC 16.2): header, accessions, t_c and nk_c read, the size of the file held against bloom_size x ceil(n / 64) words and the
    // parameters checked; the device is asked for nothing before it accepts
    BigsiFile bf; FILE *f = nullptr;
    int rc = bigsi_file_parse(path, &bf, &f);
    if (rc) return rc;
    const gs_bigsi_params prm = bf.prm;
    const uint64_t n = bf.desc.n_colours, B = prm.bloom_size;
    std::vector<std::string> &names = bf.names; std::vector<uint64_t> &t = bf.t, &q = bf.q;
    int bad = 0;
    const uint64_t cap = std::max<uint64_t>(std::max(colour_capacity, n), 1);
    gs_bigsi *bx = nullptr;
    rc = bigsi_alloc(c, &prm, cap, &bx);
    if (rc) { fclose(f); return rc; }
    GS_CTX_LOCK(c);
    const uint64_t wu = (n + 63) / 64;
    const uint64_t chunk = std::max<uint64_t>(((uint64_t)64 << 20) / (8 * std::max<uint64_t>(wu, 1)), 1);
    std::vector<uint64_t> buf;
    try { buf.resize(wu ? std::min(chunk, B) * wu : 0); }           // at most 64 MiB, and no more than the file's matrix
    catch (const std::exception &) { fclose(f); delete bx; GS_REQUIRE(false, GS_ERR_IO, "%s: not enough host memory to stage the matrix", path); }
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemcpy(bx->tc.p, t.data(), 8 * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(bx->nk.p, q.data(), 8 * n, hipMemcpyHostToDevice);
    }
    for (uint64_t r = 0; r < B && wu && !bad && e == hipSuccess; r += chunk) {
        const uint64_t nr = std::min(chunk, B - r);
        bad |= read_all(f, buf.data(), nr * wu * 8);
        if (!bad) e = hipMemcpy2D(bx->M.as<uint64_t>() + r * bx->W, bx->W * 8, buf.data(), wu * 8, wu * 8, nr, hipMemcpyHostToDevice);
    }
    fclose(f);
    if (bad || e != hipSuccess) {
        delete bx;
        GS_REQUIRE(!bad, GS_ERR_IO, "%s is cut short", path);
        GS_REQUIRE(false, GS_ERR_HIP, "loading the matrix failed: %s", hipGetErrorString(e));
    }
    bx->n = n;
    bx->m = bf.desc.minimizer_len;
    bool any = false;
    for (const std::string &s : names) any = any || !s.empty();
    if (any) bx->names.swap(names);
    *out = bx;
    return GS_OK;
}

int gs_bigsi_positions(uint64_t v, uint32_t num_hash, uint64_t bloom_size, uint64_t *pos_out)
{
    GS_REQUIRE(pos_out && num_hash >= 1 && num_hash <= GS_BIGSI_HMAX && bloom_size >= 1 && bloom_size < GS_BIGSI_BMAX, GS_ERR_INVALID, "bigsig: parameter out of range");
    uint64_t h1, st;
    gs::bigsi_hash(v, h1, st);
    for (uint32_t i = 0; i < num_hash; i++) pos_out[i] = gs::bigsi_pos(h1, st, i, bloom_size);
    return GS_OK;
}

int gs_bigsi_split(const void *text, const void *qual, uint64_t n, uint32_t min_phred, uint64_t min_len, uint64_t cap, uint64_t *seg_begin, uint64_t *seg_len,
                   uint64_t *n_out)
{
    GS_REQUIRE((text || n == 0) && n_out, GS_ERR_INVALID, "null argument");
    uint64_t cnt = 0;
    gs::split_text((const uint8_t *)text, (const uint8_t *)qual, 0, n, min_phred,
                   [&](uint64_t b, uint64_t l) {
                       if (l < min_len) return;
                       if (cnt < cap && seg_begin && seg_len) { seg_begin[cnt] = b; seg_len[cnt] = l; }
                       cnt++;
                   },
                   [](int) {});
    *n_out = cnt;
    return GS_OK;
}

int gs_bigsi_minimizers(const void *text, const void *qual, uint64_t n, uint32_t min_phred, uint32_t k, uint32_t m, uint32_t data_t, uint64_t cap, uint64_t *value_out,
                        uint64_t *pos_out, uint64_t *n_out)
{
    GS_REQUIRE((text || n == 0) && n_out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(k >= 1 && k <= GS_BIGSI_KMAX && m >= 1 && m < k, GS_ERR_INVALID, "bigsig: window %u / minimizer %u outside 1 <= m < k <= 32", k, m);
    GS_REQUIRE(data_t == GS_DATA_DNA || data_t == GS_DATA_DNA_FWD, GS_ERR_INVALID, "bigsig: data type %u is not DNA", data_t);
    const uint8_t *tx = (const uint8_t *)text;
    const bool fwd_only = data_t == GS_DATA_DNA_FWD;
    const uint32_t w = k - m + 1;
    const uint64_t mask = ((uint64_t)1 << (2 * m)) - 1;        // m <= 31
    std::vector<uint8_t> codes;
    std::vector<uint64_t> offs, vals, keys;
    uint64_t cnt = 0;
    gs::split_text(tx, (const uint8_t *)qual, 0, n, min_phred,
                   [&](uint64_t begin, uint64_t L) {
                       if (L >= k) {
                           offs.clear(); vals.clear(); keys.clear();
                           for (uint64_t i = begin; offs.size() < L; i++)
                               if (tx[i] != '\n' && tx[i] != '\r') offs.push_back(i);
                           uint64_t fwd = 0, rc = 0;
                           for (uint64_t i = 0; i < L; i++) {                 // the m-mer that ends at base i (SPEC 1.1 with k := m)
                               fwd = ((fwd << 2) | codes[i]) & mask;
                               rc = (rc >> 2) | ((uint64_t)(3 - codes[i]) << (2 * (m - 1)));
                               if (i + 1 >= m) {
                                   const uint64_t v = fwd_only || fwd < rc ? fwd : rc;
                                   uint64_t h1, st;
                                   gs::bigsi_hash(v, h1, st);
                                   vals.push_back(v); keys.push_back(h1);
                               }
                           }
                           uint64_t prev = 0;
                           for (uint64_t s = 0; s + k <= L; s++) {
                               const uint64_t a = s + gs::minimizer_pick(keys.data() + s, w);
                               if (s == 0 || a != prev) {
                                   if (cnt < cap && value_out) value_out[cnt] = vals[a];
                                   if (cnt < cap && pos_out) pos_out[cnt] = offs[a];
                                   cnt++;
                               }
                               prev = a;
                           }
                       }
                       codes.clear();
                   },
                   [&](int code) { codes.push_back((uint8_t)code); });
    *n_out = cnt;
    return GS_OK;
}

double gs_bigsi_tail(uint64_t t_c, uint64_t bloom_size, uint32_t num_hash, uint32_t n_kmers, uint32_t best_hits)
{
    return gs::bigsi_tail(t_c, bloom_size, num_hash, n_kmers, best_hits);
}

int gs_bigsig_write_reads(const char *prefix, const char *const *accessions, uint64_t n_colours, const char *const *read_ids, uint64_t n_reads,
                          const uint32_t *best_colour, const uint32_t *best_hits, const uint32_t *n_kmers, const uint8_t *accept)
{
    GS_REQUIRE(prefix && (n_colours == 0 || accessions) && (n_reads == 0 || (read_ids && best_colour && best_hits && n_kmers && accept)), GS_ERR_INVALID, "null argument");
    for (uint64_t r = 0; r < n_reads; r++)
        GS_REQUIRE(best_hits[r] == 0 || best_colour[r] < n_colours, GS_ERR_INVALID, "read %llu names colour %u of %llu", (unsigned long long)r, best_colour[r], (unsigned long long)n_colours);
    const std::string p(prefix);
    FILE *f = fopen((p + "_reads.txt").c_str(), "wb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot write %s_reads.txt: %s", prefix, strerror(errno));
    std::vector<uint64_t> per(n_colours, 0);
    uint64_t rejected = 0, no_hits = 0;
    int bad = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const bool hit = best_hits[r] > 0, ok = hit && accept[r];
        if (!hit) no_hits++;
        else if (ok) per[best_colour[r]]++;
        else rejected++;
        bad |= fprintf(f, "%s\t%s\t%u\t%u\t%s\n", read_ids[r], hit ? accessions[best_colour[r]] : "no_hits", best_hits[r], n_kmers[r], ok ? "accept" : "reject") < 0;
    }
    if (fclose(f) != 0) bad = 1;
    GS_REQUIRE(!bad, GS_ERR_IO, "writing %s_reads.txt failed", prefix);
    std::vector<uint64_t> order;
    for (uint64_t c = 0; c < n_colours; c++) if (per[c]) order.push_back(c);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (per[a] != per[b]) return per[a] > per[b];
        const int s = strcmp(accessions[a], accessions[b]);
        return s != 0 ? s < 0 : a < b;
    });
    f = fopen((p + "_counts.txt").c_str(), "wb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot write %s_counts.txt: %s", prefix, strerror(errno));
    for (uint64_t c : order) bad |= fprintf(f, "%s\t%llu\n", accessions[c], (unsigned long long)per[c]) < 0;
    bad |= fprintf(f, "reject\t%llu\nno_hits\t%llu\n", (unsigned long long)rejected, (unsigned long long)no_hits) < 0;
    if (fclose(f) != 0) bad = 1;
    GS_REQUIRE(!bad, GS_ERR_IO, "writing %s_counts.txt failed", prefix);
    return GS_OK;
}

int gs_bigsig_write_report(const char *prefix, const char *const *accessions, uint64_t n_colours, const char *const *read_ids, uint64_t n_reads, uint32_t max_ties,
                           const uint32_t *n_kmers, const uint32_t *best_hits, const uint32_t *n_tied, const uint32_t *tied, const uint8_t *verdict)
{
    GS_REQUIRE(prefix && (n_colours == 0 || accessions) && (n_reads == 0 || (read_ids && n_kmers && best_hits && n_tied && tied && verdict)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(max_ties >= 1 && max_ties <= GS_BIGSI_MAX_TIES, GS_ERR_INVALID, "bigsig: max_ties %u outside 1..%u", max_ties, GS_BIGSI_MAX_TIES);
    const auto listed = [&](uint64_t r) { return n_tied[r] < max_ties ? n_tied[r] : max_ties; };
    for (uint64_t r = 0; r < n_reads; r++) {
        GS_REQUIRE(verdict[r] <= GS_BIGSI_TIED, GS_ERR_INVALID, "read %llu has verdict %u", (unsigned long long)r, verdict[r]);
        if (verdict[r] < GS_BIGSI_UNIQUE) continue;
        GS_REQUIRE(n_tied[r] >= 1, GS_ERR_INVALID, "read %llu names a colour and has no tied colour", (unsigned long long)r);
        for (uint32_t i = 0; i < listed(r); i++)
            GS_REQUIRE(tied[r * max_ties + i] < n_colours, GS_ERR_INVALID, "read %llu names colour %u of %llu", (unsigned long long)r, tied[r * max_ties + i],
                       (unsigned long long)n_colours);
    }
    const std::string p(prefix);
    FILE *f = fopen((p + "_reads.txt").c_str(), "wb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot write %s_reads.txt: %s", prefix, strerror(errno));
    std::vector<uint64_t> per(n_colours, 0);
    uint64_t rejected = 0, no_hits = 0, too_short = 0;
    int bad = 0;
    std::string status;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint32_t v = verdict[r];
        const bool named = v >= GS_BIGSI_UNIQUE;
        if (v == GS_BIGSI_TOO_SHORT) { too_short++; status = "too_short"; }
        else if (v == GS_BIGSI_NO_HITS) { no_hits++; status = "no_hits"; }
        else if (v == GS_BIGSI_NOT_SIGNIFICANT) { rejected++; status = "no_significant_hits"; }
        else if (v == GS_BIGSI_UNIQUE) { per[tied[r * max_ties]]++; status = accessions[tied[r * max_ties]]; }
        else {
            rejected++;
            status.clear();
            for (uint32_t i = 0; i < listed(r); i++) { if (i) status += ','; status += accessions[tied[r * max_ties + i]]; }
            if (n_tied[r] > max_ties) status += ",...";
        }
        bad |= fprintf(f, "%s\t%s\t%u\t%u\t%s\t%u\n", read_ids[r], status.c_str(), named ? best_hits[r] : 0u, n_kmers[r],
                       v == GS_BIGSI_NOT_SIGNIFICANT || v == GS_BIGSI_TIED ? "reject" : "accept", v == GS_BIGSI_UNIQUE ? 1u : (v == GS_BIGSI_TIED ? n_tied[r] : 0u)) < 0;
    }
    if (fclose(f) != 0) bad = 1;
    GS_REQUIRE(!bad, GS_ERR_IO, "writing %s_reads.txt failed", prefix);
    std::vector<uint64_t> order;
    for (uint64_t c = 0; c < n_colours; c++) if (per[c]) order.push_back(c);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (per[a] != per[b]) return per[a] > per[b];
        const int s = strcmp(accessions[a], accessions[b]);
        return s != 0 ? s < 0 : a < b;
    });
    f = fopen((p + "_counts.txt").c_str(), "wb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot write %s_counts.txt: %s", prefix, strerror(errno));
    for (uint64_t c : order) bad |= fprintf(f, "%s\t%llu\n", accessions[c], (unsigned long long)per[c]) < 0;
    bad |= fprintf(f, "reject\t%llu\nno_hits\t%llu\ntoo_short\t%llu\n", (unsigned long long)rejected, (unsigned long long)no_hits, (unsigned long long)too_short) < 0;
    if (fclose(f) != 0) bad = 1;
    GS_REQUIRE(!bad, GS_ERR_IO, "writing %s_counts.txt failed", prefix);
    return GS_OK;
}

}  // extern "C"
