// gs_orf.hip — SPEC 14: stop-to-stop six-frame translation of packed nucleotide records, the stage in front of hmmsearch for a user who holds genomes.
// Not a gene caller: the HMM is the gene finder, the ORF set is not a proteome.
//
// The grid is over tiles of GS_ORF_TILE = 192 bases of one record, one wavefront each: lane l holds the three codon positions p0 + 3 l + c (c = 0..2, one
// of each class) and reads five bases, so a (strand, class) pair's stops of a tile are ONE ballot. Passes, all in (record, tile) order:
//   k_orf_rec_tiles   tiles in front of every record (one workgroup), validation of the records against seq_bytes
//   k_orf_tile<STOPS> per tile and pair the last stop, as 64 x tile + lane + 1 (0 = none)
//   scan (max)        exclusive prefix maximum over the tiles: every tile's carry-in; a value from a tile of another record counts as none
//   k_orf_tile<COUNT> every terminator (a stop, or on a record's last tile the virtual end of a class) knows begin and n from the ballot below it or the
//                     carry; keep rule; per tile the kept ORFs, their residues, the long drops
//   scan (sum)        exclusive prefix sums = every tile's ORF and residue offsets, the three totals -> ONE read-back
//   k_orf_rec_off, k_orf_tile<EMIT>  rec_orf_off; descriptors in (end, strand) order, then the residues of one ORF at a time by the whole wavefront
// No atomics: every tile writes its own range, so the result is the same whatever the scheduling.
#include <string.h>
#include "gs_internal.hpp"
#include "gs_spec.hpp"
#include "gs_orf.hpp"

namespace gs {

constexpr uint32_t ORF_T = GS_ORF_TILE;
static_assert(ORF_T == 3 * 64, "a tile is one codon of each class per lane of a wavefront");
constexpr uint32_t ORF_LIST = 6 * 64 + 6;                 // kept ORFs of a tile at most: six terminators a lane, six virtual ends
constexpr uint32_t ORF_SCAN_ROWS = 1024;                  // rows of a column one workgroup of the scans takes
enum { ORF_META_TILES = 0, ORF_META_ERR = 1, ORF_META_N_ORF = 2, ORF_META_N_AA = 3, ORF_META_N_LONG = 4, ORF_META_WORDS = 8 };
enum { ORF_ERR_RANGE = 1, ORF_ERR_TILES = 2 };
enum { ORF_STOPS = 0, ORF_COUNT = 1, ORF_EMIT = 2 };

__constant__ char orf_letters[2][65] = {GS_ORF_TABLE_11, GS_ORF_TABLE_4};

// rtoff[r] = the tiles of the records in front of r, rtoff[n_rec] = all of them; a record that does not lie inside the packed buffer gets no tile and
// sets ORF_ERR_RANGE, so that no later pass reads outside it. ONE workgroup, lanes take contiguous stretches of records (as k_bigsi_window_prefix).
__global__ __launch_bounds__(1024) void k_orf_rec_tiles(const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len, uint64_t n_rec, uint64_t seq_bases,
                                                        uint64_t cap_tiles, uint64_t *__restrict__ rtoff, uint64_t *__restrict__ meta)
{
    __shared__ uint64_t part[1024];
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const uint64_t per = (n_rec + 1023) / 1024, b0 = (uint64_t)threadIdx.x * per, b = b0 < n_rec ? b0 : n_rec, e = b + per < n_rec ? b + per : n_rec;
    auto tiles_of = [&](uint64_t r, bool &ok) -> uint64_t {
        const uint64_t s = rec_start[r], l = rec_len[r];
        ok = l <= seq_bases && s <= seq_bases - l;
        return ok ? (l + ORF_T - 1) / ORF_T : 0;
    };
    uint64_t sum = 0; bool any_bad = false;
    for (uint64_t r = b; r < e; r++) { bool ok; sum += tiles_of(r, ok); any_bad |= !ok; }
    if (any_bad) bad = 1;                                  // (every writer writes the same value)
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t r = b; r < e; r++) { bool ok; rtoff[r] = run; run += tiles_of(r, ok); }
    if (threadIdx.x == 1023) {
        const uint64_t total = part[1023];
        rtoff[n_rec] = total;
        meta[ORF_META_TILES] = total;
        meta[ORF_META_ERR] = (bad ? ORF_ERR_RANGE : 0) | (total > cap_tiles ? ORF_ERR_TILES : 0);
    }
}

// ---- exclusive scans of the per-tile columns (maximum or sum), in place: reduce per workgroup, scan the partial results, apply ------------------------------
template <bool MAX> __device__ __forceinline__ uint64_t orf_op(uint64_t a, uint64_t b) { return MAX ? (a > b ? a : b) : a + b; }
__device__ __forceinline__ uint64_t orf_rows(const uint64_t *meta, uint64_t cap_tiles) { const uint64_t n = meta[ORF_META_TILES]; return n < cap_tiles ? n : cap_tiles; }

// grid (workgroups of ORF_SCAN_ROWS rows, columns); thread t takes rows 4 t .. 4 t + 3 of its workgroup
template <bool MAX> __global__ __launch_bounds__(256) void k_orf_scan_reduce(const uint64_t *__restrict__ cols, uint64_t cap_tiles, const uint64_t *__restrict__ meta,
                                                                            uint64_t *__restrict__ partials, uint64_t cap_blocks)
{
    __shared__ uint64_t ws[256];
    const uint64_t n = orf_rows(meta, cap_tiles), row0 = (uint64_t)blockIdx.x * ORF_SCAN_ROWS + 4 * threadIdx.x;
    if ((uint64_t)blockIdx.x * ORF_SCAN_ROWS >= n) return;
    const uint64_t *col = cols + (uint64_t)blockIdx.y * cap_tiles;
    uint64_t x = 0;
    for (uint32_t i = 0; i < 4; i++) if (row0 + i < n) x = orf_op<MAX>(x, col[row0 + i]);
    ws[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) ws[threadIdx.x] = orf_op<MAX>(ws[threadIdx.x], ws[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[(uint64_t)blockIdx.y * cap_blocks + blockIdx.x] = ws[0];
}
// one workgroup per column: its partial results become exclusive, the column's total goes to totals[column] when asked for
template <bool MAX> __global__ __launch_bounds__(1024) void k_orf_scan_partials(uint64_t *__restrict__ partials, uint64_t cap_blocks, uint64_t cap_tiles,
                                                                               const uint64_t *__restrict__ meta, uint64_t *__restrict__ totals)
{
    __shared__ uint64_t part[1024];
    const uint64_t n = orf_rows(meta, cap_tiles), nb = (n + ORF_SCAN_ROWS - 1) / ORF_SCAN_ROWS;
    uint64_t *p = partials + (uint64_t)blockIdx.x * cap_blocks;
    const uint64_t per = (nb + 1023) / 1024, b0 = (uint64_t)threadIdx.x * per, b = b0 < nb ? b0 : nb, e = b + per < nb ? b + per : nb;
    uint64_t s = 0;
    for (uint64_t i = b; i < e; i++) s = orf_op<MAX>(s, p[i]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] = orf_op<MAX>(part[threadIdx.x], v);
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t i = b; i < e; i++) { const uint64_t v = p[i]; p[i] = run; run = orf_op<MAX>(run, v); }
    if (totals && threadIdx.x == 1023) totals[blockIdx.x] = part[1023];
}
template <bool MAX> __global__ __launch_bounds__(256) void k_orf_scan_apply(uint64_t *__restrict__ cols, uint64_t cap_tiles, const uint64_t *__restrict__ meta,
                                                                           const uint64_t *__restrict__ partials, uint64_t cap_blocks)
{
    __shared__ uint64_t ws[256];
    const uint64_t n = orf_rows(meta, cap_tiles), row0 = (uint64_t)blockIdx.x * ORF_SCAN_ROWS + 4 * threadIdx.x;
    if ((uint64_t)blockIdx.x * ORF_SCAN_ROWS >= n) return;
    uint64_t *col = cols + (uint64_t)blockIdx.y * cap_tiles;
    uint64_t v[4], x = 0;
    for (uint32_t i = 0; i < 4; i++) { v[i] = row0 + i < n ? col[row0 + i] : 0; x = orf_op<MAX>(x, v[i]); }
    ws[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint64_t y = threadIdx.x >= o ? ws[threadIdx.x - o] : 0;
        __syncthreads();
        ws[threadIdx.x] = orf_op<MAX>(ws[threadIdx.x], y);
        __syncthreads();
    }
    uint64_t run = orf_op<MAX>(partials[(uint64_t)blockIdx.y * cap_blocks + blockIdx.x], threadIdx.x ? ws[threadIdx.x - 1] : 0);
    for (uint32_t i = 0; i < 4; i++) { if (row0 + i < n) col[row0 + i] = run; run = orf_op<MAX>(run, v[i]); }
}

// ---- the tile passes ------------------------------------------------------------------------------------------------------------------------------------------
struct OrfEntry { uint64_t begin_strand, n, aoff; };            // begin | strand << 63
__device__ __forceinline__ uint32_t orf_top_bit(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }
__device__ __forceinline__ uint64_t orf_wave_sum(uint64_t x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down((unsigned long long)x, o);
    return __shfl((unsigned long long)x, 0);
}
// inclusive prefix sum over the lanes
__device__ __forceinline__ uint64_t orf_wave_scan(uint64_t x, uint32_t lane)
{
    for (uint32_t o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up((unsigned long long)x, o); if (lane >= o) x += y; }
    return x;
}
// codon index of the three bases at absolute base g (all inside a record, so the second byte exists whenever it is read)
__device__ __forceinline__ uint32_t orf_codon_at(const uint8_t *__restrict__ seq, uint64_t g)
{
    const uint32_t o = (uint32_t)g & 3u;
    uint32_t v = (uint32_t)seq[g >> 2] << 8;
    if (o >= 2) v |= seq[(g >> 2) + 1];
    return (v >> (10 - 2 * o)) & 63u;
}

template <int MODE> __global__ __launch_bounds__(64) void k_orf_tile(const OrfArgs a)
{
    __shared__ OrfEntry list[MODE == ORF_EMIT ? ORF_LIST : 1];
    const uint64_t g = blockIdx.x, n_tiles = orf_rows(a.meta, a.cap_tiles);
    if (g >= n_tiles) return;
    const uint32_t lane = threadIdx.x;
    // the record of tile g: rtoff[lo] <= g < rtoff[hi] throughout (rtoff[n_rec] = all tiles)
    uint64_t lo = 0, hi = a.n_rec;
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (a.rtoff[mid] <= g) lo = mid; else hi = mid; }
    const uint64_t r = lo, t0 = a.rtoff[r], rs = a.rec_start[r], L = a.rec_len[r], p0 = (g - t0) * ORF_T;
    const bool last = g + 1 == a.rtoff[r + 1];
    // five bases from this lane's first position on: bits 9..0 of x, first base highest; bytes past the record's last are not read
    const uint64_t pl = p0 + 3 * lane, gb = rs + pl;
    uint32_t x = 0;
    if (pl < L) {
        const uint64_t byte = gb >> 2, last_byte = (rs + L - 1) >> 2;
        uint32_t v = (uint32_t)a.seq[byte] << 8;
        if (byte + 1 <= last_byte) v |= a.seq[byte + 1];
        x = (v >> (6 - 2 * ((uint32_t)gb & 3u))) & 0x3FFu;
    }
    uint64_t bal[6];
    bool stop[6];
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) {
        const bool valid = pl + c + 3 <= L;
        const uint32_t f = (x >> (4 - 2 * c)) & 63u;
        stop[2 * c] = valid && ((a.stop_mask >> f) & 1u);
        stop[2 * c + 1] = valid && ((a.stop_mask >> orf_rev_codon(f)) & 1u);
    }
#pragma unroll
    for (uint32_t q = 0; q < 6; q++) bal[q] = __ballot(stop[q]);

    if constexpr (MODE == ORF_STOPS) {
#pragma unroll
        for (uint32_t q = 0; q < 6; q++)
            if (lane == q) a.stops[(uint64_t)q * a.cap_tiles + g] = bal[q] ? g * 64 + orf_top_bit(bal[q]) + 1 : 0;
        return;
    } else {
        const uint64_t below = ((uint64_t)1 << lane) - 1;
        uint64_t begin[6], n[6], vbegin[6], vn[6];
        bool keep[6], vkeep[6];
        uint32_t nk = 0, nlong = 0, vlong = 0;
        uint64_t na = 0;
#pragma unroll
        for (uint32_t q = 0; q < 6; q++) {
            const uint32_t c = q >> 1;
            // the carry: the position after the pair's last stop in the tiles in front, when that tile is one of this record; else the class's first position
            const uint64_t sc = a.stops[(uint64_t)q * a.cap_tiles + g];
            uint64_t carry = c;
            if (sc != 0 && ((sc - 1) >> 6) >= t0) carry = (((sc - 1) >> 6) - t0) * ORF_T + 3 * ((sc - 1) & 63u) + c + 3;
            const uint64_t bl = bal[q] & below;
            begin[q] = bl ? p0 + 3 * (orf_top_bit(bl) + 1) + c : carry;
            n[q] = stop[q] ? (pl + c - begin[q]) / 3 : 0;
            keep[q] = stop[q] && n[q] >= a.min_aa && (a.max_aa == 0 || n[q] <= a.max_aa);
            nlong += stop[q] && a.max_aa != 0 && n[q] > a.max_aa;
            nk += keep[q];
            na += keep[q] ? n[q] : 0;
            // the virtual end of the class (same in every lane; meaningful on the record's last tile)
            vbegin[q] = bal[q] ? p0 + 3 * (orf_top_bit(bal[q]) + 1) + c : carry;
            vn[q] = last ? (c + 3 * orf_class_codons(L, c) - vbegin[q]) / 3 : 0;
            vkeep[q] = vn[q] >= a.min_aa && (a.max_aa == 0 || vn[q] <= a.max_aa);
            vlong += a.max_aa != 0 && vn[q] > a.max_aa;
        }
        const uint64_t kscan = orf_wave_scan(nk, lane), ascan = orf_wave_scan(na, lane);
        const uint64_t k_stops = __shfl((unsigned long long)kscan, 63), a_stops = __shfl((unsigned long long)ascan, 63);
        uint64_t vk = 0, va = 0;
#pragma unroll
        for (uint32_t q = 0; q < 6; q++) { vk += vkeep[q]; va += vkeep[q] ? vn[q] : 0; }

        if constexpr (MODE == ORF_COUNT) {
            const uint64_t nl = orf_wave_sum(nlong) + vlong;
            if (lane == 0) {
                a.counts[g] = k_stops + vk;
                a.counts[a.cap_tiles + g] = a_stops + va;
                a.counts[2 * a.cap_tiles + g] = nl;
            }
        } else {
            const uint64_t obase = a.counts[g], abase = a.counts[a.cap_tiles + g];
            uint64_t o = obase + kscan - nk, ao = abase + ascan - na;
#pragma unroll
            for (uint32_t q = 0; q < 6; q++) {              // q ascending = (end, strand) ascending inside the lane
                if (keep[q]) {
                    gs_orf d; d.begin = begin[q]; d.rec = (uint32_t)r; d.strand = q & 1u;
                    a.orf[o] = d; a.aa_start[o] = ao; a.aa_len[o] = n[q];
                    list[o - obase] = OrfEntry{begin[q] | ((uint64_t)(q & 1u) << 63), n[q], ao};
                    o++; ao += n[q];
                }
            }
            if (last && lane == 0) {
                // the six virtual ends lie behind every stop of the record; among themselves in (end, strand) order
                uint64_t vo = obase + k_stops, vao = abase + a_stops;
                uint64_t key[6];
                for (uint32_t q = 0; q < 6; q++) key[q] = ((q >> 1) + 3 * orf_class_codons(L, q >> 1)) * 2 + (q & 1u);
                for (uint32_t i = 0; i < 6; i++) {
                    uint32_t q = 0; uint64_t best = ~(uint64_t)0;
                    for (uint32_t j = 0; j < 6; j++) if (key[j] < best) { best = key[j]; q = j; }
                    key[q] = ~(uint64_t)0;
                    if (vkeep[q]) {
                        gs_orf d; d.begin = vbegin[q]; d.rec = (uint32_t)r; d.strand = q & 1u;
                        a.orf[vo] = d; a.aa_start[vo] = vao; a.aa_len[vo] = vn[q];
                        list[vo - obase] = OrfEntry{vbegin[q] | ((uint64_t)(q & 1u) << 63), vn[q], vao};
                        vo++; vao += vn[q];
                    }
                }
            }
            __syncthreads();
            // the residues: one ORF at a time, the lanes stride over its codons (byte stores side by side, codons gathered from the packed bases)
            const uint32_t n_list = (uint32_t)(k_stops + vk);
            const char *letters = orf_letters[a.table_ix];
            for (uint32_t j = 0; a.aa && j < n_list; j++) {         // (no aa: the descriptors alone, gs_gene.hip)
                const OrfEntry e = list[j];
                const uint64_t b = e.begin_strand & ~((uint64_t)1 << 63), end = b + 3 * e.n;
                const bool rev = e.begin_strand >> 63;
                for (uint64_t t = lane; t < e.n; t += 64) {
                    const uint32_t f = orf_codon_at(a.seq, rs + (rev ? end - 3 - 3 * t : b + 3 * t));
                    a.aa[e.aoff + t] = (uint8_t)letters[rev ? orf_rev_codon(f) : f];
                }
            }
        }
    }
}

// rec_orf_off[r] = the ORFs in front of record r = the scanned count of its first tile (a record without tiles: of the next tile there is)
__global__ __launch_bounds__(256) void k_orf_rec_off(const uint64_t *__restrict__ rtoff, const uint64_t *__restrict__ counts, const uint64_t *__restrict__ meta, uint64_t n_rec,
                                                     uint64_t *__restrict__ rec_orf_off)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_rec) return;
    const uint64_t t = rtoff[r];
    rec_orf_off[r] = t < meta[ORF_META_TILES] ? counts[t] : meta[ORF_META_N_ORF];
}

static int orf_check_params(const gs_orf_params *prm, uint64_t n_rec)
{
    GS_REQUIRE(prm, GS_ERR_INVALID, "orf: null parameters");
    GS_REQUIRE(prm->min_aa != 0, GS_ERR_INVALID, "orf: min_aa = 0");
    GS_REQUIRE(prm->max_aa == 0 || prm->max_aa >= prm->min_aa, GS_ERR_INVALID, "orf: max_aa %u below min_aa %u", prm->max_aa, prm->min_aa);
    GS_REQUIRE(prm->flags == 0, GS_ERR_UNSUPPORTED, "orf: flags %u", prm->flags);
    GS_REQUIRE(prm->table == 11 || prm->table == 4, GS_ERR_UNSUPPORTED, "orf: translation table %u (11 and 4 are there)", prm->table);
    GS_REQUIRE(n_rec < (1ull << 32), GS_ERR_UNSUPPORTED, "orf: 2^32 records or more in one call");
    return GS_OK;
}
static int orf_check_outputs(uint64_t cap_orf, uint64_t cap_aa, const void *o0, const void *o1, const void *o2, const void *o3, const void *o4, bool *count_only)
{
    const int given = (o0 != nullptr) + (o1 != nullptr) + (o2 != nullptr) + (o3 != nullptr) + (o4 != nullptr);
    GS_REQUIRE(given == 0 || given == 5, GS_ERR_INVALID, "orf: all five outputs or none (%d given)", given);
    GS_REQUIRE(given == 5 || (cap_orf == 0 && cap_aa == 0), GS_ERR_INVALID, "orf: capacities without outputs");
    *count_only = given == 0;
    return GS_OK;
}

static int orf_check_caps(const uint64_t n_out[3], uint64_t cap_orf, uint64_t cap_aa)
{
    GS_REQUIRE(n_out[0] <= cap_orf && n_out[1] <= cap_aa, GS_ERR_INVALID, "orf: %llu ORFs of %llu residues do not fit capacities of %llu and %llu",
               (unsigned long long)n_out[0], (unsigned long long)n_out[1], (unsigned long long)cap_orf, (unsigned long long)cap_aa);
    return GS_OK;
}

// the passes up to the counts: n_out filled, the scanned per-tile state left in w for orf_emit. Waits for the stream once.
int orf_count(gs_ctx *c, const gs_orf_params *prm, const uint8_t *seq, uint64_t seq_bytes, const uint64_t *rs, const uint64_t *rl, uint64_t n_rec, OrfWork &w,
                     uint64_t n_out[3])
{
    GS_REQUIRE(seq_bytes < (1ull << 61), GS_ERR_UNSUPPORTED, "orf: seq_bytes");
    const uint64_t cap_tiles = 4 * seq_bytes / ORF_T + n_rec + 1, cap_blocks = (cap_tiles + ORF_SCAN_ROWS - 1) / ORF_SCAN_ROWS;
    GS_REQUIRE(cap_tiles < (1ull << 26), GS_ERR_UNSUPPORTED, "orf: room for %llu tiles in one call (2^26 wavefronts a launch)", (unsigned long long)cap_tiles);
    int rc;
    if ((rc = w.rtoff.alloc(8 * (n_rec + 1))) || (rc = w.meta.alloc(8 * ORF_META_WORDS)) || (rc = w.stops.alloc(8 * 6 * cap_tiles)) || (rc = w.counts.alloc(8 * 3 * cap_tiles)) ||
        (rc = w.partials.alloc(8 * 6 * cap_blocks)))
        return rc;
    OrfArgs &a = w.a;
    a.seq = seq; a.rec_start = rs; a.rec_len = rl; a.rtoff = w.rtoff.as<uint64_t>(); a.meta = w.meta.as<uint64_t>();
    a.n_rec = n_rec; a.cap_tiles = cap_tiles; a.stops = w.stops.as<uint64_t>(); a.counts = w.counts.as<uint64_t>();
    a.stop_mask = prm->table == 11 ? GS_ORF_STOPS_11 : GS_ORF_STOPS_4; a.table_ix = prm->table == 11 ? 0 : 1;
    a.min_aa = prm->min_aa; a.max_aa = prm->max_aa;
    uint64_t *meta = w.meta.as<uint64_t>(), *part = w.partials.as<uint64_t>();
    const dim3 tiles((uint32_t)cap_tiles);
    hipLaunchKernelGGL(k_orf_rec_tiles, dim3(1), dim3(1024), 0, c->stream, rs, rl, n_rec, 4 * seq_bytes, cap_tiles, w.rtoff.as<uint64_t>(), meta);
    hipLaunchKernelGGL(k_orf_tile<ORF_STOPS>, tiles, dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL(k_orf_scan_reduce<true>, dim3((uint32_t)cap_blocks, 6), dim3(256), 0, c->stream, a.stops, cap_tiles, meta, part, cap_blocks);
    hipLaunchKernelGGL(k_orf_scan_partials<true>, dim3(6), dim3(1024), 0, c->stream, part, cap_blocks, cap_tiles, meta, (uint64_t *)nullptr);
    hipLaunchKernelGGL(k_orf_scan_apply<true>, dim3((uint32_t)cap_blocks, 6), dim3(256), 0, c->stream, a.stops, cap_tiles, meta, part, cap_blocks);
    hipLaunchKernelGGL(k_orf_tile<ORF_COUNT>, tiles, dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL(k_orf_scan_reduce<false>, dim3((uint32_t)cap_blocks, 3), dim3(256), 0, c->stream, a.counts, cap_tiles, meta, part, cap_blocks);
    hipLaunchKernelGGL(k_orf_scan_partials<false>, dim3(3), dim3(1024), 0, c->stream, part, cap_blocks, cap_tiles, meta, meta + ORF_META_N_ORF);
    hipLaunchKernelGGL(k_orf_scan_apply<false>, dim3((uint32_t)cap_blocks, 3), dim3(256), 0, c->stream, a.counts, cap_tiles, meta, part, cap_blocks);
    GS_HIP_CHECK(hipGetLastError());
    uint64_t h[5];
    GS_HIP_CHECK(hipMemcpyAsync(h, meta, sizeof h, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    GS_REQUIRE(!(h[ORF_META_ERR] & ORF_ERR_RANGE), GS_ERR_INVALID, "orf: a record does not lie inside the %llu bytes of seq", (unsigned long long)seq_bytes);
    GS_REQUIRE(!(h[ORF_META_ERR] & ORF_ERR_TILES), GS_ERR_INVALID, "orf: the records overlap (their bases are more than seq holds)");
    n_out[0] = h[ORF_META_N_ORF]; n_out[1] = h[ORF_META_N_AA]; n_out[2] = h[ORF_META_N_LONG];
    return GS_OK;
}
// queued on c's stream behind orf_count; nothing is waited for
int orf_emit(gs_ctx *c, uint64_t n_rec, OrfWork &w, gs_orf *orf, uint8_t *aa, uint64_t *aa_start, uint64_t *aa_len, uint64_t *rec_orf_off)
{
    OrfArgs &a = w.a;
    a.orf = orf; a.aa = aa; a.aa_start = aa_start; a.aa_len = aa_len;
    hipLaunchKernelGGL(k_orf_rec_off, dim3((uint32_t)(n_rec / 256 + 1)), dim3(256), 0, c->stream, a.rtoff, a.counts, a.meta, n_rec, rec_orf_off);
    hipLaunchKernelGGL(k_orf_tile<ORF_EMIT>, dim3((uint32_t)a.cap_tiles), dim3(64), 0, c->stream, a);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

}  // namespace gs

int gs_orf_codon_table(uint32_t table, char out[64])
{
    GS_REQUIRE(out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(table == 11 || table == 4, GS_ERR_UNSUPPORTED, "orf: translation table %u (11 and 4 are there)", table);
    memcpy(out, table == 11 ? GS_ORF_TABLE_11 : GS_ORF_TABLE_4, 64);
    return GS_OK;
}

int gs_orf_translate_dev(gs_ctx *c, const gs_orf_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev,
                         uint64_t n_rec, uint64_t cap_orf, uint64_t cap_aa, gs_orf *orf_out_dev, uint8_t *aa_out_dev, uint64_t *aa_start_out_dev, uint64_t *aa_len_out_dev,
                         uint64_t *rec_orf_off_out_dev, uint64_t n_out[3])
{
    using namespace gs;
    GS_REQUIRE(c && n_out, GS_ERR_INVALID, "null argument");
    int rc;
    bool count_only;
    if ((rc = orf_check_params(prm, n_rec)) ||
        (rc = orf_check_outputs(cap_orf, cap_aa, orf_out_dev, aa_out_dev, aa_start_out_dev, aa_len_out_dev, rec_orf_off_out_dev, &count_only)))
        return rc;
    GS_REQUIRE(n_rec == 0 || (rec_start_dev && rec_len_dev), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(seq_dev || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_CTX_LOCK(c);
    OrfWork w(c);
    if ((rc = orf_count(c, prm, (const uint8_t *)seq_dev, seq_bytes, rec_start_dev, rec_len_dev, n_rec, w, n_out))) return rc;
    if (count_only) return GS_OK;
    if ((rc = orf_check_caps(n_out, cap_orf, cap_aa))) return rc;
    return orf_emit(c, n_rec, w, orf_out_dev, aa_out_dev, aa_start_out_dev, aa_len_out_dev, rec_orf_off_out_dev);
}

int gs_orf_translate(gs_ctx *c, const gs_orf_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                     uint64_t cap_orf, uint64_t cap_aa, gs_orf *orf_out, uint8_t *aa_out, uint64_t *aa_start_out, uint64_t *aa_len_out, uint64_t *rec_orf_off_out,
                     uint64_t n_out[3])
{
    using namespace gs;
    GS_REQUIRE(c && n_out, GS_ERR_INVALID, "null argument");
    int rc;
    bool count_only;
    if ((rc = orf_check_params(prm, n_rec)) || (rc = orf_check_outputs(cap_orf, cap_aa, orf_out, aa_out, aa_start_out, aa_len_out, rec_orf_off_out, &count_only))) return rc;
    GS_REQUIRE(n_rec == 0 || (rec_start && rec_len), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(seq || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_CTX_LOCK(c);
    PoolBuf d_seq(c, SL_ORFB_SEQ), d_rs(c, SL_ORFB_REC_START), d_rl(c, SL_ORFB_REC_LEN);
    if ((rc = d_seq.alloc(seq_bytes)) || (rc = d_rs.alloc(8 * n_rec)) || (rc = d_rl.alloc(8 * n_rec))) return rc;
    if (seq_bytes) GS_HIP_CHECK(hipMemcpyAsync(d_seq.p, seq, seq_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_rec) {
        GS_HIP_CHECK(hipMemcpyAsync(d_rs.p, rec_start, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(d_rl.p, rec_len, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
    }
    OrfWork w(c);
    if ((rc = orf_count(c, prm, d_seq.as<uint8_t>(), seq_bytes, d_rs.as<uint64_t>(), d_rl.as<uint64_t>(), n_rec, w, n_out))) return rc;
    if (count_only) return GS_OK;
    if ((rc = orf_check_caps(n_out, cap_orf, cap_aa))) return rc;
    const uint64_t no = n_out[0], na = n_out[1];
    PoolBuf d_orf(c, SL_ORFB_ORF), d_aa(c, SL_ORFB_AA), d_as(c, SL_ORFB_AA_START), d_al(c, SL_ORFB_AA_LEN), d_off(c, SL_ORFB_REC_OFF);
    if ((rc = d_orf.alloc(sizeof(gs_orf) * no)) || (rc = d_aa.alloc(na)) || (rc = d_as.alloc(8 * no)) || (rc = d_al.alloc(8 * no)) || (rc = d_off.alloc(8 * (n_rec + 1)))) return rc;
    if ((rc = orf_emit(c, n_rec, w, d_orf.as<gs_orf>(), d_aa.as<uint8_t>(), d_as.as<uint64_t>(), d_al.as<uint64_t>(), d_off.as<uint64_t>()))) return rc;
    if (no) {
        GS_HIP_CHECK(hipMemcpyAsync(orf_out, d_orf.p, sizeof(gs_orf) * no, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(aa_start_out, d_as.p, 8 * no, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(aa_len_out, d_al.p, 8 * no, hipMemcpyDeviceToHost, c->stream));
    }
    if (na) GS_HIP_CHECK(hipMemcpyAsync(aa_out, d_aa.p, na, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(rec_orf_off_out, d_off.p, 8 * (n_rec + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}
