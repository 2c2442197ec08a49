// gs_prob.hip — the ProbMinHash3a sketcher (SPEC 3.3) on gfx950: its kernels, its three host forms (tiered, bucketed, sorted) and their driver run_prob,
// the one entry point (gs_internal.hpp; called by sketch_dev_impl of gs_sketch.hip). The k-mer walkers are those of every sketcher (gs_walk.hpp).
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <optional>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"
#include "gs_walk.hpp"

namespace gs {

// =====================================================================================================
// prob (ProbMinHash3a, SPEC 3.3): multiset of canonical k-mers -> weighted per-slot argmin of (h, v).
//   1. every k-mer value is written to a buffer (composite key = genome-in-chunk << vbits | value), one global radix sort,
//      run-length encode -> distinct elements with their multiplicity w;
//   2. pass i = 1,2,..: every element still alive (w^-1 (i-1) <= max_b q[b]) replays its generator up to its i-th point
//      h = w^-1 (i-1) + w^-1 TE, slot b, and atomically lowers q[b]; the winners (h == q[b]) then race for the smallest v.
//      At genome sizes of interest all m slots are filled in pass 1 and only k-mers repeated >~ 30 times see pass 2.
// The result is the exact per-slot argmin of SPEC 3.3 (pruning is sound in any order).
// =====================================================================================================
struct ProbConst { double lambda, c1, c2, c3; };
__device__ __forceinline__ double em1_spec(double z)
{
    double t = 1.0 + z / 6.0;
    t = 1.0 + (z / 5.0) * t;
    t = 1.0 + (z / 4.0) * t;
    t = 1.0 + (z / 3.0) * t;
    t = 1.0 + (z / 2.0) * t;
    return z * t;
}
__device__ __forceinline__ double texp_sample(const ProbConst &t, Rng &g)
{
    double x = t.c1 * g.u64f();
    if (x < 1.0) return x;
    for (;;) {
        x = g.u64f();
        if (x < t.c2) return x;
        double y = 0.5 * g.u64f();
        if (y > 1.0 - x) { x = 1.0 - x; y = 1.0 - y; }
        if (x <= t.c3 * (1.0 - y)) return x;
        if (y * t.c1 <= 1.0 - x) return x;
        if ((y * t.c1) * t.lambda <= em1_spec(t.lambda * (1.0 - x))) return x;
    }
}
#define GS_INF_BITS 0x7FF0000000000000ULL

// k-mers per record -> exclusive prefix inside each genome
__global__ void k_kmer_prefix(const uint64_t *rec_len, const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t k, uint64_t *rec_kpre, uint64_t *gen_kmers)
{
    const uint64_t g = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);       // one wavefront per genome
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1];
    uint64_t base = 0;
    for (uint64_t rb = r0; rb < r1; rb += 64) {
        const uint64_t r = rb + lane;
        uint64_t u = 0;
        if (r < r1) { const uint64_t len = rec_len[r]; if (len >= k) u = len - k + 1; }
        uint64_t inc = u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
        if (r < r1) rec_kpre[r] = base + inc - u;
        base += __shfl(inc, 63);
    }
    if (lane == 0) gen_kmers[g] = base;
}
struct ValueEmit {
    uint64_t *out; const uint64_t *rec_start; const uint64_t *rec_kpre; uint64_t base; uint64_t tag; uint32_t k;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t rec, uint64_t pos) const
    {
        out[base + rec_kpre[rec] + (pos - rec_start[rec] - (k - 1))] = tag | v;
    }
};
template <bool AA>
__global__ __launch_bounds__(SK_THREADS) void k_emit_values(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                             const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ rec_kpre,
                                                             const uint64_t *__restrict__ genome_rec_off, const uint64_t *__restrict__ gen_units,
                                                             const uint64_t *__restrict__ gen_base, uint64_t g0, uint32_t k, uint32_t vbits, uint64_t *__restrict__ out)
{
    const uint64_t gl = blockIdx.y, g = g0 + gl;
    ValueEmit emit{out, rec_start, rec_kpre, gen_base[gl], vbits >= 64 ? 0 : (gl << vbits), kq_k(k)};
    walk_genome<AA>(seq, rec_start, rec_len, rec_upre, genome_rec_off[g], genome_rec_off[g + 1], gen_units[g], k, blockIdx.x, gridDim.x, emit);
}
__global__ void k_prob_init(uint64_t *q, uint64_t *qprev, uint64_t *sig, uint64_t *sigpass, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        q[i] = GS_INF_BITS; qprev[i] = GS_INF_BITS; sig[i] = ~(uint64_t)0; sigpass[i] = ~(uint64_t)0;
    }
}
// pass `it`, phase A: i-th point of every live element -> q[b] = min
__global__ void k_prob_point(const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ ucnt, uint64_t ne, uint32_t vbits, uint32_t m, uint64_t zone,
                             ProbConst pc, uint32_t it, const double *__restrict__ qmax, uint64_t *__restrict__ q, uint64_t *__restrict__ cand_h,
                             uint32_t *__restrict__ cand_b, uint32_t *__restrict__ wmax)
{
    const uint64_t vmask = vbits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << vbits) - 1);
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = ukey[e];
        const uint64_t gl = vbits >= 64 ? 0 : (key >> vbits), v = key & vmask;
        // largest multiplicity per genome (pass 1 only): read first - hundreds of millions of elements, a few hundred words; a stale
        // smaller value only costs a redundant atomic, unconditional atomics serialise on the same addresses
        if (wmax) { const uint32_t cnt = ucnt[e]; if (cnt > *(volatile uint32_t *)&wmax[gl]) atomicMax(&wmax[gl], cnt); }
        const double winv = 1.0 / (double)ucnt[e];
        const double base = winv * (double)(it - 1);
        uint32_t b = 0xFFFFFFFFu; uint64_t hb = 0;
        if (!(base > qmax[gl])) {
            Rng rg; rg.seed(v);                                 // prob: identity element hash (SPEC 2)
            double x = 0;
            for (uint32_t t = 0; t < it; t++) { x = texp_sample(pc, rg); b = (uint32_t)rng_uint(rg, (uint64_t)m, zone); }
            const double h = base + winv * x;
            hb = (uint64_t)__double_as_longlong(h);             // h >= 0: the bit pattern orders like the value
            uint64_t *slot = q + gl * (uint64_t)m + b;
            if (hb < *slot) atomicMin((unsigned long long *)slot, (unsigned long long)hb);
        }
        cand_b[e] = b; cand_h[e] = hb;
    }
}
// after pass 1: elements that can still reach a slot (w^-1 <= max q) are compacted into a list with their generator state,
// so that later passes touch only them and never replay
__global__ void k_prob_compact(const uint64_t *__restrict__ ukey, const uint32_t *__restrict__ ucnt, uint64_t ne, uint32_t vbits, uint32_t m, uint64_t zone,
                               ProbConst pc, const double *__restrict__ qmax, uint32_t cap, uint32_t *__restrict__ n_act, uint64_t *__restrict__ akey,
                               uint32_t *__restrict__ acnt, uint64_t *__restrict__ astate)
{
    const uint64_t vmask = vbits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << vbits) - 1);
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = ukey[e];
        const uint64_t gl = vbits >= 64 ? 0 : (key >> vbits);
        const double winv = 1.0 / (double)ucnt[e];
        if (winv * 1.0 > qmax[gl]) continue;
        const uint32_t pos = atomicAdd(n_act, 1u);
        if (pos >= cap) continue;                                  // overflow: the host falls back to replay mode
        Rng rg; rg.seed(key & vmask);
        (void)texp_sample(pc, rg); (void)rng_uint(rg, (uint64_t)m, zone);
        akey[pos] = key; acnt[pos] = ucnt[e];
        astate[pos] = rg.s0; astate[(uint64_t)cap + pos] = rg.s1; astate[2 * (uint64_t)cap + pos] = rg.s2; astate[3 * (uint64_t)cap + pos] = rg.s3;
    }
}
__global__ void k_prob_point_list(const uint64_t *__restrict__ akey, const uint32_t *__restrict__ acnt, uint32_t na, uint32_t cap, uint32_t vbits, uint32_t m,
                                  uint64_t zone, ProbConst pc, uint32_t it, const double *__restrict__ qmax, uint64_t *__restrict__ q, uint64_t *__restrict__ astate,
                                  uint64_t *__restrict__ cand_h, uint32_t *__restrict__ cand_b)
{
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < na; e += gridDim.x * blockDim.x) {
        const uint64_t key = akey[e];
        const uint64_t gl = vbits >= 64 ? 0 : (key >> vbits);
        const double winv = 1.0 / (double)acnt[e];
        const double base = winv * (double)(it - 1);
        uint32_t b = 0xFFFFFFFFu; uint64_t hb = 0;
        if (!(base > qmax[gl])) {
            Rng rg; rg.s0 = astate[e]; rg.s1 = astate[(uint64_t)cap + e]; rg.s2 = astate[2 * (uint64_t)cap + e]; rg.s3 = astate[3 * (uint64_t)cap + e];
            const double x = texp_sample(pc, rg);
            b = (uint32_t)rng_uint(rg, (uint64_t)m, zone);
            astate[e] = rg.s0; astate[(uint64_t)cap + e] = rg.s1; astate[2 * (uint64_t)cap + e] = rg.s2; astate[3 * (uint64_t)cap + e] = rg.s3;
            const double h = base + winv * x;
            hb = (uint64_t)__double_as_longlong(h);
            uint64_t *slot = q + gl * (uint64_t)m + b;
            if (hb < *slot) atomicMin((unsigned long long *)slot, (unsigned long long)hb);
        }
        cand_b[e] = b; cand_h[e] = hb;
    }
}
// phase B: among the points that reached the slot minimum the smallest value wins
__global__ void k_prob_claim(const uint64_t *__restrict__ ukey, uint64_t ne, uint32_t vbits, uint32_t m, const uint64_t *__restrict__ q,
                             const uint64_t *__restrict__ cand_h, const uint32_t *__restrict__ cand_b, uint64_t *__restrict__ sigpass)
{
    const uint64_t vmask = vbits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << vbits) - 1);
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = cand_b[e];
        if (b == 0xFFFFFFFFu) continue;
        const uint64_t key = ukey[e], gl = vbits >= 64 ? 0 : (key >> vbits);
        if (cand_h[e] == q[gl * (uint64_t)m + b]) atomicMin((unsigned long long *)&sigpass[gl * (uint64_t)m + b], (unsigned long long)(key & vmask));
    }
}
// The rule that keeps the pass loop going, for the device (k_prob_fold) and the host (prob_retire_flagged) alike: after pass `it` a genome whose largest multiplicity is w
// and whose largest slot minimum is qm is still active when the next point of some element, w^-1 it at the least, is not above qm. w == 0: no k-mers, or retired.
__host__ __device__ __forceinline__ bool prob_still_active(uint32_t w, uint32_t it, double qm) { return w > 0 && !((1.0 / (double)w) * (double)it > qm); }
// phase C (one workgroup per genome): fold the pass winners into sig, recompute max_b q[b], decide whether the genome is done
__global__ __launch_bounds__(256) void k_prob_fold(uint32_t m, uint32_t it, uint64_t *__restrict__ q, uint64_t *__restrict__ qprev, uint64_t *__restrict__ sig,
                                                    uint64_t *__restrict__ sigpass, const uint32_t *__restrict__ wmax, double *__restrict__ qmax,
                                                    uint32_t *__restrict__ n_active)
{
    __shared__ unsigned long long s_max;
    const uint64_t g = blockIdx.x;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    unsigned long long loc = 0;
    for (uint32_t b = threadIdx.x; b < m; b += blockDim.x) {
        const uint64_t i = g * (uint64_t)m + b;
        const uint64_t sp = sigpass[i], qq = q[i];
        if (sp != ~(uint64_t)0) { if (qq != qprev[i]) sig[i] = sp; else if (sp < sig[i]) sig[i] = sp; sigpass[i] = ~(uint64_t)0; }
        qprev[i] = qq;
        if (qq > loc) loc = qq;
    }
    atomicMax(&s_max, loc);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double qm = __longlong_as_double((long long)s_max);
        qmax[g] = qm;
        const uint32_t w = wmax[g];
        if (prob_still_active(w, it, qm)) atomicAdd(n_active, 1u);      // some element may still reach a slot in pass it+1
    }
}
template <typename T>
__global__ void k_prob_write(const uint64_t *__restrict__ q, const uint64_t *__restrict__ sig, uint64_t n, T *__restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = q[i] == GS_INF_BITS ? (T)0 : (T)sig[i];
}

// =====================================================================================================
// prob, bucketed form (round 3; DESIGN.md 3.1 "ProbMinHash3a"). The global 64-bit radix sort above moves every k-mer across HBM ~14
// times only to learn multiplicities. Here a genome's k-mers are PARTITIONED once by the top bits of a multiplicative hash into
// buckets of ~PB_AVG values (count pass -> exact offsets -> scatter pass: two cheap walks, 8 B written per k-mer), and each bucket is
// then turned into (value, multiplicity) pairs by an LDS hash table (one 64-bit LDS CAS per k-mer) inside the kernel that also
// evaluates the first ProbMinHash point of every distinct element - so the k-mers cross HBM three times (read text, write bucket,
// read bucket).
//   k_prob_count    per (genome, part): bucket histogram in LDS; the first tile of every part also applies its k-mers to q[] with
//                   w = 1: x / 1 >= x / w, so those are UPPER bounds of the final slot minima (the true points arrive later and can
//                   only be lower) - they give the bucket kernel a finite rejection threshold from its first bucket on
//   k_prob_scan     per genome: bucket offsets, per-part scatter bases, thr = max_b q[b]
//   k_prob_scatter  per (genome, part): the same walk, values appended to their buckets through LDS cursors (no global atomics)
//   k_prob_buckets  persistent workgroups over all buckets of the chunk: LDS hash -> (v, w); an element whose first point
//                   h = w^-1 TE exceeds thr (any snapshot of max_b q[b] bounds the final one) cannot win a slot and stops after two
//                   SplitMix64 mixes (exact: strict >, ties must reach the claim); the rest lower q[b] and, when they are the slot's
//                   minimum at that moment, go on a short candidate list; elements with w^-1 <= thr may see pass 2 and go on the
//                   active list with their generator state
//   k_prob_claim_list + k_prob_fold as before; passes >= 2 run over the active list only.
// Genomes the scheme does not suit fall back to the sorted form above: fewer than 64 k-mers per slot (no warm-up: every element stays
// alive for many passes), more than PB_NBMAX * PB_AVG k-mers, or a bucket with more than PB_TAB distinct values (flagged on the device).
// =====================================================================================================
constexpr int PBK_T = 1024;        // lanes of the count / scatter kernels
constexpr int PBK_WPL = 4;         // units per lane per tile
constexpr int PB2_T = 512;         // lanes of the bucket kernel
constexpr int PB_AVG = 1536;       // k-mers per bucket aimed at
constexpr int PB_TAB = 4096;       // LDS hash entries per bucket
constexpr int PB_NBMAX = 16384;    // buckets per genome (LDS cursors of the scatter kernel: 64 kB)
constexpr int PB_CST = 256;        // candidate winners staged per bucket
constexpr int PB_SVQ = 3072;       // elements (table slots) queued for the full generator per bucket
// The bucket of a value comes from a BIJECTION of the vbits-bit values (multiplication by an odd constant modulo 2^vbits): bucket = its top
// lg bits, and the low sh = vbits - lg bits identify the value inside its bucket - 30 bits for k = 21 with 4096 buckets, so the bucket
// kernel's hash table holds 4-byte ids instead of 8-byte values (half the LDS, full-rate 32-bit LDS atomics) and gets the value back by
// multiplying with the inverse constant.
#define GS_PB_MUL 0x9E3779B97F4A7C15ULL
constexpr uint64_t pb_inverse(uint64_t a) { uint64_t x = a; for (int i = 0; i < 6; i++) x *= 2 - a * x; return x; }      // Newton: a odd, inverse modulo 2^64
constexpr uint64_t GS_PB_INV = pb_inverse(GS_PB_MUL);
static_assert(GS_PB_MUL * GS_PB_INV == 1ULL, "modular inverse");
__device__ __forceinline__ uint64_t pb_hash(uint64_t v, uint64_t vmask) { return (v * GS_PB_MUL) & vmask; }
__device__ __forceinline__ uint64_t pb_unhash(uint64_t hv, uint64_t vmask) { return (hv * GS_PB_INV) & vmask; }
__device__ __forceinline__ uint32_t pb_bucket(uint64_t v, uint64_t vmask, uint32_t sh) { return sh >= 64 ? 0u : (uint32_t)(pb_hash(v, vmask) >> sh); }
struct PbCountEmit {
    uint32_t *hist; uint32_t sh; uint64_t vmask;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const { atomicAdd(&hist[pb_bucket(v, vmask, sh)], 1u); }
};
struct PbWarmEmit {
    uint32_t *hist; uint32_t sh; uint64_t vmask; uint64_t *q; uint32_t m; uint64_t zone; ProbConst pc;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const
    {
        atomicAdd(&hist[pb_bucket(v, vmask, sh)], 1u);
        Rng rg; rg.seed(v);
        const double x = texp_sample(pc, rg);
        const uint32_t b = (uint32_t)rng_uint(rg, (uint64_t)m, zone);
        const uint64_t hb = (uint64_t)__double_as_longlong(x);
        if (hb < q[b]) atomicMin((unsigned long long *)&q[b], (unsigned long long)hb);
    }
};
struct PbScatterEmit {
    uint32_t *cur; uint32_t sh; uint64_t vmask; uint64_t *out;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const { out[atomicAdd(&cur[pb_bucket(v, vmask, sh)], 1u)] = v; }
};
// MODE 0: count (+ warm-up on the first tile), MODE 1: scatter
template <bool AA, int MODE>
__global__ __launch_bounds__(PBK_T) void k_prob_partition(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                           const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off, const uint64_t *__restrict__ gen_units,
                                                           uint64_t g0, uint32_t kq, uint32_t vbits, const uint32_t *__restrict__ g_sh, const uint32_t *__restrict__ g_boff, uint32_t parts,
                                                           uint32_t *__restrict__ hist, uint64_t *__restrict__ q, uint32_t m, uint64_t zone, ProbConst pc,
                                                           uint64_t *__restrict__ vals, const uint64_t *__restrict__ g_vbase)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pb[];
    const uint32_t gl = blockIdx.y, part = blockIdx.x;
    const uint64_t g = g0 + gl;
    const uint32_t sh = g_sh[gl], NB = 1u << (vbits - sh);        // sh = vbits - log2(NB): bits of a hashed value below its bucket number
    uint32_t *hg = hist + (uint64_t)g_boff[gl] * parts + (uint64_t)part * NB;
    for (uint32_t b = threadIdx.x; b < NB; b += PBK_T) s_pb[b] = MODE == 0 ? 0u : hg[b];
    __syncthreads();
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1], units = gen_units[g];
    const uint32_t k = kq_k(kq);
    const uint64_t mask = kmer_mask(AA, k), rc_or = kq_rc_or(kq);
    const uint32_t rcshift = 2 * (k - 1);
    const uint64_t TILE = (uint64_t)PBK_T * PBK_WPL;
    for (uint64_t t0 = (uint64_t)part * TILE; t0 < units; t0 += (uint64_t)parts * TILE) {
#pragma unroll 1
        for (int j = 0; j < PBK_WPL; j++) {
            const uint64_t f = t0 + (uint64_t)j * PBK_T + threadIdx.x;
            if (f >= units) continue;
            if (MODE == 0) {
                if (t0 == (uint64_t)part * TILE) { PbWarmEmit e{s_pb, sh, mask, q + (uint64_t)gl * m, m, zone, pc}; walk_unit<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, f, k, mask, rcshift, rc_or, e); }
                else { PbCountEmit e{s_pb, sh, mask}; walk_unit<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, f, k, mask, rcshift, rc_or, e); }
            } else { PbScatterEmit e{s_pb, sh, mask, vals + g_vbase[gl]}; walk_unit<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, f, k, mask, rcshift, rc_or, e); }
        }
    }
    if (MODE == 0) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < NB; b += PBK_T) hg[b] = s_pb[b];
    }
}
// per genome: bucket sizes / starts, per-part scatter bases (hist is rewritten in place), thr = max_b q[b]
// Two-level form (g_shc != nullptr): the scatter goes through COARSE buckets first (the top lgc = lg / 2 bits of the bucket number, k_prob_partition<., 1> with
// these shifts and bases) and k_prob_refine spreads every (coarse bucket, part) slice over its fine buckets. Here: ccur[part][c] = where part `part` writes its
// values of coarse bucket c (coarse bucket c starts where its first fine bucket does; inside it the parts follow each other), ccnt = how many.
constexpr uint32_t PB_CCMAX = 8192;                            // parts x coarse buckets of a genome that the scan kernel can total in LDS
__global__ __launch_bounds__(1024) void k_prob_scan(uint32_t vbits, const uint32_t *__restrict__ g_sh, const uint32_t *__restrict__ g_boff, uint32_t parts, uint32_t *__restrict__ hist,
                                                     uint32_t *__restrict__ bstart, uint32_t *__restrict__ bsize, uint32_t *__restrict__ bgen, const uint64_t *__restrict__ q, uint32_t m,
                                                     uint64_t *__restrict__ thr, const uint32_t *__restrict__ g_shc, const uint32_t *__restrict__ g_coff, uint32_t *__restrict__ ccur,
                                                     uint32_t *__restrict__ ccnt)
{
    __shared__ uint32_t s_w[16]; __shared__ unsigned long long s_mx;
    __shared__ uint32_t s_cc[PB_CCMAX], s_cs[256];
    const uint32_t gl = blockIdx.x, sh = g_sh[gl], NB = 1u << (vbits - sh);
    const uint32_t b0 = g_boff[gl];
    uint32_t *hg = hist + (uint64_t)b0 * parts;
    const uint32_t fsh = g_shc ? g_shc[gl] - sh : 0, NC = NB >> fsh;      // fine buckets per coarse one = 1 << fsh
    if (g_shc) { for (uint32_t i = threadIdx.x; i < parts * NC; i += 1024) s_cc[i] = 0; }
    const uint32_t CH = (NB + 1023) / 1024;                    // consecutive buckets per lane
    uint32_t loc = 0;
    for (uint32_t c = 0; c < CH; c++) { const uint32_t b = threadIdx.x * CH + c; if (b < NB) for (uint32_t p = 0; p < parts; p++) loc += hg[(uint64_t)p * NB + b]; }
    uint32_t inc = loc;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
    if (lane == 63) s_w[wv] = inc;
    if (threadIdx.x == 0) s_mx = 0;
    __syncthreads();
    uint32_t run = inc - loc;
    for (uint32_t w = 0; w < wv; w++) run += s_w[w];
    for (uint32_t c = 0; c < CH; c++) {
        const uint32_t b = threadIdx.x * CH + c;
        if (b >= NB) break;
        bstart[b0 + b] = run; bgen[b0 + b] = gl;
        if (g_shc && (b & ((1u << fsh) - 1u)) == 0) s_cs[b >> fsh] = run;
        uint32_t tot = 0;
        for (uint32_t p = 0; p < parts; p++) {
            const uint32_t x = hg[(uint64_t)p * NB + b]; hg[(uint64_t)p * NB + b] = run + tot; tot += x;
            if (g_shc && x) atomicAdd(&s_cc[p * NC + (b >> fsh)], x);
        }
        bsize[b0 + b] = tot; run += tot;
    }
    if (g_shc) {
        __syncthreads();
        const uint32_t c0 = g_coff[gl];
        for (uint32_t i = threadIdx.x; i < parts * NC; i += 1024) {
            const uint32_t p = i / NC, cb = i % NC;
            uint32_t base = s_cs[cb];
            for (uint32_t p2 = 0; p2 < p; p2++) base += s_cc[p2 * NC + cb];
            ccur[(uint64_t)c0 * parts + i] = base; ccnt[(uint64_t)c0 * parts + i] = s_cc[i];
        }
    }
    unsigned long long mx = 0;
    for (uint32_t i = threadIdx.x; i < m; i += 1024) { const unsigned long long x = q[(uint64_t)gl * m + i]; mx = x > mx ? x : mx; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
    if (lane == 0) atomicMax(&s_mx, mx);
    __syncthreads();
    if (threadIdx.x == 0) thr[gl] = s_mx;
}
// second level of the partition: one workgroup per (coarse bucket, part) slice of a genome. The slice is read front to back (coalesced) and each value is
// appended to its fine bucket through an LDS cursor that starts at that part's place in the bucket (the same per-(part, bucket) bases the one-level
// scatter used). A workgroup writes to at most 128 open streams of a few hundred consecutive values each: the L2 completes their lines before they are
// evicted, where the one-level scatter's 4096 streams per workgroup left it as 32-byte sector writes (WRITE_SIZE 3.9x the values, profiles/r03_prob_pmc.txt).
constexpr int PBR_T = 512, PBR_V = 8, PBR_TILE = PBR_T * PBR_V;
__global__ __launch_bounds__(PBR_T) void k_prob_refine(const uint64_t *__restrict__ tmp, uint64_t *__restrict__ vals, const uint64_t *__restrict__ g_vbase, uint32_t vbits,
                                                       const uint32_t *__restrict__ g_sh, const uint32_t *__restrict__ g_boff, const uint32_t *__restrict__ g_shc,
                                                       const uint32_t *__restrict__ g_coff, uint32_t parts, const uint32_t *__restrict__ hist, const uint32_t *__restrict__ ccur,
                                                       const uint32_t *__restrict__ ccnt, uint32_t store32)
{
    // store32: every genome's in-bucket id fits 4 bytes - the id (low sh bits of the hashed value) is what k_prob_buckets keeps in its table, so that is
    // what is written, element i of the chunk at ((uint32_t *)vals)[i]
    // a tile of 4096 values is counting-sorted by fine bucket in LDS and written out run by run: consecutive lanes store consecutive values of one
    // bucket (8-byte stores scattered over 64 streams were bound by the number of write requests, not by bytes: 8.7 ms per 1.3e9 values)
    __shared__ uint64_t s_val[PBR_TILE];
    __shared__ uint8_t s_bk[PBR_TILE];
    __shared__ uint32_t s_cur[256], s_cnt[256], s_start[256];
    const uint32_t gl = blockIdx.y, sh = g_sh[gl], shc = g_shc[gl], fsh = shc - sh, NB = 1u << (vbits - sh), NC = NB >> fsh, NF = 1u << fsh;
    const uint32_t cb = blockIdx.x / parts, part = blockIdx.x % parts;
    if (cb >= NC) return;
    const uint32_t *hg = hist + (uint64_t)g_boff[gl] * parts + (uint64_t)part * NB + (uint64_t)cb * NF;
    for (uint32_t f = threadIdx.x; f < NF; f += PBR_T) s_cur[f] = hg[f];
    const uint64_t ci = (uint64_t)g_coff[gl] * parts + (uint64_t)part * NC + cb;
    const uint32_t n = ccnt[ci];
    const uint64_t *src = tmp + g_vbase[gl] + ccur[ci];
    uint64_t *dst = vals + g_vbase[gl];
    uint32_t *dst32 = (uint32_t *)vals + g_vbase[gl];
    const uint64_t vmask = vbits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << vbits) - 1);
    const uint64_t idmask = sh >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << sh) - 1);
    for (uint32_t i0 = 0; i0 < n; i0 += PBR_TILE) {
        const uint32_t tn = n - i0 < (uint32_t)PBR_TILE ? n - i0 : (uint32_t)PBR_TILE;
        uint64_t v[PBR_V]; uint32_t f[PBR_V], rk[PBR_V];
#pragma unroll
        for (int u = 0; u < PBR_V; u++) { const uint32_t i = u * PBR_T + threadIdx.x; v[u] = i < tn ? src[i0 + i] : 0; }
        if (threadIdx.x < 256) s_cnt[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PBR_V; u++) {
            const uint32_t i = u * PBR_T + threadIdx.x;
            f[u] = pb_bucket(v[u], vmask, sh) & (NF - 1u);
            rk[u] = i < tn ? atomicAdd(&s_cnt[f[u]], 1u) : 0u;
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                   // exclusive prefix of the <= 256 bucket counts: four per lane of one wavefront
            uint32_t c4[4], loc = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) { c4[j] = s_cnt[threadIdx.x * 4 + j]; loc += c4[j]; }
            uint32_t inc = loc;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if ((int)threadIdx.x >= o) inc += y; }
            uint32_t run = inc - loc;
#pragma unroll
            for (int j = 0; j < 4; j++) { s_start[threadIdx.x * 4 + j] = run; run += c4[j]; }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PBR_V; u++) {
            const uint32_t i = u * PBR_T + threadIdx.x;
            if (i < tn) { const uint32_t pos = s_start[f[u]] + rk[u]; s_val[pos] = v[u]; s_bk[pos] = (uint8_t)f[u]; }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PBR_V; u++) {
            const uint32_t i = u * PBR_T + threadIdx.x;
            if (i < tn) {
                const uint32_t fb = s_bk[i]; const uint32_t at = s_cur[fb] + (i - s_start[fb]);
                if (store32) dst32[at] = (uint32_t)(pb_hash(s_val[i], vmask) & idmask); else dst[at] = s_val[i];
            }
        }
        __syncthreads();
        if (threadIdx.x < 256) s_cur[threadIdx.x] += s_cnt[threadIdx.x];
    }
}
struct PbLists {
    uint64_t *cand_v, *cand_h, *cand_gb; uint32_t cand_cap, ovf_cap; uint32_t *n_cand, *seg_n;      // [0, cand_cap): per-workgroup segments; [cand_cap, + ovf_cap): shared overflow
    uint64_t *akey; uint32_t *agl, *acnt; uint64_t *astate; uint32_t act_cap; uint32_t *n_act;
    unsigned long long *prof;                                     // GS_PROB_PROFILE: cycle stamps of workgroup 0 per phase (nullptr otherwise)
};
// KT = uint32_t: the table holds the sh-bit id of a value inside its bucket (sh <= 31 for every genome of the launch; ~0 = empty);
// KT = uint64_t: it holds the value itself (k = 32, AA k = 12, or genomes with so few buckets that an id needs 32 bits).
template <typename KT>
__global__ __launch_bounds__(PB2_T, 6) void k_prob_buckets(const uint64_t *__restrict__ vals, const uint64_t *__restrict__ g_vbase, const uint32_t *__restrict__ bstart,
                                                           const uint32_t *__restrict__ bsize, uint32_t vbits, const uint32_t *__restrict__ g_sh, const uint32_t *__restrict__ g_boff,
                                                           uint32_t ng, uint32_t lg_max, uint32_t m, uint64_t zone,
                                                           ProbConst pc, uint64_t *__restrict__ q, uint64_t *__restrict__ thr, uint32_t *__restrict__ wmax, PbLists L,
                                                           uint32_t *__restrict__ ovf, uint32_t stored32)
{
    // stored32 (KT = uint32_t only): the partition left the 4-byte in-bucket ids in `vals` (element i of the chunk at ((uint32_t *)vals)[i]) instead of
    // the 8-byte values - half the bytes written by the refinement and read here; the value comes back through the inverse multiplication
    // LDS per workgroup (4-byte ids): 16 kB table + 8 kB duplicate counts + 6 kB queue + 5 kB candidates = 35 kB. What the kernel spends
    // its time on (GS_PROB_PROFILE, cycles per bucket of 1220 keys on 512 lanes, before / after this form): LDS atomics of the insert
    // 6360 / see DESIGN (one 32-bit CAS per k-mer instead of a 64-bit CAS plus an add: the LDS pipeline is shared by the whole CU, so
    // residency does not help there), the cheap test 2930 (its two SplitMix64 mixes now run during the insert, under the LDS wait), the
    // threshold read 1390 (now fetched one bucket ahead), the few full points 4600 (global read + atomicMin latency).
    __shared__ KT tab[PB_TAB];
    __shared__ uint32_t dup[PB_TAB / 2];                          // 16-bit counts of the REPEATED occurrences, two per word (65535 saturates: flagged)
    __shared__ unsigned long long s_mx;
    // elements that pass the cheap threshold test are compacted into an LDS queue (of table slots) so that the full generator (truncated
    // exponential + uniform slot) runs on dense wavefronts; possible winners are staged too and go to this workgroup's PRIVATE segment
    // of the candidate list (no global counter: one bumped per candidate by thousands of lanes serialised in the L2)
    __shared__ uint16_t sv_s[PB_SVQ];
    __shared__ uint64_t sc_v[PB_CST], sc_h[PB_CST]; __shared__ uint32_t sc_b[PB_CST];
    __shared__ uint32_t s_nc, s_ns;
    const KT EMPTY = (KT)~(KT)0;
    const uint64_t EMPTY64 = ~(uint64_t)0;
    const uint64_t vmask = vbits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << vbits) - 1);
    constexpr int KPL = 6;                                        // keys per lane held in registers (buckets of up to KPL * PB2_T keys)
    const uint32_t seg = L.cand_cap / gridDim.x;                  // this workgroup's share of the candidate list
    uint32_t my_nc = 0;
    // Work items in BUCKET-major order over the chunk: (position j of 2^lg_max, genome) - a genome with fewer buckets takes part at every
    // (2^lg_max / NB)-th position. All genomes advance together, so a genome's buckets are spread over the whole launch and its
    // threshold has time to tighten (the first buckets see max_b q[b] of the warm-up, the last ones nearly the final one); genome-major
    // order had ~1000 workgroups finish a genome's 8192 buckets within microseconds of each other, all under the loosest bound.
    // The description of the item after this one (and its genome's threshold: a slightly older bound is still a bound) is fetched while
    // this one is worked on.
    const uint64_t n_items = (uint64_t)ng << lg_max;
    auto describe = [&](uint64_t idx, uint32_t &gl_, uint32_t &n_, uint32_t &st_, uint64_t &vb_, uint32_t &pos_, uint32_t &sh_, uint32_t &bk_, uint64_t &thr_) {
        n_ = 0; gl_ = 0; st_ = 0; vb_ = 0; pos_ = 1; sh_ = 0; bk_ = 0; thr_ = 0;
        if (idx >= n_items) return;
        const uint32_t j = (uint32_t)(idx / ng), g = (uint32_t)(idx % ng);
        const uint32_t sh = g_sh[g], lg = vbits - sh, rs = lg_max - lg;          // this genome has 2^lg buckets
        if (j & ((1u << rs) - 1u)) return;
        const uint32_t fb = g_boff[g] + (j >> rs);
        gl_ = g; n_ = bsize[fb]; st_ = bstart[fb]; vb_ = g_vbase[g]; pos_ = j; sh_ = sh; bk_ = j >> rs;
        thr_ = __hip_atomic_load(&thr[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    uint64_t item = blockIdx.x;
    uint32_t n_gl, n_n, n_st, n_pos, n_sh, n_bk; uint64_t n_vb, n_thr;
    describe(item, n_gl, n_n, n_st, n_vb, n_pos, n_sh, n_bk, n_thr);
    for (; item < n_items; item += gridDim.x) {
        const uint32_t gl = n_gl, n = n_n, jpos = n_pos, sh = n_sh, bk = n_bk;
        const uint64_t *keys = vals + n_vb + n_st;
        const uint32_t *keys32 = (const uint32_t *)vals + n_vb + n_st;
        const bool st32 = sizeof(KT) == 4 && stored32;
        uint64_t *qg = q + (uint64_t)gl * m;
        uint64_t thr_b = n_thr;
        uint64_t kreg[KPL];
#pragma unroll
        for (int u = 0; u < KPL; u++) { const uint32_t i = u * PB2_T + threadIdx.x; kreg[u] = i < n ? (st32 ? (uint64_t)keys32[i] : keys[i]) : EMPTY64; }      // st32: the id, for now
        describe(item + gridDim.x, n_gl, n_n, n_st, n_vb, n_pos, n_sh, n_bk, n_thr);
        if (n == 0) continue;                                      // (workgroup-uniform) nothing of this genome at this position
        const bool pf = L.prof && blockIdx.x == 0 && threadIdx.x == 0;
        long long t0 = pf ? clock64() : 0, t1;
#define GS_PSTAMP(i) do { if (pf) { t1 = clock64(); atomicAdd(&L.prof[i], (unsigned long long)(t1 - t0)); t0 = t1; } } while (0)
        __syncthreads();                                           // the previous bucket's LDS is dead
        for (uint32_t s = threadIdx.x; s < PB_TAB; s += PB2_T) tab[s] = EMPTY;
        for (uint32_t s = threadIdx.x; s < PB_TAB / 2; s += PB2_T) dup[s] = 0;
        if (threadIdx.x == 0) { s_nc = 0; s_ns = 0; s_mx = 0; }
        // rejection threshold: any snapshot of max_b q[b] bounds the final maximum (q only ever decreases). 32 times per genome a bucket
        // rescans the genome's q[] (m loads, eight in flight per lane) and publishes the new bound; everybody else reads the published one.
        if ((jpos & ((1u << (lg_max > 5 ? lg_max - 5 : 0)) - 1u)) == 0) {
            unsigned long long mx = 0;
            for (uint32_t i0 = 0; i0 < m; i0 += 8 * PB2_T) {
                unsigned long long x[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { const uint32_t i = i0 + u * PB2_T + threadIdx.x; x[u] = i < m ? __hip_atomic_load(&qg[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull; }
#pragma unroll
                for (int u = 0; u < 8; u++) mx = x[u] > mx ? x[u] : mx;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
            __syncthreads();
            if ((threadIdx.x & 63) == 0) atomicMax(&s_mx, mx);
            __syncthreads();
            const unsigned long long t = s_mx;
            if (threadIdx.x == 0) atomicMin((unsigned long long *)&thr[gl], t);
            if (t < thr_b) thr_b = t;
        }
        const double thr_d = __longlong_as_double((long long)thr_b);
        __syncthreads();
        GS_PSTAMP(0);
        // ---- (value, multiplicity) pairs: LDS hash table, ONE atomic per k-mer. The lane whose CAS created an entry OWNS that element
        //      (count 1); a later occurrence of the same value finds it there and bumps the entry's duplicate count instead (a second
        //      atomic, for repeats only). After the barrier the owners - dense over the lanes, unlike the 70 %-empty table - go on with
        //      multiplicity 1 + duplicates. The first draw of every key (two SplitMix64 mixes) is computed here, under the LDS wait.
        bool over = false;
        uint32_t own[KPL]; double x0r[KPL];
        const uint64_t idmask = sizeof(KT) == 4 ? (((uint64_t)1 << sh) - 1) : ~(uint64_t)0;
        auto insert_at = [&](KT id, uint32_t s) -> uint32_t {
            for (uint32_t probe = 0; probe < PB_TAB; probe++) {
                const KT old = atomicCAS(&tab[s], EMPTY, id);
                if (old == EMPTY) return s;
                if (old == id) {
                    const uint32_t before = atomicAdd(&dup[s >> 1], 1u << ((s & 1) * 16));
                    if (((before >> ((s & 1) * 16)) & 0xFFFFu) == 0xFFFFu) over = true;      // a k-mer 65537 times in one genome: 16 bits wrapped
                    return 0xFFFFFFFFu;
                }
                s = (s + 1) & (PB_TAB - 1);
            }
            over = true;
            return 0xFFFFFFFFu;
        };
        auto insert = [&](uint64_t v) -> uint32_t {
            const KT id = sizeof(KT) == 4 ? (KT)(pb_hash(v, vmask) & idmask) : (KT)v;
            return insert_at(id, (uint32_t)((v * 0xD6E8FEB86659FD93ULL) >> 40) & (PB_TAB - 1));
        };
        // stored ids: the table slot comes from the id's own top bits (inside a bucket the ids are a bijection of the values and the upper bits of a
        // multiplicative hash's window are its best mixed) - no second multiplication, and the value is only needed for the draw
        auto insert_id = [&](uint32_t id) -> uint32_t { return insert_at((KT)id, (sh > 12 ? id >> (sh - 12) : id) & (uint32_t)(PB_TAB - 1)); };
        auto first_draw = [&](uint64_t v) -> double {             // x = c1 * U64f from two of the four state words; when x < 1 it IS the truncated exponential (SPEC 3.3)
            const uint64_t s0 = splitmix_mix(v + GS_GAMMA), s3 = splitmix_mix(v + 4 * GS_GAMMA);
            return pc.c1 * ((double)((rotl64(s0 + s3, 23) + s0) >> 12) * 0x1.0p-52);
        };
#pragma unroll
        for (int u = 0; u < KPL; u++) {
            own[u] = 0xFFFFFFFFu; x0r[u] = 0.0;
            if ((uint32_t)(u * PB2_T) + threadIdx.x < n) {
                if (st32) { const uint32_t id = (uint32_t)kreg[u]; own[u] = insert_id(id); x0r[u] = first_draw(pb_unhash(((uint64_t)bk << sh) | (uint64_t)id, vmask)); }
                else { own[u] = insert(kreg[u]); x0r[u] = first_draw(kreg[u]); }
            }
        }
        // (buckets beyond KPL * PB2_T keys - heavy repeats - : the tail's owners are found by the table sweep below)
        const bool tail = n > (uint32_t)(KPL * PB2_T);
        for (uint32_t i = KPL * PB2_T + threadIdx.x; i < n; i += PB2_T) { if (st32) (void)insert_id(keys32[i]); else (void)insert(keys[i]); }
        if (over) ovf[gl] = 1;                                  // table full or a count wrapped: the host redoes this genome the sorted way
        __syncthreads();
        GS_PSTAMP(1);
        // ---- cheap test of every distinct element; the ones that may matter go to the queue
        uint32_t wloc = 0;
        auto count_of = [&](uint32_t s) -> uint32_t { return 1u + ((dup[s >> 1] >> ((s & 1) * 16)) & 0xFFFFu); };
        auto value_of = [&](uint32_t s) -> uint64_t {
            if (sizeof(KT) == 4) return pb_unhash(((uint64_t)bk << sh) | (uint64_t)tab[s], vmask);
            return (uint64_t)tab[s];
        };
        auto full_point = [&](uint32_t s) {
            const uint64_t v = value_of(s);
            const uint32_t w = count_of(s);
            const double winv = w == 1 ? 1.0 : 1.0 / (double)w;
            const bool alive2 = !(winv > thr_d);
            Rng rg; rg.seed(v);
            const double x = texp_sample(pc, rg);
            const uint32_t b = (uint32_t)rng_uint(rg, (uint64_t)m, zone);
            const double h = 0.0 + winv * x;
            if (!(h > thr_d)) {
                const uint64_t hb = (uint64_t)__double_as_longlong(h);
                uint64_t *slot = qg + b;
                if (hb <= __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    // not above the slot's minimum a moment ago: a possible winner. The atomicMin's answer is not waited for (a second memory round trip per
                    // bucket): whoever passes the read is listed - a superset of those the atomic would confirm, and the claim only takes candidates whose
                    // point equals the slot's final minimum
                    (void)__hip_atomic_fetch_min((unsigned long long *)slot, (unsigned long long)hb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t sp = atomicAdd(&s_nc, 1u);
                    if (sp < (uint32_t)PB_CST) { sc_v[sp] = v; sc_h[sp] = hb; sc_b[sp] = b; }
                    else {                                       // staging full (first buckets of a genome): the shared overflow region behind the segments
                        const uint32_t pos = atomicAdd(L.n_cand, 1u);
                        if (pos < L.ovf_cap) { const uint32_t o = L.cand_cap + pos; L.cand_v[o] = v; L.cand_h[o] = hb; L.cand_gb[o] = (uint64_t)gl * m + b; }
                    }
                }
            }
            if (alive2) {                                        // may still reach a slot in pass 2 (superset: thr >= the final max q)
                const uint32_t pos = atomicAdd(L.n_act, 1u);
                if (pos < L.act_cap) {
                    L.akey[pos] = v; L.agl[pos] = gl; L.acnt[pos] = w;
                    L.astate[pos] = rg.s0; L.astate[(uint64_t)L.act_cap + pos] = rg.s1; L.astate[2 * (uint64_t)L.act_cap + pos] = rg.s2; L.astate[3 * (uint64_t)L.act_cap + pos] = rg.s3;
                }
            }
        };
        auto cheap_test = [&](double x0, uint32_t s) {
            const uint32_t w = count_of(s);
            wloc = w > wloc ? w : wloc;
            const double winv = w == 1 ? 1.0 : 1.0 / (double)w;      // (1.0 / 1.0 is exact: the common case skips the f64 division)
            if (x0 < 1.0 && winv * x0 > thr_d && winv > thr_d) return;      // cannot win a slot (strict: ties must reach the claim), dead in pass 2
            const uint32_t sp = atomicAdd(&s_ns, 1u);
            if (sp < (uint32_t)PB_SVQ) sv_s[sp] = (uint16_t)s;
            else full_point(s);                                  // queue full (a first bucket under a loose threshold): straight away
        };
        if (!tail) {
#pragma unroll
            for (int u = 0; u < KPL; u++) if (own[u] != 0xFFFFFFFFu) cheap_test(x0r[u], own[u]);
        } else {
            for (uint32_t s = threadIdx.x; s < PB_TAB; s += PB2_T) if (tab[s] != EMPTY) cheap_test(first_draw(value_of(s)), s);
        }
        __syncthreads();
        GS_PSTAMP(2);
        const uint32_t ns = s_ns < (uint32_t)PB_SVQ ? s_ns : (uint32_t)PB_SVQ;
        if (pf) { atomicAdd(&L.prof[6], (unsigned long long)ns); atomicAdd(&L.prof[7], 1ull); atomicAdd(&L.prof[8], (unsigned long long)n); }
        for (uint32_t i = threadIdx.x; i < ns; i += PB2_T) full_point(sv_s[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)wloc, o); wloc = y > wloc ? y : wloc; }
        // (wmax starts at 1 for every genome of a bucketed chunk: the common all-unique bucket sends nothing; the read goes to the L2
        // like the atomics do - a plain load may come from a stale L1 line and would let every wave of every bucket send an atomic to
        // the same address)
        if ((threadIdx.x & 63) == 0 && wloc > 1 && wloc > __hip_atomic_load(&wmax[gl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&wmax[gl], wloc);
        __syncthreads();
        GS_PSTAMP(3);
        const uint32_t nst = s_nc < (uint32_t)PB_CST ? s_nc : (uint32_t)PB_CST;
        if (pf) atomicAdd(&L.prof[9], (unsigned long long)s_nc);
        if (nst) {
            if (my_nc + nst > seg) { if (threadIdx.x == 0) atomicMax(L.n_cand, 0xFFFFFFFFu); }       // segment full: the host redoes the chunk the sorted way
            else {
                const uint32_t cb = blockIdx.x * seg + my_nc;
                for (uint32_t i = threadIdx.x; i < nst; i += PB2_T) { L.cand_v[cb + i] = sc_v[i]; L.cand_h[cb + i] = sc_h[i]; L.cand_gb[cb + i] = (uint64_t)gl * m + sc_b[i]; }
                my_nc += nst;
            }
        }
        GS_PSTAMP(4);
#undef GS_PSTAMP
    }
    if (threadIdx.x == 0) L.seg_n[blockIdx.x] = my_nc;
}
__global__ void k_prob_claim_list(const uint64_t *__restrict__ cand_v, const uint64_t *__restrict__ cand_h, const uint64_t *__restrict__ cand_gb, const uint32_t *__restrict__ seg_n,
                                  uint32_t seg, uint32_t nseg, uint32_t cand_cap, const uint32_t *__restrict__ n_ovf, uint32_t ovf_cap, const uint64_t *__restrict__ q,
                                  uint64_t *__restrict__ sigpass)
{
    // one workgroup per segment (the bucket kernel's workgroups each filled their own), then the shared overflow region, dealt over all workgroups (it holds
    // the first buckets' candidates - every point is one while a slot is empty: millions, 13 ms when one workgroup walked them)
    for (uint32_t sgm = blockIdx.x; sgm < nseg; sgm += gridDim.x) {
        const uint32_t base = sgm * seg, n = seg_n[sgm];
        for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) {
            const uint64_t gb = cand_gb[base + e];
            if (cand_h[base + e] == q[gb]) atomicMin((unsigned long long *)&sigpass[gb], (unsigned long long)cand_v[base + e]);
        }
    }
    uint32_t n = *n_ovf;
    if (n > ovf_cap) n = ovf_cap;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const uint64_t gb = cand_gb[cand_cap + e];
        if (cand_h[cand_cap + e] == q[gb]) atomicMin((unsigned long long *)&sigpass[gb], (unsigned long long)cand_v[cand_cap + e]);
    }
}
// passes >= 2 over the active list (generator state carried from point to point)
__global__ void k_prob_point_act(const uint64_t *__restrict__ akey, const uint32_t *__restrict__ agl, const uint32_t *__restrict__ acnt, uint32_t na, uint32_t cap, uint32_t m,
                                 uint64_t zone, ProbConst pc, uint32_t it, const double *__restrict__ qmax, uint64_t *__restrict__ q, uint64_t *__restrict__ astate,
                                 uint64_t *__restrict__ cand_h, uint32_t *__restrict__ cand_b)
{
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < na; e += gridDim.x * blockDim.x) {
        const uint32_t gl = agl[e];
        const double winv = 1.0 / (double)acnt[e];
        const double base = winv * (double)(it - 1);
        uint32_t b = 0xFFFFFFFFu; uint64_t hb = 0;
        if (!(base > qmax[gl])) {
            Rng rg; rg.s0 = astate[e]; rg.s1 = astate[(uint64_t)cap + e]; rg.s2 = astate[2 * (uint64_t)cap + e]; rg.s3 = astate[3 * (uint64_t)cap + e];
            const double x = texp_sample(pc, rg);
            b = (uint32_t)rng_uint(rg, (uint64_t)m, zone);
            astate[e] = rg.s0; astate[(uint64_t)cap + e] = rg.s1; astate[2 * (uint64_t)cap + e] = rg.s2; astate[3 * (uint64_t)cap + e] = rg.s3;
            const double h = base + winv * x;
            hb = (uint64_t)__double_as_longlong(h);
            uint64_t *slot = q + (uint64_t)gl * m + b;
            if (hb < *slot) atomicMin((unsigned long long *)slot, (unsigned long long)hb);
        }
        cand_b[e] = b; cand_h[e] = hb;
    }
}
__global__ void k_prob_claim_act(const uint64_t *__restrict__ akey, const uint32_t *__restrict__ agl, uint32_t na, uint32_t m, const uint64_t *__restrict__ q,
                                 const uint64_t *__restrict__ cand_h, const uint32_t *__restrict__ cand_b, uint64_t *__restrict__ sigpass)
{
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < na; e += gridDim.x * blockDim.x) {
        const uint32_t b = cand_b[e];
        if (b == 0xFFFFFFFFu) continue;
        const uint64_t gb = (uint64_t)agl[e] * m + b;
        if (cand_h[e] == q[gb]) atomicMin((unsigned long long *)&sigpass[gb], (unsigned long long)akey[e]);
    }
}

// =====================================================================================================
// prob, TIERED form (round 6; DESIGN.md 3.1 "ProbMinHash3a, tiers"). Two observations carry it:
//  (1) every copy of a k-mer v draws from the same RNG(H(v)), so its first truncated-exponential draw x1 is a property of the VALUE, and its smallest point
//      is h1 = x1 / w. With thr >= max_b q[b] (final), v can only matter when x1 <= w thr: a k-mer whose x1 lies in [T thr, (T + 1) thr) needs a multiplicity
//      above T to matter at all - at thr ~ 0.04 (5 Mbp, s = 18000) 96 % of the k-mers need w >= 2, 85 % need w >= 5.
//  (2) an UPPER bound c >= w is enough to drop such a k-mer (1 / c and the product are monotone in c, in IEEE arithmetic too), and a count-min cell - the sum
//      of the multiplicities of everything that shares the cell - is one: one non-returning 16-bit LDS add per k-mer instead of a CAS insert with probing.
// So a bucket is counted twice: pass A adds every k-mer to its count-min cell; pass B reads the cell, draws x1 and drops the k-mer when even c copies could
// not bring its first point under thr (nor keep it alive for pass 2: 1 / c > thr). What is not dropped - the ~thr fraction that matters as singletons, the
// real repeats, and the false alarms of shared cells - enters the exact LDS hash table (CAS + duplicate count, as in k_prob_buckets: ALL copies of a value
// see the same cell, so they enter or stay out together and the multiplicity is exact), and the table is swept by the cheap test / full generator of the
// bucketed form. thr starts at a SPECULATIVE cap (m / N)(ln m + c) per genome (total k-mers N: the point process has rate sum w = N whatever the repeats) and
// is verified afterwards: max_b q[b] <= cap proves that nothing dropped could have been a slot minimum (a dropped point lies above the cap, hence above a
// point that stayed in its slot); a genome that fails the check, overflows a slice or a table is redone by the bucketed form (exact fallback).
// The partition is ONE pass without a count pass: a workgroup walks its tiles of the genome twice (count, place), counting-sorts each tile of <= 32 768
// k-mers by bucket in LDS and appends run by run to its PRIVATE slice of every bucket (fixed capacity: mean + 5 sigma; an overflow flags the genome) - 4 bytes
// per k-mer cross HBM twice (the in-bucket id of a bijection of the values, pt_bucket / pt_value) where the two-level partition moved 8 + 8 + 4 + 4.
// =====================================================================================================
constexpr int PT_T = 1024;            // lanes of the partition kernel = units (32 symbols) per tile
constexpr int PT_LGMAX = 11;          // buckets per genome <= 2048 (three LDS arrays of NB words beside the 128 kB tile)
constexpr int PT_AVG = 4096;          // k-mers per bucket aimed at (2048 .. 4096)
constexpr int PT_MINB = 256;          // fewer k-mers per bucket than this: the bucketed / sorted forms
constexpr int PT2_T = 512;            // lanes of the bucket kernel
constexpr int PT_CM = 8192;           // count-min cells per bucket (16 bits each)
constexpr int PT_Q = 1536;            // ids queued for the exact table per bucket
// The tiered form's bijection of the vbits-bit values is cheaper than pb_hash (one 32-bit multiplication instead of a 64-bit one - the bucket kernel undoes it
// once per k-mer and is bound by exactly these quarter-rate multiplications): id = the low sh bits of the value as they are, bucket = its top lg bits XOR a
// lg-bit hash of the id. Given (bucket, id) the top bits come back by the same XOR. Buckets are as even as the hash of the low 31 bits; whatever indexes a
// table by the id hashes it first (the raw low bits of a k-mer are its last bases).
__device__ __forceinline__ uint32_t pt_mix(uint32_t id, uint32_t lg) { return lg ? (id * 0x9E3779B1u) >> (32 - lg) : 0u; }
__device__ __forceinline__ uint32_t pt_bucket(uint64_t v, uint32_t sh, uint32_t lg, uint32_t idmask) { return (uint32_t)(v >> sh) ^ pt_mix((uint32_t)v & idmask, lg); }
__device__ __forceinline__ uint64_t pt_value(uint32_t bk, uint32_t id, uint32_t sh, uint32_t lg) { return ((uint64_t)(bk ^ pt_mix(id, lg)) << sh) | (uint64_t)id; }
struct PtCountEmit {
    uint32_t *cnt; uint32_t sh, lg, idmask;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const { atomicAdd(&cnt[pt_bucket(v, sh, lg, idmask)], 1u); }
};
struct PtPlaceEmit {
    uint32_t *pos, *ids; uint32_t sh, lg, idmask;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const { ids[atomicAdd(&pos[pt_bucket(v, sh, lg, idmask)], 1u)] = (uint32_t)v & idmask; }
};
// grid (parts, genomes of the chunk). vals32[g_vbase[gl] + (b * parts + part) * g_cap[gl] + i] = i-th id this part found for bucket b; cnt[(g_boff[gl] + b) * parts + part] = how many.
template <bool AA>
__global__ __launch_bounds__(PT_T) void k_prob_part1(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                     const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off, const uint64_t *__restrict__ gen_units,
                                                     uint64_t g0, uint32_t kq, uint32_t vbits, const uint32_t *__restrict__ g_sh, const uint32_t *__restrict__ g_boff,
                                                     const uint64_t *__restrict__ g_vbase, const uint32_t *__restrict__ g_cap, uint32_t parts, uint32_t *__restrict__ vals32,
                                                     uint32_t *__restrict__ cnt, uint32_t *__restrict__ ovf)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pt[];
    __shared__ uint32_t s_w[16];
    const uint32_t gl = blockIdx.y, part = blockIdx.x;
    const uint64_t g = g0 + gl;
    const uint32_t sh = g_sh[gl], NB = 1u << (vbits - sh), cap = g_cap[gl];
    uint32_t *s_cnt = s_pt, *s_start = s_pt + NB, *s_cur = s_pt + 2 * NB, *s_ids = s_pt + 3 * NB;       // s_cnt doubles as the placement cursor of walk B
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1], units = gen_units[g];
    const uint32_t k = kq_k(kq);
    const uint64_t mask = kmer_mask(AA, k), rc_or = kq_rc_or(kq);
    const uint32_t idmask = (uint32_t)(((uint64_t)1 << sh) - 1), lg = vbits - sh;      // sh <= 31
    const uint32_t rcshift = 2 * (k - 1);
    const uint64_t tiles = (units + PT_T - 1) / PT_T, t_lo = tiles * part / parts, t_hi = tiles * (part + 1) / parts;
    uint32_t *out = vals32 + g_vbase[gl];
    for (uint32_t b = threadIdx.x; b < NB; b += PT_T) s_cur[b] = 0;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t CH = NB > (uint32_t)PT_T ? NB / PT_T : 1u;     // consecutive buckets per lane in the prefix
    bool over = false;
    for (uint64_t t = t_lo; t < t_hi; t++) {
        for (uint32_t b = threadIdx.x; b < NB; b += PT_T) s_cnt[b] = 0;
        __syncthreads();
        const uint64_t f = t * PT_T + threadIdx.x;
        if (f < units) { PtCountEmit e{s_cnt, sh, lg, idmask}; walk_unit<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, f, k, mask, rcshift, rc_or, e); }
        __syncthreads();
        // exclusive prefix of the bucket counts -> s_start, and the cursors of walk B
        uint32_t loc = 0;
        for (uint32_t c = 0; c < CH; c++) { const uint32_t b = threadIdx.x * CH + c; if (b < NB) loc += s_cnt[b]; }
        uint32_t inc = loc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint32_t run = inc - loc;
        for (uint32_t w = 0; w < wv; w++) run += s_w[w];
        for (uint32_t c = 0; c < CH; c++) { const uint32_t b = threadIdx.x * CH + c; if (b < NB) { const uint32_t x = s_cnt[b]; s_start[b] = run; s_cnt[b] = run; run += x; } }
        __syncthreads();
        if (f < units) { PtPlaceEmit e{s_cnt, s_ids, sh, lg, idmask}; walk_unit<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, f, k, mask, rcshift, rc_or, e); }
        __syncthreads();
        // run by run to this part's slices: half a wavefront per bucket (a run is ~16-32 ids)
        const uint32_t hw = threadIdx.x >> 5, hl = threadIdx.x & 31;
        for (uint32_t b = hw; b < NB; b += PT_T / 32) {
            const uint32_t a = s_start[b], e = s_cnt[b], cur = s_cur[b], nb = e - a;
            if (nb == 0) continue;
            if (cur + nb > cap) { over = true; continue; }
            uint32_t *dst = out + ((uint64_t)b * parts + part) * cap + cur;
            for (uint32_t i = hl; i < nb; i += 32) dst[i] = s_ids[a + i];
            if (hl == 0) s_cur[b] = cur + nb;
        }
        __syncthreads();
    }
    if (over) ovf[gl] = 1;
    uint32_t *cg = cnt + (uint64_t)g_boff[gl] * parts;
    for (uint32_t b = threadIdx.x; b < NB; b += PT_T) cg[(uint64_t)b * parts + part] = s_cur[b];
}

// DNA form of k_prob_part1 with ONE walk per tile (the two-walk form above stays for amino acids): a lane keeps the 32 k-mers of its unit in registers - the id
// and (bucket, rank), the rank being what the counting atomic returns - so that after the prefix over the bucket counts each id goes straight to
// s_ids[start[bucket] + rank]: no second walk (the walk is ~half of the kernel's instructions), no second atomic.
template <bool CHECK>
__device__ __forceinline__ void pt_walk_dna(uint64_t w, uint64_t fwd, uint64_t rc, uint64_t mask, uint32_t rcshift, uint64_t rc_or, uint32_t jlo, uint32_t jhi, uint32_t sh, uint32_t lg,
                                            uint32_t idmask, uint32_t *s_cnt, uint32_t (&idr)[32], uint32_t (&pkr)[32])
{
#pragma unroll
    for (uint32_t j = 0; j < 32; j++) {
        const uint64_t c = w >> 62; w <<= 2;
        fwd = ((fwd << 2) | c) & mask;
        rc = (rc >> 2) | ((3 - c) << rcshift) | rc_or;
        const uint64_t v = fwd < rc ? fwd : rc;
        const uint32_t id = (uint32_t)v & idmask, b = (uint32_t)(v >> sh) ^ pt_mix(id, lg);
        idr[j] = id;
        if (!CHECK || (j >= jlo && j < jhi)) pkr[j] = (b << 16) | atomicAdd(&s_cnt[b], 1u);      // rank < 32 768: 15 bits
        else pkr[j] = 0xFFFFFFFFu;
    }
}
// inclusive maximum over the lanes 0 .. l of a wavefront (DPP: shifts inside the rows of 16, then the row totals broadcast to the rows behind)
__device__ __forceinline__ uint32_t wave_incl_max_scan(uint32_t v)
{
#define GS_DPP_MAX(ctrl, rows) do { const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xF, false); v = y > v ? y : v; } while (0)
    GS_DPP_MAX(0x111, 0xF); GS_DPP_MAX(0x112, 0xF); GS_DPP_MAX(0x114, 0xF); GS_DPP_MAX(0x118, 0xF);      // row_shr:1 / 2 / 4 / 8
    GS_DPP_MAX(0x142, 0xA);                                                                            // row_bcast:15 -> rows 1 and 3
    GS_DPP_MAX(0x143, 0xC);                                                                            // row_bcast:31 -> rows 2 and 3
#undef GS_DPP_MAX
    return v;
}
__global__ __launch_bounds__(PT_T) void k_prob_part1_dna(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                         const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off, const uint64_t *__restrict__ gen_units,
                                                         uint64_t g0, uint32_t kq, uint32_t vbits, const uint32_t *__restrict__ g_sh, const uint32_t *__restrict__ g_boff,
                                                         const uint64_t *__restrict__ g_vbase, const uint32_t *__restrict__ g_cap, uint32_t parts, uint32_t *__restrict__ vals32,
                                                         uint32_t *__restrict__ cnt, uint32_t *__restrict__ ovf)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pt[];
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_mark[PT_T];                             // a 64-word mark row per wavefront (the copy-out below)
    const uint32_t gl = blockIdx.y, part = blockIdx.x;
    const uint64_t g = g0 + gl;
    const uint32_t sh = g_sh[gl], NB = 1u << (vbits - sh), cap = g_cap[gl];
    uint32_t *s_cnt = s_pt, *s_start = s_pt + NB, *s_cur = s_pt + 2 * NB + 1, *s_ids = s_pt + 3 * NB + 4;      // s_start has NB + 1 entries (the total closes the last bucket)
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1], units = gen_units[g];
    const uint32_t k = kq_k(kq);
    const uint64_t mask = kmer_mask(false, k), rc_or = kq_rc_or(kq);
    const uint32_t idmask = (uint32_t)(((uint64_t)1 << sh) - 1), lg = vbits - sh;
    const uint32_t rcshift = 2 * (k - 1);
    const uint64_t tiles = (units + PT_T - 1) / PT_T, t_lo = tiles * part / parts, t_hi = tiles * (part + 1) / parts;
    uint32_t *out = vals32 + g_vbase[gl];
    const uint64_t *w64 = (const uint64_t *)seq;
    for (uint32_t b = threadIdx.x; b < NB; b += PT_T) s_cur[b] = 0;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t CH = NB > (uint32_t)PT_T ? NB / PT_T : 1u;
    bool over = false;
    // a lane's unit of a tile: the packed word, the word in front of it (the k - 1 bases before the unit) and which of its 32 windows are k-mers of its record.
    // The unit of tile t + 1 is fetched while tile t is worked on: with one workgroup per CU nothing else hides the two dependent round trips to HBM.
    struct Unit { uint64_t w, pw; uint32_t jlo, jhi; bool init; };
    auto fetch = [&](uint64_t t) -> Unit {
        Unit un{0, 0, 0, 0, false};
        const uint64_t f = t * PT_T + threadIdx.x;
        if (t < t_hi && f < units) {
            uint64_t lo = r0, hi = r1;
            while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (rec_upre[mid] <= f) lo = mid; else hi = mid; }
            const uint64_t rb = rec_start[lo], re = rb + rec_len[lo];
            const uint64_t u = (rb >> 5) + (f - rec_upre[lo]), a0 = u << 5, first_valid = rb + k - 1;
            un.w = w64[u];
            un.init = a0 > rb && k > 1;
            if (un.init) un.pw = w64[u - 1];
            un.jlo = first_valid > a0 ? (uint32_t)std::min<uint64_t>(first_valid - a0, 32) : 0u;
            un.jhi = re > a0 ? (uint32_t)std::min<uint64_t>(re - a0, 32) : 0u;
            if (un.jhi <= un.jlo) { un.jlo = 0; un.jhi = 0; }
        }
        return un;
    };
    Unit cur = fetch(t_lo);
    for (uint64_t t = t_lo; t < t_hi; t++) {
        for (uint32_t b = threadIdx.x; b < NB; b += PT_T) s_cnt[b] = 0;
        const Unit nxt = fetch(t + 1);
        __syncthreads();
        uint32_t idr[32], pkr[32];
        {
            const uint64_t w = __builtin_bswap64(cur.w);
            uint64_t fwd = 0, rc = 0;
            if (cur.init) {
                // the state after the k - 1 bases in front of the word, in closed form (walk_unit)
                const uint64_t pw = __builtin_bswap64(cur.pw);
                const uint64_t lowm = ((uint64_t)1 << (2 * (k - 1))) - 1;
                fwd = pw & lowm;
                rc = ((rc64(pw) >> (2 * (33 - k))) << 2) | rc_or;
            }
            const bool have = cur.jhi > cur.jlo, full = cur.jlo == 0 && cur.jhi == 32;
            if (__ballot(full) == __ballot(true)) pt_walk_dna<false>(w, fwd, rc, mask, rcshift, rc_or, 0, 32, sh, lg, idmask, s_cnt, idr, pkr);      // (wavefront-uniform)
            else if (__ballot(have)) pt_walk_dna<true>(w, fwd, rc, mask, rcshift, rc_or, cur.jlo, cur.jhi, sh, lg, idmask, s_cnt, idr, pkr);
            else {
#pragma unroll
                for (int j = 0; j < 32; j++) pkr[j] = 0xFFFFFFFFu;
            }
        }
        __syncthreads();
        uint32_t loc = 0;
        for (uint32_t c = 0; c < CH; c++) { const uint32_t b = threadIdx.x * CH + c; if (b < NB) loc += s_cnt[b]; }
        uint32_t inc = loc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint32_t run = inc - loc;
        for (uint32_t w = 0; w < wv; w++) run += s_w[w];
        for (uint32_t c = 0; c < CH; c++) { const uint32_t b = threadIdx.x * CH + c; if (b < NB) { s_start[b] = run; run += s_cnt[b]; } }
        if (threadIdx.x == PT_T - 1) s_start[NB] = run;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 32; j++) if (pkr[j] != 0xFFFFFFFFu) s_ids[s_start[pkr[j] >> 16] + (pkr[j] & 0xFFFFu)] = idr[j];
        __syncthreads();
        // to this part's slices: a wavefront takes 64 buckets at a time - their ids are one contiguous stretch of s_ids, walked in windows of 64 positions. The
        // buckets that START inside a window leave their number at their start position (a 64-word mark row per wavefront); an inclusive max-scan over the lanes
        // (the marks increase along the window) tells every position its bucket, the bucket's destination comes from its lane by one permute. ~25 wave
        // instructions per 64 ids (a 6-step search per id over the 64 starts was ~45, a half wavefront per run a chain of LDS round trips per ~16 ids).
        {
            uint32_t *mk = s_mark + wv * 64;
            for (uint32_t b0 = wv * 64; b0 < NB; b0 += (PT_T / 64) * 64) {
                const uint32_t nbk = NB - b0 < 64u ? NB - b0 : 64u;
                const uint32_t st = lane < nbk ? s_start[b0 + lane] : 0u, en = lane < nbk ? s_start[b0 + lane + 1] : 0u, sc = lane < nbk ? s_cur[b0 + lane] : 0u;
                const uint32_t nb = en - st;
                const bool fits = sc + nb <= cap;
                if (nb && !fits) over = true;
                const uint64_t okb = __ballot(fits);
                const uint32_t dbase = (uint32_t)(((uint64_t)(b0 + lane) * parts + part) * cap) + sc - st;      // destination of position pos = dbase + pos (mod 2^32)
                const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)st), p1 = s_start[b0 + nbk];
                const uint64_t nz = __ballot(nb != 0);
                uint32_t carry = nz ? (uint32_t)__builtin_ctzll(nz) : 0u;                                      // the bucket (lane) that holds position p0
                for (uint32_t pw = p0; pw < p1; pw += 64) {
                    mk[lane] = 0;
                    __builtin_amdgcn_wave_barrier();
                    if (nb && st >= pw && st - pw < 64u) mk[st - pw] = lane + 1;
                    __builtin_amdgcn_wave_barrier();
                    uint32_t v = mk[lane];
                    __builtin_amdgcn_wave_barrier();
                    v = wave_incl_max_scan(v);
                    v = v ? v - 1 : carry;
                    carry = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
                    const uint32_t pos = pw + lane;
                    const uint32_t d = (uint32_t)__shfl((int)dbase, (int)v);
                    if (pos < p1 && ((okb >> v) & 1ull)) out[d + pos] = s_ids[pos];
                }
                if (lane < nbk) s_cur[b0 + lane] = fits ? sc + nb : cap;
            }
        }
        __syncthreads();
        cur = nxt;
    }
    if (over) ovf[gl] = 1;
    uint32_t *cg = cnt + (uint64_t)g_boff[gl] * parts;
    for (uint32_t b = threadIdx.x; b < NB; b += PT_T) cg[(uint64_t)b * parts + part] = s_cur[b];
}

// ---- the bucket work of the tiered form, in two kernels (one kernel with both halves ran at three workgroups per CU - 52 kB of LDS, 80 VGPRs - and 0.66 of its
//      VALU issue; the filter half is 9/10 of the instructions and needs neither the table nor the registers of the generator):
// k_prob_tier_filter  workgroup per bucket: count-min of every id (pass A), first draw of every id against the bound its cell allows (pass B); what may matter
//                     (~1 id in 12) is compacted to a list in global memory, (offset, count) per bucket in `desc`. 22 kB of LDS, <= 64 VGPRs: four workgroups per CU.
// k_prob_tier_points  one WAVEFRONT per bucket (no barriers; T = 64, table of 1024) - or a workgroup for the few buckets with more than 512 kept ids (T = 512,
//                     table of 4096, the ones the wavefront form lists in `big`): the kept ids enter the exact table, the owners of the entries run the
//                     generator with the exact multiplicity and lower q[], exactly as k_prob_buckets does from its table.
__global__ __launch_bounds__(PT2_T, 8) void k_prob_tier_filter(const uint32_t *__restrict__ vals32, const uint64_t *__restrict__ g_vbase, const uint32_t *__restrict__ g_cap,
                                                               const uint32_t *__restrict__ cnt, uint32_t parts, uint32_t vbits, const uint32_t *__restrict__ g_sh,
                                                               const uint32_t *__restrict__ g_boff, uint32_t ng, uint32_t lg_max, ProbConst pc, const uint64_t *__restrict__ thr,
                                                               uint32_t *__restrict__ kept, uint32_t kept_cap, uint32_t *__restrict__ kept_n, uint2 *__restrict__ desc,
                                                               uint32_t *__restrict__ ovf, unsigned long long *__restrict__ prof)
{
    __shared__ __attribute__((aligned(16))) uint32_t cm[PT_CM / 2];
    __shared__ uint32_t s_q[PT_Q];
    __shared__ uint32_t s_ns;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr uint32_t NW = PT2_T / 64;
    constexpr int KPL = 8;                                        // ids per lane held in registers between the two passes (more: re-read from the slices)
    const uint64_t n_items = (uint64_t)ng << lg_max;              // bucket-major over the chunk, as k_prob_buckets
    const uint32_t region = kept_cap / gridDim.x; uint32_t my_kept = 0;
    // (jpos, gl) of item = jpos ng + gl, stepped without a division per bucket (a 64-bit division is ~150 instructions: a fifth of a bucket's work)
    const uint32_t dj = gridDim.x / ng, dg = gridDim.x % ng;
    uint32_t jpos = blockIdx.x / ng, gl = blockIdx.x % ng;
    const uint64_t k_one = (uint64_t)(0x1.0p52 / pc.c1 * (1.0 - 0x1.0p-40));
    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x, jpos += dj, gl += dg) {
        if (gl >= ng) { gl -= ng; jpos++; }
        const uint32_t sh = g_sh[gl], lg = vbits - sh, rs = lg_max - lg;
        if (jpos & ((1u << rs) - 1u)) continue;                    // (workgroup-uniform) this genome has fewer buckets: it takes part at every 2^rs-th position
        const uint32_t bk = jpos >> rs;
        const uint64_t fb = (uint64_t)g_boff[gl] + bk;
        const bool pf = prof && blockIdx.x == 0 && threadIdx.x == 0;
        long long t0 = pf ? clock64() : 0, t1;
#define GS_PSTAMP(i) do { if (pf) { t1 = clock64(); atomicAdd(&prof[i], (unsigned long long)(t1 - t0)); t0 = t1; } } while (0)
        const uint32_t capg = g_cap[gl];
        const uint32_t *base = vals32 + g_vbase[gl] + (uint64_t)bk * parts * capg;
        // ---- this wavefront's share of the bucket's slices: whole slices (parts >= 8) or an equal piece of one; the ids go to registers at once (every load
        //      in flight together: the slices are cold in HBM and a load per loop trip was a round trip per trip)
        const uint32_t mycnt = lane < parts ? cnt[fb * parts + lane] : 0u;      // (every wavefront reads the counts itself: no barrier in front of the loads)
        uint32_t n = mycnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
        const uint32_t IT = capg >> 6;                             // 64-id trips per slice (the capacity is a multiple of 64)
        uint32_t lo = 0, hi = 0, p_small = 0, NU;
        if (parts >= NW) NU = (parts / NW) * IT;
        else {
            const uint32_t lgp = 31u - (uint32_t)__builtin_clz(parts), lgs = 3u - lgp, piece = wv >> lgp; p_small = wv & (parts - 1u);      // parts is a power of two below NW = 8
            const uint32_t np = (uint32_t)__shfl((int)mycnt, (int)p_small);
            lo = (np * piece) >> lgs; hi = (np * (piece + 1)) >> lgs;
            NU = (hi - lo + 63) >> 6;
        }
        auto key_at = [&](uint32_t u, uint32_t &id) -> bool {      // u-th trip of this wavefront: the lane's id, or false
            if (parts >= NW) {
                const uint32_t p = wv + NW * (u / IT), i = (u % IT) * 64 + lane;
                if (p >= parts || i >= (uint32_t)__shfl((int)mycnt, (int)p)) return false;
                id = base[(uint64_t)p * capg + i];
                return true;
            }
            const uint32_t i = lo + u * 64 + lane;
            if (i >= hi) return false;
            id = base[(uint64_t)p_small * capg + i];
            return true;
        };
        uint32_t kreg[KPL]; uint32_t kval = 0;                     // kval: bit u = kreg[u] holds an id
#pragma unroll
        for (int u = 0; u < KPL; u++) { kreg[u] = 0; if ((uint32_t)u < NU && key_at(u, kreg[u])) kval |= 1u << u; }
        // the genome's cap (q[] moves only in the second kernel), as thresholds on the 52 uniform bits K of the first draw x0 = c1 K 2^-52: x0 < 1 for K < k_one, and
        // x0 > c thr for K > c t_one - both with a margin of 2^-40 relative on the safe side (a k-mer that is kept needlessly costs time, never the result)
        const uint64_t t_one = thr[ng + gl];                       // (the host's: run_prob_tiers)
        __syncthreads();                                           // the previous bucket's LDS is dead
        for (uint32_t s = threadIdx.x; s < PT_CM / 8; s += PT2_T) ((uint4 *)cm)[s] = make_uint4(0, 0, 0, 0);
        if (threadIdx.x == 0) s_ns = 0;
        __syncthreads();
        if (n == 0) { if (threadIdx.x == 0) desc[fb] = make_uint2(0u, 0u); continue; }      // (workgroup-uniform)
        GS_PSTAMP(0);
        auto cell_of = [&](uint32_t id) -> uint32_t { return (id * 0x9E3779B1u) >> 19; };      // 13 bits: PT_CM cells (the product pt_mix takes its lg bits from: one multiplication)
        const bool wide = n > 65535u;                              // a 16-bit cell could wrap: everything counts as "many copies" (the queue overflows: redone)
        // ---- pass A: every k-mer into its count-min cell (one non-returning LDS add)
        if (!wide) {
#pragma unroll
            for (int u = 0; u < KPL; u++) if (kval & (1u << u)) { const uint32_t c = cell_of(kreg[u]); atomicAdd(&cm[c >> 1], 1u << ((c & 1) * 16)); }
            for (uint32_t u = KPL; u < NU; u++) { uint32_t id; if (key_at(u, id)) { const uint32_t c = cell_of(id); atomicAdd(&cm[c >> 1], 1u << ((c & 1) * 16)); } }
        }
        __syncthreads();
        GS_PSTAMP(1);
        // ---- pass B: first draw of every k-mer against the bound its cell allows; what may matter is queued, compacted across the wavefront
        auto keep_b = [&](uint32_t id) -> bool {
            const uint32_t ce = cell_of(id);
            const uint32_t c = wide ? 0xFFFFu : ((cm[ce >> 1] >> ((ce & 1) * 16)) & 0xFFFFu);      // >= the multiplicity of this value
            const uint64_t v = pt_value(bk, id, sh, lg);
            const uint64_t s0 = splitmix_mix(v + GS_GAMMA), s3 = splitmix_mix(v + 4 * GS_GAMMA);
            const uint64_t K = (rotl64(s0 + s3, 23) + s0) >> 12;     // x0 = c1 K 2^-52; when < 1 it IS the first truncated exponential (SPEC 3.3)
            // even c copies leave its first point above every slot minimum (x1 / w > thr), and it is dead in pass 2 (1 / w > thr), for every w <= c: tested without
            // the division and in integers - x0 > c thr (1 + 2^-40) implies fl(fl(1 / w) x0) > thr (the margin covers the roundings), and with x0 < 1 also 1 / w > thr
            return !(c < 2048u && K < k_one && K > (uint64_t)c * t_one);
        };
        auto queue_b = [&](bool valid, uint32_t id) {
            const bool keep = valid && keep_b(id);
            const uint64_t bal = __ballot(keep);
            if (bal) {                                               // (wavefront-uniform)
                uint32_t qb = 0;
                if (lane == 0) qb = atomicAdd(&s_ns, (uint32_t)__popcll(bal));
                qb = (uint32_t)__builtin_amdgcn_readfirstlane((int)qb);
                const uint32_t at = qb + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                if (keep && at < (uint32_t)PT_Q) s_q[at] = id;
            }
        };
#pragma unroll
        for (int u = 0; u < KPL; u++) if ((uint32_t)u < NU) queue_b((kval >> u) & 1u, kreg[u]);
        for (uint32_t u = KPL; u < NU; u++) { uint32_t id = 0; const bool ok = key_at(u, id); queue_b(ok, id); }
        __syncthreads();
        GS_PSTAMP(2);
        // ---- the kept ids to the global list (one returning atomic per bucket reserves their place)
        // ---- the kept ids to this workgroup's own stretch of the global list (one cursor for all workgroups was a same-address returning atomic per bucket:
        //      13 ns each, serialised - the whole kernel's time)
        const uint32_t nk = s_ns;
        uint32_t off = 0xFFFFFFFFu;
        if (nk <= (uint32_t)PT_Q && my_kept + nk <= region) { off = blockIdx.x * region + my_kept; my_kept += nk; }
        if (threadIdx.x == 0) {
            if (off == 0xFFFFFFFFu) ovf[gl] = 1;                    // more than the queue holds (a loose cap over a large bucket) or the stretch is full: the genome is redone
            desc[fb] = make_uint2(off, off == 0xFFFFFFFFu ? 0u : nk);
        }
        if (off != 0xFFFFFFFFu) for (uint32_t i = threadIdx.x; i < nk; i += PT2_T) kept[off + i] = s_q[i];
        if (pf) { atomicAdd(&prof[6], (unsigned long long)nk); atomicAdd(&prof[7], 1ull); atomicAdd(&prof[8], (unsigned long long)n); }
        GS_PSTAMP(3);
#undef GS_PSTAMP
    }
    if (threadIdx.x == 0 && my_kept) atomicAdd(kept_n, my_kept);      // (statistics)
}
// T lanes per bucket (64: a wavefront, no other wavefront shares its LDS; 512: a workgroup), TAB table entries. BIG: the items come from the list `big`.
template <int T, int TAB, bool BIG>
__global__ __launch_bounds__(T) void k_prob_tier_points(const uint32_t *__restrict__ kept, const uint2 *__restrict__ desc, uint32_t vbits, const uint32_t *__restrict__ g_sh,
                                                        const uint32_t *__restrict__ g_boff, uint32_t ng, uint32_t lg_max, uint32_t m, uint64_t zone, ProbConst pc,
                                                        uint64_t *__restrict__ q, uint64_t *__restrict__ thr, uint32_t *__restrict__ wmax, PbLists L, uint32_t *__restrict__ ovf,
                                                        uint32_t *__restrict__ big, uint32_t *__restrict__ n_big, uint32_t big_cap)
{
    constexpr int NT = T == 64 ? 8 : (PT_Q + T - 1) / T;        // trips over the kept ids: <= 512 for a wavefront, <= PT_Q for a workgroup
    __shared__ __attribute__((aligned(16))) uint32_t tab[TAB];
    __shared__ __attribute__((aligned(16))) uint32_t dup[TAB / 2];
    __shared__ uint32_t s_nc; __shared__ unsigned long long s_mx;
    const uint32_t EMPTY = 0xFFFFFFFFu;
    const uint32_t seg = BIG ? 0u : L.cand_cap / gridDim.x;      // possible winners go straight to this block's segment of the candidate list (BIG: the shared region behind
    uint32_t my_nc = 0;                                           // the segments - they belong to the wavefront form's blocks)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_items = BIG ? (uint64_t)min(*n_big, big_cap) : ((uint64_t)ng << lg_max);
    // A bucket's description and its kept ids are fetched ONE ITERATION AHEAD (a wavefront works alone on its bucket: nothing else hides the two dependent
    // round trips - description, then ids - in front of the table insert).
    struct Item { uint32_t jpos, gl, bk, sh, nk; uint32_t id[NT]; };
    auto fetch = [&](uint64_t it0, Item &x) {
        x.nk = 0; x.jpos = 0; x.gl = 0; x.bk = 0; x.sh = 1;
        if (it0 >= n_items) return;
        const uint32_t item = BIG ? big[it0] : (uint32_t)it0;      // (n_items < 2^32: <= 65 535 genomes x 2048 buckets)
        x.jpos = item / ng; x.gl = item - x.jpos * ng;
        x.sh = g_sh[x.gl];
        const uint32_t rs = lg_max - (vbits - x.sh);
        if (x.jpos & ((1u << rs) - 1u)) return;                     // (uniform) this genome has fewer buckets
        x.bk = x.jpos >> rs;
        const uint2 d = desc[(uint64_t)g_boff[x.gl] + x.bk];
        x.nk = d.y;
        if (!BIG && x.nk > (uint32_t)(TAB / 2)) return;            // (listed for the workgroup form below: no ids needed)
#pragma unroll
        for (int t = 0; t < NT; t++) { const uint32_t i = t * T + threadIdx.x; x.id[t] = i < x.nk ? kept[d.x + i] : 0u; }
    };
    Item nx;
    fetch(blockIdx.x, nx);
    for (uint64_t it0 = blockIdx.x; it0 < n_items; it0 += gridDim.x) {
        const Item cu = nx;
        fetch(it0 + gridDim.x, nx);
        const uint32_t jpos = cu.jpos, gl = cu.gl, bk = cu.bk, sh = cu.sh, lg = vbits - sh, nk = cu.nk;
        if (nk == 0) continue;
        if (!BIG && nk > (uint32_t)(TAB / 2)) {                    // too many for a wavefront's table: listed for the workgroup form
            if (threadIdx.x == 0) { const uint32_t at = atomicAdd(n_big, 1u); if (at < big_cap) big[at] = (uint32_t)it0; else ovf[gl] = 1; }
            continue;
        }
        uint64_t *qg = q + (uint64_t)gl * m;
        __syncthreads();                                           // the previous bucket's LDS is dead
        for (uint32_t s = threadIdx.x; s < TAB / 4; s += T) ((uint4 *)tab)[s] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
        for (uint32_t s = threadIdx.x; s < TAB / 8; s += T) ((uint4 *)dup)[s] = make_uint4(0, 0, 0, 0);
        if (threadIdx.x == 0) { s_nc = 0; s_mx = 0; }
        uint64_t thr_b = __hip_atomic_load(&thr[gl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((jpos & ((1u << (lg_max > 4 ? lg_max - 4 : 0)) - 1u)) == 0 && jpos != 0) {      // 15 times per genome: rescan q[], publish the tighter bound
            unsigned long long mx = 0;
            for (uint32_t i0 = 0; i0 < m; i0 += 8 * T) {
                unsigned long long x[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { const uint32_t i = i0 + u * T + threadIdx.x; x[u] = i < m ? __hip_atomic_load(&qg[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull; }
#pragma unroll
                for (int u = 0; u < 8; u++) mx = x[u] > mx ? x[u] : mx;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
            __syncthreads();
            if (lane == 0) atomicMax(&s_mx, mx);
            __syncthreads();
            const unsigned long long t = s_mx;
            if (threadIdx.x == 0) atomicMin((unsigned long long *)&thr[gl], t);
            if (t < thr_b) thr_b = t;
        }
        const double thr_d = __longlong_as_double((long long)thr_b);
        __syncthreads();
        // ---- the kept ids enter the exact table: CAS + duplicate count as in k_prob_buckets; the lane whose CAS created an entry owns it
        bool over = false;
        auto insert_id = [&](uint32_t id) -> uint32_t {
            uint32_t s = ((id * 0x85EBCA6Bu) >> 16) & (uint32_t)(TAB - 1);      // (the raw id is the k-mer's last bases)
            for (uint32_t probe = 0; probe < (uint32_t)TAB; probe++) {
                const uint32_t old = atomicCAS(&tab[s], EMPTY, id);
                if (old == EMPTY) return s;
                if (old == id) {
                    const uint32_t before = atomicAdd(&dup[s >> 1], 1u << ((s & 1) * 16));
                    if (((before >> ((s & 1) * 16)) & 0xFFFFu) == 0xFFFFu) over = true;
                    return 0xFFFFFFFFu;
                }
                s = (s + 1) & (uint32_t)(TAB - 1);
            }
            over = true;
            return 0xFFFFFFFFu;
        };
        uint32_t own[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) { const uint32_t i = t * T + threadIdx.x; own[t] = 0xFFFFFFFFu; if ((uint32_t)(t * T) < nk && i < nk) own[t] = insert_id(cu.id[t]); }
        if (over) ovf[gl] = 1;
        __syncthreads();
        // ---- the exact (value, multiplicity) pairs
        uint32_t wloc = 0;
        auto entry = [&](uint32_t s) {
            const uint64_t v = pt_value(bk, tab[s], sh, lg);
            const uint32_t w = 1u + ((dup[s >> 1] >> ((s & 1) * 16)) & 0xFFFFu);
            wloc = w > wloc ? w : wloc;
            const double winv = w == 1 ? 1.0 : 1.0 / (double)w;
            const bool alive2 = !(winv > thr_d);
            Rng rg; rg.seed(v);
            const double x = texp_sample(pc, rg);
            const double h = 0.0 + winv * x;
            if (h > thr_d && !alive2) return;                        // the exact multiplicity: the false alarms of shared cells end here
            const uint32_t b = (uint32_t)rng_uint(rg, (uint64_t)m, zone);
            if (!(h > thr_d)) {
                const uint64_t hb = (uint64_t)__double_as_longlong(h);
                uint64_t *slot = qg + b;
                if (hb <= __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    // a possible winner: listed without waiting for the atomic's answer - the claim only takes candidates whose point equals the slot's final minimum
                    (void)__hip_atomic_fetch_min((unsigned long long *)slot, (unsigned long long)hb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t sp = BIG ? seg : my_nc + atomicAdd(&s_nc, 1u);
                    if (sp < seg) { const uint32_t o = blockIdx.x * seg + sp; L.cand_v[o] = v; L.cand_h[o] = hb; L.cand_gb[o] = (uint64_t)gl * m + b; }
                    else {
                        const uint32_t pos = atomicAdd(L.n_cand, 1u);
                        if (pos < L.ovf_cap) { const uint32_t o = L.cand_cap + pos; L.cand_v[o] = v; L.cand_h[o] = hb; L.cand_gb[o] = (uint64_t)gl * m + b; }
                    }
                }
            }
            if (alive2) {                                            // may still reach a slot in pass 2 (superset: thr >= the final max q)
                const uint32_t pos = atomicAdd(L.n_act, 1u);
                if (pos < L.act_cap) {
                    L.akey[pos] = v; L.agl[pos] = gl; L.acnt[pos] = w;
                    L.astate[pos] = rg.s0; L.astate[(uint64_t)L.act_cap + pos] = rg.s1; L.astate[2 * (uint64_t)L.act_cap + pos] = rg.s2; L.astate[3 * (uint64_t)L.act_cap + pos] = rg.s3;
                }
            }
        };
#pragma unroll
        for (int t = 0; t < NT; t++) if ((uint32_t)(t * T) < nk && own[t] != 0xFFFFFFFFu) entry(own[t]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)wloc, o); wloc = y > wloc ? y : wloc; }
        if (lane == 0 && wloc > 1 && wloc > __hip_atomic_load(&wmax[gl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&wmax[gl], wloc);
        __syncthreads();
        if (!BIG) { const uint32_t room = seg - my_nc, got = s_nc; my_nc += got < room ? got : room; }      // (what did not fit went to the shared region)
    }
    if (!BIG && threadIdx.x == 0) L.seg_n[blockIdx.x] = my_nc;
}

// ---- prob, host side: what the forms share, then the bucketed, tiered and sorted forms and their driver
static ProbConst prob_const(uint32_t m)
{
    const double l = log((double)m / (double)(m - 1));
    return ProbConst{l, expm1(l) / l, log(2.0 / (1.0 + exp(-l))) / l, (1.0 - exp(-l)) / l};
}
// The GS_PROB_* variables, read once per call of run_prob and handed down: a process may change them between two calls.
struct ProbEnv {
    bool sort, tiers, verbose, profile, id64, one_level, two_walk;      // GS_PROB_IMPL = sort: the sorted form alone, = buckets: no tiered form; the others: set or not
    uint32_t parts;                   // GS_PROB_PARTS, rounded down to a power of two in 1 .. 32; 0 = not set
    double cap_c;                     // GS_PROB_CAP_C: P(a genome fails the tiered form's check) = e^-c
    uint64_t pt_avg, chunk_kmers;     // GS_PROB_PT_AVG; GS_PROB_CHUNK_KMERS (0 = not set)
};
static ProbEnv prob_env()
{
    const auto set = [](const char *name) { return getenv(name) != nullptr; };
    const char *s = getenv("GS_PROB_IMPL");
    ProbEnv e{s && !strcmp(s, "sort"), !(s && !strcmp(s, "buckets")), set("GS_PROB_VERBOSE"), set("GS_PROB_PROFILE"), set("GS_PROB_ID64"), set("GS_PROB_ONELEVEL"), set("GS_PROB_TWOWALK"),
              0, 10.0, (uint64_t)PT_AVG, 0};
    if ((s = getenv("GS_PROB_PARTS"))) { e.parts = 1; const uint32_t want = (uint32_t)atoi(s); while (e.parts * 2 <= want && e.parts < 32) e.parts *= 2; }
    if ((s = getenv("GS_PROB_CAP_C"))) e.cap_c = atof(s);
    if ((s = getenv("GS_PROB_PT_AVG"))) e.pt_avg = (uint64_t)std::max(256, atoi(s));
    if ((s = getenv("GS_PROB_CHUNK_KMERS"))) e.chunk_kmers = std::max<uint64_t>(1, (uint64_t)atoll(s));
    return e;
}
// signature rows of n slots from their minima and winners (32- or 64-bit values)
static int prob_write_rows(gs_ctx *c, int sigbits, const uint64_t *q, const uint64_t *sig, uint64_t n, void *rows)
{
    if (sigbits == 32) hipLaunchKernelGGL(k_prob_write<uint32_t>, dim3(c->n_cu * 4), dim3(256), 0, c->stream, q, sig, n, (uint32_t *)rows);
    else hipLaunchKernelGGL(k_prob_write<uint64_t>, dim3(c->n_cu * 4), dim3(256), 0, c->stream, q, sig, n, (uint64_t *)rows);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

// Genomes that will be redone anyway must not keep the pass loop alive (round 6, found by tools/prob_fuzz.py): a flagged genome can be left with an EMPTY slot - its largest slot
// minimum is then +inf, no element of it ever falls out of "w^-1 (pass - 1) <= max q", and the loop over passes >= 2 never ended. Their multiplicity bound is zeroed on
// the device (k_prob_fold skips a genome with wmax == 0) and the count of active genomes recomputed from the survivors. hq: the genomes' max_b q[b] after pass 1 (host).
static int prob_retire_flagged(gs_ctx *c, const std::vector<uint8_t> &redo, uint32_t ng, uint32_t *wmax_dev, const std::vector<double> &hq, uint32_t &na)
{
    if (std::find(redo.begin(), redo.end(), (uint8_t)1) == redo.end()) return GS_OK;
    std::vector<uint32_t> hw(ng);
    GS_HIP_CHECK(hipMemcpyAsync(hw.data(), wmax_dev, 4 * (size_t)ng, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    na = 0;
    for (uint32_t i = 0; i < ng; i++) { if (redo[i]) hw[i] = 0; na += prob_still_active(hw[i], 1u, hq[i]); }      // (w = 0 is never active)
    GS_HIP_CHECK(hipMemcpyAsync(wmax_dev, hw.data(), 4 * (size_t)ng, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

// One chunk of genomes in the bucketed or the tiered form: slot minima and winners, the lists the first-pass kernels fill (PbLists: possible winners per workgroup segment
// plus a shared overflow region; the elements that may see pass 2, with their generator state), counters, capacities - and what the two forms do alike: start() before the
// form's own kernels, finish() after them. A form supplies its partition, the kernels of its first pass (they lower q, list candidates and active elements through L, raise
// wmax, set ovf) and its rule for flagging a genome. A ProbChunk is a local of the form's function: its leases end before run_prob hands genomes to the next form, whose
// slots are other names for this memory - no lease may cross that hand-over.
struct ProbChunk {
    gs_ctx *c; const gs_sketch_params *p; const uint32_t ng; const ProbConst &pc; const ProbEnv &env;
    const uint32_t m = p->sketch_size;
    PoolBuf q{c, SL_PROB_Q}, qprev{c, SL_PROB_QPREV}, sig{c, SL_PROB_SIG}, sigpass{c, SL_PROB_SIGPASS}, thr{c, SL_PROB_THR}, wmax{c, SL_PROB_WMAX}, qmax{c, SL_PROB_QMAX}, ctr{c, SL_PROB_CTR},
        cv{c, SL_PROB_CAND_V}, chh{c, SL_PROB_CAND_H}, cgb{c, SL_PROB_CAND_GB}, akey{c, SL_PROB_AKEY}, agl{c, SL_PROB_AGL}, acnt{c, SL_PROB_ACNT}, astate{c, SL_PROB_ASTATE}, ph{c, SL_PROB_PH},
        pb{c, SL_PROB_PB}, ovf{c, SL_PROB_OVF}, segn{c, SL_PROB_SEGN};
    const uint32_t cand_cap = (uint32_t)std::min<uint64_t>((uint64_t)ng * m * 16 + 65536, (uint64_t)1 << 30), ovf_cap = cand_cap / 4, act_cap = 1u << 24;
    uint32_t *ctr32 = nullptr;        // [0..1] work counter, [2] n_cand, [3] n_act, [4] n_active genomes, [5] kept ids, [6] big buckets (tiered form)
    PbLists L{};
    bool alloc_failed = false;        // start() failed for want of memory (and not later)
    std::optional<ProfScope> span;    // pass 1: open from the end of start() to the first fold

    // Leases and first values: q = +inf, no winners, a multiplicity bound of 1 per genome (each has k-mers: >= 64 per slot), flags and counters zero. thr: thr_bytes per genome (8: the
    // form's kernels set it; 16: the tiered form's caps, copied from thr_init); segn: a word per workgroup that may own a candidate segment. One host round trip, which also ends the
    // form's own host-to-device copies queued before the call.
    int start(size_t thr_bytes, const void *thr_init, size_t segn_words)
    {
        int rc;
        const size_t slots = (size_t)8 * ng * m, cands = (size_t)8 * (cand_cap + ovf_cap);
        if ((rc = q.alloc(slots)) || (rc = qprev.alloc(slots)) || (rc = sig.alloc(slots)) || (rc = sigpass.alloc(slots)) || (rc = thr.alloc(thr_bytes * ng)) ||
            (rc = wmax.alloc(4 * (size_t)ng)) || (rc = qmax.alloc(8 * (size_t)ng)) || (rc = ctr.alloc(64)) || (rc = cv.alloc(cands)) || (rc = chh.alloc(cands)) ||
            (rc = cgb.alloc(cands)) || (rc = ovf.alloc(4 * (size_t)ng)) || (rc = segn.alloc(4 * segn_words)) || (rc = akey.alloc((size_t)8 * act_cap)) ||
            (rc = agl.alloc((size_t)4 * act_cap)) || (rc = acnt.alloc((size_t)4 * act_cap)) || (rc = astate.alloc((size_t)32 * act_cap))) { alloc_failed = true; return rc; }
        if (thr_init) GS_HIP_CHECK(hipMemcpyAsync(thr.p, thr_init, thr_bytes * ng, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_prob_init, dim3(c->n_cu * 4), dim3(256), 0, c->stream, q.as<uint64_t>(), qprev.as<uint64_t>(), sig.as<uint64_t>(), sigpass.as<uint64_t>(), ng * (uint64_t)m);
        const std::vector<uint32_t> ones(ng, 1u);
        GS_HIP_CHECK(hipMemcpyAsync(wmax.p, ones.data(), 4 * (size_t)ng, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        GS_HIP_CHECK(hipMemsetAsync(ovf.p, 0, 4 * (size_t)ng, c->stream));
        GS_HIP_CHECK(hipMemsetAsync(ctr.p, 0, 64, c->stream));
        ctr32 = ctr.as<uint32_t>();
        L = PbLists{cv.as<uint64_t>(), chh.as<uint64_t>(), cgb.as<uint64_t>(), cand_cap, ovf_cap, ctr32 + 2, segn.as<uint32_t>(), akey.as<uint64_t>(), agl.as<uint32_t>(), acnt.as<uint32_t>(),
                    astate.as<uint64_t>(), act_cap, ctr32 + 3, nullptr};
        span.emplace(c, FAM_SKETCH);
        return GS_OK;
    }
    void fold(uint32_t it)
    {
        hipLaunchKernelGGL(k_prob_fold, dim3(ng), dim3(256), 0, c->stream, m, it, q.as<uint64_t>(), qprev.as<uint64_t>(), sig.as<uint64_t>(), sigpass.as<uint64_t>(), wmax.as<uint32_t>(),
                           qmax.as<double>(), ctr32 + 4);
    }
    // The common ending: claim and fold of pass 1 (wgs = workgroups of the form's points kernel, a candidate segment each), the verdict on every genome, the later passes over the
    // active list, the signature rows. flag(i, overflowed, qmax): must genome i be redone by the next form, given its ovf flag and its max_b q[b] after pass 1? `redo` takes the answers;
    // a list that overflowed flags the whole chunk (GS_OK). Host round trips: one when the chunk finishes in pass 1 with nothing flagged, two more to retire genomes, one per later pass.
    template <class Flag>
    int finish(uint32_t wgs, void *sig_rows, std::vector<uint8_t> &redo, Flag flag)
    {
        int rc;
        const uint64_t zone = uint_zone(m);
        hipLaunchKernelGGL(k_prob_claim_list, dim3(wgs + 1), dim3(256), 0, c->stream, cv.as<uint64_t>(), chh.as<uint64_t>(), cgb.as<uint64_t>(), segn.as<uint32_t>(), cand_cap / wgs, wgs,
                           cand_cap, ctr32 + 2, ovf_cap, q.as<uint64_t>(), sigpass.as<uint64_t>());
        fold(1u);
        GS_HIP_CHECK(hipGetLastError());
        span.reset();
        uint32_t hc[8]; std::vector<uint32_t> hovf(ng); std::vector<double> hq(ng);
        GS_HIP_CHECK(hipMemcpyAsync(hc, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(hovf.data(), ovf.p, 4 * (size_t)ng, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(hq.data(), qmax.p, 8 * (size_t)ng, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));               // the one host round trip of a chunk whose genomes finish in pass 1
        redo.assign(ng, 0);
        if (hc[2] > ovf_cap || hc[3] > act_cap) { redo.assign(ng, 1); return GS_OK; }      // a list overflowed: the whole chunk goes to the next form
        for (uint32_t i = 0; i < ng; i++) redo[i] = flag(i, hovf[i] != 0, hq[i]) ? 1 : 0;
        uint32_t na = hc[4];
        if ((rc = prob_retire_flagged(c, redo, ng, wmax.as<uint32_t>(), hq, na))) return rc;
        const uint32_t n_list = hc[3];
        if (na && n_list) {
            if ((rc = ph.alloc((size_t)8 * n_list)) || (rc = pb.alloc((size_t)4 * n_list))) return rc;
            const uint32_t lg = std::max<uint32_t>(1, std::min<uint32_t>((n_list + 255) / 256, (uint32_t)c->n_cu * 16));
            for (uint32_t it = 2; na; it++) {
                GS_HIP_CHECK(hipMemsetAsync(ctr32 + 4, 0, 4, c->stream));
                hipLaunchKernelGGL(k_prob_point_act, dim3(lg), dim3(256), 0, c->stream, akey.as<uint64_t>(), agl.as<uint32_t>(), acnt.as<uint32_t>(), n_list, act_cap, m, zone, pc, it,
                                   qmax.as<double>(), q.as<uint64_t>(), astate.as<uint64_t>(), ph.as<uint64_t>(), pb.as<uint32_t>());
                hipLaunchKernelGGL(k_prob_claim_act, dim3(lg), dim3(256), 0, c->stream, akey.as<uint64_t>(), agl.as<uint32_t>(), n_list, m, q.as<uint64_t>(), ph.as<uint64_t>(), pb.as<uint32_t>(),
                                   sigpass.as<uint64_t>());
                fold(it);
                GS_HIP_CHECK(hipGetLastError());
                GS_HIP_CHECK(hipMemcpyAsync(&na, ctr32 + 4, 4, hipMemcpyDeviceToHost, c->stream));
                GS_HIP_CHECK(hipStreamSynchronize(c->stream));
                if (env.verbose && (it < 8 || (it & (it - 1)) == 0)) fprintf(stderr, "[GS_PROB] pass %u done: %u genomes still active, %u elements on the active list\n", it, na, n_list);
            }
        }
        return prob_write_rows(c, gs_value_bits(p), q.as<uint64_t>(), sig.as<uint64_t>(), ng * (uint64_t)m, sig_rows);
    }
};

// one chunk of genomes [g0, g0 + ng) through the bucketed form; hk = k-mers per genome (host). *redo (ng flags, host) marks genomes that
// must be redone by the sorted form; returns GS_OK with every flag set when a list overflowed.
static int run_prob_buckets(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *upre,
                            const uint64_t *genome_rec_off, const uint64_t *gunits, uint64_t g0, uint32_t ng, const uint64_t *hk, const ProbConst &pc, const ProbEnv &env,
                            void *sig_rows, std::vector<uint8_t> &redo)
{
    const uint32_t m = p->sketch_size, k = p->k;
    const bool aa = p->data_t == GS_DATA_AA;
    const uint64_t zone = uint_zone(m);
    int rc;
    // host plan: buckets per genome, flat bucket offsets, value offsets
    const uint32_t vbits = aa ? 5 * k : 2 * k;
    std::vector<uint32_t> sh(ng), boff(ng + 1); std::vector<uint64_t> vbase(ng);
    uint64_t T = 0, maxk = 0; uint32_t nbmax = 1, nbt = 0, shmax = 0;
    for (uint32_t i = 0; i < ng; i++) {
        uint32_t lg = 0; while (((uint64_t)PB_AVG << lg) < hk[i] && lg < vbits) lg++;
        sh[i] = vbits - lg; shmax = std::max(shmax, sh[i]); boff[i] = nbt; nbt += 1u << lg; nbmax = std::max(nbmax, 1u << lg);
        vbase[i] = T; T += hk[i]; maxk = std::max(maxk, hk[i]);
    }
    const bool id32 = shmax <= 31 && !env.id64;                     // every genome's in-bucket id fits 4 bytes (with ~0 left over for "empty")
    boff[ng] = nbt;
    // two-level partition: coarse buckets = the top half of the bucket bits
    std::vector<uint32_t> cinfo(2 * (size_t)ng + 1);                // [0, ng): coarse shifts, [ng, 2 ng]: flat coarse-bucket offsets
    uint32_t nct = 0, ncmax = 1, nfmax = 1;
    for (uint32_t i = 0; i < ng; i++) {
        const uint32_t lg = vbits - sh[i], lgc = lg / 2;
        cinfo[i] = sh[i] + (lg - lgc); cinfo[ng + i] = nct; nct += 1u << lgc; ncmax = std::max(ncmax, 1u << lgc); nfmax = std::max(nfmax, 1u << (lg - lgc));
    }
    cinfo[2 * (size_t)ng] = nct;
    const uint64_t avg_units = maxk / 32 + 1;
    const uint32_t parts = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(avg_units / ((uint64_t)PBK_T * PBK_WPL) + 1, std::max<uint64_t>(1, (2 * (uint64_t)c->n_cu + ng - 1) / ng)));
    PoolBuf dsh(c, SL_PROB_INFO), dboff(c, SL_PROB_BOFF), dvb(c, SL_PROB_VBASE), hist(c, SL_PROB_HIST), bst(c, SL_PROB_BST), bsz(c, SL_PROB_BSZ), bgn(c, SL_PROB_BGN), vals(c, SL_PROB_VALS),
        tmpv(c, SL_PROB_TMPV), dcin(c, SL_PROB_COARSE);
    ProbChunk ch{c, p, ng, pc, env};
    bool two_level = !env.one_level && (uint64_t)parts * ncmax <= PB_CCMAX && ncmax <= 256 && nfmax <= 256;
    // the second copy of the values is the price of the two levels: a device that has no room for it (an index with its pair cache beside the
    // sketcher, say) partitions in one level as in round 3
    if (two_level && tmpv.alloc(8 * (size_t)T + 64) != GS_OK) { (void)hipGetLastError(); two_level = false; }
    uint32_t *d_shc = nullptr, *d_coff = nullptr, *d_ccur = nullptr, *d_ccnt = nullptr;
    if (two_level) {
        if ((rc = dcin.alloc(4 * (cinfo.size() + 2 * (size_t)nct * parts) + 64))) return rc;
        d_shc = dcin.as<uint32_t>(); d_coff = d_shc + ng; d_ccur = d_coff + ng + 1; d_ccnt = d_ccur + (size_t)nct * parts;
        GS_HIP_CHECK(hipMemcpyAsync(dcin.p, cinfo.data(), 4 * cinfo.size(), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = dsh.alloc(4 * (size_t)ng)) || (rc = dboff.alloc(4 * (size_t)(ng + 1))) || (rc = dvb.alloc(8 * (size_t)ng)) || (rc = hist.alloc((size_t)4 * nbt * parts)) ||
        (rc = bst.alloc((size_t)4 * nbt)) || (rc = bsz.alloc((size_t)4 * nbt)) || (rc = bgn.alloc((size_t)4 * nbt)) || (rc = vals.alloc(8 * (size_t)T + 64)))
        return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dsh.p, sh.data(), 4 * (size_t)ng, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dboff.p, boff.data(), 4 * (size_t)(ng + 1), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dvb.p, vbase.data(), 8 * (size_t)ng, hipMemcpyHostToDevice, c->stream));
    if ((rc = ch.start(8, nullptr, (size_t)c->n_cu * 8))) return rc;
    uint64_t *q = ch.q.as<uint64_t>(), *thr = ch.thr.as<uint64_t>();
    size_t lds = (size_t)4 * nbmax;
    dim3 grid(parts, ng), block(PBK_T);
#define GS_LAUNCH_PBP(AAV, MODE)                                                                                              \
    do {                                                                                                                      \
        auto kern = k_prob_partition<AAV, MODE>;                                                                              \
        if (lds > 48 * 1024) GS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(kern, grid, block, lds, c->stream, seq, rec_start, rec_len, upre, genome_rec_off, gunits, g0, kq_of(p), vbits, dsh.as<uint32_t>(), dboff.as<uint32_t>(), parts, \
                           hist.as<uint32_t>(), q, m, zone, pc, vals.as<uint64_t>(), dvb.as<uint64_t>());                     \
    } while (0)
    if (aa) GS_LAUNCH_PBP(true, 0); else GS_LAUNCH_PBP(false, 0);
    hipLaunchKernelGGL(k_prob_scan, dim3(ng), dim3(1024), 0, c->stream, vbits, dsh.as<uint32_t>(), dboff.as<uint32_t>(), parts, hist.as<uint32_t>(), bst.as<uint32_t>(), bsz.as<uint32_t>(),
                       bgn.as<uint32_t>(), q, m, thr, d_shc, d_coff, d_ccur, d_ccnt);
    if (!two_level) { if (aa) GS_LAUNCH_PBP(true, 1); else GS_LAUNCH_PBP(false, 1); }
    else {
        // coarse scatter: the same kernel with the coarse shifts, offsets and per-part bases, into the intermediate copy; then the refinement
        const size_t lds_c = (size_t)4 * ncmax;
#define GS_LAUNCH_PBC(AAV)                                                                                                   \
    hipLaunchKernelGGL((k_prob_partition<AAV, 1>), grid, block, lds_c, c->stream, seq, rec_start, rec_len, upre, genome_rec_off, gunits, g0, kq_of(p), vbits, d_shc, d_coff, parts, \
                       d_ccur, q, m, zone, pc, tmpv.as<uint64_t>(), dvb.as<uint64_t>())
        if (aa) GS_LAUNCH_PBC(true); else GS_LAUNCH_PBC(false);
#undef GS_LAUNCH_PBC
        hipLaunchKernelGGL(k_prob_refine, dim3(parts * ncmax, ng), dim3(PBR_T), 0, c->stream, tmpv.as<uint64_t>(), vals.as<uint64_t>(), dvb.as<uint64_t>(), vbits, dsh.as<uint32_t>(),
                           dboff.as<uint32_t>(), d_shc, d_coff, parts, hist.as<uint32_t>(), d_ccur, d_ccnt, (uint32_t)id32);
    }
#undef GS_LAUNCH_PBP
    GS_HIP_CHECK(hipGetLastError());
    DevBuf profbuf;
    if (env.profile) { if ((rc = profbuf.alloc(128))) return rc; GS_HIP_CHECK(hipMemsetAsync(profbuf.p, 0, 128, c->stream)); ch.L.prof = profbuf.as<unsigned long long>(); }
    int per_cu = 3;
    if (id32) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_prob_buckets<uint32_t>, PB2_T, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_prob_buckets<uint64_t>, PB2_T, 0);
    uint32_t lg_max = 0; while ((1u << lg_max) < nbmax) lg_max++;
    const uint32_t wgs = (uint32_t)std::min<uint64_t>((uint64_t)ng << lg_max, (uint64_t)c->n_cu * std::min(std::max(per_cu, 1), 8));     // resident workgroups only: the items are dealt statically
#define GS_LAUNCH_PBB(KT)                                                                                                     \
    hipLaunchKernelGGL(k_prob_buckets<KT>, dim3(wgs), dim3(PB2_T), 0, c->stream, vals.as<uint64_t>(), dvb.as<uint64_t>(), bst.as<uint32_t>(), bsz.as<uint32_t>(), vbits, \
                       dsh.as<uint32_t>(), dboff.as<uint32_t>(), ng, lg_max, m, zone, pc, q, thr, ch.wmax.as<uint32_t>(), ch.L, ch.ovf.as<uint32_t>(), (uint32_t)(two_level && id32))
    if (id32) GS_LAUNCH_PBB(uint32_t); else GS_LAUNCH_PBB(uint64_t);
#undef GS_LAUNCH_PBB
    if (ch.L.prof) {
        unsigned long long h[16];
        GS_HIP_CHECK(hipMemcpyAsync(h, ch.L.prof, 128, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        const double it = (double)std::max<unsigned long long>(h[7], 1);
        fprintf(stderr, "[GS_PROB_PROFILE] workgroup 0 of %u (%d per CU): %llu buckets, keys/bucket %.0f, queued %.0f, candidates %.1f | cycles per bucket: zero+thr %.0f, insert %.0f, cheap test %.0f, full points %.0f, flush %.0f\n",
                wgs, per_cu, h[7], h[8] / it, h[6] / it, h[9] / it, h[0] / it, h[1] / it, h[2] / it, h[3] / it, h[4] / it);
    }
    return ch.finish(wgs, sig_rows, redo, [](uint32_t, bool overflowed, double) { return overflowed; });      // (a bucket's table was full or a count wrapped)
}

// one chunk of genomes [g0, g0 + ng) through the tiered form; lgs = log2(buckets) per genome (host plan). redo as run_prob_buckets.
static int run_prob_tiers(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *upre,
                          const uint64_t *genome_rec_off, const uint64_t *gunits, uint64_t g0, uint32_t ng, const uint64_t *hk, const uint32_t *lgs, const ProbConst &pc,
                          const ProbEnv &env, void *sig_rows, std::vector<uint8_t> &redo, bool &no_room)
{
    const uint32_t m = p->sketch_size, k = p->k;
    no_room = false;
    const bool aa = p->data_t == GS_DATA_AA;
    const uint64_t zone = uint_zone(m);
    int rc;
    const uint32_t vbits = aa ? 5 * k : 2 * k;
    uint64_t maxk = 0; uint32_t nbmax = 1, nbt = 0;
    for (uint32_t i = 0; i < ng; i++) maxk = std::max(maxk, hk[i]);
    // parts per genome (one for the chunk), a power of two (the filter kernel deals slices to its eight wavefronts): four where the chunk has the genomes to fill the
    // device with them (fewer, longer slices: 1.11e11 k-mers/s at 4 against 0.99e11 at 16 over 256 x 5 Mbp), more for a handful of genomes - down to 8 tiles per part
    uint32_t parts = 1;
    {
        const uint64_t tiles = maxk / ((uint64_t)PT_T * 32) + 1;
        while (parts < 4 && (uint64_t)parts * 2 * 8 <= tiles) parts *= 2;
        while (parts < 32 && (uint64_t)parts * 2 * 8 <= tiles && (uint64_t)ng * parts < 2 * (uint64_t)c->n_cu) parts *= 2;
    }
    if (env.parts) parts = env.parts;
    // per genome: shift, flat bucket offset, slice capacity (mean + 5 sigma of a slice's Poisson-like fill), offset of its slices (in 4-byte ids)
    std::vector<uint32_t> info(3 * (size_t)ng + 1); std::vector<uint64_t> vbase(ng); std::vector<uint64_t> capbits(2 * (size_t)ng); std::vector<double> capd(ng);      // capbits: [ng] caps, then [ng] t_one (below)
    uint32_t *sh = info.data(), *boff = sh + ng, *cap = boff + ng + 1;
    uint64_t T32 = 0;
    for (uint32_t i = 0; i < ng; i++) {
        const uint32_t lg = lgs[i];
        sh[i] = vbits - lg; boff[i] = nbt; nbt += 1u << lg; nbmax = std::max(nbmax, 1u << lg);
        const double e = (double)hk[i] / ((double)(1u << lg) * parts);
        cap[i] = ((uint32_t)(e + 5.0 * sqrt(e) + 16.0) + 63u) & ~63u;       // (a multiple of 64: the bucket kernel reads a slice in whole wavefront trips)
        vbase[i] = T32; T32 += ((uint64_t)parts << lg) * cap[i];
        // speculative cap of max_b q[b]: the points of a genome form a process of rate N (its k-mers with multiplicity) over m slots
        const double t = (double)m / (double)hk[i] * (log((double)m) + env.cap_c);
        capd[i] = t > 0.0 ? t : 0x1.0p-1000;
        memcpy(&capbits[i], &capd[i], 8);
        // the cap as a threshold on the 52 uniform bits K of a first draw x0 = c1 K 2^-52 (k_prob_tier_filter): x0 > c cap for K > c t_one, with a margin of 2^-40 relative
        // on the safe side (+ 4: the roundings of this line and the truncation leave t_one >= the exact product + 1) - once per genome here, not per bucket and lane there
        const double t1d = capd[i] / pc.c1 * 0x1.0p52 * (1.0 + 0x1.0p-40) + 4.0;
        capbits[ng + i] = t1d < 0x1.0p52 ? (uint64_t)t1d : ((uint64_t)1 << 52);
    }
    boff[ng] = nbt;
    PoolBuf dinfo(c, SL_PROB_INFO), dvb(c, SL_PROB_VBASE), cnt(c, SL_PROB_HIST), vals(c, SL_PROB_VALS), kept(c, SL_PROBT_KEPT), desc(c, SL_PROBT_DESC), big(c, SL_PROBT_BIG);
    ProbChunk ch{c, p, ng, pc, env};
    // the list of kept ids: what the caps let through (x1 < cap as singletons) plus the false alarms of shared cells and the real repeats, with room to spare
    uint64_t kept_want = 1u << 20;
    for (uint32_t i = 0; i < ng; i++) kept_want += (uint64_t)((double)hk[i] * std::min(1.0, 1.5 * capd[i] + 0.05));
    const uint32_t kept_cap = (uint32_t)std::min<uint64_t>(kept_want, 0xFFFF0000u), big_cap = 1u << 16;
    const uint32_t pts_max = (uint32_t)c->n_cu * 32;              // blocks of the wavefront-per-bucket kernel at most (segment counts)
    if ((rc = dinfo.alloc(4 * info.size())) || (rc = dvb.alloc(8 * (size_t)ng)) || (rc = cnt.alloc((size_t)4 * nbt * parts)) || (rc = vals.alloc(4 * (size_t)T32 + 64)) ||
        (rc = kept.alloc(4 * (size_t)kept_cap + 64)) || (rc = desc.alloc(8 * (size_t)nbt)) || (rc = big.alloc(4 * (size_t)big_cap))) {
        no_room = true;                                               // (the one failure the caller answers with the older forms; anything later is an error)
        return rc;
    }
    const uint32_t *d_sh = dinfo.as<uint32_t>(), *d_boff = d_sh + ng, *d_cap = d_boff + ng + 1;
    GS_HIP_CHECK(hipMemcpyAsync(dinfo.p, info.data(), 4 * info.size(), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dvb.p, vbase.data(), 8 * (size_t)ng, hipMemcpyHostToDevice, c->stream));
    if ((rc = ch.start(16, capbits.data(), pts_max))) { no_room = ch.alloc_failed; return rc; }
    uint64_t *q = ch.q.as<uint64_t>(), *thr = ch.thr.as<uint64_t>(); uint32_t *wmax = ch.wmax.as<uint32_t>(), *ovf = ch.ovf.as<uint32_t>(), *ctr32 = ch.ctr32;
    const size_t lds = ((size_t)3 * nbmax + 8 + (size_t)PT_T * 32) * 4;
    dim3 grid(parts, ng), block(PT_T);
#define GS_LAUNCH_PT1(AAV)                                                                                                  \
    do {                                                                                                                    \
        auto kern = k_prob_part1<AAV>;                                                                                      \
        GS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));        \
        hipLaunchKernelGGL(kern, grid, block, lds, c->stream, seq, rec_start, rec_len, upre, genome_rec_off, gunits, g0, kq_of(p), vbits, d_sh, d_boff, dvb.as<uint64_t>(), d_cap, \
                           parts, vals.as<uint32_t>(), cnt.as<uint32_t>(), ovf);                                            \
    } while (0)
    if (aa) GS_LAUNCH_PT1(true);
    else if (env.two_walk) GS_LAUNCH_PT1(false);
    else {
        GS_HIP_CHECK(hipFuncSetAttribute((const void *)k_prob_part1_dna, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_prob_part1_dna, grid, block, lds, c->stream, seq, rec_start, rec_len, upre, genome_rec_off, gunits, g0, kq_of(p), vbits, d_sh, d_boff, dvb.as<uint64_t>(), d_cap,
                           parts, vals.as<uint32_t>(), cnt.as<uint32_t>(), ovf);
    }
#undef GS_LAUNCH_PT1
    GS_HIP_CHECK(hipGetLastError());
    DevBuf profbuf; unsigned long long *prof = nullptr;
    if (env.profile) { if ((rc = profbuf.alloc(128))) return rc; GS_HIP_CHECK(hipMemsetAsync(profbuf.p, 0, 128, c->stream)); prof = profbuf.as<unsigned long long>(); }
    uint32_t lg_max = 0; while ((1u << lg_max) < nbmax) lg_max++;
    const uint64_t n_items = (uint64_t)ng << lg_max;
    int f_cu = 4, w_cu = 16, b_cu = 2;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&f_cu, (const void *)k_prob_tier_filter, PT2_T, 0);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&w_cu, (const void *)k_prob_tier_points<64, 1024, false>, 64, 0);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&b_cu, (const void *)k_prob_tier_points<512, 4096, true>, 512, 0);
    const uint32_t fwgs = (uint32_t)std::min<uint64_t>(n_items, (uint64_t)c->n_cu * std::min(std::max(f_cu, 1), 8));
    const uint32_t pwgs = (uint32_t)std::min<uint64_t>(n_items, std::min<uint64_t>((uint64_t)c->n_cu * std::min(std::max(w_cu, 1), 32), pts_max));
    hipLaunchKernelGGL(k_prob_tier_filter, dim3(fwgs), dim3(PT2_T), 0, c->stream, vals.as<uint32_t>(), dvb.as<uint64_t>(), d_cap, cnt.as<uint32_t>(), parts, vbits, d_sh, d_boff, ng, lg_max,
                       pc, thr, kept.as<uint32_t>(), kept_cap, ctr32 + 5, desc.as<uint2>(), ovf, prof);
    hipLaunchKernelGGL((k_prob_tier_points<64, 1024, false>), dim3(pwgs), dim3(64), 0, c->stream, kept.as<uint32_t>(), desc.as<uint2>(), vbits, d_sh, d_boff, ng, lg_max, m, zone, pc,
                       q, thr, wmax, ch.L, ovf, big.as<uint32_t>(), ctr32 + 6, big_cap);
    hipLaunchKernelGGL((k_prob_tier_points<512, 4096, true>), dim3((uint32_t)c->n_cu * std::min(std::max(b_cu, 1), 2)), dim3(512), 0, c->stream, kept.as<uint32_t>(), desc.as<uint2>(), vbits,
                       d_sh, d_boff, ng, lg_max, m, zone, pc, q, thr, wmax, ch.L, ovf, big.as<uint32_t>(), ctr32 + 6, big_cap);
    if (prof) {
        unsigned long long h[16]; uint32_t hcn[8];
        GS_HIP_CHECK(hipMemcpyAsync(h, prof, 128, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(hcn, ch.ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        const double it = (double)std::max<unsigned long long>(h[7], 1);
        fprintf(stderr, "[GS_PROB_PROFILE] tiers: filter workgroup 0 of %u (%d per CU, %u parts; points: %u wavefronts, %d per CU): %llu buckets, keys/bucket %.0f, kept %.0f | cycles per bucket: load+zero %.0f, count %.0f, draw+queue %.0f, write %.0f | kept ids %u of %u, big buckets %u\n",
                fwgs, f_cu, parts, pwgs, w_cu, h[7], h[8] / it, h[6] / it, h[0] / it, h[1] / it, h[2] / it, h[3] / it, hcn[5], kept_cap, hcn[6]);
    }
    // the speculation is checked in the ending: q only decreases in later passes, so a maximum under the cap after pass 1 stays there
    return ch.finish(pwgs, sig_rows, redo, [&](uint32_t i, bool overflowed, double qm) {
        const bool bad = overflowed || !(qm <= capd[i]);
        if (bad && env.verbose) fprintf(stderr, "[GS_PROB] tiered form: genome %llu flagged (%s; max slot minimum %g, cap %g)\n", (unsigned long long)(g0 + i),
                                        overflowed ? "a slice, the kept-id queue or a table overflowed" : "cap not confirmed", qm, capd[i]);
        return bad;
    });
}

static int run_prob_sorted(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len,
                           uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, void *sig_out)
{
    const uint32_t m = p->sketch_size, k = p->k;
    const bool aa = p->data_t == GS_DATA_AA;
    const uint32_t vbits = aa ? 5 * k : 2 * k;
    const int sigbits = gs_value_bits(p);
    const uint64_t zone = uint_zone(m);
    const ProbConst pc = prob_const(m);
    int rc;
    PoolBuf upre(c, SL_PROBS_REC_UNITS), gunits(c, SL_PROBS_GENOME_UNITS), kpre(c, SL_PROBS_REC_KMERS), gkm(c, SL_PROBS_GENOME_KMERS);
    if ((rc = upre.alloc(8 * (n_rec + 1)))) return rc;
    if ((rc = gunits.alloc(8 * n_genomes))) return rc;
    if ((rc = kpre.alloc(8 * (n_rec + 1)))) return rc;
    if ((rc = gkm.alloc(8 * n_genomes))) return rc;
    const uint32_t gb = (uint32_t)((n_genomes + 3) / 4);                 // one wavefront per genome
    hipLaunchKernelGGL(k_unit_prefix, dim3(gb), dim3(256), 0, c->stream, rec_start, rec_len, genome_rec_off, n_genomes, k, upre.as<uint64_t>(), gunits.as<uint64_t>());
    hipLaunchKernelGGL(k_kmer_prefix, dim3(gb), dim3(256), 0, c->stream, rec_len, genome_rec_off, n_genomes, k, kpre.as<uint64_t>(), gkm.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    std::vector<uint64_t> hk(n_genomes);
    GS_HIP_CHECK(hipMemcpyAsync(hk.data(), gkm.p, 8 * n_genomes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    // chunks of genomes: the composite sort key needs log2(chunk) spare bits; memory bounds the k-mer count
    const uint64_t max_items = (uint64_t)3 << 28;                       // ~8e8 k-mers per chunk (6.4 GB of keys, twice)
    const uint64_t max_g = vbits >= 64 ? 1 : std::min<uint64_t>((uint64_t)1 << std::min<uint32_t>(64 - vbits, 16), 65535);
    const size_t row = (size_t)m * (sigbits / 8);
    for (uint64_t g0 = 0; g0 < n_genomes;) {
        uint64_t ng = 0, T = 0;
        std::vector<uint64_t> base;
        while (g0 + ng < n_genomes && ng < max_g && (ng == 0 || T + hk[g0 + ng] <= max_items)) { base.push_back(T); T += hk[g0 + ng]; ng++; }
        GS_REQUIRE(T < ((uint64_t)1 << 31), GS_ERR_UNSUPPORTED, "a single genome with more than 2^31 k-mers is not supported by the prob sketcher");
        PoolBuf dbase(c, SL_PROBS_BASE), q(c, SL_PROBS_Q), qprev(c, SL_PROBS_QPREV), sig(c, SL_PROBS_SIG), sigpass(c, SL_PROBS_SIGPASS), wmax(c, SL_PROBS_WMAX), qmax(c, SL_PROBS_QMAX), nact(c, SL_PROBS_NACT);
        if ((rc = dbase.alloc(8 * ng))) return rc;
        if ((rc = q.alloc(8 * ng * m))) return rc;
        if ((rc = qprev.alloc(8 * ng * m))) return rc;
        if ((rc = sig.alloc(8 * ng * m))) return rc;
        if ((rc = sigpass.alloc(8 * ng * m))) return rc;
        if ((rc = wmax.alloc(4 * ng))) return rc;
        if ((rc = qmax.alloc(8 * ng))) return rc;
        if ((rc = nact.alloc(64))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(dbase.p, base.data(), 8 * ng, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_prob_init, dim3(c->n_cu * 4), dim3(256), 0, c->stream, q.as<uint64_t>(), qprev.as<uint64_t>(), sig.as<uint64_t>(), sigpass.as<uint64_t>(), ng * (uint64_t)m);
        GS_HIP_CHECK(hipMemsetAsync(wmax.p, 0, 4 * ng, c->stream));
        {   // qmax = +inf
            std::vector<double> inf(ng, INFINITY);
            GS_HIP_CHECK(hipMemcpyAsync(qmax.p, inf.data(), 8 * ng, hipMemcpyHostToDevice, c->stream));
            GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        if (T > 0) {
            PoolBuf vals(c, SL_PROBS_VALS), sorted(c, SL_PROBS_SORTED), ucnt(c, SL_PROBS_UCNT), nruns(c, SL_PROBS_NRUNS), tmp(c, SL_PROBS_RADIX), candh(c, SL_PROBS_CAND_H), candb(c, SL_PROBS_CAND_B);
            if ((rc = vals.alloc(8 * T))) return rc;
            if ((rc = sorted.alloc(8 * T))) return rc;
            const uint64_t avg_units = (aa ? seq_bytes / 32 : seq_bytes / 8) / n_genomes + 1;
            uint32_t parts = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(avg_units / SK_THREADS + 1, (4 * (uint64_t)c->n_cu + ng - 1) / ng));
            {
                ProfScope ps(c, FAM_SKETCH);
                dim3 grid(parts, (uint32_t)ng), block(SK_THREADS);
                if (aa) hipLaunchKernelGGL(k_emit_values<true>, grid, block, 0, c->stream, seq, rec_start, rec_len, upre.as<uint64_t>(), kpre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(), dbase.as<uint64_t>(), g0, kq_of(p), vbits, vals.as<uint64_t>());
                else hipLaunchKernelGGL(k_emit_values<false>, grid, block, 0, c->stream, seq, rec_start, rec_len, upre.as<uint64_t>(), kpre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(), dbase.as<uint64_t>(), g0, kq_of(p), vbits, vals.as<uint64_t>());
                GS_HIP_CHECK(hipGetLastError());
            }
            int endbit = 64;
            if (vbits < 64) { endbit = (int)vbits; uint64_t x = ng - 1; while (x) { endbit++; x >>= 1; } if (endbit > 64) endbit = 64; }
            // multiplicities = run lengths of the sorted (genome, value) keys: own LSD radix sort + run-length encoding (gs_radix.hip)
            PoolBuf pos(c, SL_PROBS_POS);
            if ((rc = tmp.alloc(radix_scratch_bytes(T)))) return rc;
            if ((rc = pos.alloc(4 * T))) return rc;
            uint64_t *srt = nullptr;
            if ((rc = radix_sort_u64(c, vals.as<uint64_t>(), sorted.as<uint64_t>(), T, endbit, tmp.p, &srt))) return rc;
            // distinct elements + multiplicities: the unique keys go to the buffer the sorted keys are NOT in, which the rest of the pass calls `vals`
            if (srt == vals.as<uint64_t>()) { std::swap(vals.p, sorted.p); std::swap(vals.bytes, sorted.bytes); }
            if ((rc = ucnt.alloc(4 * T))) return rc;
            if ((rc = nruns.alloc(64))) return rc;
            if ((rc = run_length_encode_u64(c, sorted.as<uint64_t>(), T, vals.as<uint64_t>(), ucnt.as<uint32_t>(), nruns.as<uint32_t>(), pos.as<uint32_t>(), tmp.p))) return rc;
            uint32_t ne32 = 0;
            GS_HIP_CHECK(hipMemcpyAsync(&ne32, nruns.p, 4, hipMemcpyDeviceToHost, c->stream));
            GS_HIP_CHECK(hipStreamSynchronize(c->stream));
            const uint64_t ne = ne32;
            sorted.release();
            if ((rc = candh.alloc(8 * ne))) return rc;
            if ((rc = candb.alloc(4 * ne))) return rc;
            const uint32_t eg = (uint32_t)std::min<uint64_t>((ne + 255) / 256, (uint64_t)c->n_cu * 16);
            const uint32_t ACT_CAP = 1u << 24;                       // 16 M live elements keep their generator state (0.5 GB)
            PoolBuf akey(c, SL_PROBS_AKEY), acnt(c, SL_PROBS_ACNT), astate(c, SL_PROBS_ASTATE), nlist(c, SL_PROBS_NLIST);
            uint32_t n_list = 0; bool use_list = false;
            for (uint32_t it = 1;; it++) {
                GS_HIP_CHECK(hipMemsetAsync(nact.p, 0, 4, c->stream));
                if (!use_list) {
                    hipLaunchKernelGGL(k_prob_point, dim3(eg), dim3(256), 0, c->stream, vals.as<uint64_t>(), ucnt.as<uint32_t>(), ne, vbits, m, zone, pc, it, qmax.as<double>(),
                                       q.as<uint64_t>(), candh.as<uint64_t>(), candb.as<uint32_t>(), it == 1 ? wmax.as<uint32_t>() : nullptr);
                    hipLaunchKernelGGL(k_prob_claim, dim3(eg), dim3(256), 0, c->stream, vals.as<uint64_t>(), ne, vbits, m, q.as<uint64_t>(), candh.as<uint64_t>(), candb.as<uint32_t>(), sigpass.as<uint64_t>());
                } else {
                    const uint32_t lg = std::max<uint32_t>(1, std::min<uint32_t>((n_list + 255) / 256, (uint32_t)c->n_cu * 16));
                    hipLaunchKernelGGL(k_prob_point_list, dim3(lg), dim3(256), 0, c->stream, akey.as<uint64_t>(), acnt.as<uint32_t>(), n_list, ACT_CAP, vbits, m, zone, pc, it,
                                       qmax.as<double>(), q.as<uint64_t>(), astate.as<uint64_t>(), candh.as<uint64_t>(), candb.as<uint32_t>());
                    hipLaunchKernelGGL(k_prob_claim, dim3(lg), dim3(256), 0, c->stream, akey.as<uint64_t>(), (uint64_t)n_list, vbits, m, q.as<uint64_t>(), candh.as<uint64_t>(), candb.as<uint32_t>(), sigpass.as<uint64_t>());
                }
                hipLaunchKernelGGL(k_prob_fold, dim3((uint32_t)ng), dim3(256), 0, c->stream, m, it, q.as<uint64_t>(), qprev.as<uint64_t>(), sig.as<uint64_t>(), sigpass.as<uint64_t>(),
                                   wmax.as<uint32_t>(), qmax.as<double>(), nact.as<uint32_t>());
                GS_HIP_CHECK(hipGetLastError());
                uint32_t na = 0;
                GS_HIP_CHECK(hipMemcpyAsync(&na, nact.p, 4, hipMemcpyDeviceToHost, c->stream));
                GS_HIP_CHECK(hipStreamSynchronize(c->stream));
                if (na == 0) break;
                if (it == 1) {      // survivors of pass 1 -> compact list with generator state (falls back to replay when it overflows)
                    if ((rc = nlist.alloc(64))) return rc;
                    if ((rc = akey.alloc(8 * (size_t)ACT_CAP))) return rc;
                    if ((rc = acnt.alloc(4 * (size_t)ACT_CAP))) return rc;
                    if ((rc = astate.alloc(32 * (size_t)ACT_CAP))) return rc;
                    GS_HIP_CHECK(hipMemsetAsync(nlist.p, 0, 4, c->stream));
                    hipLaunchKernelGGL(k_prob_compact, dim3(eg), dim3(256), 0, c->stream, vals.as<uint64_t>(), ucnt.as<uint32_t>(), ne, vbits, m, zone, pc, qmax.as<double>(), ACT_CAP,
                                       nlist.as<uint32_t>(), akey.as<uint64_t>(), acnt.as<uint32_t>(), astate.as<uint64_t>());
                    GS_HIP_CHECK(hipGetLastError());
                    GS_HIP_CHECK(hipMemcpyAsync(&n_list, nlist.p, 4, hipMemcpyDeviceToHost, c->stream));
                    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
                    use_list = n_list <= ACT_CAP;
                }
            }
        }
        if ((rc = prob_write_rows(c, sigbits, q.as<uint64_t>(), sig.as<uint64_t>(), ng * (uint64_t)m, (uint8_t *)sig_out + row * g0))) return rc;
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        g0 += ng;
    }
    return GS_OK;
}

// [lo, hi) in maximal runs on which `flag` keeps one value: fn(a, b, that value) per run [a, b), until one fails
template <class Flag, class Fn>
static int prob_each_run(uint64_t lo, uint64_t hi, Flag flag, Fn fn)
{
    for (uint64_t a = lo, b; a < hi; a = b) {
        const bool v = flag(a);
        for (b = a + 1; b < hi && flag(b) == v; b++) {}
        if (const int rc = fn(a, b, v)) return rc;
    }
    return GS_OK;
}
// One form over the genomes [lo, hi): the runs it suits in chunks, grown while they have fewer than 65535 genomes (a grid's rows) and their k-mers fit the budget -
// chunk(g0, g1, redo) runs one and flags what must be redone; the flagged genomes and the runs the form does not suit go to next(a, b, flagged)
template <class Suits, class Chunk, class Next>
static int prob_form_range(uint64_t lo, uint64_t hi, const std::vector<uint64_t> &hk, uint64_t budget, Suits suits, Chunk chunk, Next next)
{
    return prob_each_run(lo, hi, suits, [&](uint64_t r0, uint64_t r1, bool suited) -> int {
        if (!suited) return next(r0, r1, false);
        for (uint64_t g0 = r0, g1; g0 < r1; g0 = g1) {
            uint64_t T = hk[g0];
            for (g1 = g0 + 1; g1 < r1 && g1 - g0 < 65535 && T + hk[g1] <= budget; g1++) T += hk[g1];
            std::vector<uint8_t> redo;
            int rc = chunk(g0, g1, redo);
            if (!rc) rc = prob_each_run(g0, g1, [&](uint64_t g) { return redo[g - g0] != 0; }, [&](uint64_t a, uint64_t b, bool flagged) -> int { return flagged ? next(a, b, true) : GS_OK; });
            if (rc) return rc;
        }
        return GS_OK;
    });
}

// prob driver: runs of genomes the tiered form suits go through it in chunks; what it flags, and the genomes it does not suit, go through the bucketed form
// (chunks again), and what that one flags or does not suit through the sorted form
int run_prob(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len,
             uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, void *sig_out)
{
    const uint32_t m = p->sketch_size, k = p->k;
    const ProbEnv env = prob_env();
    if (env.sort) return run_prob_sorted(c, p, seq, seq_bytes, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, sig_out);
    const ProbConst pc = prob_const(m);
    int rc;
    PoolBuf upre(c, SL_PROB_REC_UNITS), gunits(c, SL_PROB_GENOME_UNITS), kpre(c, SL_PROB_REC_KMERS), gkm(c, SL_PROB_GENOME_KMERS);   // (alive around the forms below: slots of their own)
    if ((rc = upre.alloc(8 * (n_rec + 1))) || (rc = gunits.alloc(8 * n_genomes)) || (rc = kpre.alloc(8 * (n_rec + 1))) || (rc = gkm.alloc(8 * n_genomes))) return rc;
    const uint32_t gb = (uint32_t)((n_genomes + 3) / 4);
    hipLaunchKernelGGL(k_unit_prefix, dim3(gb), dim3(256), 0, c->stream, rec_start, rec_len, genome_rec_off, n_genomes, k, upre.as<uint64_t>(), gunits.as<uint64_t>());
    hipLaunchKernelGGL(k_kmer_prefix, dim3(gb), dim3(256), 0, c->stream, rec_len, genome_rec_off, n_genomes, k, kpre.as<uint64_t>(), gkm.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    std::vector<uint64_t> hk(n_genomes);
    GS_HIP_CHECK(hipMemcpyAsync(hk.data(), gkm.p, 8 * n_genomes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t row = (size_t)m * (gs_value_bits(p) / 8);
    auto suits = [&](uint64_t g) { return hk[g] >= (uint64_t)64 * m && hk[g] <= (uint64_t)PB_NBMAX * PB_AVG; };
    // tiered form: the in-bucket id must fit 4 bytes (>= vbits - 31 bucket bits), <= 2^PT_LGMAX buckets of PT_MINB .. 3 PT_AVG k-mers
    const uint32_t vbits = p->data_t == GS_DATA_AA ? 5 * k : 2 * k;
    std::vector<uint32_t> lgs(n_genomes, 0xFFFFFFFFu);
    if (env.tiers && vbits <= 31 + (uint32_t)PT_LGMAX)
        for (uint64_t g = 0; g < n_genomes; g++) {
            if (hk[g] < (uint64_t)64 * m) continue;
            uint32_t lg = vbits > 31 ? vbits - 31 : 0;
            while ((env.pt_avg << lg) < hk[g] && lg < (uint32_t)PT_LGMAX && lg + 1 < vbits) lg++;
            if ((hk[g] >> lg) >= (uint64_t)PT_MINB && (hk[g] >> lg) <= 3 * env.pt_avg) lgs[g] = lg;
        }
    auto suits_tiers = [&](uint64_t g) { return lgs[g] != 0xFFFFFFFFu; };
    const uint64_t max_items = (uint64_t)3 << 29;                 // ~1.6e9 k-mers per chunk (12.9 GB of bucketed values)
    // the tiered form's chunks: ~8 bytes of scratch per k-mer (slices of 4-byte ids with their slack, kept ids, lists), so twice the k-mers of a bucketed chunk where a quarter of
    // the free device memory holds them (2048 x 5 Mbp: 1.07e11 k-mers/s at 1.6e9 per chunk, 1.11e11 at 3.2e9, 1.13e11 at 6.4e9 - a chunk ends in a host round trip)
    uint64_t tier_items = 2 * max_items;
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) tier_items = std::min<uint64_t>(tier_items, std::max<uint64_t>(max_items / 4, (uint64_t)fr / 4 / 8));
        else (void)hipGetLastError();
        if (env.chunk_kmers) tier_items = env.chunk_kmers;
    }
    // the sorted form, the last way down (no lease of the other forms is alive here: its slots share their memory)
    auto sorted_range = [&](uint64_t a, uint64_t b, bool) -> int {
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return run_prob_sorted(c, p, seq, seq_bytes, rec_start, rec_len, n_rec, genome_rec_off + a, b - a, (uint8_t *)sig_out + row * a);
    };
    // [a, b) through the bucketed form where it suits, else (and what it flags) through the sorted form
    auto old_range = [&](uint64_t a, uint64_t b) -> int {
        return prob_form_range(a, b, hk, max_items, suits, [&](uint64_t g0, uint64_t g1, std::vector<uint8_t> &redo) -> int {
            return run_prob_buckets(c, p, seq, rec_start, rec_len, upre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(), g0, (uint32_t)(g1 - g0), hk.data() + g0, pc, env,
                                    (uint8_t *)sig_out + row * g0, redo);
        }, sorted_range);
    };
    rc = prob_form_range(0, n_genomes, hk, tier_items, suits_tiers, [&](uint64_t g0, uint64_t g1, std::vector<uint8_t> &redo) -> int {
        bool no_room = false;
        const int rc = run_prob_tiers(c, p, seq, rec_start, rec_len, upre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(), g0, (uint32_t)(g1 - g0), hk.data() + g0, lgs.data() + g0, pc, env,
                                      (uint8_t *)sig_out + row * g0, redo, no_room);
        if (!(rc && no_room)) return rc;
        // its scratch did not fit (an index with its pair cache beside the sketcher): the chunk takes the older forms, which work in smaller chunks and have their own ways down
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        if (env.verbose) fprintf(stderr, "[GS_PROB] tiered form: no room for the scratch of genomes [%llu, %llu) (%s): the bucketed form takes them\n", (unsigned long long)g0,
                                 (unsigned long long)g1, gs_last_error());
        redo.assign(g1 - g0, 1);
        return GS_OK;
    }, [&](uint64_t a, uint64_t b, bool flagged) -> int {             // flagged: a slice / table overflow, cap not confirmed - the exact fallback
        if (flagged) {
            GS_HIP_CHECK(hipStreamSynchronize(c->stream));
            if (env.verbose) fprintf(stderr, "[GS_PROB] tiered form flagged genomes [%llu, %llu): redone by the bucketed form\n", (unsigned long long)a, (unsigned long long)b);
        }
        return old_range(a, b);
    });
    if (rc) return rc;
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

}  // namespace gs
