// gs_sketch.hip — k-mer extraction + MinHash-family sketching on gfx950.
//
// Replaces, at batch level, SeqSketcherT::sketch_compressedkmer{,_seqs} (call sites
// /root/reference/src/dna/dnasketch.rs:336,357, src/dna/dnarequest.rs:272,287, src/aa/aasketch.rs:313,329,
// src/aa/aarequest.rs:268,283) together with the kmer_hash_fn closures (dnasketch.rs:164-169,
// aasketch.rs:156-160) and the probminhash sketchers they feed. Arithmetic: SPEC.md 1-3. The k-mer walkers are in gs_walk.hpp, the
// ProbMinHash3a sketcher (run_prob) in gs_prob.hip; the slot-min, SuperMinHash, SetSketch and HyperMinHash sketchers and the entry points are here.
//
// Layout: a genome is a flat range of 32-symbol "units" (DNA: one 8-byte packed word, AA: 32 bytes).
// One workgroup (or `parts` workgroups) per genome; every lane owns one unit per iteration, rebuilds the
// rolling forward / reverse-complement state from the k-1 symbols before it, and pushes every valid
// k-mer through the element hash into an m-slot min table held in LDS (ds_min_u32). HBM traffic is the
// algorithmic minimum: each packed word is read once (plus an L1/L2-served halo word) and m slots written.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"
#include "gs_skq.hpp"
#include "gs_hiword.hpp"
#include "gs_walk.hpp"

namespace gs {

#define GS_EMPTY32 0xFFFFFFFFu

__constant__ uint8_t c_aa_code[32] = {
    // index = ASCII & 31 : @ A B C D E F G H I J K L M N O P Q R S T U V W X Y Z ...
    0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 0, 8, 9, 10, 11, 0, 12, 13, 14, 15, 16, 0, 17, 18, 0, 19, 0, 0, 0, 0, 0, 0};

// per-record unit counts -> exclusive prefix inside each genome (one thread per genome; record lists are short)
__global__ void k_unit_prefix(const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *genome_rec_off,
                              uint64_t n_genomes, uint32_t k, uint64_t *rec_upre, uint64_t *gen_units)
{
    // one wavefront per genome, 64 records per trip (a proteome has thousands of records: a serial loop of dependent loads per
    // genome cost more than sketching it)
    const uint64_t g = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1];
    uint64_t base = 0;
    for (uint64_t rb = r0; rb < r1; rb += 64) {
        const uint64_t r = rb + lane;
        uint64_t u = 0;
        if (r < r1) { const uint64_t len = rec_len[r]; if (len >= k) { const uint64_t s = rec_start[r]; u = ((s + len - 1) >> 5) - (s >> 5) + 1; } }
        uint64_t inc = u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
        if (r < r1) rec_upre[r] = base + inc - u;
        base += __shfl(inc, 63);
    }
    if (lane == 0) gen_units[g] = base;
}

// level-0 candidate of every slot-min sketcher (SPEC 3.1 / 3.2): element hash -> (key, slot) -> min.
//   optdens, revoptdens, super : key = 23-bit mantissa of U32f          (T = u32)
//   super2 / u32               : key = next32                            (T = u32)
//   super2 / u64               : key = next64                            (T = u64)
template <int ALGO, int VBITS, typename T, bool LDS_TABLE>
struct MinEmit {
    T *table; uint32_t m; uint64_t zone;
    uint16_t *bound;              // !LDS_TABLE: per-slot upper bound (top 16 bits) of this workgroup's minima, in LDS
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t /*rec*/, uint64_t /*pos*/) const
    {
        uint64_t o1; uint32_t b;
        two_draw(elem_hash<ALGO, VBITS>(v), m, zone, o1, b);
        T key;
        if (ALGO == ALGO_SUPER2) key = sizeof(T) == 8 ? (T)o1 : (T)(o1 >> 32);
        else key = (T)(o1 >> 41);
        if (LDS_TABLE) atomicMin(&table[b], key);
        else {
            // The slot table does not fit in LDS (e.g. 24000 x u64 = 192 kB): it lives in global memory, but a 2-byte LDS filter
            // keeps all but the ~ln(n)/n fraction of k-mers that can still lower a minimum away from it. bound[b] only ever holds
            // the top bits of a key this workgroup has applied, so it is >= the top bits of the true minimum: skipping keys whose
            // top bits exceed it is exact; plain (racy) 16-bit stores can only leave it staler, i.e. more conservative.
            const uint16_t hi = (uint16_t)(key >> (8 * sizeof(T) - 16));
            if (hi <= bound[b]) { atomicMin(&table[b], key); bound[b] = hi; }
        }
    }
};

// Filtered form of MinEmit for an LDS-resident slot table. The key of a k-mer only needs two of the three SplitMix64
// outputs (o1 = f(s0, s3)); its slot needs the third and the second xoshiro output. A key that is not below `thr` - an upper bound of
// EVERY slot's current minimum, refreshed from the table now and then - cannot lower any slot, whichever slot it falls in, so the rest
// of its arithmetic is skipped: exact. Lanes diverge on that test, so the survivors (a few % once the table has warmed up) are
// compacted through a per-wave LDS queue of element hashes and finished 64 at a time by the whole wave. Only full waves use the queue
// (its fill count stays wave-uniform in a register); record boundaries and partial waves take the direct form.
// The queue holds SKQ = 128 hashes per wave (gs_skq.hpp): fewer than 64 pending and at most 64 new ones; the k-mers of an interior word come two at
// a time and share one push (full2). An entry is h + gamma alone: carrying s0 or s3 beside it (16-byte entries, 64 of them, a push split around the
// flush) spares the flush a mix and was measured slower - DESIGN.md 3.1, "One push per pair of k-mers".
template <int ALGO, int VBITS, typename T>
struct MinEmitF {
    T *table; uint32_t m; uint64_t zone;
    uint64_t *q;                                  // this wave's queue
    uint32_t lane;
    mutable uint32_t qn, words;                   // wave-uniform: pending survivors, full-wave words walked
    mutable T thr;                                // wave-uniform: every slot's minimum is <= thr
    // Round 5, the SPECULATIVE bound: `thr` starts at - and never exceeds - `cap`, a guess of where the largest slot minimum of THIS genome will end
    // ((m / N)(ln m + c): the coupon-collector tail of N k-mers over m slots). Every k-mer whose key is not below the cap is dropped from the first word
    // on - no warm-up during which everything passes, ~6 % survivors instead of the ~15 % a running maximum lets through over a 5 Mbp genome - and the
    // kernel CHECKS the guess afterwards: a slot whose minimum is below the cap has seen every k-mer that could matter to it (only keys >= cap were
    // dropped), a slot that is not sends the workgroup through the genome again under the running bound alone (same table: minima are idempotent).
    // The cap is a performance parameter only - the signature never depends on it. EMPTY = no cap.
    T cap;
    mutable uint32_t lim;                         // wave-uniform: limit_of(thr), what the drop test compares with
    static __device__ __forceinline__ T key_of(uint64_t o1)
    {
        if (ALGO == ALGO_SUPER2) return sizeof(T) == 8 ? (T)o1 : (T)(o1 >> 32);
        return (T)(o1 >> 41);
    }
    static __device__ __forceinline__ T direct_above()        // survivor rate >= 1/4: the queue costs more than it saves (break-even ~0.34)
    {
        if (ALGO == ALGO_SUPER2) return (T)((T)1 << (8 * sizeof(T) - 2));
        return (T)((T)1 << 21);
    }
    __device__ __forceinline__ void apply(uint64_t h) const
    {
        uint64_t o1; uint32_t b;
        two_draw(h, m, zone, o1, b);
        atomicMin(&table[b], key_of(o1));
    }
    // The drop test, on the high word of s0 and nine bits of s3's alone (gs_hiword.hpp): `lim` is the bound of the key form plus the slack of
    // everything the other bits can add to hi32(o1), so a k-mer whose key is below thr always passes and 0.78 % of all k-mers pass beside them - their
    // exact key, rebuilt from the queued hash in the flush, decides. Only full() / full2() ask, and only while thr < direct_above(), so no limit overflows.
    static __device__ __forceinline__ uint32_t limit_of(T t)
    {
        uint32_t l;
        if (ALGO == ALGO_SUPER2) l = sizeof(T) == 8 ? hiword_limit_x_u64((uint64_t)t) : hiword_limit_x_u32((uint32_t)t);
        else l = hiword_limit_x_r23((uint32_t)t);
        return (uint32_t)__builtin_amdgcn_readfirstlane(l);
    }
    __device__ __forceinline__ bool key_below(uint32_t s0_hi, uint32_t s3_x) const
    {
        return hiword_may_be_below_x(s0_hi, s3_x, lim);
    }
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const { apply(elem_hash<ALGO, VBITS>(v)); }
    // The lanes of `bal` (bal != 0) queue a hash each - hg_a where in_a, hg_b where in_b, never both; 64 pending survivors are flushed on the way.
    __device__ __forceinline__ void push(uint64_t bal, bool in_a, uint64_t hg_a, bool in_b, uint64_t hg_b) const
    {
        // the slot is qn + the lanes below that pass: qn rides in the mbcnt pair's addend, and with the wave's queue base uniform
        // (an SGPR) the LDS address is one v_lshl_add_u32 - instead of two shifts and a v_add3_u32
        const uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, qn));
        // two masked writes, kept apart: merged into one write of a selected hash they would cost two v_cndmask_b32, and the kernel is bound
        // by VALU issue, not by LDS writes
        if (in_a) q[idx] = hg_a;
        asm volatile("" ::: "memory");
        if (in_b) q[idx] = hg_b;
        const SkqPush p = skq_push(qn, (uint32_t)__popcll(bal));
        if (p.flush) {
            apply(q[lane] - GS_GAMMA);
            const uint64_t mv = q[SKQ_FLUSH + lane];
            if (lane < p.pending) q[lane] = mv;
        }
        qn = p.pending;
    }
    // h + gamma of a k-mer
    static __device__ __forceinline__ uint64_t hash_gamma(uint64_t v)
    {
        // one hash chain: h + gamma straight from the element hash (gamma rides in the addend of its low v_mad_u64_u32), h + 4 gamma from
        // that (one v_lshl_add_u64), and the queue holds h + gamma - instead of h, h + gamma and h + 4 gamma each from h (-1 mad, -1 add3)
        uint64_t hg = elem_hash<ALGO, VBITS>(v, GS_GAMMA);
        asm("" : "+v"(hg));         // opaque: the compiler would otherwise rebuild h beside h + gamma and derive h + 4 gamma from h
        return hg;
    }
    // the key only needs two of the three SplitMix64 outputs, and the test only their high words
    __device__ __forceinline__ bool filter(uint64_t hg) const
    {
        return key_below(splitmix_mix_hi(hg), splitmix_mix_hi9(hg + 3 * GS_GAMMA));
    }
    __device__ __forceinline__ void full(uint64_t v) const
    {
        const uint64_t hg = hash_gamma(v);
        if (thr >= direct_above()) { apply(hg - GS_GAMMA); return; }            // wave-uniform
        const bool pass = filter(hg);
        const uint64_t bal = __ballot(pass);
        if (bal) push(bal, pass, hg, false, hg);
    }
    // Two k-mers, ONE push for the lanes where either survives. At ~7 % survivors a wave of 64 lanes nearly always holds one, so the push -
    // ballot, mbcnt pair, address, masked write, fill count, flush test - ran per k-mer; the lanes where BOTH survive (a wave holds one in
    // about a quarter of the pairs) push their second hash behind a wave-uniform branch. The survivors reach the table in another order
    // than one by one, which a slot minimum does not see.
    __device__ __forceinline__ void full2(uint64_t v_a, uint64_t v_b) const
    {
        const uint64_t hg_a = hash_gamma(v_a), hg_b = hash_gamma(v_b);
        if (thr >= direct_above()) { apply(hg_a - GS_GAMMA); apply(hg_b - GS_GAMMA); return; }            // wave-uniform
        const bool pass_a = filter(hg_a), pass_b = filter(hg_b);
        const uint64_t bal_a = __ballot(pass_a), bal_b = __ballot(pass_b);
        if (bal_a | bal_b) {
            // the compares leave lane masks in SGPR pairs: only b / both are scalar operations on them
            push(bal_a | bal_b, pass_a, hg_a, pass_b && !pass_a, hg_b);
            if (bal_a & bal_b) push(bal_a & bal_b, pass_a && pass_b, hg_b, false, hg_b);
        }
    }
    __device__ __forceinline__ void word_done() const
    {
        words++;
        if (cap != (T)~(T)0) { if ((words & 63u) != 0) return; }                                             // under a cap the running maximum only matters late in the genome
        else if (words <= 8 ? (words & (words - 1)) != 0 : (words & (words <= 128 ? 7 : 15)) != 0) return;     // 1, 2, 4, 8, then every 8th word, every 16th after 128
        T mx = 0;
        for (uint32_t i = lane; i < m; i += 64) { const T x = table[i]; mx = x > mx ? x : mx; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const T y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
        // every lane holds the same maximum; taken through an SGPR so that the compiler knows it too: the filter test compares against a scalar
        // and the branch to the direct form is a scalar one
        thr = uniform(mx < cap ? mx : cap);
        lim = limit_of(thr);
    }
    static __device__ __forceinline__ T uniform(T x)
    {
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
        if (sizeof(T) == 4) return (T)lo;
        return (T)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32)) << 32) | lo);
    }
    __device__ __forceinline__ void finish() const
    {
        if (lane < qn) apply(q[lane] - GS_GAMMA);
        qn = 0;
    }
};
template <int ALGO, int VBITS, typename T> __device__ __forceinline__ void emit_full_wave(const MinEmitF<ALGO, VBITS, T> &e, uint64_t v, uint64_t, uint64_t) { e.full(v); }
template <int ALGO, int VBITS, typename T> __device__ __forceinline__ void emit_full_wave2(const MinEmitF<ALGO, VBITS, T> &e, uint64_t v_a, uint64_t v_b, uint64_t, uint64_t) { e.full2(v_a, v_b); }
template <int ALGO, int VBITS, typename T> __device__ __forceinline__ void emit_word_done(const MinEmitF<ALGO, VBITS, T> &e) { e.word_done(); }
template <int ALGO, int VBITS, typename T> __device__ __forceinline__ void emit_finish(const MinEmitF<ALGO, VBITS, T> &e) { e.finish(); }

// ---- main kernel of optdens / revoptdens / super / super2: per-slot minimum over all k-mers (SPEC 3.1, 3.2 level 0)
template <bool AA, bool LDS_TABLE, int ALGO, int VBITS, typename T, bool FILT, int RCM = 0>
__global__ __launch_bounds__(SK_THREADS) void k_sketch_min(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start,
                                                            const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ rec_upre,
                                                            const uint64_t *__restrict__ genome_rec_off, const uint64_t *__restrict__ gen_units,
                                                            uint32_t k, uint32_t m, uint64_t zone, T *__restrict__ table_out, float cap_c)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_raw_table[];
    T *s_table = (T *)s_raw_table;
    const T EMPTY = (T)~(T)0;
    const uint64_t g = blockIdx.y;
    const uint32_t part = blockIdx.x, parts = gridDim.x;
    T *gtab = table_out + g * (uint64_t)m;
    T *table = LDS_TABLE ? s_table : gtab;
    uint16_t *s_bound = (uint16_t *)s_raw_table;
    if (LDS_TABLE) {
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) s_table[i] = EMPTY;
        __syncthreads();
    } else {
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) s_bound[i] = 0xFFFFu;
        __syncthreads();
    }
    if (FILT) {
        uint64_t *qbase = (uint64_t *)(s_raw_table + (((size_t)m * sizeof(T) + 15) & ~(size_t)15));
        // speculative bound (MinEmitF::cap): whole genomes only (a part's table is not the genome's), and only where it is a real cut (< 1/4 of the key range)
        T cap = EMPTY;
        if (LDS_TABLE && parts == 1 && cap_c != 0.0f) {
            const float nk = (float)gen_units[g] * 32.0f;                        // k-mers of the genome, from above
            const float frac = (float)m / nk * (__logf((float)m) + cap_c);
            if (frac > 0.0f && frac < 0.25f) {
                const float scale = ALGO == ALGO_SUPER2 ? (sizeof(T) == 8 ? 0x1.0p64f : 0x1.0p32f) : 0x1.0p23f;
                cap = (T)(frac * scale);
            }
        }
        for (int pass = 0; pass < 2; pass++) {
            MinEmitF<ALGO, VBITS, T> emit{table, m, zone, qbase + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * SKQ, threadIdx.x & 63, 0u, 0u, cap, cap, MinEmitF<ALGO, VBITS, T>::limit_of(cap)};
            walk_genome<AA, MinEmitF<ALGO, VBITS, T>, RCM>(seq, rec_start, rec_len, rec_upre, genome_rec_off[g], genome_rec_off[g + 1], gen_units[g], k, part, parts, emit);
            if (cap == EMPTY) break;
            __syncthreads();
            int bad = 0;
            for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) bad |= (int)(s_table[i] >= cap);
            if (!__syncthreads_or(bad)) break;                                   // every slot's minimum lies below the cap: nothing that was dropped could have mattered
            cap = EMPTY;                                                         // (~1 genome in 1000 at c = 7: once more, under the running bound alone)
        }
    } else {
        MinEmit<ALGO, VBITS, T, LDS_TABLE> emit{table, m, zone, s_bound};
        walk_genome<AA, MinEmit<ALGO, VBITS, T, LDS_TABLE>, RCM>(seq, rec_start, rec_len, rec_upre, genome_rec_off[g], genome_rec_off[g + 1], gen_units[g], k, part, parts, emit);
    }
    if (LDS_TABLE) {
        __syncthreads();
        if (parts == 1) { for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) gtab[i] = s_table[i]; }
        else { for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) { T v = s_table[i]; if (v != EMPTY) atomicMin(&gtab[i], v); } }
    }
}

// ---- finish: u32 min table -> f32 signature, densification of empty bins (cold path) ----------------
template <int ALGO>
__global__ __launch_bounds__(256) void k_oph_finish(const uint32_t *__restrict__ table, uint32_t m, uint64_t zone,
                                                     uint32_t *__restrict__ win_scratch, float *__restrict__ sig)
{
    __shared__ uint32_t s_filled, s_nempty;
    const uint64_t g = blockIdx.x;
    const uint32_t *slot = table + g * (uint64_t)m;
    float *out = sig + g * (uint64_t)m;
    if (threadIdx.x == 0) s_filled = 0;
    __syncthreads();
    uint32_t loc = 0;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) loc += (slot[i] != GS_EMPTY32);
    if (loc) atomicAdd(&s_filled, loc);
    __syncthreads();
    const uint32_t nf = s_filled;
    if (nf == m) { for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) out[i] = (float)slot[i] * 0x1.0p-23f; return; }
    if (nf == 0) { for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) out[i] = 1.0f; return; }
    if (ALGO == ALGO_OPTDENS) {
        for (uint32_t b = threadIdx.x; b < m; b += blockDim.x) {
            uint32_t v = slot[b];
            if (v == GS_EMPTY32) {
                Rng rg; rg.seed((uint64_t)b);
                for (;;) { uint32_t j = (uint32_t)rng_uint(rg, (uint64_t)m, zone); v = slot[j]; if (v != GS_EMPTY32) break; }
            }
            out[b] = (float)v * 0x1.0p-23f;
        }
    } else {
        uint32_t *dens = (uint32_t *)out;            // u32 image until the final conversion
        uint32_t *win = win_scratch + g * (uint64_t)m;
        for (uint32_t b = threadIdx.x; b < m; b += blockDim.x) dens[b] = slot[b];
        if (threadIdx.x == 0) s_nempty = m - nf;
        __syncthreads();
        for (uint64_t t = 0; s_nempty > 0; t++) {
            for (uint32_t b = threadIdx.x; b < m; b += blockDim.x) win[b] = GS_EMPTY32;
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < m; j += blockDim.x) {
                if (slot[j] == GS_EMPTY32) continue;
                Rng rg; rg.seed(((uint64_t)j << 20) + t);
                uint32_t i = (uint32_t)rng_uint(rg, (uint64_t)m, zone);
                if (dens[i] == GS_EMPTY32) atomicMin(&win[i], j);
            }
            __syncthreads();
            uint32_t got = 0;
            for (uint32_t b = threadIdx.x; b < m; b += blockDim.x) if (win[b] != GS_EMPTY32) { dens[b] = slot[win[b]]; got++; }
            if (got) atomicSub(&s_nempty, got);
            __syncthreads();
        }
        for (uint32_t b = threadIdx.x; b < m; b += blockDim.x) out[b] = (float)dens[b] * 0x1.0p-23f;
    }
}

// ---- super / super2 finish: every slot filled at level 0 (always true at BASELINE sizes) -> done; otherwise the genome
// is flagged for the exact sequential walk below.
template <int ALGO, typename T>
__global__ __launch_bounds__(256) void k_smh_finish(const T *__restrict__ table, uint32_t m, void *__restrict__ sig, uint8_t *__restrict__ cold)
{
    __shared__ uint32_t s_filled;
    const uint64_t g = blockIdx.x;
    const T *slot = table + g * (uint64_t)m;
    const T EMPTY = (T)~(T)0;
    if (threadIdx.x == 0) s_filled = 0;
    __syncthreads();
    uint32_t loc = 0;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) loc += (slot[i] != EMPTY);
    if (loc) atomicAdd(&s_filled, loc);
    __syncthreads();
    if (threadIdx.x == 0) cold[g] = s_filled != m;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        if (ALGO == ALGO_SUPER) ((float *)sig)[g * (uint64_t)m + i] = slot[i] == EMPTY ? INFINITY : 0.0f + (float)slot[i] * 0x1.0p-23f;
        else ((T *)sig)[g * (uint64_t)m + i] = slot[i];
    }
}

// ---- cold path of super / super2: Ertl's SuperMinHash walk (SPEC 3.2) executed exactly, one lane per genome.
// Only genomes with fewer than ~m ln m distinct k-mers get here (plasmids, test inputs).
struct SmhScratch { uint32_t *lvl, *perm, *hist, *q; uint64_t *rr; uint8_t *filled; };
template <int ALGO, int VBITS, typename T>
struct SmhSeqEmit {
    SmhScratch s; uint32_t m; uint32_t *a; uint32_t *item;
    __device__ void operator()(uint64_t v) const
    {
        Rng g; g.seed(elem_hash<ALGO, VBITS>(v));
        const uint32_t it = (*item)++;
        for (uint32_t j = 0; j <= *a; j++) {
            uint64_t r;
            if (ALGO == ALGO_SUPER) r = g.r23();
            else r = sizeof(T) == 8 ? g.next64() : (uint64_t)g.next32();
            const uint64_t range = (uint64_t)(m - j);
            const uint32_t t = j + (uint32_t)rng_uint(g, range, uint_zone(range));
            if (s.q[j] != it) { s.q[j] = it; s.perm[j] = j; }
            if (s.q[t] != it) { s.q[t] = it; s.perm[t] = t; }
            const uint32_t tmp = s.perm[j]; s.perm[j] = s.perm[t]; s.perm[t] = tmp;
            const uint32_t sl = s.perm[j];
            const bool better = !s.filled[sl] || j < s.lvl[sl] || (j == s.lvl[sl] && r < s.rr[sl]);
            if (better) {
                const uint32_t jp = s.lvl[sl];
                s.filled[sl] = 1; s.lvl[sl] = j; s.rr[sl] = r;
                if (j < jp) { s.hist[jp]--; s.hist[j]++; while (s.hist[*a] == 0) (*a)--; }
            }
        }
    }
};
template <bool AA, class Emit>
__device__ void walk_genome_seq(const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t r0, uint64_t r1, uint32_t kq, const Emit &emit)
{
    const uint32_t k = kq_k(kq);
    const uint64_t rc_or = kq_rc_or(kq);
    for (uint64_t r = r0; r < r1; r++) {
        const uint64_t rb = rec_start[r], len = rec_len[r];
        if (len < k) continue;
        if (!AA) {
            const uint64_t mask = k == 32 ? ~(uint64_t)0 : (((uint64_t)1 << (2 * k)) - 1);
            uint64_t fwd = 0, rc = 0;
            for (uint64_t i = 0; i < len; i++) {
                const uint64_t a = rb + i;
                const uint64_t c = (seq[a >> 2] >> (6 - 2 * (a & 3))) & 3;
                fwd = ((fwd << 2) | c) & mask;
                rc = (rc >> 2) | ((3 - c) << (2 * (k - 1))) | rc_or;
                if (i + 1 >= k) emit((fwd < rc ? fwd : rc) & mask);
            }
        } else {
            const uint64_t mask = ((uint64_t)1 << (5 * k)) - 1;
            uint64_t val = 0;
            for (uint64_t i = 0; i < len; i++) {
                val = ((val << 5) | c_aa_code[seq[rb + i] & 31]) & mask;
                if (i + 1 >= k) emit(val);
            }
        }
    }
}
// ---- cold path, parallel form: one workgroup per genome, every lane walks its own elements. The signature is an order-free
// lexicographic minimum over (level j, r_j) keys (SPEC 3.2), so the slots take atomicMin of packed keys in LDS and the histogram
// bound `a` of the paper (largest level still held by a slot; only a pruning device) is shared: hist[] is incremented BEFORE a key is
// published and decremented after it is displaced, so it never under-counts a level that holds a slot and `a` can only be lowered
// when that is safe. Lane-private Fisher-Yates state (perm / stamp arrays, m words each) lives in global scratch, element i of lane
// l at [i * CW_T + l]. u64 signatures need 64 + 16 bits per key: pass A orders by (level, top 48 bits of r), pass B re-walks the
// elements and takes the minimum of the full r among the visits that tie with the winner.
constexpr int CW_T = 256;
template <int ALGO, int VBITS, typename T, bool PASS_B>
struct SmhWgEmit {
    uint64_t *K, *K2; uint32_t *hist, *sa, *q, *perm; uint32_t m; uint32_t *stamp;
    static __device__ __forceinline__ uint64_t pack(uint32_t j, uint64_t r) { return sizeof(T) == 8 ? (((uint64_t)j << 48) | (r >> 16)) : (((uint64_t)j << 32) | r); }
    static __device__ __forceinline__ uint32_t level(uint64_t key) { return (uint32_t)(key >> (sizeof(T) == 8 ? 48 : 32)); }
    __device__ void operator()(uint64_t v, uint64_t, uint64_t) const
    {
        Rng g; g.seed(elem_hash<ALGO, VBITS>(v));
        const uint32_t st = (*stamp)++, l = threadIdx.x;
        for (uint32_t j = 0; j <= *(volatile uint32_t *)&sa[0]; j++) {
            uint64_t r;
            if (ALGO == ALGO_SUPER) r = g.r23();
            else r = sizeof(T) == 8 ? g.next64() : (uint64_t)g.next32();
            const uint64_t range = (uint64_t)(m - j);
            const uint32_t t = j + (uint32_t)rng_uint(g, range, uint_zone(range));
            const uint64_t ij = (uint64_t)j * CW_T + l, it = (uint64_t)t * CW_T + l;
            if (q[ij] != st) { q[ij] = st; perm[ij] = j; }
            if (q[it] != st) { q[it] = st; perm[it] = t; }
            const uint32_t tmp = perm[ij]; perm[ij] = perm[it]; perm[it] = tmp;
            const uint32_t sl = perm[ij];
            const uint64_t key = pack(j, r);
            if (PASS_B) { if (key == K[sl]) atomicMin((unsigned long long *)&K2[sl], (unsigned long long)r); continue; }
            if (key < K[sl]) {                                    // a stale (larger) read only costs a redundant attempt
                atomicAdd(&hist[j], 1u);
                const uint64_t old = atomicMin((unsigned long long *)&K[sl], (unsigned long long)key);
                if (key < old) {
                    const uint32_t jp = old == ~(uint64_t)0 ? m - 1 : level(old);
                    atomicSub(&hist[jp], 1u);                     // jp == j: same level, smaller r -> undoes the increment
                    uint32_t a0 = *(volatile uint32_t *)&sa[0];
                    const uint32_t a1 = a0;
                    while (a0 > 0 && *(volatile uint32_t *)&hist[a0] == 0) a0--;
                    if (a0 < a1) atomicMin(&sa[0], a0);
                } else atomicSub(&hist[j], 1u);                   // another lane got there first
            }
        }
    }
};
template <bool AA, int ALGO, int VBITS, typename T>
__global__ __launch_bounds__(CW_T) void k_smh_cold_wg(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                      const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off,
                                                      const uint64_t *__restrict__ gen_units, const uint32_t *__restrict__ cold_list, uint32_t ncold, uint32_t k,
                                                      uint32_t m, uint32_t *__restrict__ lane_q, uint32_t *__restrict__ lane_perm,
                                                      unsigned long long *__restrict__ counter, void *__restrict__ sig)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_cw[];
    uint64_t *K = (uint64_t *)s_cw;
    uint64_t *K2 = sizeof(T) == 8 ? K + m : K;
    uint32_t *hist = (uint32_t *)(K + (sizeof(T) == 8 ? 2 * (size_t)m : (size_t)m));
    uint32_t *sa = hist + m;                                      // sa[0] = a, sa[1] = work item
    uint32_t *q = lane_q + (uint64_t)blockIdx.x * m * CW_T, *perm = lane_perm + (uint64_t)blockIdx.x * m * CW_T;
    uint32_t stamp = 0;                                           // unique per (lane, element) for the whole launch; the host fills q with 0xFF
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) sa[1] = (uint32_t)atomicAdd(counter, 1ull);
        __syncthreads();
        const uint32_t c = sa[1];
        if (c >= ncold) break;
        const uint64_t g = cold_list[c];
        for (uint32_t i = threadIdx.x; i < m; i += CW_T) { K[i] = ~(uint64_t)0; if (sizeof(T) == 8) K2[i] = ~(uint64_t)0; hist[i] = 0; }
        __syncthreads();
        if (threadIdx.x == 0) { hist[m - 1] = m; sa[0] = m - 1; }
        __syncthreads();
        const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1], units = gen_units[g];
        {
            SmhWgEmit<ALGO, VBITS, T, false> emit{K, K2, hist, sa, q, perm, m, &stamp};
            walk_genome<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, units, k, 0, 1, emit);
        }
        __syncthreads();
        if (sizeof(T) == 8) {
            SmhWgEmit<ALGO, VBITS, T, true> emit{K, K2, hist, sa, q, perm, m, &stamp};
            walk_genome<AA>(seq, rec_start, rec_len, rec_upre, r0, r1, units, k, 0, 1, emit);
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < m; i += CW_T) {
            const uint64_t key = K[i];
            if (ALGO == ALGO_SUPER) ((float *)sig)[g * (uint64_t)m + i] = key == ~(uint64_t)0 ? INFINITY : (float)(uint32_t)(key >> 32) + (float)(uint32_t)key * 0x1.0p-23f;
            else if (sizeof(T) == 8) ((T *)sig)[g * (uint64_t)m + i] = (T)K2[i];
            else ((T *)sig)[g * (uint64_t)m + i] = key == ~(uint64_t)0 ? (T)~(T)0 : (T)(uint32_t)key;
        }
    }
}

template <bool AA, int ALGO, int VBITS, typename T>
__global__ void k_smh_cold(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                           const uint64_t *__restrict__ genome_rec_off, const uint32_t *__restrict__ cold_list, uint32_t ncold, uint32_t k, uint32_t m,
                           uint8_t *__restrict__ scratch, void *__restrict__ sig)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncold) return;
    const uint64_t g = cold_list[c];
    uint8_t *base = scratch + (uint64_t)c * 32 * m;
    SmhScratch s;
    s.rr = (uint64_t *)base; s.lvl = (uint32_t *)(base + 8 * (uint64_t)m); s.perm = s.lvl + m; s.hist = s.perm + m; s.q = s.hist + m;
    s.filled = (uint8_t *)(s.q + m);
    for (uint32_t i = 0; i < m; i++) { s.lvl[i] = m - 1; s.rr[i] = ~(uint64_t)0; s.q[i] = 0xFFFFFFFFu; s.hist[i] = 0; s.filled[i] = 0; }
    s.hist[m - 1] = m;
    uint32_t a = m - 1, item = 0;
    SmhSeqEmit<ALGO, VBITS, T> emit{s, m, &a, &item};
    walk_genome_seq<AA>(seq, rec_start, rec_len, genome_rec_off[g], genome_rec_off[g + 1], k, emit);
    for (uint32_t i = 0; i < m; i++) {
        if (ALGO == ALGO_SUPER) ((float *)sig)[g * (uint64_t)m + i] = s.filled[i] ? (float)s.lvl[i] + (float)(uint32_t)s.rr[i] * 0x1.0p-23f : INFINITY;
        else ((T *)sig)[g * (uint64_t)m + i] = s.filled[i] ? (T)s.rr[i] : (T)~(T)0;
    }
}

// launch geometry shared by the slot-min sketchers
struct MinGeom { uint32_t parts; bool use_lds; size_t lds; };
static MinGeom min_geom(gs_ctx *c, uint32_t m, size_t esz, uint64_t n_genomes, uint64_t avg_units)
{
    MinGeom g;
    g.lds = (size_t)m * esz;
    g.use_lds = g.lds <= 160 * 1024 - 256;
    g.parts = 1;
    if (n_genomes < (uint64_t)2 * c->n_cu) {
        g.parts = (uint32_t)((2 * (uint64_t)c->n_cu + n_genomes - 1) / n_genomes);
        uint64_t maxp = avg_units / SK_THREADS + 1;       // at least one full sweep per part
        if (g.parts > maxp) g.parts = (uint32_t)maxp;
        if (g.parts < 1) g.parts = 1;
    }
    return g;
}

template <int ALGO, int VBITS, typename T>
static int launch_min(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len,
                      const uint64_t *rec_upre, const uint64_t *genome_rec_off, const uint64_t *gen_units, uint64_t n_genomes,
                      uint64_t avg_units, T *table)
{
    const uint32_t m = p->sketch_size;
    const uint64_t zone = uint_zone(m);
    const MinGeom ge = min_geom(c, m, sizeof(T), n_genomes, avg_units);
    if (!ge.use_lds || ge.parts > 1) GS_HIP_CHECK(hipMemsetAsync(table, 0xFF, (size_t)n_genomes * m * sizeof(T), c->stream));
    const bool aa = p->data_t == GS_DATA_AA;
    const size_t lds = ge.lds;
    // survivor queues of the filtered emitter (DNA, table in LDS): only where they do not cost a resident workgroup
    const size_t lds_f = ((lds + 15) & ~(size_t)15) + (size_t)(SK_THREADS / 64) * SKQ * 8;
    const size_t half_cu = (160 * 1024) / 2 / 1280 * 1280;
    // (and only for genomes long enough to warm the table up: >= 64 k-mers per slot; below that the survivor rate stays above 1/4)
    const bool filt = !aa && ge.use_lds && !(getenv("GS_SKETCH_FILTER") && !atoi(getenv("GS_SKETCH_FILTER"))) && avg_units * 32 >= (uint64_t)64 * m &&
                      (lds_f <= half_cu || (lds > half_cu && lds_f <= 160 * 1024 - 256));
    c->last_sketch[0] = filt; c->last_sketch[1] = ge.use_lds; c->last_sketch[2] = ge.parts; c->last_sketch[3] = 0;
    // GS_SKETCH_CAP: the c of the speculative bound (m / N)(ln m + c) of the filtered emitter (default 7: ~1 genome in 1000 walks twice); 0 = off
    const float cap_c = getenv("GS_SKETCH_CAP") ? (float)atof(getenv("GS_SKETCH_CAP")) : 7.0f;
    for (uint64_t g0 = 0; g0 < n_genomes; g0 += 65535) {       // grid.y limit
        uint64_t ng = n_genomes - g0 < 65535 ? n_genomes - g0 : 65535;
        dim3 grid(ge.parts, (uint32_t)ng), block(SK_THREADS);
        c->last_sketch[3]++;
        const uint64_t *gro = genome_rec_off + g0; const uint64_t *gu = gen_units + g0;
        T *tab = table + g0 * m;
        ProfScope ps(c, FAM_SKETCH);
#define GS_LAUNCH_MIN(AAV, LDSV, FV) do { if (!AAV && p->data_t == GS_DATA_DNA_FWD) GS_LAUNCH_MIN_RC(AAV, LDSV, FV, AAV ? 0 : 1); else GS_LAUNCH_MIN_RC(AAV, LDSV, FV, 0); } while (0)
#define GS_LAUNCH_MIN_RC(AAV, LDSV, FV, RC)                                                                             \
    do {                                                                                                                \
        auto kern = k_sketch_min<AAV, LDSV, ALGO, VBITS, T, FV, RC>;                                                    \
        const size_t l0_ = LDSV ? (FV ? lds_f : lds) : ((size_t)2 * m + 15) & ~(size_t)15;    /* slot table (+ survivor queues), or its 2-byte filter */  \
        const size_t l = std::min<size_t>(l0_, 160 * 1024 - 256);                                                       \
        if (l > 48 * 1024) GS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l)); \
        hipLaunchKernelGGL(kern, grid, block, l, c->stream, seq, rec_start, rec_len, rec_upre, gro, gu, kq_of(p), m, zone, tab, cap_c); \
    } while (0)
        if (aa) { if (ge.use_lds) GS_LAUNCH_MIN(true, true, false); else GS_LAUNCH_MIN(true, false, false); }
        else if (!ge.use_lds) GS_LAUNCH_MIN(false, false, false);
        else if (filt) GS_LAUNCH_MIN(false, true, true);
        else GS_LAUNCH_MIN(false, true, false);
#undef GS_LAUNCH_MIN
#undef GS_LAUNCH_MIN_RC
        GS_HIP_CHECK(hipGetLastError());
    }
    return GS_OK;
}

// super / super2 driver: level-0 pass, finish, then the exact cold walk for the (rare) genomes with empty slots
template <int ALGO, int VBITS, typename T>
static int run_smh(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len,
                   const uint64_t *rec_upre, const uint64_t *genome_rec_off, const uint64_t *gen_units, uint64_t n_genomes, uint64_t avg_units,
                   void *sig_out)
{
    const uint32_t m = p->sketch_size;
    PoolBuf table(c, SL_SMH_TABLE), cold(c, SL_SMH_COLD_FLAGS);
    int rc;
    if ((rc = table.alloc((size_t)n_genomes * m * sizeof(T)))) return rc;
    if ((rc = cold.alloc(n_genomes))) return rc;
    if ((rc = launch_min<ALGO, VBITS, T>(c, p, seq, rec_start, rec_len, rec_upre, genome_rec_off, gen_units, n_genomes, avg_units, table.as<T>()))) return rc;
    hipLaunchKernelGGL((k_smh_finish<ALGO, T>), dim3((uint32_t)n_genomes), dim3(256), 0, c->stream, table.as<T>(), m, sig_out, cold.as<uint8_t>());
    GS_HIP_CHECK(hipGetLastError());
    std::vector<uint8_t> h(n_genomes);
    GS_HIP_CHECK(hipMemcpyAsync(h.data(), cold.p, n_genomes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> list;
    for (uint64_t g = 0; g < n_genomes; g++) if (h[g]) list.push_back((uint32_t)g);
    const bool aa = p->data_t == GS_DATA_AA;
    // parallel form (one workgroup per genome) when the slot keys + level histogram fit in LDS
    const size_t lds_wg = (sizeof(T) == 8 ? 20 : 12) * (size_t)m + 16;
    if (!list.empty() && lds_wg <= 150 * 1024 && m <= 65535 && !getenv("GS_SMH_COLD_SERIAL")) {
        const uint32_t nc = (uint32_t)list.size();
        const uint32_t wgs = std::min<uint32_t>(nc, (uint32_t)c->n_cu * 2);
        PoolBuf dl(c, SL_SMH_COLD_LIST), lq(c, SL_SMH_COLD_Q), lp(c, SL_SMH_COLD_P), cnt(c, SL_SMH_COLD_CNT);
        if ((rc = dl.alloc(4 * (size_t)nc))) return rc;
        if ((rc = lq.alloc((size_t)4 * wgs * m * CW_T))) return rc;
        if ((rc = lp.alloc((size_t)4 * wgs * m * CW_T))) return rc;
        if ((rc = cnt.alloc(64))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(dl.p, list.data(), 4 * (size_t)nc, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemsetAsync(lq.p, 0xFF, (size_t)4 * wgs * m * CW_T, c->stream));
        GS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 8, c->stream));
#define GS_LAUNCH_COLDWG(AAV)                                                                                                  \
    do {                                                                                                                       \
        auto kern = k_smh_cold_wg<AAV, ALGO, VBITS, T>;                                                                        \
        if (lds_wg > 48 * 1024) GS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wg)); \
        hipLaunchKernelGGL(kern, dim3(wgs), dim3(CW_T), lds_wg, c->stream, seq, rec_start, rec_len, rec_upre, genome_rec_off, gen_units, dl.as<uint32_t>(), nc, kq_of(p), m, \
                           lq.as<uint32_t>(), lp.as<uint32_t>(), cnt.as<unsigned long long>(), sig_out);                       \
    } while (0)
        if (aa) GS_LAUNCH_COLDWG(true); else GS_LAUNCH_COLDWG(false);
#undef GS_LAUNCH_COLDWG
        GS_HIP_CHECK(hipGetLastError());
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    // one lane per cold genome: take as many genomes per launch as 16 GB of per-lane scratch (32 m bytes each) allows - a launch lasts
    // as long as its slowest lane, so 4096-genome chunks serialised 25 launches for 10^5 small genomes
    const size_t per_launch = std::max<size_t>(4096, std::min<size_t>(((size_t)16 << 30) / ((size_t)32 * m), (size_t)1 << 20));
    for (size_t l0 = 0; l0 < list.size(); l0 += per_launch) {
        const uint32_t nc = (uint32_t)std::min<size_t>(per_launch, list.size() - l0);
        PoolBuf dl(c, SL_SMH_COLD_LIST), scratch(c, SL_SMH_COLD_Q);
        if ((rc = dl.alloc(4 * (size_t)nc))) return rc;
        if ((rc = scratch.alloc((size_t)nc * 32 * m))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(dl.p, list.data() + l0, 4 * (size_t)nc, hipMemcpyHostToDevice, c->stream));
        if (aa) hipLaunchKernelGGL((k_smh_cold<true, ALGO, VBITS, T>), dim3((nc + 63) / 64), dim3(64), 0, c->stream, seq, rec_start, rec_len, genome_rec_off, dl.as<uint32_t>(), nc, kq_of(p), m, scratch.as<uint8_t>(), sig_out);
        else hipLaunchKernelGGL((k_smh_cold<false, ALGO, VBITS, T>), dim3((nc + 63) / 64), dim3(64), 0, c->stream, seq, rec_start, rec_len, genome_rec_off, dl.as<uint32_t>(), nc, kq_of(p), m, scratch.as<uint8_t>(), sig_out);
        GS_HIP_CHECK(hipGetLastError());
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return GS_OK;
}

static int launch_oph(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len,
                      const uint64_t *rec_upre, const uint64_t *genome_rec_off, const uint64_t *gen_units, uint64_t n_genomes,
                      uint64_t avg_units, uint32_t *table, uint32_t *win, float *sig)
{
    const uint32_t m = p->sketch_size;
    const uint64_t zone = uint_zone(m);
    int rc = launch_min<ALGO_OPTDENS, 64, uint32_t>(c, p, seq, rec_start, rec_len, rec_upre, genome_rec_off, gen_units, n_genomes, avg_units, table);
    if (rc) return rc;
    if (p->algo == GS_ALGO_OPTDENS)
        hipLaunchKernelGGL(k_oph_finish<ALGO_OPTDENS>, dim3((uint32_t)n_genomes), dim3(256), 0, c->stream, table, m, zone, win, sig);
    else
        hipLaunchKernelGGL(k_oph_finish<ALGO_REVOPTDENS>, dim3((uint32_t)n_genomes), dim3(256), 0, c->stream, table, m, zone, win, sig);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

// everything on the device; scratch owned by the call (freed after the stream drains)

// ======================================================================================================
// hll = SetSketch1 with u16 registers (SPEC 3.4; kmerutils HyperLogLogSketch<Kmer,u16> over probminhash's SetSketcher,
// /root/reference/src/dna/dnasketch.rs:541-574, src/aa/aasketch.rs:481-500). Registers are per-slot MAXIMA over (element, j) of
// k_j = trunc(1 - log_b x_j): order free, so the sequential lower-bound pruning of the paper becomes two passes per genome inside
// one workgroup (register table in LDS, ds_max_u32):
//   pass A  level j = 0 of every k-mer (one exponential draw, one uniform slot) under the workgroup's RUNNING minimum register as a
//           filter - a conservative integer threshold on the 52 uniform bits decides without evaluating a logarithm for all but a
//           few percent of the k-mers (U > a*m*b^-(K-2) implies k_0 < K because -ln(1-U) >= U; table ucut[K] from the host);
//   pass B  with the exact minimum K_low of pass A as the bound every k-mer is hashed again, the ~3 % whose first point beats K_low
//           walk on (j = 1, 2, ...: exponential spacings through a lazily materialised Fisher-Yates permutation) until k_j <= K_low.
// The permutation of a walking lane is a short list of displaced positions in registers (walks are a few steps once K_low is
// realistic); a genome whose walks outgrow it - few k-mers per register, K_low ~ 0, walks of ~m steps - is flagged and redone by
// the COLD instantiation, whose lanes keep stamped perm arrays in global scratch (same scheme as k_smh_cold_wg).
// ======================================================================================================
constexpr int HL_T = 512;          // lanes per workgroup
constexpr int HL_JR = 12;          // displaced positions a warm lane can remember
constexpr int HL_CT = 256;         // lanes per workgroup of the cold instantiation
// GTAB (register files beyond the LDS: sketch_size > ~40 000, the reference takes sketch_size as is, dnasketch.rs:541-574): the u32
// registers live in a per-workgroup global table and LDS holds a 2-byte FILTER per register - a value that is never above the
// register (the last k this workgroup sent there, refreshed from the table between chunks). A k that does not exceed the filter
// cannot raise the register and stops after one LDS read; the rest go to atomicMax in memory. Racy plain 16-bit stores can only leave
// the filter lower, i.e. more conservative: exact. Beyond ~80 000 registers the filter does not fit either (filt == nullptr) and every
// k above K_low goes to memory.
__device__ __forceinline__ uint32_t hll_xthr_bits(uint32_t klow, double inv_lnb)
{
    // k(x) = trunc(1 - ln x / ln b) <= klow  <=  x > b^-klow; the margin (2e-5 relative) covers the float rounding and spec_ln's last bits by far
    return __float_as_uint((float)(exp(-(double)klow / inv_lnb) * (1.0 + 2e-5)));
}
struct HllShared { uint32_t *tab; volatile uint32_t *ctl; uint16_t *filt; };   // ctl: [0] klow, [1] work item, [2] scratch min, [3] overflow flag, [4,5] ucut[klow], [7] float bits of a value safely ABOVE b^-klow (x >= it => k(x) <= klow without the logarithm)
template <bool COLD, bool GTAB>
struct HllEmit {
    HllShared S; uint32_t m; uint64_t zone_m; double inv_lnb, am;
    uint32_t *q, *perm; uint32_t *stamp; bool walk;
    // warm instantiation: per-wave LDS queue of the element hashes that pass the cheap cut (round 3, the MinEmitF scheme). ~3 % of the k-mers
    // go on to the logarithm / walk; left in place, nearly every wave iteration had a lane or two in that branch and all 64 paid for it
    // (rocprofv3: 733 VALU wave-instructions per 64 k-mers, 8x the OPH sketch). Queued, the slow part runs on full wavefronts.
    uint64_t *sq; uint32_t lane; mutable uint32_t qn; mutable uint64_t cutr;
    // Round 4: pass A also RECORDS the hashes that pass its cut (ctl[6] counts them, `surv` holds up to surv_cap of them per workgroup). The cut only
    // ever tightens (registers only grow), so every k-mer pass B would look at is among them: pass B walks this list instead of hashing the whole
    // genome a second time (a list that overflowed falls back to the second walk).
    uint64_t *surv; uint32_t surv_cap;
    __device__ __forceinline__ void record_wave(uint64_t h, uint32_t cnt) const          // the first `cnt` lanes of the wave append their h
    {
        if (!surv || walk) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd((uint32_t *)&S.ctl[6], cnt);
        base = __builtin_amdgcn_readfirstlane(base);
        if (lane < cnt && base + lane < surv_cap) surv[base + lane] = h;
    }
    __device__ __forceinline__ void refresh() const { cutr = ((uint64_t)S.ctl[5] << 32) | S.ctl[4]; }
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const { process(elem_hash<ALGO_HLL, 64>(v), true); }
    __device__ __forceinline__ void full(uint64_t v) const
    {
        const uint64_t h = elem_hash<ALGO_HLL, 64>(v);
        const uint64_t s0 = splitmix_mix(h + GS_GAMMA), s3 = splitmix_mix(h + 4 * GS_GAMMA);       // the first output needs two of the four state words
        const bool pass = ((rotl64(s0 + s3, 23) + s0) >> 12) <= cutr;
        const uint64_t bal = __ballot(pass);
        if (bal) {
            if (pass) sq[qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = h;
            qn += (uint32_t)__popcll(bal);
            if (qn >= 64) {
                const uint64_t hq = sq[lane];
                record_wave(hq, 64u);
                process(hq, false);
                const uint32_t rest = qn - 64;
                const uint64_t mv = sq[64 + lane];
                if (lane < rest) sq[lane] = mv;
                qn = rest;
            }
        }
    }
    __device__ __forceinline__ void finish() const
    {
        if (sq && qn) { const uint64_t hq = lane < qn ? sq[lane] : 0; record_wave(hq, qn); if (lane < qn) process(hq, false); }
        qn = 0;
    }
    __device__ __forceinline__ void process(uint64_t h, bool record) const
    {
        Rng g; g.seed(h);
        const uint64_t u52 = g.next64() >> 12;
        const uint64_t cut = ((uint64_t)S.ctl[5] << 32) | S.ctl[4];
        if (u52 > cut) return;                                    // its first point cannot reach the lower bound: nor can any later one
        if (record && surv && !walk) { const uint32_t at = atomicAdd((uint32_t *)&S.ctl[6], 1u); if (at < surv_cap) surv[at] = h; }      // (lanes outside full waves: record boundaries)
        const uint32_t klow = S.ctl[0];
        double x = -spec_ln(1.0 - (double)u52 * 0x1.0p-52) / am;
        uint32_t k = hll_k(x, inv_lnb);
        if (k <= klow) return;
        uint32_t t = (uint32_t)rng_uint(g, (uint64_t)m, zone_m);
        reg_max(t, k);                                            // j = 0: p[0] after swap(p[0], p[t]) is t
        if (!walk) return;
        // j >= 1: lazily materialised permutation. Position 0 now holds t and position t holds 0.
        uint32_t tpos[HL_JR], tval[HL_JR]; uint32_t nt = 0;
        const uint32_t st = COLD ? (*stamp)++ : 0, l = threadIdx.x;
        if (COLD) { q[(uint64_t)0 * HL_CT + l] = st; perm[(uint64_t)0 * HL_CT + l] = t; q[(uint64_t)t * HL_CT + l] = st; perm[(uint64_t)t * HL_CT + l] = 0; }
        else if (t != 0) { tpos[0] = t; tval[0] = 0; nt = 1; }
        const double xthr = (double)__uint_as_float(S.ctl[7]);
        for (uint32_t j = 1; j < m; j++) {
            const double uj = g.u64f();
            const double den = GS_HLL_A * (double)(m - j);
            // (round 5) -ln(1 - u) >= u: the next point lies at or beyond x + u / den; when already that is safely past b^-klow the walk ends here, without
            // the two logarithms (the spacing and k of the point) - the case for ~94 % of the walkers' second points. Nothing reads the generator afterwards.
            if (x + uj / den >= xthr) break;
            const double te = -spec_ln(1.0 - uj);
            x = x + te / den;
            k = hll_k(x, inv_lnb);
            if (k <= klow) break;
            const uint64_t range = (uint64_t)(m - j);
            t = j + (uint32_t)rng_uint(g, range, uint_zone(range));
            uint32_t sl;
            if (COLD) {
                const uint64_t ij = (uint64_t)j * HL_CT + l, it = (uint64_t)t * HL_CT + l;
                if (q[ij] != st) { q[ij] = st; perm[ij] = j; }
                if (q[it] != st) { q[it] = st; perm[it] = t; }
                const uint32_t tmp = perm[ij]; perm[ij] = perm[it]; perm[it] = tmp;
                sl = perm[ij];
            } else {
                uint32_t pj = j, pt = t; int hit = -1;
#pragma unroll
                for (int i = 0; i < HL_JR; i++) if ((uint32_t)i < nt) { if (tpos[i] == j) pj = tval[i]; if (tpos[i] == t) { pt = tval[i]; hit = i; } }
                if (t != j) {
                    if (hit >= 0) {
#pragma unroll
                        for (int i = 0; i < HL_JR; i++) if (i == hit) tval[i] = pj;
                    } else {
                        if (nt == HL_JR) { S.ctl[3] = 1; return; }       // outgrown: the genome is redone by the cold instantiation
#pragma unroll
                        for (int i = 0; i < HL_JR; i++) if ((uint32_t)i == nt) { tpos[i] = t; tval[i] = pj; }
                        nt++;
                    }
                }
                sl = (t != j) ? pt : pj;
            }
            reg_max(sl, k);
        }
    }
    __device__ __forceinline__ void reg_max(uint32_t t, uint32_t k) const
    {
        if (!GTAB) { atomicMax(&S.tab[t], k); return; }
        if (S.filt) { if (k <= S.filt[t]) return; S.filt[t] = (uint16_t)k; }      // k <= q + 1 = 65535
        atomicMax(&S.tab[t], k);
    }
};
template <bool GTAB> __device__ __forceinline__ void emit_full_wave(const HllEmit<false, GTAB> &e, uint64_t v, uint64_t r, uint64_t p) { if (e.sq) e.full(v); else e(v, r, p); }
template <bool GTAB> __device__ __forceinline__ void emit_finish(const HllEmit<false, GTAB> &e) { e.finish(); }
// TIGHT (warm form only): 128 VGPRs at most. The 72 kB register table lets two workgroups share a CU, the 160 registers the compiler takes by itself (the
// walker's double-precision logarithms) let only ONE: 2 waves per SIMD, VALU issue 55 % busy, 40 % of the wave cycles waiting (profiles/r05_hll_pmc.txt).
// Capped, 31 registers of the walker spill and two workgroups are resident: 512 genomes of 1 / 2 / 3 / 5 / 20 Mbp in 6.7 / 7.0 / 8.3 / 9.8 / 25.2 ms against
// 8.0 / 8.4 / 9.4 / 11.9 / 30.6 (5 Mbp: 2.1 -> 2.6e11 k-mers/s, 3.0e11 at 2048 genomes). The uncapped instantiation stays for batches of very short
// genomes (< 16 k-mers per register: the walker is most of the work there) and for A/B (GS_HLL_TIGHT=0).
template <bool AA, bool COLD, bool GTAB, bool TIGHT = false>
__global__ __launch_bounds__(COLD ? HL_CT : HL_T, (!COLD && TIGHT) ? 4 : 1) void k_sketch_hll(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start,
        const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off,
        const uint64_t *__restrict__ gen_units, const uint32_t *__restrict__ list, uint32_t n_items, uint32_t k, uint32_t m, double inv_lnb,
        const uint64_t *__restrict__ ucut, uint32_t *__restrict__ lane_q, uint32_t *__restrict__ lane_perm, unsigned long long *__restrict__ counter,
        uint8_t *__restrict__ cold_flag, uint16_t *__restrict__ sig, uint32_t *__restrict__ gtab, int use_filter, uint32_t queue_off,
        uint64_t *__restrict__ surv_all, uint32_t surv_cap, uint32_t surv_min_chunks, float spec_c)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_hll[];
    HllShared S;
    if (!GTAB) { S.tab = (uint32_t *)s_hll; S.ctl = (volatile uint32_t *)(S.tab + m); S.filt = nullptr; }
    else { S.ctl = (volatile uint32_t *)s_hll; S.filt = use_filter ? (uint16_t *)(s_hll + 32) : nullptr; S.tab = gtab + (uint64_t)blockIdx.x * m; }
    const uint32_t T = COLD ? HL_CT : HL_T;
    uint32_t *q = COLD ? lane_q + (uint64_t)blockIdx.x * m * HL_CT : nullptr, *perm = COLD ? lane_perm + (uint64_t)blockIdx.x * m * HL_CT : nullptr;
    uint32_t stamp = 0;
    const uint64_t zone_m = uint_zone(m);
    const double am = GS_HLL_A * (double)m;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) S.ctl[1] = (uint32_t)atomicAdd(counter, 1ull);
        __syncthreads();
        const uint32_t c = S.ctl[1];
        if (c >= n_items) break;
        const uint64_t g = list ? list[c] : c;
        for (uint32_t i = threadIdx.x; i < m; i += T) { S.tab[i] = 0; if (GTAB && S.filt) S.filt[i] = 0; }
        if (threadIdx.x == 0) { S.ctl[0] = 0; S.ctl[3] = 0; S.ctl[4] = 0xFFFFFFFFu; S.ctl[5] = 0xFFFFFFFFu; S.ctl[6] = 0; S.ctl[7] = hll_xthr_bits(0, inv_lnb); }
        __syncthreads();
        const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1], units = gen_units[g];
        const uint32_t nchunks = (uint32_t)std::max<uint64_t>(1, units / ((uint64_t)T * 8));
        bool outgrown = false;                                    // workgroup-uniform: some warm lane's walk outgrew its registers
        // Round 4: with survivor lists the genome is hashed ~1.1 times instead of twice: a WARM-UP over the first eighth of the chunks (pass -1: registers
        // only) gives pass A a realistic bound from its first k-mer on, so the hashes it records (the ones that pass its running cut: ~5 % then, a third
        // of the genome without the warm-up) fit the list, and pass B reads the list. Genomes of fewer than four chunks keep the two plain passes.
        // (measured, 512 genomes, m = 18000: 20 Mbp 67.0 -> 47.9 ms; 5 Mbp 23.7 -> 24.4 ms - there the time is the survivors' logarithms and walks, not
        // the filtering the lists save; 1 Mbp 12.0 -> 17.4 ms. Lists from `surv_min_chunks` chunks of 131 072 k-mers on: 64 = 8.4 Mbp.)
        uint64_t *surv_wg = (!COLD && surv_all && nchunks >= surv_min_chunks) ? surv_all + (uint64_t)blockIdx.x * surv_cap : nullptr;
        const uint32_t nwarm = nchunks / 8 ? nchunks / 8 : 1;
        // the minimum register of the workgroup's table -> S.ctl[2] (all lanes return it)
        auto min_register = [&]() -> uint32_t {
            __syncthreads();
            if (threadIdx.x == 0) S.ctl[2] = 0xFFFFFFFFu;
            __syncthreads();
            uint32_t lo = 0xFFFFFFFFu;
            for (uint32_t i = threadIdx.x; i < m; i += T) {
                // (a global table is only ever written by atomics performed in the L2: read it there too, not through the vector L1)
                const uint32_t r = GTAB ? __hip_atomic_load(&S.tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : S.tab[i];
                if (GTAB && S.filt) S.filt[i] = (uint16_t)r;
                lo = min(lo, r);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lo = min(lo, (uint32_t)__shfl_down((int)lo, o));
            if ((threadIdx.x & 63) == 0) atomicMin((uint32_t *)&S.ctl[2], lo);
            __syncthreads();
            return S.ctl[2];
        };
        // Round 5, ONE speculative pass instead of two (the bound of k_sketch_min's filtered emitter): every register ends as the maximum of
        // k = trunc(1 - log_b x) over one Exp(a)-distributed point per distinct k-mer, so the smallest register of N k-mers sits near
        // K = 1 - log_b((ln m + G) / (a N)), G Gumbel. With a guess K_g taken at G = c the genome is walked ONCE - level 0 and the walks of the ~m (ln m + c) / N
        // k-mers whose first point can beat K_g, everything at or below K_g dropped - and the guess is CHECKED: if no register ended below K_g, nothing
        // that was dropped could have raised one (max semantics) and the table is the exact one; otherwise (c = 7: ~1 genome in 1000; genomes of many
        // repeated k-mers) the table is kept - registers only grow - and the two exact passes below run over it.
        bool spec_done = false;
        if (!COLD && spec_c != 0.0f && units > 0) {
            const float xg = (__logf((float)m) + spec_c) / ((float)GS_HLL_A * (float)units * 32.0f);
            uint32_t kg = 0;
            if (xg > 0.0f && xg < 1.0f) { const float y = 1.0f - __logf(xg) * (float)inv_lnb; kg = y >= 4.0f ? (uint32_t)fminf(y, (float)GS_HLL_Q) - 1u : 0u; }
            if (kg >= 2) {
                if (threadIdx.x == 0) { const uint64_t cu = ucut[kg]; S.ctl[0] = kg; S.ctl[4] = (uint32_t)cu; S.ctl[5] = (uint32_t)(cu >> 32); S.ctl[7] = hll_xthr_bits(kg, inv_lnb); }
                __syncthreads();
                uint64_t *sq = queue_off ? (uint64_t *)(s_hll + queue_off) + (threadIdx.x >> 6) * 128 : nullptr;
                HllEmit<COLD, GTAB> emit{S, m, zone_m, inv_lnb, am, q, perm, &stamp, true, sq, threadIdx.x & 63, 0u, ~(uint64_t)0, nullptr, 0u};
                // (walk_genome on its one-stage loop: the registers of the two-stage one would cost every form of this kernel a wave per SIMD,
                // 156 -> 171 and 116 -> 130 VGPRs, or more scratch under the 128-register bound - profiles/sketch_ahead_resource_usage.txt)
                for (uint32_t ch = 0; ch < nchunks; ch++) {
                    emit.refresh();
                    walk_genome<AA, HllEmit<COLD, GTAB>, 2, false>(seq, rec_start, rec_len, rec_upre, r0, r1, units, k, ch, nchunks, emit);
                    if (__syncthreads_or(S.ctl[3] != 0)) { outgrown = true; break; }
                }
                if (!outgrown) {
                    if (min_register() >= kg) spec_done = true;
                    else {
                        if (threadIdx.x == 0) { S.ctl[0] = 0; S.ctl[4] = 0xFFFFFFFFu; S.ctl[5] = 0xFFFFFFFFu; S.ctl[7] = hll_xthr_bits(0, inv_lnb); }
                        __syncthreads();
                    }
                }
            }
        }
        for (int pass = surv_wg ? -1 : 0; pass < 2 && !outgrown && !spec_done; pass++) {
            // (queue_off != 0: the warm instantiation has room in LDS for its survivor queues, 128 hashes per wave)
            uint64_t *sq = (!COLD && queue_off) ? (uint64_t *)(s_hll + queue_off) + (threadIdx.x >> 6) * 128 : nullptr;
            uint64_t *surv = pass == 0 ? surv_wg : nullptr;
            HllEmit<COLD, GTAB> emit{S, m, zone_m, inv_lnb, am, q, perm, &stamp, pass == 1, sq, threadIdx.x & 63, 0u, ~(uint64_t)0, surv, surv_cap};
            if (!COLD && pass == 1 && surv_wg && S.ctl[6] <= surv_cap) {
                // pass B over the recorded survivors of pass A (S.ctl[6] is stable here: pass A ended with barriers)
                const uint32_t nl = S.ctl[6];
                for (uint32_t i = threadIdx.x; i < nl; i += T) emit.process(surv_wg[i], false);
                if (__syncthreads_or(S.ctl[3] != 0)) outgrown = true;
                break;
            }
            for (uint32_t ch = 0; ch < (pass < 0 ? nwarm : nchunks); ch++) {
                emit.refresh();
                walk_genome<AA, HllEmit<COLD, GTAB>, 2, false>(seq, rec_start, rec_len, rec_upre, r0, r1, units, k, ch, nchunks, emit);
                if (pass <= 0 || ch + 1 == nchunks) {
                    // refresh the lower bound: minimum register (pass A: running, between chunks; after pass A: exact)
                    const uint32_t kl_ = min_register();
                    if (threadIdx.x == 0) { const uint32_t kl = kl_; const uint64_t cu = ucut[kl]; S.ctl[0] = kl; S.ctl[4] = (uint32_t)cu; S.ctl[5] = (uint32_t)(cu >> 32); S.ctl[7] = hll_xthr_bits(kl, inv_lnb); }
                    __syncthreads();
                }
                // the overflow flag is raised by single lanes in mid-walk: every wave must take the SAME decision here (a wave that read
                // it a moment earlier than the others would leave the loop alone and pair its barriers with the wrong ones), so the flag
                // goes through a barrier-wide OR
                if (!COLD && __syncthreads_or(S.ctl[3] != 0)) { outgrown = true; break; }
            }
        }
        __syncthreads();
        if (!COLD && outgrown) { if (threadIdx.x == 0) cold_flag[g] = 1; continue; }
        for (uint32_t i = threadIdx.x; i < m; i += T)
            sig[g * (uint64_t)m + i] = (uint16_t)(GTAB ? __hip_atomic_load(&S.tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : S.tab[i]);
    }
}

static int run_hll(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len,
                   const uint64_t *rec_upre, const uint64_t *genome_rec_off, const uint64_t *gen_units, uint64_t n_genomes, uint64_t total_units, uint16_t *sig_out)
{
    const uint32_t m = p->sketch_size;
    const bool aa = p->data_t == GS_DATA_AA;
    const double inv_lnb = 1.0 / spec_ln(GS_HLL_B);
    // conservative skip thresholds on the 52 uniform bits, one per possible lower bound K (see the kernel comment)
    std::vector<uint64_t> ucut((size_t)GS_HLL_Q + 2);
    for (uint32_t K = 0; K <= GS_HLL_Q + 1; K++) {
        double f = K < 2 ? 1.0 : GS_HLL_A * (double)m * pow(GS_HLL_B, -(double)(K - 2));
        if (!(f < 1.0)) f = 1.0;
        ucut[K] = (uint64_t)floor(f * 0x1.0p52);                  // u52 < 2^52 always: f = 1 never skips
    }
    PoolBuf dcut(c, SL_HLL_CUT), cold(c, SL_HLL_COLD_FLAGS), cnt(c, SL_HLL_CNT);
    int rc;
    if ((rc = dcut.alloc(8 * ucut.size()))) return rc;
    if ((rc = cold.alloc(n_genomes))) return rc;
    if ((rc = cnt.alloc(64))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dcut.p, ucut.data(), 8 * ucut.size(), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemsetAsync(cold.p, 0, n_genomes, c->stream));
    GS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 8, c->stream));
    // register file: u32 in LDS while it fits; beyond that a per-workgroup global table behind a 2-byte LDS filter (while THAT fits)
    const size_t lds_cap = 160 * 1024 - 256;
    const bool gtab = 4 * ((size_t)m + 8) > lds_cap;
    const int use_filter = gtab && 32 + 2 * (size_t)m <= lds_cap;
    const size_t lds0 = !gtab ? 4 * ((size_t)m + 8) : (use_filter ? 32 + 2 * (size_t)m : 32);
    // survivor queues of the warm kernel (8 kB): only where they do not cost a resident workgroup
    const size_t lds_q = ((lds0 + 15) & ~(size_t)15) + (size_t)(HL_T / 64) * 128 * 8, half_cu = (160 * 1024) / 2 / 1280 * 1280;
    const bool use_q = !(getenv("GS_HLL_QUEUE") && !atoi(getenv("GS_HLL_QUEUE"))) && (lds_q <= half_cu || (lds0 > half_cu && lds_q <= lds_cap));
    const uint32_t queue_off = use_q ? (uint32_t)((lds0 + 15) & ~(size_t)15) : 0u;
    const size_t lds = use_q ? lds_q : lds0;
    const uint32_t wgs = (uint32_t)std::min<uint64_t>(n_genomes, (uint64_t)c->n_cu * 2);
    PoolBuf gt(c, SL_HLL_GTAB), sv(c, SL_HLL_SURVIVORS);
    if (gtab && (rc = gt.alloc((size_t)4 * m * std::max<uint32_t>(wgs, (uint32_t)c->n_cu)))) return rc;
    // survivor lists of pass A: 2^20 hashes (8 MB) per workgroup - ~8 % of the k-mers of a 5 Mbp genome survive the running cut; a longer genome
    // overflows its list and takes the second walk as before (GS_HLL_SURVIVORS=n: lists of n hashes, 0 = always the second walk)
    uint32_t surv_cap = getenv("GS_HLL_SURVIVORS") ? (uint32_t)std::max(0, std::min(1 << 24, atoi(getenv("GS_HLL_SURVIVORS")))) : (1u << 20);
    // GS_HLL_SPEC: the c of the speculative single pass (k_sketch_hll; default 8, 0 = the two exact passes only)
    const float spec_c = getenv("GS_HLL_SPEC") ? (float)atof(getenv("GS_HLL_SPEC")) : 8.0f;   // (one genome per workgroup and launch tail: a failed guess doubles that workgroup's time)
    const uint32_t surv_minch = getenv("GS_HLL_SURVIVORS_MINCHUNKS") ? (uint32_t)std::max(4, atoi(getenv("GS_HLL_SURVIVORS_MINCHUNKS"))) : 64u;
    //  the lists are only allocated when some genome of the batch can reach `surv_minch` chunks - no genome holds more units than the whole
    // batch does -, and a batch whose lists do not fit takes the plain second walk instead of failing the call
    if (total_units / ((uint64_t)HL_T * 8) < surv_minch) surv_cap = 0;
    if (surv_cap && sv.alloc((size_t)8 * surv_cap * wgs) != GS_OK) { (void)hipGetLastError(); surv_cap = 0; }
    {
        ProfScope ps(c, FAM_SKETCH);
    // (GS_HLL_TIGHT=0/1 overrides the choice for A/B)
    const double per_reg = 32.0 * (double)total_units / (double)std::max<uint64_t>(n_genomes, 1) / (double)m;       // (a unit is 32 symbols)
    const bool tight = getenv("GS_HLL_TIGHT") ? atoi(getenv("GS_HLL_TIGHT")) != 0 : per_reg >= 16.0;       // (measured from 55 k-mers per register up: always)
#define GS_LAUNCH_HLL(AAV, GV) do { if (tight) GS_LAUNCH_HLL_T(AAV, GV, true); else GS_LAUNCH_HLL_T(AAV, GV, false); } while (0)
#define GS_LAUNCH_HLL_T(AAV, GV, TV)                                                                                           \
    do {                                                                                                                       \
        auto kern = k_sketch_hll<AAV, false, GV, TV>;                                                                          \
        if (lds > 48 * 1024) GS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(kern, dim3(wgs), dim3(HL_T), lds, c->stream, seq, rec_start, rec_len, rec_upre, genome_rec_off, gen_units, (const uint32_t *)nullptr, \
                           (uint32_t)n_genomes, kq_of(p), m, inv_lnb, dcut.as<uint64_t>(), (uint32_t *)nullptr, (uint32_t *)nullptr, cnt.as<unsigned long long>(), cold.as<uint8_t>(), sig_out, \
                           gt.as<uint32_t>(), use_filter, queue_off, surv_cap ? sv.as<uint64_t>() : (uint64_t *)nullptr, surv_cap, surv_minch, spec_c); \
    } while (0)
        if (aa) { if (gtab) GS_LAUNCH_HLL(true, true); else GS_LAUNCH_HLL(true, false); }
        else { if (gtab) GS_LAUNCH_HLL(false, true); else GS_LAUNCH_HLL(false, false); }
#undef GS_LAUNCH_HLL
#undef GS_LAUNCH_HLL_T
    }
    GS_HIP_CHECK(hipGetLastError());
    std::vector<uint8_t> h(n_genomes);
    GS_HIP_CHECK(hipMemcpyAsync(h.data(), cold.p, n_genomes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> list;
    for (uint64_t g = 0; g < n_genomes; g++) if (h[g]) list.push_back((uint32_t)g);
    if (list.empty()) return GS_OK;
    // cold genomes (few k-mers per register): exact walks with the permutation in per-lane global scratch
    const uint32_t nc = (uint32_t)list.size();
    // one workgroup needs 2 x 4 x m x HL_CT bytes of per-lane scratch (205 MB at m = 100 000): as many workgroups as a quarter of the free memory
    // (at most 16 GB) holds - they pull the cold genomes from a shared counter, fewer workgroups only take more turns
    uint32_t cw = std::min<uint32_t>(nc, (uint32_t)c->n_cu);
    {
        size_t fr = 0, tot = 0;
        uint64_t budget = (uint64_t)4 << 30;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::min<uint64_t>((uint64_t)16 << 30, std::max<uint64_t>((uint64_t)fr / 4, (uint64_t)64 << 20));
        cw = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cw, budget / ((uint64_t)8 * m * HL_CT)));
    }
    PoolBuf dl(c, SL_HLL_COLD_LIST), lq(c, SL_HLL_COLD_Q), lp(c, SL_HLL_COLD_P);
    if ((rc = dl.alloc(4 * (size_t)nc))) return rc;
    if ((rc = lq.alloc((size_t)4 * cw * m * HL_CT))) return rc;
    if ((rc = lp.alloc((size_t)4 * cw * m * HL_CT))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dl.p, list.data(), 4 * (size_t)nc, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemsetAsync(lq.p, 0xFF, (size_t)4 * cw * m * HL_CT, c->stream));
    GS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 8, c->stream));
#define GS_LAUNCH_HLLC(AAV, GV)                                                                                                \
    do {                                                                                                                       \
        auto kern = k_sketch_hll<AAV, true, GV>;                                                                               \
        if (lds > 48 * 1024) GS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(kern, dim3(cw), dim3(HL_CT), lds, c->stream, seq, rec_start, rec_len, rec_upre, genome_rec_off, gen_units, dl.as<uint32_t>(), nc, kq_of(p), m, \
                           inv_lnb, dcut.as<uint64_t>(), lq.as<uint32_t>(), lp.as<uint32_t>(), cnt.as<unsigned long long>(), cold.as<uint8_t>(), sig_out, \
                           gt.as<uint32_t>(), use_filter, 0u, (uint64_t *)nullptr, 0u, 0u, 0.0f);                              \
    } while (0)
    if (aa) { if (gtab) GS_LAUNCH_HLLC(true, true); else GS_LAUNCH_HLLC(true, false); }
    else { if (gtab) GS_LAUNCH_HLLC(false, true); else GS_LAUNCH_HLLC(false, false); }
#undef GS_LAUNCH_HLLC
    GS_HIP_CHECK(hipGetLastError());
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

// =====================================================================================================
// hmh (HyperMinHash of hypermash, SPEC 7): per k-mer one hash chain (fx64, two SplitMix64 outputs) and a register max. The 16384 registers
// live in LDS as u32 (64 KB: two workgroups per CU) and take ds_max_u32. A genome split over `parts` workgroups (fewer genomes than
// 2 x CUs: a metagenome) merges its parts by max into a u32 table in global memory, narrowed to u16 by k_hmh_narrow.
// =====================================================================================================
struct HmhEmit {
    uint32_t *table;
    __device__ __forceinline__ void operator()(uint64_t v, uint64_t, uint64_t) const
    {
        uint32_t idx, reg;
        hmh_update(v, idx, reg);
        atomicMax(&table[idx], reg);
    }
};
__global__ __launch_bounds__(SK_THREADS) void k_sketch_hmh(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start,
                                                           const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ rec_upre,
                                                           const uint64_t *__restrict__ genome_rec_off, const uint64_t *__restrict__ gen_units,
                                                           uint32_t k, uint16_t *__restrict__ sig, uint32_t *__restrict__ gtab)
{
    __shared__ uint32_t s_tab[GS_HMH_M];
    const uint64_t g = blockIdx.y;
    const uint32_t part = blockIdx.x, parts = gridDim.x;
    for (uint32_t i = threadIdx.x; i < GS_HMH_M; i += blockDim.x) s_tab[i] = 0;
    __syncthreads();
    HmhEmit emit{s_tab};
    walk_genome<false, HmhEmit, 0>(seq, rec_start, rec_len, rec_upre, genome_rec_off[g], genome_rec_off[g + 1], gen_units[g], k, part, parts, emit);
    __syncthreads();
    if (parts == 1) {
        uint16_t *o = sig + g * (uint64_t)GS_HMH_M;
        for (uint32_t i = threadIdx.x; i < GS_HMH_M; i += blockDim.x) o[i] = (uint16_t)s_tab[i];
    } else {
        uint32_t *t = gtab + g * (uint64_t)GS_HMH_M;
        for (uint32_t i = threadIdx.x; i < GS_HMH_M; i += blockDim.x) { const uint32_t v = s_tab[i]; if (v) atomicMax(&t[i], v); }
    }
}
__global__ void k_hmh_narrow(const uint32_t *__restrict__ gtab, uint64_t n, uint16_t *__restrict__ sig)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) sig[i] = (uint16_t)gtab[i];
}

static int run_hmh(gs_ctx *c, const gs_sketch_params *p, const uint8_t *seq, const uint64_t *rec_start, const uint64_t *rec_len,
                   const uint64_t *rec_upre, const uint64_t *genome_rec_off, const uint64_t *gen_units, uint64_t n_genomes, uint64_t avg_units, uint16_t *sig_out)
{
    const MinGeom ge = min_geom(c, GS_HMH_M, 4, n_genomes, avg_units);
    PoolBuf gt(c, SL_HMH_GTAB);
    int rc;
    if (ge.parts > 1) {
        if ((rc = gt.alloc((size_t)n_genomes * GS_HMH_M * 4))) return rc;
        GS_HIP_CHECK(hipMemsetAsync(gt.p, 0, (size_t)n_genomes * GS_HMH_M * 4, c->stream));
    }
    c->last_sketch[0] = 0; c->last_sketch[1] = 1; c->last_sketch[2] = ge.parts; c->last_sketch[3] = 0;
    for (uint64_t g0 = 0; g0 < n_genomes; g0 += 65535) {       // grid.y limit
        const uint64_t ng = n_genomes - g0 < 65535 ? n_genomes - g0 : 65535;
        c->last_sketch[3]++;
        ProfScope ps(c, FAM_SKETCH);
        hipLaunchKernelGGL(k_sketch_hmh, dim3(ge.parts, (uint32_t)ng), dim3(SK_THREADS), 0, c->stream, seq, rec_start, rec_len, rec_upre, genome_rec_off + g0,
                           gen_units + g0, p->k, sig_out + g0 * GS_HMH_M, ge.parts > 1 ? gt.as<uint32_t>() + g0 * GS_HMH_M : (uint32_t *)nullptr);
        GS_HIP_CHECK(hipGetLastError());
    }
    if (ge.parts > 1) {
        const uint64_t n = n_genomes * GS_HMH_M;
        hipLaunchKernelGGL(k_hmh_narrow, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 65536)), dim3(256), 0, c->stream, gt.as<uint32_t>(), n, sig_out);
        GS_HIP_CHECK(hipGetLastError());
    }
    return GS_OK;
}

// what every slot-min algorithm starts with: the unit prefix of the records and the units of each genome, queued on c's stream
static int unit_prefix(gs_ctx *c, uint32_t k, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes,
                       PoolBuf &upre, PoolBuf &gunits)
{
    int rc;
    if ((rc = upre.alloc(8 * (n_rec + 1))) || (rc = gunits.alloc(8 * n_genomes))) return rc;
    hipLaunchKernelGGL(k_unit_prefix, dim3((uint32_t)((n_genomes + 3) / 4)), dim3(256), 0, c->stream, rec_start, rec_len, genome_rec_off, n_genomes, k, upre.as<uint64_t>(),
                       gunits.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

int sketch_dev_impl(gs_ctx *c, const gs_sketch_params *p, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start,
                    const uint64_t *rec_len, uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, void *sig_out, bool sync_at_end)
{
    int rc = gs_check_params(p);
    if (rc) return rc;
    GS_REQUIRE(c && (n_genomes == 0 || (seq && rec_start && rec_len && genome_rec_off && sig_out)), GS_ERR_INVALID, "null argument");
    if (n_genomes == 0) return GS_OK;
    GS_REQUIRE(n_genomes < ((uint64_t)1 << 31), GS_ERR_INVALID, "too many genomes in one batch");
    GS_CTX_LOCK(c);
    GS_HIP_CHECK(hipSetDevice(c->device));
    const uint32_t m = p->sketch_size;
    if (p->algo == GS_ALGO_OPTDENS || p->algo == GS_ALGO_REVOPTDENS) {
        PoolBuf upre(c, SL_SK_REC_UNITS), gunits(c, SL_SK_GENOME_UNITS), table(c, SL_OPH_TABLE), win(c, SL_OPH_WIN);
        rc = unit_prefix(c, p->k, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, upre, gunits); if (rc) return rc;
        rc = table.alloc((size_t)n_genomes * m * 4); if (rc) return rc;
        if (p->algo == GS_ALGO_REVOPTDENS) { rc = win.alloc((size_t)n_genomes * m * 4); if (rc) return rc; }
        uint64_t avg_units = (p->data_t == GS_DATA_AA ? seq_bytes / 32 : seq_bytes / 8) / n_genomes + 1;
        rc = launch_oph(c, p, (const uint8_t *)seq, rec_start, rec_len, upre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(),
                        n_genomes, avg_units, table.as<uint32_t>(), win.as<uint32_t>(), (float *)sig_out);
        if (rc) return rc;
        // (the leases end here with the kernels still queued: the slots are only reused by later calls on this context, i.e. behind these kernels on
        // its stream - a caller that pipelines several sketches, gs_index_sketch_and_search_dev, may leave the wait to its own events)
        if (sync_at_end) GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    if (p->algo == GS_ALGO_SUPER || p->algo == GS_ALGO_SUPER2) {
        PoolBuf upre(c, SL_SK_REC_UNITS), gunits(c, SL_SK_GENOME_UNITS);
        rc = unit_prefix(c, p->k, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, upre, gunits); if (rc) return rc;
        const uint64_t avg_units = (p->data_t == GS_DATA_AA ? seq_bytes / 32 : seq_bytes / 8) / n_genomes + 1;
        const uint8_t *sq = (const uint8_t *)seq;
        const uint64_t *up = upre.as<uint64_t>(), *gu = gunits.as<uint64_t>();
        const int vb = gs_value_bits(p);
        if (p->algo == GS_ALGO_SUPER) rc = run_smh<ALGO_SUPER, 64, uint32_t>(c, p, sq, rec_start, rec_len, up, genome_rec_off, gu, n_genomes, avg_units, sig_out);
        else if (vb == 32) rc = run_smh<ALGO_SUPER2, 32, uint32_t>(c, p, sq, rec_start, rec_len, up, genome_rec_off, gu, n_genomes, avg_units, sig_out);
        else rc = run_smh<ALGO_SUPER2, 64, uint64_t>(c, p, sq, rec_start, rec_len, up, genome_rec_off, gu, n_genomes, avg_units, sig_out);
        if (rc) return rc;
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    if (p->algo == GS_ALGO_HLL) {
        PoolBuf upre(c, SL_SK_REC_UNITS), gunits(c, SL_SK_GENOME_UNITS);
        rc = unit_prefix(c, p->k, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, upre, gunits); if (rc) return rc;
        rc = run_hll(c, p, (const uint8_t *)seq, rec_start, rec_len, upre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(), n_genomes, (p->data_t == GS_DATA_AA ? seq_bytes / 32 : seq_bytes / 8) + n_rec + 1, (uint16_t *)sig_out);
        if (rc) return rc;
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    if (p->algo == GS_ALGO_HMH) {
        PoolBuf upre(c, SL_SK_REC_UNITS), gunits(c, SL_SK_GENOME_UNITS);
        rc = unit_prefix(c, p->k, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, upre, gunits); if (rc) return rc;
        rc = run_hmh(c, p, (const uint8_t *)seq, rec_start, rec_len, upre.as<uint64_t>(), genome_rec_off, gunits.as<uint64_t>(), n_genomes,
                     seq_bytes / 8 / n_genomes + 1, (uint16_t *)sig_out);
        if (rc) return rc;
        if (sync_at_end) GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    if (p->algo == GS_ALGO_PROB3A) {
        rc = run_prob(c, p, (const uint8_t *)seq, seq_bytes, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, sig_out);
        if (rc) return rc;
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    GS_REQUIRE(false, GS_ERR_UNSUPPORTED, "sketch algo %u is not implemented on the device", p->algo);
}

}  // namespace gs

extern "C" {

int gs_sketch_batch_dev(gs_ctx *c, const gs_sketch_params *p, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev,
                        const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes,
                        void *sig_out_dev)
{
    return gs::sketch_dev_impl(c, p, seq_dev, seq_bytes, rec_start_dev, rec_len_dev, n_rec, genome_rec_off_dev, n_genomes, sig_out_dev, true);
}

int gs_sketch_batch(gs_ctx *c, const gs_sketch_params *p, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start,
                    const uint64_t *rec_len, uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, void *sig_out)
{
    int rc = gs_check_params(p);
    if (rc) return rc;
    GS_REQUIRE(c && (n_genomes == 0 || (rec_start && rec_len && genome_rec_off && sig_out)), GS_ERR_INVALID, "null argument");
    if (n_genomes == 0) return GS_OK;
    GS_REQUIRE(seq || seq_bytes == 0, GS_ERR_INVALID, "null sequence buffer");
    // every record must lie inside the buffer
    const uint64_t sym_cap = p->data_t == GS_DATA_AA ? seq_bytes : seq_bytes * 4;
    for (uint64_t r = 0; r < n_rec; r++)
        GS_REQUIRE(rec_start[r] + rec_len[r] <= sym_cap, GS_ERR_INVALID, "record %llu exceeds the sequence buffer", (unsigned long long)r);
    GS_REQUIRE(genome_rec_off[n_genomes] <= n_rec, GS_ERR_INVALID, "genome_rec_off exceeds n_rec");
    // (a worker thread of the host runs on its own stream and scratch, see gs_internal.hpp; a device failure there is repeated on the main context)
    return gs::on_worker(c, [&](gs_ctx *c) -> int {
    int rc;
    GS_CTX_LOCK(c);
    GS_HIP_CHECK(hipSetDevice(c->device));
    // staging from the context's grow-only pool: a hipMalloc / hipFree pair per call costs more than a small sketch and, worse, hipFree waits for
    // every stream of the device - which would serialise the worker contexts of other host threads
    gs::PoolBuf dseq(c, gs::SL_SKB_SEQ), drs(c, gs::SL_SKB_REC_START), drl(c, gs::SL_SKB_REC_LEN), dgo(c, gs::SL_SKB_GENOME_OFF), dsig(c, gs::SL_SKB_SIG);
    const uint64_t padded = gs::round_up(seq_bytes, 32) + 32;
    const size_t sigbytes = (size_t)n_genomes * p->sketch_size * gs_sig_elem_bytes(p);
    if ((rc = dseq.alloc(padded))) return rc;
    if ((rc = drs.alloc(8 * (n_rec + 1)))) return rc;
    if ((rc = drl.alloc(8 * (n_rec + 1)))) return rc;
    if ((rc = dgo.alloc(8 * (n_genomes + 1)))) return rc;
    if ((rc = dsig.alloc(sigbytes))) return rc;
    GS_HIP_CHECK(hipMemsetAsync((uint8_t *)dseq.p + (padded - 64), 0, 64, c->stream));
    if (seq_bytes) GS_HIP_CHECK(hipMemcpyAsync(dseq.p, seq, seq_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_rec) {
        GS_HIP_CHECK(hipMemcpyAsync(drs.p, rec_start, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(drl.p, rec_len, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
    }
    GS_HIP_CHECK(hipMemcpyAsync(dgo.p, genome_rec_off, 8 * (n_genomes + 1), hipMemcpyHostToDevice, c->stream));
    rc = gs::sketch_dev_impl(c, p, dseq.p, padded, drs.as<uint64_t>(), drl.as<uint64_t>(), n_rec, dgo.as<uint64_t>(), n_genomes, dsig.p, true);
    if (rc) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(sig_out, dsig.p, sigbytes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
    });
}

}  // extern "C"
