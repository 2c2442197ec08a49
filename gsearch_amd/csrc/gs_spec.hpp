// gs_spec.hpp — SPEC.md section 2 (hashing + random numbers) for device and host code of the product.
// Every [CHOICE] of SPEC.md that touches arithmetic lives in this header or, for the units of SPEC 13, in gs_hmm_parse.hpp,
// which it includes (and, independently restated, in oracle/gs_oracle.c). Replaces what gsearch reaches through fxhash / rand_xoshiro / rand
// (Cargo.toml:26,122 of the reference; crates not vendored).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "gs_bigsi_file.hpp"
#include "gs_hmm_parse.hpp"

#define GS_HD __host__ __device__ __forceinline__

namespace gs {

GS_HD uint64_t rotl64(uint64_t x, int r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // two v_alignbit_b32 (one funnel shift per half) instead of the v_lshlrev_b64 + v_lshrrev_b32 + v_or_b32 the compiler picks for the
    // constant rotates of xoshiro (23, 45)
    if (__builtin_constant_p(r) && r > 0 && r < 64 && r != 32) {
        const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
        const uint32_t a = r < 32 ? hi : lo, b = r < 32 ? lo : hi, s = 32 - (r & 31);
        uint64_t y = ((uint64_t)__builtin_amdgcn_alignbit(a, b, s) << 32) | __builtin_amdgcn_alignbit(b, a, s);
        asm("" : "+v"(y));          // keep the result one 64-bit value: otherwise `rotl64(x, r) + y` is split into a 32-bit add, a move and a 64-bit add
        return y;
    }
#endif
    return (x << r) | (x >> (64 - r));
}
GS_HD uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// x * c + a mod 2^64 for constants c and a. On the device hipcc selects v_mad_u64_u32 (x_lo c_lo + a) + 2 v_mul_lo_u32 (the cross terms) +
// v_add3_u32. Here the cross sum lo32(x_hi c_lo + x_lo c_hi) is one v_mul_lo_u32 and the low half of a v_mad_u64_u32 that adds it; it then
// enters the high half of the addend of the last v_mad_u64_u32 (x_lo c_lo + (cross << 32)): three multiplies and two moves, 171 instead of
// 181 issue cycles per dropped k-mer of the whole hash chain (tools/ubench_valu). A non-zero a joins that addend as
// a_lo : (a_hi + cross), so that its carry out of the low half stays inside the multiply-add.
GS_HD uint64_t mulc64(uint64_t x, uint64_t c, uint64_t a = 0)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32), cl = (uint32_t)c, ch = (uint32_t)(c >> 32);
    uint64_t cr = (uint64_t)xh * cl + (uint32_t)(xl * ch);
    asm("" : "+v"(cr));         // keep the 64-bit multiply-add: narrowed to 32 bits it becomes a v_mul_lo_u32 that a v_add3_u32 takes back in
    if (a == 0) return (uint64_t)xl * cl + ((uint64_t)(uint32_t)cr << 32);
    uint32_t zh = (uint32_t)(a >> 32) + (uint32_t)cr;
    asm("" : "+v"(zh));
    uint64_t z = ((uint64_t)zh << 32) | (uint32_t)a;
    asm("" : "+v"(z));          // one addend: otherwise a is split off and follows the multiply-add as a 64-bit add
    return (uint64_t)xl * cl + z;
#else
    return x * c + a;
#endif
}

// fxhash::FxHasher64 over one integer write (+ a: an offset the caller adds, folded into the multiply-add on the device)
GS_HD uint64_t fx64(uint64_t v, uint64_t a = 0) { return mulc64(v, 0x517cc1b727220a95ULL, a); }
// fxhash::FxHasher32: 32-bit words, low first
GS_HD uint64_t fx32_w32(uint32_t v) { return (uint64_t)(uint32_t)(v * 0x9e3779b9u); }

enum { ALGO_PROB3A = 0, ALGO_SUPER = 1, ALGO_SUPER2 = 2, ALGO_HLL = 3, ALGO_OPTDENS = 4, ALGO_REVOPTDENS = 5 };

// SPEC 2 table "element hash" (+ a: an offset the caller adds, folded into fx64's multiply-add on the device)
template <int ALGO, int VBITS>
GS_HD uint64_t elem_hash(uint64_t v, uint64_t a = 0)
{
    if (ALGO == ALGO_PROB3A) return v + a;
    if (ALGO == ALGO_HLL) return fx64(v, a);
    if (ALGO == ALGO_SUPER2 && VBITS == 32) return fx32_w32((uint32_t)v) + a;
    return fx64(v, a);
}

// one SplitMix64 output for counter value x (already advanced)
GS_HD uint64_t splitmix_mix(uint64_t z)
{
    z = mulc64(z ^ (z >> 30), 0xbf58476d1ce4e5b9ULL);
    z = mulc64(z ^ (z >> 27), 0x94d049bb133111ebULL);
    return z ^ (z >> 31);
}
// The high word of splitmix_mix(z) alone, for a caller that decides on it (the drop test of MinEmitF, gs_hiword.hpp): the last xor-shift is
// b_hi ^ (b_hi >> 31) - one 32-bit shift and one xor instead of a 64-bit shift and two xors - and the low word of the second product is dead
// (hipcc then takes a v_mul_hi_u32 in place of mulc64's last v_mad_u64_u32 by itself).
GS_HD uint32_t splitmix_mix_hi(uint64_t z)
{
    z = mulc64(z ^ (z >> 30), 0xbf58476d1ce4e5b9ULL);
    const uint32_t b = (uint32_t)(mulc64(z ^ (z >> 27), 0x94d049bb133111ebULL) >> 32);
    return b ^ (b >> 31);
}
// The LOW 9 BITS of that high word before its last xor-shift (b_hi above; splitmix_mix_hi(z) = b_hi ^ (b_hi >> 31) differs from it by at most one
// unit). The bits above the ninth are not the mix's: on the device the two cross terms of the second product come from 24-bit multiply-adds, which
// are right in their low 24 bits. For hiword_may_be_below_x (gs_hiword.hpp), which shifts s3's word up by 23 and so reads no other bit of it.
GS_HD uint32_t splitmix_mix_hi9(uint64_t z)
{
    z = mulc64(z ^ (z >> 30), 0xbf58476d1ce4e5b9ULL);
    z ^= z >> 27;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t xl = (uint32_t)z, xh = (uint32_t)(z >> 32), cl = 0x133111ebu, ch = 0x94d049bbu;
    uint32_t t = __umulhi(xl, cl);
    asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(t) : "v"(xl), "s"(ch));
    asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(t) : "v"(xh), "s"(cl));
    return t;
#else
    return (uint32_t)((z * 0x94d049bb133111ebULL) >> 32);
#endif
}
#define GS_GAMMA 0x9e3779b97f4a7c15ULL

struct Rng {   // xoshiro256++ seeded through SplitMix64 (rand_xoshiro seed_from_u64)
    uint64_t s0, s1, s2, s3;
    GS_HD void seed(uint64_t x)
    {
        s0 = splitmix_mix(x + GS_GAMMA);
        s1 = splitmix_mix(x + 2 * GS_GAMMA);
        s2 = splitmix_mix(x + 3 * GS_GAMMA);
        s3 = splitmix_mix(x + 4 * GS_GAMMA);
    }
    GS_HD uint64_t next64()
    {
        uint64_t r = rotl64(s0 + s3, 23) + s0;
        uint64_t t = s1 << 17;
        s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3;
        s2 ^= t; s3 = rotl64(s3, 45);
        return r;
    }
    GS_HD uint32_t next32() { return (uint32_t)(next64() >> 32); }
    GS_HD uint32_t r23() { return next32() >> 9; }                       // U32f = r23 * 2^-23
    GS_HD double u64f() { return (double)(next64() >> 12) * 0x1.0p-52; }  // U64f
};

GS_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// rand 0.8 UniformInt<usize>::sample for range [0,n): zone = 2^64-1 - (2^64 mod n)
GS_HD uint64_t uint_zone(uint64_t n) { return ~(uint64_t)0 - ((0 - n) % n); }
GS_HD uint64_t rng_uint(Rng &g, uint64_t n, uint64_t zone)
{
    for (;;) {
        uint64_t x = g.next64();
        uint64_t lo = x * n;
        if (lo <= zone) return mulhi64(x, n);
    }
}

// ---- the two-draw fast path of optdens (SPEC 3.1): r = U32f bits, b = Uint(m) ---------------------
// Only s0,s1,s3 are needed for two outputs; the full generator is re-run in the (probability m/2^64)
// rejection case so that the result is exactly the sequential definition.
// two_draw: first output o1 (the r draw: U32f bits = o1>>41, next32 = o1>>32, next64 = o1) and b = Uint(m) from the second.
// two_draw_from: the same from the three states a caller already holds some of (s0, s1, s3 of Rng::seed(h)); h itself only for the re-run.
GS_HD void two_draw_from(uint64_t h, uint64_t s0, uint64_t s1, uint64_t s3, uint32_t m, uint64_t zone, uint64_t &o1, uint32_t &bin)
{
    o1 = rotl64(s0 + s3, 23) + s0;
    uint64_t n3 = s3 ^ s1;           // s3 after the first step, before rotation
    uint64_t n0 = s0 ^ n3;           // s0 after the first step
    uint64_t o2 = rotl64(n0 + rotl64(n3, 45), 23) + n0;
    // Uint(g, m) with m < 2^32: the 96-bit product o2 * m from two 32 x 32 -> 64 multiply-adds. Its top 32 bits are the draw, its low 64
    // bits the rejection test `lo <= zone` - and zone >= 2^64 - 2^32, so a rejection needs the upper half of lo to be all ones: one
    // 32-bit compare on the hot path, the exact 64-bit test (and the re-run of the full generator) only behind it.
    const uint64_t t = (uint64_t)(uint32_t)o2 * m;
    const uint64_t u = (uint64_t)(uint32_t)(o2 >> 32) * m + (t >> 32);
    bin = (uint32_t)(u >> 32);
    if (__builtin_expect((uint32_t)u != 0xFFFFFFFFu, 1)) return;
    const uint64_t lo = (u << 32) | (uint32_t)t;
    if (lo <= zone) return;
    Rng g; g.seed(h); (void)g.next64();
    bin = (uint32_t)rng_uint(g, (uint64_t)m, zone);
}
GS_HD void two_draw(uint64_t h, uint32_t m, uint64_t zone, uint64_t &o1, uint32_t &bin)
{
    two_draw_from(h, splitmix_mix(h + GS_GAMMA), splitmix_mix(h + 2 * GS_GAMMA), splitmix_mix(h + 4 * GS_GAMMA), m, zone, o1, bin);
}
GS_HD void oph_draw(uint64_t h, uint32_t m, uint64_t zone, uint32_t &r23, uint32_t &bin)
{
    uint64_t o1;
    two_draw(h, m, zone, o1, bin);
    r23 = (uint32_t)(o1 >> 41);
}

// ---- SPEC 2 LN / TEXP, SPEC 3.4 hll (SetSketch1): natural logarithm from IEEE + - * / only (no fma contraction: the library is
// built with -ffp-contract=off), so the host oracle and the device evaluate the same instruction sequence
GS_HD double spec_ln(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
#else
    uint64_t bits; __builtin_memcpy(&bits, &x, 8);
#endif
    long long e = (long long)((bits >> 52) & 0x7FF) - 1023;
    const uint64_t mb = (bits & 0x000FFFFFFFFFFFFFULL) | 0x3FF0000000000000ULL;
#if defined(__HIP_DEVICE_COMPILE__)
    double t = __longlong_as_double((long long)mb);
#else
    double t; __builtin_memcpy(&t, &mb, 8);
#endif
    if (t > 1.4142135623730951) { t = t * 0.5; e += 1; }
    const double s = (t - 1.0) / (t + 1.0), z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0; p = p * z + 1.0 / 19.0; p = p * z + 1.0 / 17.0; p = p * z + 1.0 / 15.0; p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0; p = p * z + 1.0 / 9.0; p = p * z + 1.0 / 7.0; p = p * z + 1.0 / 5.0; p = p * z + 1.0 / 3.0; p = p * z + 1.0;
    return (double)e * 0.6931471805599453 + 2.0 * s * p;
}
#define GS_HLL_B 1.001
#define GS_HLL_A 20.0
#define GS_HLL_Q 65534u
GS_HD uint32_t hll_k(double x, double inv_lnb)
{
    if (!(x > 0.0)) return GS_HLL_Q + 1;
    const double y = 1.0 - spec_ln(x) * inv_lnb;
    if (y < 0.0) return 0;
    if (y >= (double)(GS_HLL_Q + 1)) return GS_HLL_Q + 1;
    return (uint32_t)y;
}

// ---- SPEC 7 hmh (HyperMinHash, Yu & Weber 2017, as axiomhq/hyperminhash implements it) [PUB, recalled, unverified]: every constant and the
// element hash live here so that they can be re-aligned if the `hyperminhash` crate's source ever appears
#define GS_HMH_P 14u                     // m = 2^p registers
#define GS_HMH_Q 6u
#define GS_HMH_R 10u
#define GS_HMH_M 16384u
#define GS_HMH_SMALL 524288.0            // 2^(p+5): above it the closed form of the expected collisions
#define GS_HMH_NP 65536u                 // 2^q x 2^r terms of the small-set sum
// [CHOICE] h1, h2 = the first two SplitMix64 outputs from state fx64(v); register = (lz << r) | (h2 & (2^r - 1)), lz in [1, 51]
GS_HD void hmh_update(uint64_t v, uint32_t &idx, uint32_t &reg)
{
    const uint64_t x = fx64(v);
    const uint64_t h1 = splitmix_mix(x + GS_GAMMA), h2 = splitmix_mix(x + 2 * GS_GAMMA);
    idx = (uint32_t)(h1 >> (64 - GS_HMH_P));
    const uint32_t lz = (uint32_t)__builtin_clzll((h1 << GS_HMH_P) ^ 0x3FFFull) + 1;   // the low p bits are ones: never all-zero
    reg = (lz << GS_HMH_R) | (uint32_t)(h2 & ((1u << GS_HMH_R) - 1));
}
// a non-negative integer hi:lo (128 bits) rounded once (to nearest, ties to even) to f64
GS_HD double u128_to_f64(uint64_t hi, uint64_t lo)
{
    if (hi == 0) {
        // (double)lo with one rounding: the two 32-bit halves are exact, their sum is rounded once
        return (double)(uint32_t)(lo >> 32) * 4294967296.0 + (double)(uint32_t)lo;
    }
    const int s = 64 - __builtin_clzll(hi);                    // 1..64: bits of hi
    const uint64_t top = s == 64 ? hi : (hi << (64 - s)) | (lo >> s);
    const bool sticky = s == 64 ? lo != 0 : (lo << (64 - s)) != 0;
    uint64_t r = top >> 11;
    const uint64_t rem = top & 0x7FF;
    if (rem > 0x400 || (rem == 0x400 && (sticky || (r & 1)))) r++;
    double d = (double)(uint32_t)(r >> 32) * 4294967296.0 + (double)(uint32_t)r;     // r <= 2^53: exact
    d = d * 2048.0;
    for (int i = 0; i < s; i += 16) d = d * (double)(1u << (s - i < 16 ? s - i : 16));   // exact powers of two
    return d;
}
// cardinality from the number of empty registers ez and the exact register sum (units of 2^-51, 128-bit hi:lo)
GS_HD uint64_t hmh_card(uint32_t ez, uint64_t sum_hi, uint64_t sum_lo)
{
    const double m = (double)GS_HMH_M;
    const double sum = u128_to_f64(sum_hi, sum_lo) * 0x1.0p-51;
    const double ezf = (double)ez;
    const double zl = spec_ln(ezf + 1.0);
    const double z2 = zl * zl, z3 = z2 * zl, z4 = z3 * zl, z5 = z4 * zl, z6 = z5 * zl, z7 = z6 * zl;
    double beta = -0.370393911 * ezf;
    beta = beta + 0.070471823 * zl;
    beta = beta + 0.17393686 * z2;
    beta = beta + 0.16339839 * z3;
    beta = beta - 0.09237745 * z4;
    beta = beta + 0.03738027 * z5;
    beta = beta - 0.005384159 * z6;
    beta = beta + 0.00042419 * z7;
    const double alpha = 0.7213 / (1.0 + 1.079 / m);
    const double c = ((alpha * m) * (m - ezf)) / (beta + sum);
    return c >= 18446744073709551615.0 ? ~(uint64_t)0 : (uint64_t)c;
}
// the two parameters of the term index t in [0, 65536) of the small-set sum: i = t / 1024 + 1, j = t % 1024 + 1
GS_HD void hmh_b(uint32_t t, double &b1, double &b2)
{
    const uint32_t i = t / (1u << GS_HMH_R) + 1, j = t % (1u << GS_HMH_R) + 1;
    if (i < (1u << GS_HMH_Q)) {
        const double inv = ldexp(1.0, -(int)(GS_HMH_P + GS_HMH_R + i));                     // 2^-(24+i), exact
        b1 = (double)(1024 + j) * inv; b2 = (double)(1025 + j) * inv;
    } else {
        b1 = (double)j * 0x1.0p-87; b2 = (double)(j + 1) * 0x1.0p-87;
    }
}
// expected collisions in the closed form (n = max card > 2^(p+5), mn = min card)
GS_HD double hmh_ec_closed(double n, double mn)
{
    const double t = (1.0 + n) / mn;
    const double d = (4.0 * n / mn) / (t * t);
    return 0.169919487159739093975315012348 * 16.0 * d + 0.5;
}
GS_HD double hmh_sim_from(uint32_t C, uint32_t N, double ec)
{
    const double c = (double)C;
    if (c < ec) return 0.0;
    return (c - ec) / (double)N;
}

// ---- SPEC 2 EXP: e^x from IEEE f64 + - * / only (built with -ffp-contract=off, like spec_ln). Cody-Waite reduction x = k ln2 + r (ln2 split
// so that k * GS_LN2_HI is exact for |k| < 2^11), a degree-13 Horner Taylor polynomial of e^r (|r| <= 0.35), and an exact power-of-two scale
// (two factors below 2^-1022, so that a subnormal result is rounded once)
#define GS_LN2_HI 6.93147180369123816490e-01
#define GS_LN2_LO 1.90821492927058770002e-10
#define GS_INV_LN2 1.44269504088896338700e+00
GS_HD double pow2_int(long long k)        // 2^k for -1022 <= k <= 1023, built from its bits
{
    const uint64_t b = (uint64_t)(k + 1023) << 52;
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double d; __builtin_memcpy(&d, &b, 8); return d;
#endif
}
GS_HD double spec_exp(double x)
{
    if (x != x) return x;
    if (x < -745.2) return 0.0;
    if (x > 709.7) return 1.0 / 0.0;
    const long long k = (long long)(x * GS_INV_LN2 + (x < 0.0 ? -0.5 : 0.5));     // round half away from zero (the cast truncates)
    const double r = (x - (double)k * GS_LN2_HI) - (double)k * GS_LN2_LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0; p = p * r + 1.0 / 39916800.0; p = p * r + 1.0 / 3628800.0; p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0; p = p * r + 1.0 / 5040.0; p = p * r + 1.0 / 720.0; p = p * r + 1.0 / 120.0; p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0; p = p * r + 0.5; p = p * r + 1.0; p = p * r + 1.0;
    if (k < -1022) return (p * pow2_int(k + 1000)) * pow2_int(-1000);
    return p * pow2_int(k);
}

// ---- SPEC 8 ann (UMAP-like embedding of the k-NN graph, McInnes, Healy & Melville 2018, a = b = 1) [PUB] / [CHOICE]: every constant here
#define GS_EMBED_KNBN 8u                  // [REF] embed.rs:19 kgraph_from_hnsw_all(hnsw, 8)
#define GS_EMBED_DIM 2u                   // [REF] 2-D output
#define GS_EMBED_DIM_MAX 4u
#define GS_EMBED_EPOCHS 300u              // [CHOICE] E
#define GS_EMBED_NEG 8u                   // [CHOICE] S negative samples per node and epoch
#define GS_EMBED_NEG_RATE 1.0f            // [CHOICE] r
#define GS_EMBED_LR 0.25f                 // [CHOICE] lr
#define GS_EMBED_SEED 0x5eedULL           // [CHOICE]
#define GS_EMBED_INIT_HALF 10.0f          // [CHOICE] seeded positions in [-10, 10)
#define GS_EMBED_LIGHT 64u                // [CHOICE] L_H: a longer adjacency is summed by one wavefront
#define GS_EMBED_CLAMP 4.0f               // [PUB] umap's gradient clip
#define GS_EMBED_EPS 0.001f               // [PUB] umap's repulsion offset
#define GS_EMBED_BISECT 64                // [PUB] umap smooth_knn_dist n_iter
#define GS_EMBED_TOL 1e-5                 // [PUB] SMOOTH_K_TOLERANCE
#define GS_EMBED_MIN_SCALE 1e-3           // [PUB] MIN_K_DIST_SCALE (floor of sigma, times the row's mean distance)
#define GS_EMBED_HIST_BINS 64u            // [CHOICE] B: k-occurrence bins 0..B-1, then one overflow bin
#define GS_EMBED_HUBS 16u
#define GS_EMBED_TAG_INIT 0x696e6974ULL   // "init"
#define GS_EMBED_TAG_NEG 0x6e6567ULL      // "neg"
// initial coordinate t of node i: 24 bits of a counter-based hash, exact in f32, then * 2 * INIT_HALF - INIT_HALF
GS_HD float embed_init_coord(uint64_t seed, uint64_t i, uint32_t dim, uint32_t t)
{
    const uint64_t h = splitmix_mix(splitmix_mix(seed ^ GS_EMBED_TAG_INIT) + GS_GAMMA * (i * dim + t + 1));
    const float u = (float)(uint32_t)(h >> 40) * 0x1.0p-24f;
    return u * (2.0f * GS_EMBED_INIT_HALF) - GS_EMBED_INIT_HALF;
}
// the per-epoch key of the negative samples, and the s-th sample of node i in [0, n): 64 x 64 -> high 64 multiply
GS_HD uint64_t embed_epoch_key(uint64_t seed, uint32_t e) { return splitmix_mix(seed ^ GS_EMBED_TAG_NEG) + GS_GAMMA * ((uint64_t)e + 1); }
GS_HD uint64_t embed_neg(uint64_t ekey, uint64_t i, uint32_t S, uint32_t s, uint64_t n)
{
    return mulhi64(splitmix_mix(splitmix_mix(ekey) + GS_GAMMA * (i * S + s + 1)), n);
}

// ---- SPEC 9: FracMinHash / bottom-k sketches of superaai (binaux/src/bin/superaai.rs) ------------------------------------------------
#define GS_FRAC_SEED 42ULL               // [REF] superaai.rs:123,133,143,153: the literal seed of every hash
#define GS_FRAC_KMAX 32u                 // [CHOICE] 1 <= k <= 32
#define GS_MM3_C1 0x87c37b91114253d5ULL  // [PUB] SMHasher MurmurHash3_x64_128
#define GS_MM3_C2 0x4cf5ad432745937fULL
GS_HD uint64_t mm3_fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}
// h1 of MurmurHash3_x64_128 over len (<= 32) bytes held little-endian in w0..w3 (bytes past len are zero), seed GS_FRAC_SEED:
// 16-byte blocks, then the tail (its bytes 8..14 into k2, 0..7 into k1), then the finalisation. sourmash's _hash_murmur keeps h1.
GS_HD void mm3_block(uint64_t &h1, uint64_t &h2, uint64_t k1, uint64_t k2)
{
    k1 *= GS_MM3_C1; k1 = rotl64(k1, 31); k1 *= GS_MM3_C2; h1 ^= k1;
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= GS_MM3_C2; k2 = rotl64(k2, 33); k2 *= GS_MM3_C1; h2 ^= k2;
    h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
}
GS_HD uint64_t mm3_h1_4(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t len)
{
    uint64_t h1 = GS_FRAC_SEED, h2 = GS_FRAC_SEED;
    if (len >= 16) mm3_block(h1, h2, w0, w1);
    if (len >= 32) mm3_block(h1, h2, w2, w3);
    const uint32_t rem = len & 15;
    const uint64_t t1 = len >= 16 ? w2 : w0, t2 = len >= 16 ? w3 : w1;
    if (rem > 8) { uint64_t k2 = t2; k2 *= GS_MM3_C2; k2 = rotl64(k2, 33); k2 *= GS_MM3_C1; h2 ^= k2; }
    if (rem > 0) { uint64_t k1 = t1; k1 *= GS_MM3_C1; k1 = rotl64(k1, 31); k1 *= GS_MM3_C2; h1 ^= k1; }
    h1 ^= len; h2 ^= len;
    h1 += h2; h2 += h1;
    h1 = mm3_fmix64(h1); h2 = mm3_fmix64(h2);
    return h1 + h2;
}
// sourmash max_hash_for_scaled (recalled): 0 -> 0 (no filter), 1 -> 2^64-1, else (u64)((f64)(2^64-1) / (f64)scaled), truncated
inline uint64_t frac_max_hash(uint32_t scaled)
{
    if (scaled == 0) return 0;
    if (scaled == 1) return ~0ULL;
    return (uint64_t)((double)~0ULL / (double)scaled);
}

// ---- SPEC 10: coreset sampling of hnswcore ---------------------------------------------------------------------------------------------
// h(r, i): the draw of node i in sampling round r
GS_HD uint64_t cluster_hash(uint64_t seed, uint32_t r, uint64_t i) { return splitmix_mix((seed ^ ((uint64_t)r << 56) ^ i) + GS_GAMMA); }
// round 0 keeps i with (h >> 32) n < t0 << 32, round 1 with (h >> 40) D < (t1 d0) << 24: both sides fit 64 bits for n < 2^32, n m < 2^40
GS_HD bool cluster_keep0(uint64_t h, uint64_t n, uint64_t t0) { return (h >> 32) * n < (t0 << 32); }
GS_HD bool cluster_keep1(uint64_t h, uint64_t D, uint64_t t1, uint32_t d0) { return (h >> 40) * D < ((t1 * d0) << 24); }

// ---- SPEC 11: bigsig (binaux/src/bin/bigsig.rs) - row positions of a k-mer in the bit-sliced Bloom index and the significance of a read's best hit.
// [CHOICE] (the `bigsig` crate's hash and test are not vendored): every constant and step lives here
// GS_BIGSI_KMAX / _HMAX / _BMAX (1 <= k <= 32, 1 <= num_hash <= 16, 1 <= bloom_size < 2^40): gs_bigsi_file.hpp, the host-only reader of .gsbx files checks them too
#define GS_BIGSI_TAIL_CUT 0x1.0p-60      // the tail sum stops at a term below tail x 2^-60
// h1 and the odd step of the double hashing: the first two SplitMix64 outputs from state fx64(v), as hmh_update
GS_HD void bigsi_hash(uint64_t v, uint64_t &h1, uint64_t &step)
{
    const uint64_t x = fx64(v);
    h1 = splitmix_mix(x + GS_GAMMA);
    step = splitmix_mix(x + 2 * GS_GAMMA) | 1;
}
GS_HD uint64_t bigsi_pos(uint64_t h1, uint64_t step, uint32_t i, uint64_t B) { return mulhi64(h1 + (uint64_t)i * step, B); }
// SPEC 11.1: the minimizer of one window - the offset in [0, w) of the smallest of key[0..w), the leftmost of equal keys. Host (gs_bigsi_minimizers, keys in a
// vector) and device (k_bigsi_minimizers, keys in LDS) share it; the occurrences are window 0's and every later window's that differs from the one before.
GS_HD uint32_t minimizer_pick(const uint64_t *key, uint32_t w)
{
    uint64_t bk = key[0];
    uint32_t bp = 0;
    for (uint32_t i = 1; i < w; i++) {
        const uint64_t x = key[i];
        if (x < bk) { bk = x; bp = i; }
    }
    return bp;
}
// P(X >= x0), X ~ Binomial(n, p), p = (t_c / B)^h: each line one IEEE f64 operation per operator, LN / EXP of SPEC 2
GS_HD double bigsi_tail(uint64_t t_c, uint64_t B, uint32_t h, uint32_t n, uint32_t x0)
{
    const double q = (double)t_c / (double)B;
    double p = q;
    for (uint32_t i = 1; i < h; i++) p = p * q;
    if (x0 > n) x0 = n;                   // (hits never exceed the k-mers used)
    if (x0 == 0) return 1.0;
    if (p == 0.0) return 0.0;
    if (p >= 1.0) return 1.0;
    const double l1 = spec_ln(1.0 - p), lq = spec_ln(p) - l1;
    double lp = (double)n * l1;
    for (uint32_t x = 0; x < x0; x++) lp = lp + (spec_ln((double)(n - x) / (double)(x + 1)) + lq);
    double tail = 0.0;
    for (uint32_t x = x0;; x++) {
        const double term = spec_exp(lp);
        tail = tail + term;
        if (x >= n || (x > x0 && term < tail * GS_BIGSI_TAIL_CUT)) break;
        lp = lp + (spec_ln((double)(n - x) / (double)(x + 1)) + lq);
    }
    return tail < 1.0 ? tail : 1.0;
}
// SPEC 11.2: the verdict table, the first row that holds (the codes: GS_BIGSI_TOO_SHORT .. GS_BIGSI_TIED of gsearch_amd.h). A tail equal to the threshold is
// not significant, and neither is a NaN.
GS_HD uint8_t bigsi_verdict(uint32_t n, uint32_t best_hits, uint32_t n_tied, double tail, double fp)
{
    if (n == 0) return 0;
    if (best_hits == 0) return 1;
    if (!(tail < fp)) return 2;
    return n_tied == 1 ? 3 : 4;
}

// ---- SPEC 12: superani (binaux/src/bin/superani.rs) - seed-chaining ANI of genome pairs. [CHOICE] throughout (the `skani` crate is not vendored).
#define GS_ANI_KMIN 8u
#define GS_ANI_KMAX 16u                  // a canonical value is 32 bits
#define GS_ANI_MAX_OCC 4u                // a value carried by more seeds of either genome gives no anchors
#define GS_ANI_W 20                      // score of an anchor
#define GS_ANI_B 64u                     // predecessors looked at: one wave64
#define GS_ANI_G 2500u                   // largest step of a chain on either genome, bases
#define GS_ANI_MIN_ANCHORS 3u            // a chain with fewer anchors is dropped
#define GS_ANI_MAX_PAIR_ANCHORS (1ULL << 26)
#define GS_ANI_MIN_AF 0.10               // min_aligned_frac of superani.rs
#define GS_ANI_NONE 0xFFFFFFFFu          // pred of an anchor that starts a chain
GS_HD uint64_t ani_threshold(uint32_t c) { return ~0ULL / c; }
GS_HD bool ani_is_seed(uint32_t v, uint64_t thr) { return splitmix_mix((uint64_t)v) <= thr; }
// reverse complement of a k-mer held in the low 2k bits (first base highest)
GS_HD uint32_t ani_revcomp(uint32_t x, uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t br = __builtin_bitreverse32(x);
#else
    uint32_t br = 0;
    for (int i = 0; i < 32; i++) br |= ((x >> i) & 1u) << (31 - i);
#endif
    br = ((br >> 1) & 0x55555555u) | ((br & 0x55555555u) << 1);
    return (~br) >> (32 - 2 * k);
}

// ---- SPEC 13: hmmsearch. Its units, constants and length model (hmm_lgq .. hmm_tbm) live in gs_hmm_parse.hpp, which the host-only reader of profile
// files shares; what is left here needs the device.
// a byte of a record -> residue index 0..19, or -1 (either case is read, as the sketchers do)
GS_HD int hmm_residue(uint8_t c)
{
    const uint32_t u = (c & 0xDFu) - 'A';
    if (u > 25u || !((GS_HMM_AA_MASK >> u) & 1u)) return -1;
    const uint32_t below = GS_HMM_AA_MASK & ((1u << u) - 1u);
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(below);
#else
    return __builtin_popcount(below);
#endif
}

// ---- SPEC 14: orfs - stop-to-stop six-frame translation of 2-bit packed records. [CHOICE] throughout (the reference calls FragGeneScanRs; this is the
// model-free stage of esl-translate / getorf / orfM). A codon of bases b0 b1 b2 (A C G T = 0 1 2 3) has index 16 b0 + 4 b1 + b2.
#define GS_ORF_TABLE_11 "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"      // [PUB] NCBI translation table 11 (= 1 without its start rule)
#define GS_ORF_TABLE_4 "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSSWCWCLFLF"       // [PUB] table 4: TGA (index 56) = W
#define GS_ORF_STOPS_11 ((1ULL << 48) | (1ULL << 50) | (1ULL << 56))                             // TAA TAG TGA
#define GS_ORF_STOPS_4 ((1ULL << 48) | (1ULL << 50))
#define GS_ORF_MIN_AA 30u                // default min_aa: the shortest profile of the reference's two sets has 57 nodes
// the codon of the reverse strand that occupies the bases of forward codon x: complement every base, reverse their order
GS_HD uint32_t orf_rev_codon(uint32_t x) { x ^= 63u; return ((x & 3u) << 4) | (x & 12u) | (x >> 4); }
// the codon positions of class c (p = c, c + 3, ... <= L - 3) of a record of L bases
GS_HD uint64_t orf_class_codons(uint64_t L, uint32_t c) { return L >= 3 + (uint64_t)c ? (L - 3 - c) / 3 + 1 : 0; }

// ---- SPEC 15: genes - a self-trained gene caller. [CHOICE] throughout (the self-trained kind of [PUB] Prodigal / GeneMarkS; the reference calls
// FragGeneScanRs, whose trained model files it does not hold). All integer arithmetic; what the host functions and the kernels share is below.
#define GS_GENE_TRAIN_MIN_AA 250u        // round 1 trains on the whole ORFs of this many codons and more
#define GS_GENE_MIN_TRAIN_CODONS 15000u  // a genome with fewer training dicodons is untrained (the method was tried at 19 252, nothing lower)
#define GS_GENE_PRIOR 4096u              // A: pseudo-count mass of the prior, spread in proportion to the background
#define GS_GENE_MIN_SCORE 5120           // 5 bits
#define GS_GENE_MAX_OVERLAP 60u
#define GS_GENE_ROUNDS 2u
#define GS_GENE_BONUS_GTG (-2048)
#define GS_GENE_BONUS_TTG (-3072)
#define GS_GENE_S_LIMIT 32768            // |S[h]| <= 32 bits x 1024 whatever the counts (SPEC 15); a table entry outside is not a table's
#define GS_GENE_MAX_NB ((1ull << 31) + 4096)     // Nb of a genome of 2^30 hexamer positions; beyond it, or with Nc + A > 2^32, a product may leave 64 bits
#define GS_GENE_MAX_NC_A (1ull << 32)
#define GS_GENE_MAX_INTERVAL (1u << 24)  // codons of one training interval (a workgroup counts 256 intervals in 32-bit LDS words)
#define GS_GENE_ATG 14u
#define GS_GENE_GTG 46u
#define GS_GENE_TTG 62u
// floor(65536 log2 x) for x >= 1, never above it and less than 2^-16 + 2^-28 below log2 x: normalise to a mantissa m in [2^31, 2^32) (bits below are
// cut), then sixteen times square m (a 64-bit product), cut to 32 bits again, and take the next fraction bit = whether the square reached 2
GS_HD uint32_t gene_log2_q16(uint64_t x)
{
    if (x == 0) return 0;
    const uint32_t e = 63u - (uint32_t)__builtin_clzll(x);
    uint64_t m = e >= 31 ? x >> (e - 31) : x << (31 - e);
    uint32_t r = e;
    for (int i = 0; i < 16; i++) {
        m = (m * m) >> 31;
        r <<= 1;
        if (m >> 32) { m >>= 1; r |= 1u; }
    }
    return r;
}
// S[h] = the difference of the two logarithms, rounded half up to 10 fraction bits
GS_HD int32_t gene_table_entry(uint64_t cod, uint64_t b, uint64_t Nc, uint64_t Nb)
{
    const int64_t d = (int64_t)gene_log2_q16(cod * Nb + (uint64_t)GS_GENE_PRIOR * b) - (int64_t)gene_log2_q16((Nc + GS_GENE_PRIOR) * b);
    return (int32_t)((d + 32 + ((int64_t)1 << 40)) / 64 - ((int64_t)1 << 34));          // floor((d + 32) / 64), by a division of a positive number
}
// the hexamer of the reverse strand that occupies the bases of forward hexamer h
GS_HD uint32_t gene_rev_hexamer(uint32_t h)
{
    h ^= 0xFFFu;
    return ((h & 3u) << 10) | ((h & 0xCu) << 6) | ((h & 0x30u) << 2) | ((h & 0xC0u) >> 2) | ((h & 0x300u) >> 6) | (h >> 10);
}
// start type of a codon: 0 ATG, 1 GTG, 2 TTG, -1 no start
GS_HD int gene_start_type(uint32_t codon) { return codon == GS_GENE_ATG ? 0 : codon == GS_GENE_GTG ? 1 : codon == GS_GENE_TTG ? 2 : -1; }
GS_HD int64_t gene_start_bonus(int type) { return type == 1 ? GS_GENE_BONUS_GTG : type == 2 ? GS_GENE_BONUS_TTG : 0; }

}  // namespace gs
