// gs_hiword.hpp — the drop test of the filtered slot-min emitter (MinEmitF, gs_sketch.hip) on the HIGH words of s0 and s3 alone. Plain integer C++
// (no HIP builtins): the emitter executes it on the device, tests/test_sketch_hiword_cpu.py compiles it with the host compiler alone.
//
// The key of a k-mer is cut from o1 = rotl64(s0 + s3, 23) + s0, and every key form the filter compares - o1 >> 41, o1 >> 32, o1 itself - is decided,
// up to a bounded slack, by hi32(o1). With S = s0 + s3 mod 2^64:
//   hi32(rotl64(S, 23)) = bits 9..40 of S = ((s0_hi + s3_hi + c1) << 23) + (S_lo >> 9)      mod 2^32, c1 = carry out of s0_lo + s3_lo
//   hi32(o1)            = hi32(rotl64(S, 23)) + s0_hi + c2                                   mod 2^32, c2 = carry out of lo32(rotl64(S, 23)) + s0_lo
// so hi32(o1) = (B + d) mod 2^32 with B = ((s0_hi + s3_hi) << 23) + s0_hi mod 2^32 and d = c1 2^23 + (S_lo >> 9) + c2, 0 <= d <= 2^24
// (2^23 + (2^23 - 1) + 1). The filter may pass any SUPERSET of the k-mers whose key is below the bound (a survivor's exact key is recomputed from
// its hash in the flush and decides there; the cap check relies on "dropped => key >= bound" alone), so it asks a question that only B answers:
//   hi32(o1) = x < T   =>   (B + 2^24) mod 2^32 = x + (2^24 - d) <= x + 2^24 < T + 2^24     (no wrap: x < T and T + 2^24 <= 2^32)
// i.e. "(B + 2^24) mod 2^32 < T + 2^24" is never false for a key below the bound, whatever the low words hold; where B + 2^24 wraps although
// hi32(o1) does not (or the other way round), the implication above is all that is used. It passes 2^24 / 2^32 = 0.39 % of all k-mers beyond the
// exact test. T < 2^30 + 1 for every caller (MinEmitF::direct_above), so T + 2^24 does not overflow.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_HIW_HD __host__ __device__ __forceinline__
#else
#define GS_HIW_HD inline
#endif

namespace gs {

constexpr uint32_t HIW_SLACK = 1u << 24;       // the bound on d above

// the limit T + 2^24 for the three key forms
GS_HIW_HD uint32_t hiword_limit_r23(uint32_t thr) { return (thr << 9) + HIW_SLACK; }                       // key = o1 >> 41 < thr   <=> hi32(o1) < thr << 9   (thr < 2^21)
GS_HIW_HD uint32_t hiword_limit_u32(uint32_t thr) { return thr + HIW_SLACK; }                              // key = o1 >> 32 < thr                             (thr < 2^30)
GS_HIW_HD uint32_t hiword_limit_u64(uint64_t thr) { return (uint32_t)(thr >> 32) + 1u + HIW_SLACK; }       // key = o1 < thr          => hi32(o1) < hi32(thr) + 1 (thr < 2^62)

// false only where the key of (s0, s3) is certainly not below the bound that `limit` was made from: (s0_hi + s3_hi + 2) << 23 is
// ((s0_hi + s3_hi) << 23) + 2^24 mod 2^32. This is the test as derived above, on the true high words; the emitter runs the form below.
GS_HIW_HD bool hiword_may_be_below(uint32_t s0_hi, uint32_t s3_hi, uint32_t limit)
{
    return (uint32_t)(((s0_hi + s3_hi + 2u) << 23) + s0_hi) < limit;
}

// The form the emitter runs: s3's word WITHOUT the last xor-shift of its mix, s3_x = b_hi where s3_hi = b_hi ^ (b_hi >> 31) - and of s3_x only the
// low 9 bits, all that << 23 keeps (splitmix_mix_hi9, gs_spec.hpp). The xor moves bit 0 alone: s3_hi = s3_x + e, e in {-1, 0, 1}, so
// B = B_x + e 2^23 with B_x = ((s0_hi + s3_x) << 23) + s0_hi, and hi32(o1) = (B_x - 2^23) + d_x with d_x = d + (e + 1) 2^23, 0 <= d_x <= 2^25:
// the same argument with the slack 2^25 from the base B_x - 2^23,
//   hi32(o1) < T   =>   (B_x + 3 2^23) mod 2^32 < T + 2^25,
// which passes 2^25 / 2^32 = 0.78 % of all k-mers beyond the exact test and spares a shift, a xor and one multiply per k-mer (measured faster in
// the kernel). On the device: v_add3_u32, v_lshl_add_u32 and a compare with a scalar. T + 2^25 < 2^31 for every caller.
constexpr uint32_t HIW_SLACK_X = 1u << 25;
GS_HIW_HD uint32_t hiword_limit_x_r23(uint32_t thr) { return (thr << 9) + HIW_SLACK_X; }
GS_HIW_HD uint32_t hiword_limit_x_u32(uint32_t thr) { return thr + HIW_SLACK_X; }
GS_HIW_HD uint32_t hiword_limit_x_u64(uint64_t thr) { return (uint32_t)(thr >> 32) + 1u + HIW_SLACK_X; }
GS_HIW_HD bool hiword_may_be_below_x(uint32_t s0_hi, uint32_t s3_x, uint32_t limit_x)
{
    return (uint32_t)(((s0_hi + s3_x + 3u) << 23) + s0_hi) < limit_x;
}

}  // namespace gs
