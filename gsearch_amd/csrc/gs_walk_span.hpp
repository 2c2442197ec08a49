// gs_walk_span.hpp — which record of a genome owns a flat unit, and which packed words the walk of that unit loads. Plain integer C++ (no HIP
// builtins): the walkers of gs_walk.hpp execute it on the device, tests/test_walk_span_cpu.py compiles it with the host compiler alone.
//
// A genome is the records [r0, r1); record r holds the symbols [rec_start[r], rec_start[r] + rec_len[r]) of the packed stream and owns the flat units
// [rec_upre[r], rec_upre[r + 1]) of its genome (the last record up to the genome's `units`), one unit per 32-symbol word the record touches. A record
// shorter than k owns no unit: its prefix value is repeated by the record behind it, and "the last r with rec_upre[r] <= f" skips it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_WALK_HD __host__ __device__ __forceinline__
#else
#define GS_WALK_HD inline
#endif

namespace gs {

// record `lo`, its symbols [rb, re) and its span of flat units [upre, uend). All zero: the empty span, which holds no unit.
struct WalkSpan { uint64_t lo, rb, re, upre, uend; };

// record owning flat unit f: last r in [r0, r1) with rec_upre[r] <= f (r1 > r0, f < the genome's units). `uend` is left at upre: the span is not known
GS_WALK_HD WalkSpan locate_record(const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *rec_upre, uint64_t r0, uint64_t r1, uint64_t f)
{
    uint64_t lo = r0, hi = r1;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (rec_upre[mid] <= f) lo = mid; else hi = mid; }
    const uint64_t rb = rec_start[lo], up = rec_upre[lo];
    return WalkSpan{lo, rb, rb + rec_len[lo], up, up};
}
// the same with the record's span of units: every f' in [upre, uend) has the same owner, so a lane that stays inside needs no second look-up (WalkCursor)
GS_WALK_HD WalkSpan locate_span(const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *rec_upre, uint64_t r0, uint64_t r1, uint64_t units, uint64_t f)
{
    WalkSpan s = locate_record(rec_start, rec_len, rec_upre, r0, r1, f);
    s.uend = s.lo + 1 < r1 ? rec_upre[s.lo + 1] : units;
    return s;
}
// unit f of the span -> word u of the packed stream; its first symbol is a0 = 32 u, the first symbol a k-mer of the record can end in is rb + k - 1
GS_WALK_HD uint64_t span_word(const WalkSpan &s, uint64_t f) { return (s.rb >> 5) + (f - s.upre); }
GS_WALK_HD uint64_t span_first_valid(const WalkSpan &s, uint32_t k) { return s.rb + k - 1; }
// the k - 1 symbols in front of word u belong to the record too (and a k-mer is longer than one symbol): the walk needs the word before
GS_WALK_HD bool word_has_halo(const WalkSpan &s, uint64_t u, uint32_t k) { return (u << 5) > s.rb && k > 1; }
// the second word a DNA unit loads: u - 1 where there is a halo, u itself (a word the lane loads anyway, whose value nobody reads) where not - the load
// is unconditional and only its ADDRESS is selected. u - 1 >= rb >> 5 >= 0 under a halo.
GS_WALK_HD uint64_t halo_word(const WalkSpan &s, uint64_t u, uint32_t k) { return u - (word_has_halo(s, u, k) ? 1u : 0u); }

// What a lane of the two-stage walk (walk_genome, gs_walk.hpp) carries from trip to trip: the record of its unit, the unit's word u, and how many
// units of the record's span lie at and behind the unit (`left` = uend - f, held in 32 bits: a larger count saturates, which only makes the lane
// look the record up again earlier than it had to). upre and uend of `s` are dead after cursor_locate: u and left stand for them.
struct WalkCursor { WalkSpan s; uint64_t u; uint32_t left; };

// the look-up: binary search and table loads
GS_WALK_HD void cursor_locate(WalkCursor &c, const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *rec_upre, uint64_t r0, uint64_t r1, uint64_t units,
                              uint64_t f)
{
    c.s = locate_span(rec_start, rec_len, rec_upre, r0, r1, units, f);
    c.u = span_word(c.s, f);
    const uint64_t left = c.s.uend - f;
    c.left = left > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)left;
}
// the trip stride as cursor_inside takes it: a stride that does not fit 32 bits leaves every span
GS_WALK_HD uint32_t cursor_stride(uint64_t stride) { return stride >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stride; }
// the span cache: is the unit `stride` units on still one of this record's? One 32-bit compare, no table load.
GS_WALK_HD bool cursor_inside(const WalkCursor &c, uint32_t stride32) { return stride32 < c.left; }
// ... then it is word u + stride of the same record, and it has a halo whenever k > 1 (a word behind another word of its record does not hold the
// record's first symbol), so its halo word needs no look at the record either
GS_WALK_HD uint64_t inside_word(const WalkCursor &c, uint32_t stride32) { return c.u + stride32; }
GS_WALK_HD uint64_t inside_halo_word(uint64_t u, uint32_t k) { return u - (k > 1 ? 1u : 0u); }
GS_WALK_HD void cursor_advance(WalkCursor &c, uint32_t stride32) { c.u += stride32; c.left -= stride32; }

}  // namespace gs
