// gs_walk.hpp — the k-mer walkers every sketcher streams a genome through (gs_sketch.hip, gs_prob.hip): flat unit -> valid canonical k-mer values -> an emitter.
// Device code only; included after gs_internal.hpp. Layout and the funnel-shift windows: DESIGN.md 3.1.
#pragma once
#include "gs_internal.hpp"
#include "gs_walk_span.hpp"

namespace gs {

static constexpr int SK_THREADS = 512;

// the same table as c_aa_code (gs_sketch.hip), packed 8 codes x 5 bits per word and kept in registers: a per-lane (divergent) index into
// __constant__ memory is a vector memory load per residue, this is four VALU operations
__device__ __forceinline__ uint32_t aa_code_reg(uint32_t ch)
{
    const uint32_t idx = ch & 31, sh = (idx & 7) * 5;
    const uint64_t lo = (idx & 8) ? 0x2d49400e6ull : 0x2906208000ull, hi = (idx & 8) ? 0x260ull : 0x944107b9acull;
    return (uint32_t)(((idx & 16) ? hi : lo) >> sh) & 31u;
}

// per-record unit counts -> exclusive prefix inside each genome, one wavefront per genome (defined in gs_sketch.hip)
__global__ void k_unit_prefix(const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *genome_rec_off,
                              uint64_t n_genomes, uint32_t k, uint64_t *rec_upre, uint64_t *gen_units);

// Hooks of walk_genome that only the filtered emitter overrides: a k-mer emitted by a FULL wavefront (all 64 lanes inside a record),
// two consecutive ones (positions pos and pos + 1: an emitter that compacts across the wave may push them together), the end of such a
// word, and the end of the walk.
template <class E> __device__ __forceinline__ void emit_full_wave(const E &e, uint64_t v, uint64_t rec, uint64_t pos) { e(v, rec, pos); }
template <class E> __device__ __forceinline__ void emit_full_wave2(const E &e, uint64_t v_a, uint64_t v_b, uint64_t rec, uint64_t pos)
{
    emit_full_wave(e, v_a, rec, pos);
    emit_full_wave(e, v_b, rec, pos + 1);
}
template <class E> __device__ __forceinline__ void emit_word_done(const E &) {}
template <class E> __device__ __forceinline__ void emit_finish(const E &) {}

// reverse complement of 32 packed bases: base i (bits 63-2i..62-2i) complemented at bits 2i+1..2i
__device__ __forceinline__ uint64_t rc64(uint64_t x)
{
    const uint64_t br = __builtin_bitreverse64(x);
    return ~(((br >> 1) & 0x5555555555555555ull) | ((br & 0x5555555555555555ull) << 1));
}
// The 32 windows of an interior word of a full wave by funnel shifts. With the previous word pw and the word w in front of
// it, X = pw:w is a 64-base stream and the forward k-mer ending at base j of w is (X >> 2(31 - j)) & mask; with Y = rc(w):rc(pw) the
// reverse-complement k-mer is (Y >> 2(33 + j - k)) & mask. Each is two v_alignbit_b32 (one per 32-bit half; one when k <= 16) and an AND,
// with the wave-uniform shift in an SGPR, against the eight operations of the rolling update (two 64-bit shifts, the base extraction, two
// ORs, two ANDs and the complement) - 33 instead of 42 issue cycles for window and canonical minimum at k > 16. The three 32-bit words a
// window can touch change only at uniform points (j = 16 for the forward window, 33 + j - k crossing 16 or 32 for the reverse one): the
// loop runs in up to four segments of fixed word roles, and the roles move down one word between segments, never per k-mer.
// WIDE: k > 16 (a window spans both halves; the low half needs no mask). !WIDE: k <= 16 (the high half is zero).
template <bool WIDE, int RCM, class Emit>
__device__ __forceinline__ void walk_word_funnel(uint64_t w, uint64_t pw, uint32_t k, uint64_t mask, uint64_t rc_or, uint64_t rec, uint64_t a0,
                                                 const Emit &emit)
{
    const uint32_t x0 = (uint32_t)w, x1 = (uint32_t)(w >> 32);
    const uint64_t yl = rc64(pw), yh = rc64(w);
    const uint32_t y0 = (uint32_t)yl, y1 = (uint32_t)(yl >> 32), y2 = (uint32_t)yh, y3 = (uint32_t)(yh >> 32);
    const uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32), olo = (uint32_t)rc_or, ohi = (uint32_t)(rc_or >> 32);
    // forward roles for j < 16: the window starts in word 1 of X (words 0..3 = low w, high w, low pw, high pw)
    uint32_t f0 = x1, f1 = (uint32_t)pw, f2 = (uint32_t)(pw >> 32);
    // reverse roles: the window at j starts in word (33 + j - k) >> 4 of Y (words 0..3 = low rc(pw) .. high rc(w), 4 and 5 zero)
    uint32_t t = 33 - k, qy = t >> 4;                      // 1 <= t <= 32: qy in 0..2
    uint32_t r0 = qy == 0 ? y0 : qy == 1 ? y1 : y2, r1 = qy == 0 ? y1 : qy == 1 ? y2 : y3, r2 = qy == 0 ? y2 : qy == 1 ? y3 : 0u;
    uint32_t j = 0;
    // the window that ends at base j under the word roles of its segment
    auto window = [&](uint32_t j, uint32_t t) -> uint64_t {
        const uint32_t sf = 62 - 2 * j, sr = 2 * t;        // alignbit takes the shift mod 32
        if (WIDE) {
            const uint32_t fl = __builtin_amdgcn_alignbit(f1, f0, sf), fh = __builtin_amdgcn_alignbit(f2, f1, sf) & mhi;
            if (RCM == 1) return ((uint64_t)fh << 32) | fl;
            uint32_t rl = __builtin_amdgcn_alignbit(r1, r0, sr), rh = __builtin_amdgcn_alignbit(r2, r1, sr) & mhi;
            if (RCM == 2) { rl |= olo; rh |= ohi; }
            const uint64_t fw = ((uint64_t)fh << 32) | fl, rc = ((uint64_t)rh << 32) | rl;
            return fw < rc ? fw : rc;
        }
        const uint32_t fl = __builtin_amdgcn_alignbit(f1, f0, sf) & mlo;
        if (RCM == 1) return fl;
        uint32_t rl = __builtin_amdgcn_alignbit(r1, r0, sr) & mlo;
        if (RCM == 2) rl |= olo;
        return min(fl, rl);
    };
    for (;;) {
        const uint32_t je = min(j < 16 ? 16u : 32u, j + 16 - (t & 15));
        // two windows at a time, never across a segment's end (the word roles move there); a segment of odd length - even k: t & 15 is odd - ends on one
        for (; j + 1 < je; j += 2, t += 2) {
            const uint64_t va = window(j, t), vb = window(j + 1, t + 1);
            emit_full_wave2(emit, va, vb, rec, a0 + j);
        }
        if (j < je) { emit_full_wave(emit, window(j, t), rec, a0 + j); j++; t++; }
        if (j == 32) break;
        if (j == 16) { f2 = f1; f1 = f0; f0 = x0; }
        if ((t & 15) == 0) { r0 = r1; r1 = r2; r2 = qy == 0 ? y3 : 0u; qy++; }
    }
}

// The streaming part shared by every sketcher. walk_unit: flat unit f of a genome (32 symbols: one packed word of DNA, 32 bytes of AA) ->
// emit(v) for each valid canonical k-mer value that starts... ends in it; walk_genome: the units of genome g assigned to this workgroup.
// walk_unit is three steps: LOCATE the record of the unit (gs_walk_span.hpp), FETCH its words, WALK their windows. walk_genome runs them a trip apart.
// RCM: how the strand rule reaches the loop - 2 = at run time through rc_or (every sketcher but the hot one), 0 / 1 = compiled in (canonical / forward only):
// k_sketch_min is VALU-issue bound and the run-time form turns its two v_or_b32 per k-mer into three-operand v_or3_b32, which issue 1.6x slower
// (profiles/r02_ubench_valu.txt: 1.75 against 1.08 ns) - 115.7 instead of 112.5 ms per 10 000 genomes (profiles/r05_bench_request_rc_runtime.log)

// fetch (DNA): word u of a located unit and the word its halo lies in, AS LOADED - no instruction here reads them, so nothing waits; the byte swap
// belongs to the walk. Both loads are unconditional, the second with its address selected (halo_word): no load behind a divergent branch.
__device__ __forceinline__ void fetch_words(const uint64_t *__restrict__ w64, const WalkSpan &s, uint64_t u, uint32_t k, uint64_t &w_raw, uint64_t &pw_raw)
{
    w_raw = w64[u];
    pw_raw = w64[halo_word(s, u, k)];
}
// walk (DNA): the 32 windows that end in word u of record s. w: the word, pw: the word in front of it where the unit has a halo (any value where not:
// no path reads it then), both byte-swapped. Three paths, chosen by wave-uniform ballots: funnel shifts (every lane holds an interior word), rolling
// (a full wave, some words at a record's edge), rolling with a bounds test per window (a partial wave).
template <int RCM, class Emit>
__device__ __forceinline__ void walk_word(uint64_t w, uint64_t pw, const WalkSpan &s, uint64_t u, uint32_t k, uint64_t mask, uint32_t rcshift, uint64_t rc_or,
                                          const Emit &emit)
{
    const uint64_t lo = s.lo, re = s.re, a0 = u << 5, first_valid = span_first_valid(s, k);
    // When every lane of the wave holds an interior word - all 32 windows inside its record, the case for all but the first and last word of a
    // record - the per-window bounds test (two 64-bit compares, an exec save / restore and a branch per k-mer) is dropped for the whole word.
    const bool interior = a0 >= first_valid && a0 + 32 <= re;
    const uint64_t bint = __ballot(interior);
    if (bint == ~(uint64_t)0) {                      // all 64 lanes: emitters that compact across the wave may do so
        // (k > 1 here: an interior word has a halo and pw is the previous word; k = 1: no window reaches the bases of pw)
        if (k > 16) walk_word_funnel<true, RCM>(w, pw, k, mask, rc_or, lo, a0, emit);
        else walk_word_funnel<false, RCM>(w, pw, k, mask, rc_or, lo, a0, emit);
        emit_word_done(emit);
        return;
    }
    uint64_t fwd = 0, rc = 0;
    if (word_has_halo(s, u, k)) {
        // the state after the k-1 bases in front of this word, in closed form (round 5: the loop over them - k-1 = 20 trips of ~9 instructions per 32 k-mers -
        // was 5.6 of the ~82 VALU instructions per k-mer): the forward window is the low 2(k-1) bits of the previous word; the reverse-complement
        // register holds base i of those k-1 at bit 2i, complemented - the 2-bit groups in reverse order, one group up. Only the two rolling
        // paths read it; the funnel path takes its own rc64(pw).
        const uint64_t lowm = ((uint64_t)1 << (2 * (k - 1))) - 1;            // k - 1 <= 31
        fwd = pw & lowm;
        rc = ((rc64(pw) >> (2 * (33 - k))) << 2) | rc_or;                    // the top 2(k - 1) bits of rc64(pw): the last k - 1 bases
    }
    // (rc never exceeds 2k bits and fwd is masked every step: the minimum needs no further mask.)
    if (bint == __ballot(true)) {
#pragma unroll 2
        for (uint32_t j = 0; j < 32; j++) {
            uint64_t c = w >> 62; w <<= 2;
            fwd = ((fwd << 2) | c) & mask;
            rc = (rc >> 2) | ((3 - c) << rcshift) | rc_or;
            emit(fwd < rc ? fwd : rc, lo, a0 + j);
        }
    } else {
#pragma unroll 2
        for (uint32_t j = 0; j < 32; j++) {
            uint64_t c = w >> 62; w <<= 2;
            fwd = ((fwd << 2) | c) & mask;
            rc = (rc >> 2) | ((3 - c) << rcshift) | rc_or;
            uint64_t a = a0 + j;
            if (a >= first_valid && a < re) emit(fwd < rc ? fwd : rc, lo, a);
        }
    }
}
// walk (AA): the 32 residues of unit u, read where they are used
template <class Emit>
__device__ __forceinline__ void walk_unit_aa(const uint8_t *__restrict__ seq, const WalkSpan &s, uint64_t u, uint32_t k, uint64_t mask, const Emit &emit)
{
    const uint64_t *w64 = (const uint64_t *)seq;
    const uint64_t lo = s.lo, re = s.re, a0 = u << 5, first_valid = span_first_valid(s, k);
    uint64_t val = 0;
    if (word_has_halo(s, u, k)) {
        // previous k-1 residues: bytes a0-(k-1) .. a0-1 (k-1 <= 11 -> inside the previous two 8-byte words)
        for (uint32_t j = 0; j + 1 < k; j++) {
            uint64_t a = a0 - (k - 1) + j;
            uint8_t ch = seq[a];
            val = ((val << 5) | aa_code_reg(ch)) & mask;
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        uint64_t x = w64[u * 4 + q];
#pragma unroll 2
        for (uint32_t j = 0; j < 8; j++) {
            uint32_t ch = (uint32_t)(x & 0xFF); x >>= 8;
            val = ((val << 5) | aa_code_reg(ch)) & mask;
            uint64_t a = a0 + q * 8 + j;
            if (a >= first_valid && a < re) emit(val, lo, a);
        }
    }
}
template <bool AA, class Emit, int RCM = 2>
__device__ __forceinline__ void walk_unit(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                          const uint64_t *__restrict__ rec_upre, uint64_t r0, uint64_t r1, uint64_t f, uint32_t k, uint64_t mask, uint32_t rcshift,
                                          uint64_t rc_or_rt, const Emit &emit)
{
    const uint64_t rc_or = RCM == 0 ? (uint64_t)0 : RCM == 1 ? ~(uint64_t)0 : rc_or_rt;
    const WalkSpan s = locate_record(rec_start, rec_len, rec_upre, r0, r1, f);
    const uint64_t u = span_word(s, f);
    if (!AA) {
        uint64_t w, pw;
        fetch_words((const uint64_t *)seq, s, u, k, w, pw);
        walk_word<RCM>(__builtin_bswap64(w), __builtin_bswap64(pw), s, u, k, mask, rcshift, rc_or, emit);
    } else walk_unit_aa(seq, s, u, k, mask, emit);
}
// Kernels that walk sequences take `kq` = k | KQ_FWD: bit 8 set means GS_DATA_DNA_FWD - the k-mer is the forward window itself, no
// reverse-complement minimum (the k <= 14 closure of /root/reference/src/bin/bindash.rs:346-354: `kmer.get_compressed_value() & mask`).
// The walkers keep ONE code path: rc_or = ~0 pins the reverse-complement register at all ones, so `min(fwd, rc)` is fwd (the OR folds into the
// v_or3 that already merges the shifted halves - no instruction more on the canonical path).
enum { KQ_FWD = 0x100 };
__device__ __forceinline__ uint32_t kq_k(uint32_t kq) { return kq & 0xFFu; }
__device__ __forceinline__ uint64_t kq_rc_or(uint32_t kq) { return (kq & KQ_FWD) ? ~(uint64_t)0 : (uint64_t)0; }
static inline uint32_t kq_of(const gs_sketch_params *p) { return p->k | (p->data_t == GS_DATA_DNA_FWD ? (uint32_t)KQ_FWD : 0u); }
__device__ __forceinline__ uint64_t kmer_mask(bool aa, uint32_t k) { return aa ? (((uint64_t)1 << (5 * k)) - 1) : (k == 32 ? ~(uint64_t)0 : (((uint64_t)1 << (2 * k)) - 1)); }
// AHEAD (DNA only): the two-stage loop below. A kernel that would lose a wave of occupancy to its registers stays on the one-stage loop.
template <bool AA, class Emit, int RCM = 2, bool AHEAD = !AA>
__device__ __forceinline__ void walk_genome(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start,
                                            const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ rec_upre,
                                            uint64_t r0, uint64_t r1, uint64_t units, uint32_t kq, uint32_t part,
                                            uint32_t parts, const Emit &emit)
{
    const uint32_t k = kq_k(kq);
    const uint64_t mask = kmer_mask(AA, k), rc_or_rt = kq_rc_or(kq);
    const uint32_t rcshift = 2 * (k - 1);
    const uint64_t stride = (uint64_t)parts * blockDim.x;
    uint64_t f = (uint64_t)part * blockDim.x + threadIdx.x;
    if constexpr (AA || !AHEAD) {
        for (; f < units; f += stride)
            walk_unit<AA, Emit, RCM>(seq, rec_start, rec_len, rec_upre, r0, r1, f, k, mask, rcshift, rc_or_rt, emit);
    } else {
        // Two stages, one trip apart: before a lane walks the word of trip i it issues the two loads of trip i + 1, which nothing reads until
        // that walk is over. That needs no look-up: the lane keeps a cursor (gs_walk_span.hpp) that knows how many
        // units of its record's span are left, and while the next unit lies inside (every trip of a one-record genome) the next word is
        // u + stride of the same record - one 32-bit compare, no search, no table load. A lane whose next unit lies in another record looks it
        // up after the walk and loads its words there, as the prologue does: its pipeline starts afresh once per record, and the cursor of the
        // word being walked is never held beside a second one (the bounds of a second record would be six more registers through the walk).
        // Invariants (tests/test_walk_span_cpu.py holds them on the host, tests/test_gpu_sketch_ahead.py on the device):
        //  * no new addresses: a lane loads ahead exactly words the one-stage loop loads for it in its next trip - word u of f + stride and
        //    word u - 1 (u again at k = 1); nothing for f + stride >= units, nothing below the record's first word, nothing behind its last;
        //  * every wave-uniform decision (the ballots of walk_word, emit_word_done, emit_finish) sees the same lanes with the same values as in
        //    the one-stage loop: only WHEN a word is loaded has changed, so the emitted k-mers and their order are the same;
        //  * each call starts the pipeline afresh (the second walk of the filtered sketcher included): no state outlives it.
        const uint64_t rc_or = RCM == 0 ? (uint64_t)0 : RCM == 1 ? ~(uint64_t)0 : rc_or_rt;
        const uint64_t *__restrict__ w64 = (const uint64_t *)seq;
        const uint32_t stride32 = cursor_stride(stride);
        WalkCursor c{{0, 0, 0, 0, 0}, 0, 0};
        uint64_t w_raw = 0, pw_raw = 0;
        if (f < units) {
            cursor_locate(c, rec_start, rec_len, rec_upre, r0, r1, units, f);
            fetch_words(w64, c.s, c.u, k, w_raw, pw_raw);
        }
        while (f < units) {
            const uint64_t cw = w_raw, cpw = pw_raw;
            f += stride;
            const bool inside = cursor_inside(c, stride32);            // (a span ends at or before `units`: inside implies f < units)
            if (inside) {
                uint64_t un = inside_word(c, stride32);
                asm("" : "+v"(un));         // opaque: the loads' address stays a value of its own, apart from the sum cursor_advance forms behind the walk
                w_raw = w64[un];
                pw_raw = w64[inside_halo_word(un, k)];
            }
            walk_word<RCM>(__builtin_bswap64(cw), __builtin_bswap64(cpw), c.s, c.u, k, mask, rcshift, rc_or, emit);
            if (inside) cursor_advance(c, stride32);
            else if (f < units) {
                cursor_locate(c, rec_start, rec_len, rec_upre, r0, r1, units, f);
                fetch_words(w64, c.s, c.u, k, w_raw, pw_raw);
            }
        }
    }
    emit_finish(emit);
}

}  // namespace gs
