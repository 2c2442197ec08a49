// gs_ani.hip — superani (binaux/src/bin/superani.rs of the reference): FracMinHash seeds of genomes in position order, the anchors of a pair,
// colinear chaining and the per-side counts the ANI and the aligned fractions are closed forms of (SPEC.md 12).
//
//   k_ani_seeds      one lane per 32-base unit through walk_unit (gs_walk.hpp), forward windows; the emitter forms the canonical value and the
//                    strand flag, applies mix() <= threshold. Count pass, scan of the per-unit counts (k_scan_u32), write pass: a unit's seeds
//                    leave in window order and units are in position order, so the list needs no sort.
//   k_ani_keys       seed index << 32 | value per seed; radix_sort_u64 on the low 32 bits per genome (stable: equal values keep index order).
//   k_ani_anchors    one wavefront per slice of AN_SLICE seeds of the reference side of a pair, lanes walk them in position order, binary search
//                    in both value-ordered lists (multiplicities from the runs), count pass / write pass: anchors leave in SPEC order.
//   k_ani_seg_*      the anchors of a block are cut where no predecessor can reach across (another pair, another r contig, an r gap > G).
//   k_ani_chain      the banded dynamic program: one wavefront per segment, lane (i - segment start) mod 64 holds anchor i as a ring, the new
//                    anchor is wave-uniform (v_readlane), the maximum goes through DPP inside the rows and four v_readlane across them, the
//                    winner among equal candidates is picked from a ballot with scalar instructions. No LDS, no atomics.
//   k_ani_ends / k_ani_mark / k_ani_sides   best end per root (integer atomicMax), the kept chains marked back by one wavefront per segment with the
//                    wanted anchors as a ring of 64 bits in scalar registers, the per-side scan.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"
#include "gs_walk.hpp"

namespace gs {
__global__ void k_scan_u32(uint32_t *__restrict__ a, uint64_t cnt, uint32_t *__restrict__ total_out);     // gs_radix.hip

constexpr uint32_t AS_T = 256;                       // seed kernel: lanes (units) per workgroup
constexpr uint64_t AS_BLOCK_UNITS = 1ull << 24;      // units of a block of genomes (a longer genome is a block of its own)
constexpr uint32_t AN_SLICE = 2048;                  // r seeds per wavefront of the anchor kernel
constexpr uint64_t AN_SUPER = 1ull << 22;            // slices counted per readback
constexpr uint32_t AN_TILE = 4096;                   // anchors per wavefront of the segment kernels
constexpr uint64_t AN_BLOCK_ANCHORS = 1ull << 24;    // default anchors of a block of pairs
constexpr uint64_t AN_BLOCK_SEEDS = 1ull << 26;      // seeds (both sides) of a block of pairs

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
    return x;
}
// last g in [0, n) with off[g] <= t (off ascending, off[0] <= t)
__device__ __forceinline__ uint64_t last_le(const uint64_t *__restrict__ off, uint64_t n, uint64_t t)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}

// ---- seeds ---------------------------------------------------------------------------------------------------------------------------------
struct AniSeedEmit {
    uint32_t k; uint64_t thr; const uint64_t *rec_start; uint64_t rec0;
    uint32_t *n;                 // seeds of this lane's unit so far
    uint4 *dst; uint32_t room;   // write pass: where the unit's seeds go and how many still fit the row
    __device__ __forceinline__ void operator()(uint64_t vf, uint64_t rec, uint64_t a) const
    {
        const uint32_t f = (uint32_t)vf, r = ani_revcomp(f, k), v = f < r ? f : r;
        if (!ani_is_seed(v, thr)) return;
        const uint32_t i = *n;
        if (dst && i < room) dst[i] = make_uint4(v, (uint32_t)(rec - rec0), (uint32_t)(a + 1 - k - rec_start[rec]), v == f ? 1u : 0u);
        *n = i + 1;
    }
};
// unit t of a block of genomes (gunit[g] = first unit of genome g of the block). WRITE = false: cnt[t] = its seeds. WRITE = true: scan[t] = seeds in
// front of it; cap = 0: one list, dst[scan[t] ...]; cap > 0: rows of cap seeds, genome g at row g, cut at cap.
template <bool WRITE>
__global__ __launch_bounds__(AS_T) void k_ani_seeds(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                    const uint64_t *__restrict__ rec_upre, const uint64_t *__restrict__ genome_rec_off,
                                                    const uint64_t *__restrict__ gunit, uint64_t ng, uint64_t units, uint32_t k, uint64_t thr,
                                                    uint32_t *__restrict__ cnt, const uint32_t *__restrict__ gbase, uint4 *__restrict__ dst, uint32_t cap)
{
    const uint64_t t = (uint64_t)blockIdx.x * AS_T + threadIdx.x;
    if (t >= units) return;
    const uint64_t g = last_le(gunit, ng, t);
    const uint64_t r0 = genome_rec_off[g], r1 = genome_rec_off[g + 1];
    uint32_t n = 0;
    AniSeedEmit emit{k, thr, rec_start, r0, &n, nullptr, 0};
    if (WRITE) {
        const uint32_t before = cnt[t];
        if (cap == 0) { emit.dst = dst + before; emit.room = 0xFFFFFFFFu; }
        else {
            const uint32_t local = before - gbase[g];
            emit.dst = dst + g * (uint64_t)cap + local;
            emit.room = local < cap ? cap - local : 0u;
        }
    }
    walk_unit<false, AniSeedEmit, 1>(seq, rec_start, rec_len, rec_upre, r0, r1, t - gunit[g], k, kmer_mask(false, k), 2 * (k - 1), ~(uint64_t)0, emit);
    if (!WRITE) cnt[t] = n;
}
__global__ void k_ani_gather_u32(const uint32_t *__restrict__ a, const uint64_t *__restrict__ at, uint64_t n, uint32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[at[i]];
}

// ---- value order -----------------------------------------------------------------------------------------------------------------------------
__global__ void k_ani_keys(const uint4 *__restrict__ seeds, const uint64_t *__restrict__ off, uint64_t ng, uint64_t n, uint64_t *__restrict__ keys)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = last_le(off, ng, i);
    keys[i] = ((i - off[g]) << 32) | seeds[i].x;
}
// first index of keys[0..n) whose value (low 32 bits) is >= v
__device__ __forceinline__ uint32_t ani_lower(const uint64_t *__restrict__ keys, uint32_t n, uint32_t v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)keys[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}
// length of the run of v that starts at L, counted up to MAX_OCC + 1
__device__ __forceinline__ uint32_t ani_occ(const uint64_t *__restrict__ keys, uint32_t n, uint32_t L, uint32_t v)
{
    uint32_t o = 0;
    while (o <= GS_ANI_MAX_OCC && L + o < n && (uint32_t)keys[L + o] == v) o++;
    return o;
}

// ---- anchors -----------------------------------------------------------------------------------------------------------------------------------
struct AniSlice { uint32_t pair, r0; };        // r seeds [r0, r0 + AN_SLICE) of pair `pair` of the call
struct AniAnchorsOut { uint32_t *rctg, *rpos, *qctg, *qpos, *strand, *ridx, *qidx; };
template <bool WRITE>
__global__ __launch_bounds__(64) void k_ani_anchors(const uint4 *__restrict__ Q, const uint64_t *__restrict__ qoff, const uint64_t *__restrict__ qkeys,
                                                    const uint4 *__restrict__ R, const uint64_t *__restrict__ roff, const uint64_t *__restrict__ rkeys,
                                                    const uint32_t *__restrict__ pair_q, const uint32_t *__restrict__ pair_r,
                                                    const AniSlice *__restrict__ slices, uint32_t *__restrict__ slice_cnt,
                                                    const uint32_t *__restrict__ slice_base, AniAnchorsOut out)
{
    const AniSlice s = slices[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint64_t qb = qoff[pair_q[s.pair]], rb = roff[pair_r[s.pair]];
    const uint32_t nq = (uint32_t)(qoff[pair_q[s.pair] + 1] - qb), nr = (uint32_t)(roff[pair_r[s.pair] + 1] - rb);
    const uint32_t end = s.r0 + AN_SLICE < nr ? s.r0 + AN_SLICE : nr;
    const uint64_t *qk = qkeys + qb, *rk = rkeys + rb;
    uint32_t run = WRITE ? slice_base[blockIdx.x] : 0u;
    for (uint32_t i0 = s.r0; i0 < end; i0 += 64) {
        const uint32_t i = i0 + lane;
        uint32_t cnt = 0, L = 0;
        uint4 rs = make_uint4(0, 0, 0, 0);
        if (i < end) {
            rs = R[rb + i];
            const uint32_t Lr = ani_lower(rk, nr, rs.x);
            if (ani_occ(rk, nr, Lr, rs.x) <= GS_ANI_MAX_OCC) {
                L = ani_lower(qk, nq, rs.x);
                const uint32_t oq = ani_occ(qk, nq, L, rs.x);
                if (oq <= GS_ANI_MAX_OCC) cnt = oq;
            }
        }
        const uint32_t incl = wave_incl_scan(cnt, lane);
        if (WRITE) {
            for (uint32_t j = 0; j < cnt; j++) {
                const uint32_t a = run + incl - cnt + j, qi = (uint32_t)(qk[L + j] >> 32);
                const uint4 qs = Q[qb + qi];
                out.rctg[a] = rs.y; out.rpos[a] = rs.z; out.qctg[a] = qs.y; out.qpos[a] = qs.z; out.strand[a] = (rs.w ^ qs.w) & 1u;
                out.ridx[a] = i; out.qidx[a] = qi;
            }
        }
        run += __shfl(incl, 63);
    }
    if (!WRITE && lane == 0) slice_cnt[blockIdx.x] = run;
}

// ---- segments ----------------------------------------------------------------------------------------------------------------------------------
__global__ void k_ani_fill_pair(const uint64_t *__restrict__ aoff, uint64_t np, uint64_t n, uint32_t *__restrict__ apair)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) apair[i] = (uint32_t)last_le(aoff, np, i);
}
// anchor i starts a segment: no anchor at or behind it has a predecessor in front of it (SPEC 12; needs the r side in order inside a pair,
// which *bad reports when it does not hold)
__device__ __forceinline__ bool ani_seg_head(const uint32_t *__restrict__ apair, const uint32_t *__restrict__ rctg, const uint32_t *__restrict__ rpos, uint64_t i,
                                             uint32_t *__restrict__ bad)
{
    if (i == 0) return true;
    if (apair[i] != apair[i - 1]) return true;
    const uint32_t c1 = rctg[i], c0 = rctg[i - 1], p1 = rpos[i], p0 = rpos[i - 1];
    if (c1 < c0 || (c1 == c0 && p1 < p0)) { if (bad) atomicOr(bad, 1u); return true; }
    return c1 != c0 || p1 - p0 > GS_ANI_G;
}
__global__ __launch_bounds__(64) void k_ani_seg_count(const uint32_t *__restrict__ apair, const uint32_t *__restrict__ rctg, const uint32_t *__restrict__ rpos,
                                                      uint64_t n, uint32_t *__restrict__ tile_heads, uint32_t *__restrict__ bad)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * AN_TILE, t1 = t0 + AN_TILE < n ? t0 + AN_TILE : n;
    uint32_t c = 0;
    for (uint64_t i = t0 + lane; i < t1; i += 64) c += ani_seg_head(apair, rctg, rpos, i, bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (lane == 0) tile_heads[blockIdx.x] = c;
}
__global__ __launch_bounds__(64) void k_ani_seg_write(const uint32_t *__restrict__ apair, const uint32_t *__restrict__ rctg, const uint32_t *__restrict__ rpos,
                                                      uint64_t n, const uint32_t *__restrict__ tile_base, uint32_t *__restrict__ seg_start)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * AN_TILE, t1 = t0 + AN_TILE < n ? t0 + AN_TILE : n;
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    uint32_t run = tile_base[blockIdx.x];
    for (uint64_t s = t0; s < t1; s += 64) {
        const uint64_t i = s + lane;
        const bool head = i < t1 && ani_seg_head(apair, rctg, rpos, i, nullptr);
        const uint64_t bal = __ballot(head);
        if (head) seg_start[run + (uint32_t)__popcll(bal & lt)] = (uint32_t)i;
        run += (uint32_t)__popcll(bal);
    }
    if (t1 == n && lane == 0) seg_start[run] = (uint32_t)n;          // the last tile closes the list
}

// ---- chaining ----------------------------------------------------------------------------------------------------------------------------------
// maximum over the wavefront, the same value in every lane: four DPP steps inside each row of 16 (lane pairs, quads, half rows, rows), then the
// four rows through v_readlane and scalar maxima
__device__ __forceinline__ int wave_max_i32(int x)
{
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));       // quad_perm [1,0,3,2]
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false));       // quad_perm [2,3,0,1]
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false));      // row_half_mirror
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x140, 0xF, 0xF, false));      // row_mirror
    const int a = __builtin_amdgcn_readlane(x, 0), b = __builtin_amdgcn_readlane(x, 16), c = __builtin_amdgcn_readlane(x, 32),
              d = __builtin_amdgcn_readlane(x, 48);
    return max(max(a, b), max(c, d));
}
// One wavefront per segment [seg_start[s], seg_start[s + 1]). Lane l holds, as the ring, the last anchor at segment position = l mod 64: at step t
// of a chunk the lanes below t hold this chunk's anchors and the lanes from t on the previous chunk's - together exactly the B = 64 anchors in
// front of anchor i, the one 64 back in lane t itself, which takes the new anchor once its f is known. ring_s = 2 marks a lane that holds nothing.
__global__ __launch_bounds__(64) void k_ani_chain(const uint32_t *__restrict__ rctg, const uint32_t *__restrict__ rpos, const uint32_t *__restrict__ qctg,
                                                  const uint32_t *__restrict__ qpos, const uint32_t *__restrict__ strand, const uint32_t *__restrict__ apair,
                                                  const uint64_t *__restrict__ aoff, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ nseg_p,
                                                  int32_t *__restrict__ f_out, uint32_t *__restrict__ pred_out, uint32_t *__restrict__ root_out)
{
    const int lane = (int)threadIdx.x;
    const uint32_t nseg = *nseg_p;
    for (uint32_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const uint32_t s0 = seg_start[s], s1 = seg_start[s + 1];
        const uint32_t pbase = (uint32_t)aoff[apair[s0]];                   // pred and root are counted from the pair's first anchor
        uint32_t g_rp = 0, g_qp = 0, g_rc = 0, g_qc = 0, g_s = 2, g_root = 0;
        int g_f = 0;
        for (uint32_t c0 = s0; c0 < s1; c0 += 64) {
            const uint32_t i = c0 + (uint32_t)lane;
            const bool in = i < s1;
            const uint32_t n_rp = in ? rpos[i] : 0u, n_qp = in ? qpos[i] : 0u, n_rc = in ? rctg[i] : 0u, n_qc = in ? qctg[i] : 0u, n_s = in ? (strand[i] & 1u) : 0u;
            int o_f = 0;
            uint32_t o_pred = GS_ANI_NONE, o_root = 0;
            const int nt = (int)(s1 - c0 < 64u ? s1 - c0 : 64u);
            for (int t = 0; t < nt; t++) {
                const uint32_t x_rp = (uint32_t)__builtin_amdgcn_readlane((int)n_rp, t), x_qp = (uint32_t)__builtin_amdgcn_readlane((int)n_qp, t),
                               x_rc = (uint32_t)__builtin_amdgcn_readlane((int)n_rc, t), x_qc = (uint32_t)__builtin_amdgcn_readlane((int)n_qc, t),
                               x_s = (uint32_t)__builtin_amdgcn_readlane((int)n_s, t);
                const uint32_t hi = x_s ? g_qp : x_qp, lo = x_s ? x_qp : g_qp;          // dq = hi - lo along the strand
                const bool ok = g_s == x_s && g_rc == x_rc && g_qc == x_qc && x_rp > g_rp && x_rp - g_rp <= GS_ANI_G && hi > lo && hi - lo <= GS_ANI_G;
                const int d = (int)(x_rp - g_rp) - (int)(hi - lo);
                const int cand = ok ? g_f + GS_ANI_W - (d < 0 ? -d : d) : 0;            // 0 <= W: never taken
                const int m = wave_max_i32(cand);
                int fi = GS_ANI_W;
                uint32_t pred = GS_ANI_NONE, root = c0 + (uint32_t)t - pbase;
                if (m > GS_ANI_W) {
                    // the lanes that hold the best candidate, turned so that bit r is the anchor r + 1 of 64 back: the highest bit is the largest j
                    const uint64_t bal = __ballot(cand == m);
                    const uint64_t rot = t ? (bal >> t) | (bal << (64 - t)) : bal;
                    const int pl = (63 - __builtin_clzll(rot) + t) & 63;
                    fi = m;
                    pred = (pl < t ? c0 + (uint32_t)pl : c0 - 64u + (uint32_t)pl) - pbase;
                    root = (uint32_t)__builtin_amdgcn_readlane((int)g_root, pl);
                }
                if (lane == t) {
                    g_rp = x_rp; g_qp = x_qp; g_rc = x_rc; g_qc = x_qc; g_s = x_s; g_f = fi; g_root = root;
                    o_f = fi; o_pred = pred; o_root = root;
                }
            }
            if (in) { f_out[i] = o_f; pred_out[i] = o_pred; root_out[i] = o_root; }
        }
    }
}

// ---- chain ends, marks, sides ------------------------------------------------------------------------------------------------------------------
// best[root] = max over the anchors of the root of (f, smallest index first)
__global__ void k_ani_ends(const uint32_t *__restrict__ apair, const uint64_t *__restrict__ aoff, const int32_t *__restrict__ f, const uint32_t *__restrict__ root,
                           uint64_t n, unsigned long long *__restrict__ best)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t base = aoff[apair[i]];
    atomicMax(&best[base + root[i]], ((unsigned long long)(uint32_t)f[i] << 32) | (0xFFFFFFFFu - (uint32_t)(i - base)));
}
// The kept chains marked back without chasing pointers: one wavefront per segment (a chain never leaves its segment), from the last chunk of 64 to
// the first. `wanted` is a ring of 64 bits in scalar registers, bit b = the not yet visited anchor at segment position b mod 64 lies on a kept chain.
// An anchor that is its root's best end and has two anchors behind it (MIN_ANCHORS = 3) starts a chain; visiting an anchor clears its bit and sets
// its predecessor's, which is at most 64 back: the bit of the anchor just cleared, or a lower one. Only anchors on chains are visited. The marks of
// both sides (soff[2 p + side]: where the n + 1 entries of that side of pair p start) are plain stores of 1, the [lo, hi] of a chain and the count of
// chains integer atomicAdd.
__global__ __launch_bounds__(64) void k_ani_mark(const uint32_t *__restrict__ apair, const uint64_t *__restrict__ aoff, const uint64_t *__restrict__ soff,
                                                 const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ nseg_p, const uint32_t *__restrict__ pred,
                                                 const uint32_t *__restrict__ root, const uint32_t *__restrict__ qidx, const uint32_t *__restrict__ ridx,
                                                 const unsigned long long *__restrict__ best, uint8_t *__restrict__ matched, int32_t *__restrict__ diff,
                                                 uint32_t *__restrict__ nchain)
{
    static_assert(GS_ANI_MIN_ANCHORS == 3, "k_ani_mark looks two anchors behind an end");
    const uint32_t lane = threadIdx.x, nseg = *nseg_p;
    for (uint32_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const uint32_t s0 = seg_start[s], s1 = seg_start[s + 1], p = apair[s0];
        const uint64_t base = aoff[p], sq = soff[2 * (uint64_t)p], sr = soff[2 * (uint64_t)p + 1];
        uint64_t wanted = 0;
        for (uint32_t c = (s1 - s0 + 63) / 64; c-- > 0;) {
            const uint32_t c0 = s0 + c * 64, i = c0 + lane, nt = s1 - c0 < 64u ? s1 - c0 : 64u;
            const bool in = i < s1;
            const uint32_t pr = in ? pred[i] : GS_ANI_NONE;
            const uint32_t rt = in ? root[i] : 0u;
            bool end = false;
            if (in && pr != GS_ANI_NONE && (uint32_t)best[base + rt] == 0xFFFFFFFFu - (uint32_t)(i - base)) end = pred[base + pr] != GS_ANI_NONE;
            const uint64_t E = __ballot(end);
            const uint32_t pslot = (uint32_t)(base + pr - s0) & 63u;
            uint64_t on = 0, lim = ~0ull >> (64 - nt);
            for (;;) {
                const uint64_t todo = (wanted | E) & lim;
                if (!todo) break;
                const int t = 63 - __builtin_clzll(todo);
                const uint64_t bit = 1ull << t;
                lim = bit - 1; wanted &= ~bit; on |= bit;
                if ((uint32_t)__builtin_amdgcn_readlane((int)pr, t) != GS_ANI_NONE) wanted |= 1ull << (uint32_t)__builtin_amdgcn_readlane((int)pslot, t);
            }
            if ((on >> lane) & 1) { matched[sq + qidx[i]] = 1; matched[sr + ridx[i]] = 1; }
            if (end) {
                atomicAdd(&nchain[p], 1u);
                const uint32_t q0 = qidx[base + rt], q1 = qidx[i], r0 = ridx[base + rt], r1 = ridx[i];
                atomicAdd(&diff[sq + min(q0, q1)], 1); atomicAdd(&diff[sq + max(q0, q1) + 1], -1);
                atomicAdd(&diff[sr + min(r0, r1)], 1); atomicAdd(&diff[sr + max(r0, r1) + 1], -1);
            }
        }
    }
}
// one wavefront per (pair, side): covered = running sum of the difference array > 0; M, C and A of SPEC 12 into the pair's row of eight
__global__ __launch_bounds__(64) void k_ani_sides(const uint4 *__restrict__ Q, const uint64_t *__restrict__ qoff, const uint4 *__restrict__ R,
                                                  const uint64_t *__restrict__ roff, const uint32_t *__restrict__ pair_q, const uint32_t *__restrict__ pair_r,
                                                  uint64_t p0, const uint64_t *__restrict__ aoff, const uint64_t *__restrict__ soff,
                                                  const uint8_t *__restrict__ matched, const int32_t *__restrict__ diff, const uint32_t *__restrict__ nchain,
                                                  uint32_t k, uint64_t *__restrict__ out)
{
    const uint64_t p = blockIdx.x >> 1;
    const uint32_t side = blockIdx.x & 1, lane = threadIdx.x;
    const uint64_t g = side ? pair_r[p0 + p] : pair_q[p0 + p];
    const uint64_t gb = side ? roff[g] : qoff[g], n = (side ? roff[g + 1] : qoff[g + 1]) - gb, so = soff[2 * p + side];
    const uint4 *S = (side ? R : Q) + gb;
    int32_t run = 0;
    uint32_t M = 0, Cn = 0, c_cov = 0, c_ctg = 0, c_pos = 0;       // c_*: the seed in front of the chunk
    uint64_t A = 0;
    for (uint64_t i0 = 0; i0 < n + 1; i0 += 64) {                  // one position past the end closes a run that reaches it
        const uint64_t i = i0 + lane;
        const bool in = i < n;
        const int32_t d = in ? diff[so + i] : 0;
        const int32_t incl = (int32_t)wave_incl_scan((uint32_t)d, lane);
        const uint32_t cov = in && run + incl > 0;
        const uint4 sd = in ? S[i] : make_uint4(0, 0, 0, 0);
        uint32_t p_cov = __shfl_up(cov, 1), p_ctg = __shfl_up(sd.y, 1), p_pos = __shfl_up(sd.z, 1);
        if (lane == 0) { p_cov = c_cov; p_ctg = c_ctg; p_pos = c_pos; }
        const bool brk = !p_cov || !cov || p_ctg != sd.y;
        if (p_cov && brk) A += (uint64_t)p_pos + k;
        if (cov && brk) A -= (uint64_t)sd.z;
        Cn += cov;
        M += cov && matched[so + i];
        run += __shfl(incl, 63);
        c_cov = __shfl(cov, 63); c_ctg = __shfl(sd.y, 63); c_pos = __shfl(sd.z, 63);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { M += __shfl_down(M, o); Cn += __shfl_down(Cn, o); A += __shfl_down(A, o); }
    if (lane == 0) {
        uint64_t *row = out + 8 * (p0 + p);
        if (side == 0) { row[0] = aoff[p + 1] - aoff[p]; row[1] = nchain[p]; }
        row[2 + 3 * side] = M; row[3 + 3 * side] = Cn; row[4 + 3 * side] = A;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------
static int ani_check(uint32_t k, uint32_t cc)
{
    GS_REQUIRE(k >= GS_ANI_KMIN && k <= GS_ANI_KMAX, GS_ERR_INVALID, "superani: k = %u, only %u <= k <= %u", k, GS_ANI_KMIN, GS_ANI_KMAX);
    GS_REQUIRE(cc >= 1, GS_ERR_INVALID, "superani: c must be >= 1");
    return GS_OK;
}

// The seeds of n_genomes genomes whose packed bases are on the device (all four arrays both on the host and on the device). counts[g] = seeds of genome g.
// flat != nullptr: every genome's seeds end to end into *flat (host, 4 u32 each). Otherwise rows of `cap` seeds at rows_dev, cut at cap.
static int ani_seed_core(gs_ctx *c, uint32_t k, uint32_t cc, const uint8_t *seq_dev, uint64_t seq_bytes, const uint64_t *rs, const uint64_t *rl, uint64_t n_rec,
                         const uint64_t *go, uint64_t ng, const uint64_t *rs_dev, const uint64_t *rl_dev, const uint64_t *go_dev, std::vector<uint64_t> &counts,
                         std::vector<uint32_t> *flat, uint32_t cap, uint32_t *rows_dev)
{
    counts.assign(ng, 0);
    if (flat) flat->clear();
    if (ng == 0) return GS_OK;
    GS_REQUIRE(go[0] == 0 && go[ng] == n_rec, GS_ERR_INVALID, "genome_rec_off must run from 0 to n_rec");
    std::vector<uint64_t> upre(n_rec + 1, 0), gunits(ng, 0);
    for (uint64_t g = 0; g < ng; g++) {
        GS_REQUIRE(go[g] <= go[g + 1], GS_ERR_INVALID, "genome_rec_off must not decrease");
        GS_REQUIRE(go[g + 1] - go[g] < (1ull << 32), GS_ERR_UNSUPPORTED, "superani: genome %llu has 2^32 records or more", (unsigned long long)g);
        uint64_t u = 0, bases = 0;
        for (uint64_t r = go[g]; r < go[g + 1]; r++) {
            GS_REQUIRE(rs[r] + rl[r] >= rs[r] && (rs[r] + rl[r] + 3) / 4 <= seq_bytes, GS_ERR_INVALID, "record %llu outside the sequence", (unsigned long long)r);
            upre[r] = u;
            if (rl[r] >= k) u += ((rs[r] + rl[r] - 1) >> 5) - (rs[r] >> 5) + 1;
            bases += rl[r];
        }
        GS_REQUIRE(bases < (1ull << 32), GS_ERR_UNSUPPORTED, "superani: genome %llu has 2^32 bases or more", (unsigned long long)g);
        gunits[g] = u;
    }
    PoolBuf dupre(c, SL_ANI_UPRE), dgunit(c, SL_ANI_GUNIT), dcnt(c, SL_ANI_UCNT), dgbase(c, SL_ANI_GBASE), dseeds(c, SL_ANI_SEEDS);
    int rc;
    if ((rc = dupre.alloc(8 * (n_rec + 1)))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dupre.p, upre.data(), 8 * (n_rec + 1), hipMemcpyHostToDevice, c->stream));
    const uint64_t thr = ani_threshold(cc);
    for (uint64_t g0 = 0; g0 < ng;) {
        uint64_t g1 = g0, units = 0;
        while (g1 < ng && (g1 == g0 || units + gunits[g1] <= AS_BLOCK_UNITS)) units += gunits[g1++];
        const uint64_t nb = g1 - g0;
        if (units) {
            GS_REQUIRE(units < (1ull << 31) * AS_T / 64, GS_ERR_UNSUPPORTED, "superani: genome too long");
            std::vector<uint64_t> gunit(nb + 1, 0);
            for (uint64_t g = 0; g < nb; g++) gunit[g + 1] = gunit[g] + gunits[g0 + g];
            if ((rc = dgunit.alloc(8 * (nb + 1))) || (rc = dcnt.alloc(4 * (units + 1))) || (rc = dgbase.alloc(4 * (nb + 1)))) return rc;
            GS_HIP_CHECK(hipMemcpyAsync(dgunit.p, gunit.data(), 8 * (nb + 1), hipMemcpyHostToDevice, c->stream));
            GS_HIP_CHECK(hipMemsetAsync(dcnt.as<uint32_t>() + units, 0, 4, c->stream));
            const dim3 grid((uint32_t)((units + AS_T - 1) / AS_T)), blk(AS_T);
            {
                ProfScope ps(c, FAM_SKETCH);
                hipLaunchKernelGGL(k_ani_seeds<false>, grid, blk, 0, c->stream, seq_dev, rs_dev, rl_dev, dupre.as<uint64_t>(), go_dev + g0, dgunit.as<uint64_t>(), nb,
                                   units, k, thr, dcnt.as<uint32_t>(), (const uint32_t *)nullptr, (uint4 *)nullptr, 0u);
            }
            hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, dcnt.as<uint32_t>(), units + 1, (uint32_t *)nullptr);
            hipLaunchKernelGGL(k_ani_gather_u32, dim3((uint32_t)((nb + 1 + 255) / 256)), dim3(256), 0, c->stream, dcnt.as<uint32_t>(), dgunit.as<uint64_t>(), nb + 1,
                               dgbase.as<uint32_t>());
            GS_HIP_CHECK(hipGetLastError());
            std::vector<uint32_t> gbase(nb + 1);
            GS_HIP_CHECK(hipMemcpyAsync(gbase.data(), dgbase.p, 4 * (nb + 1), hipMemcpyDeviceToHost, c->stream));
            GS_HIP_CHECK(stream_wait(c));
            const uint64_t total = gbase[nb];
            for (uint64_t g = 0; g < nb; g++) counts[g0 + g] = gbase[g + 1] - gbase[g];
            uint4 *dst = nullptr;
            if (flat) {
                if ((rc = dseeds.alloc(16 * total))) return rc;
                dst = dseeds.as<uint4>();
            } else dst = (uint4 *)rows_dev + g0 * (uint64_t)cap;
            if (total && (flat || cap)) {
                ProfScope ps(c, FAM_SKETCH);
                hipLaunchKernelGGL(k_ani_seeds<true>, grid, blk, 0, c->stream, seq_dev, rs_dev, rl_dev, dupre.as<uint64_t>(), go_dev + g0, dgunit.as<uint64_t>(), nb,
                                   units, k, thr, dcnt.as<uint32_t>(), dgbase.as<uint32_t>(), dst, flat ? 0u : cap);
                GS_HIP_CHECK(hipGetLastError());
            }
            if (flat && total) {
                const size_t at = flat->size();
                flat->resize(at + 4 * total);
                GS_HIP_CHECK(hipMemcpyAsync(flat->data() + at, dseeds.p, 16 * total, hipMemcpyDeviceToHost, c->stream));
            }
            GS_HIP_CHECK(stream_wait(c));
        }
        g0 = g1;
    }
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

// value order of every genome of a seed CSR on the device: keys[off[g] ...] = (index << 32 | value) ascending by value, then index
static int ani_sort_keys(gs_ctx *c, const uint4 *seeds, const uint64_t *off_dev, const uint64_t *off, uint64_t ng, PoolBuf &keys, PoolBuf &alt, PoolBuf &radix)
{
    const uint64_t n = off[ng];
    int rc;
    uint64_t longest = 0;
    for (uint64_t g = 0; g < ng; g++) longest = std::max(longest, off[g + 1] - off[g]);
    if ((rc = keys.alloc(8 * n)) || (rc = alt.alloc(8 * longest)) || (rc = radix.alloc(radix_scratch_bytes(longest)))) return rc;
    if (n == 0) return GS_OK;
    hipLaunchKernelGGL(k_ani_keys, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, seeds, off_dev, ng, n, keys.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    for (uint64_t g = 0; g < ng; g++) {
        const uint64_t m = off[g + 1] - off[g];
        uint64_t *seg = keys.as<uint64_t>() + off[g], *sorted = nullptr;
        if ((rc = radix_sort_u64(c, seg, alt.as<uint64_t>(), m, 32, radix.p, &sorted))) return rc;
        if (sorted != seg) GS_HIP_CHECK(hipMemcpyAsync(seg, sorted, 8 * m, hipMemcpyDeviceToDevice, c->stream));
    }
    return GS_OK;
}

struct AniAnchors { const uint32_t *rctg, *rpos, *qctg, *qpos, *strand; };
// the dynamic program over n anchors of np pairs (aoff_dev: np + 1 offsets): apair, the segments, f / pred / root. *bad_out (optional): the r side
// of some pair was not in order.
static int ani_chain_block(gs_ctx *c, const AniAnchors &a, const uint64_t *aoff_dev, uint64_t np, uint64_t n, PoolBuf &dpair, PoolBuf &dtiles, PoolBuf &dseg,
                           PoolBuf &dsegn, int32_t *f, uint32_t *pred, uint32_t *root, uint32_t *bad_out)
{
    int rc;
    const uint32_t nt = (uint32_t)((n + AN_TILE - 1) / AN_TILE);
    if ((rc = dpair.alloc(4 * n)) || (rc = dtiles.alloc(4 * ((size_t)nt + 4))) || (rc = dseg.alloc(4 * (n + 1))) || (rc = dsegn.alloc(16))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(dsegn.p, 0, 16, c->stream));
    uint32_t *segn = dsegn.as<uint32_t>();
    hipLaunchKernelGGL(k_ani_fill_pair, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, aoff_dev, np, n, dpair.as<uint32_t>());
    hipLaunchKernelGGL(k_ani_seg_count, dim3(nt), dim3(64), 0, c->stream, dpair.as<uint32_t>(), a.rctg, a.rpos, n, dtiles.as<uint32_t>(), segn + 1);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, dtiles.as<uint32_t>(), (uint64_t)nt, segn);
    hipLaunchKernelGGL(k_ani_seg_write, dim3(nt), dim3(64), 0, c->stream, dpair.as<uint32_t>(), a.rctg, a.rpos, n, dtiles.as<uint32_t>(), dseg.as<uint32_t>());
    GS_HIP_CHECK(hipGetLastError());
    if (bad_out) {      // before the program runs: it relies on the order
        GS_HIP_CHECK(hipMemcpyAsync(bad_out, segn + 1, 4, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(stream_wait(c));
        if (*bad_out) return GS_OK;
    }
    {
        ProfScope ps(c, FAM_HAMMING);
        const uint32_t grid = (uint32_t)std::min<uint64_t>(n, (uint64_t)c->n_cu * 32);
        hipLaunchKernelGGL(k_ani_chain, dim3(grid), dim3(64), 0, c->stream, a.rctg, a.rpos, a.qctg, a.qpos, a.strand, dpair.as<uint32_t>(), aoff_dev, dseg.as<uint32_t>(),
                           segn, f, pred, root);
        GS_HIP_CHECK(hipGetLastError());
    }
    return GS_OK;
}

// all arrays on the device and, the offsets and the pair lists, on the host too
static int ani_pairs_impl(gs_ctx *c, uint32_t k, const uint4 *Q, const uint64_t *qoff_dev, const uint64_t *qoff, uint64_t nq, const uint4 *R, const uint64_t *roff_dev,
                          const uint64_t *roff, uint64_t nr, const uint32_t *pq_dev, const uint32_t *pr_dev, const uint32_t *pq, const uint32_t *pr, uint64_t n_pairs,
                          uint64_t max_block_anchors, uint64_t *out_dev)
{
    if (n_pairs == 0) return GS_OK;
    GS_REQUIRE(n_pairs < (1ull << 32), GS_ERR_UNSUPPORTED, "superani: 2^32 pairs or more in one call");
    GS_REQUIRE(qoff[0] == 0 && roff[0] == 0, GS_ERR_INVALID, "superani: offsets must start at 0");
    for (uint64_t g = 0; g < nq; g++) GS_REQUIRE(qoff[g + 1] >= qoff[g] && qoff[g + 1] - qoff[g] < 0xFFFFFFFFull, GS_ERR_INVALID, "superani: bad query offsets at %llu", (unsigned long long)g);
    for (uint64_t g = 0; g < nr; g++) GS_REQUIRE(roff[g + 1] >= roff[g] && roff[g + 1] - roff[g] < 0xFFFFFFFFull, GS_ERR_INVALID, "superani: bad reference offsets at %llu", (unsigned long long)g);
    for (uint64_t p = 0; p < n_pairs; p++) GS_REQUIRE(pq[p] < nq && pr[p] < nr, GS_ERR_INVALID, "superani: pair %llu names a genome that is not there", (unsigned long long)p);
    const uint64_t cap_anchors = max_block_anchors ? max_block_anchors : AN_BLOCK_ANCHORS;
    PoolBuf dqk(c, SL_ANI_QKEYS), drk(c, SL_ANI_RKEYS), dalt(c, SL_ANI_KEYS_ALT), dradix(c, SL_ANI_RADIX);
    PoolBuf dsl(c, SL_ANI_SLICES), dslc(c, SL_ANI_SLICE_CNT), dslb(c, SL_ANI_SLICE_BASE), daoff(c, SL_ANI_AOFF), dsoff(c, SL_ANI_SOFF);
    PoolBuf d_rctg(c, SL_ANI_A_RCTG), d_rpos(c, SL_ANI_A_RPOS), d_qctg(c, SL_ANI_A_QCTG), d_qpos(c, SL_ANI_A_QPOS), d_str(c, SL_ANI_A_STRAND), d_ridx(c, SL_ANI_A_RIDX),
        d_qidx(c, SL_ANI_A_QIDX), d_pair(c, SL_ANI_A_PAIR), d_tiles(c, SL_ANI_SEG_TILES), d_seg(c, SL_ANI_SEG_START), d_segn(c, SL_ANI_SEG_N);
    PoolBuf d_f(c, SL_ANI_F), d_pred(c, SL_ANI_PRED), d_root(c, SL_ANI_ROOT), d_best(c, SL_ANI_BEST), d_nch(c, SL_ANI_NCHAIN), d_mat(c, SL_ANI_MATCHED), d_diff(c, SL_ANI_DIFF);
    int rc;
    if ((rc = ani_sort_keys(c, Q, qoff_dev, qoff, nq, dqk, dalt, dradix)) || (rc = ani_sort_keys(c, R, roff_dev, roff, nr, drk, dalt, dradix))) return rc;
    const AniAnchorsOut none{};
    for (uint64_t sp0 = 0; sp0 < n_pairs;) {
        // a stretch of pairs whose slices are counted with one readback
        std::vector<AniSlice> slices;
        std::vector<uint64_t> first_slice;                  // of each pair of the stretch, and one past the last
        uint64_t sp1 = sp0;
        while (sp1 < n_pairs && (sp1 == sp0 || slices.size() < AN_SUPER)) {
            first_slice.push_back(slices.size());
            const uint64_t n_r = roff[pr[sp1] + 1] - roff[pr[sp1]];
            for (uint64_t r0 = 0; r0 < n_r; r0 += AN_SLICE) slices.push_back({(uint32_t)sp1, (uint32_t)r0});
            sp1++;
        }
        first_slice.push_back(slices.size());
        const uint64_t ns = slices.size();
        GS_REQUIRE(ns < (1ull << 31), GS_ERR_UNSUPPORTED, "superani: pair too large");
        std::vector<uint32_t> scnt(ns, 0);
        if (ns) {
            if ((rc = dsl.alloc(sizeof(AniSlice) * ns)) || (rc = dslc.alloc(4 * ns)) || (rc = dslb.alloc(4 * ns))) return rc;
            GS_HIP_CHECK(hipMemcpyAsync(dsl.p, slices.data(), sizeof(AniSlice) * ns, hipMemcpyHostToDevice, c->stream));
            {
                ProfScope ps(c, FAM_HAMMING);
                hipLaunchKernelGGL(k_ani_anchors<false>, dim3((uint32_t)ns), dim3(64), 0, c->stream, Q, qoff_dev, dqk.as<uint64_t>(), R, roff_dev, drk.as<uint64_t>(), pq_dev,
                                   pr_dev, dsl.as<AniSlice>(), dslc.as<uint32_t>(), (const uint32_t *)nullptr, none);
                GS_HIP_CHECK(hipGetLastError());
            }
            GS_HIP_CHECK(hipMemcpyAsync(scnt.data(), dslc.p, 4 * ns, hipMemcpyDeviceToHost, c->stream));
            GS_HIP_CHECK(stream_wait(c));
        }
        std::vector<uint64_t> pa(sp1 - sp0, 0);             // anchors of each pair
        for (uint64_t p = sp0; p < sp1; p++) {
            for (uint64_t s = first_slice[p - sp0]; s < first_slice[p - sp0 + 1]; s++) pa[p - sp0] += scnt[s];
            GS_REQUIRE(pa[p - sp0] <= GS_ANI_MAX_PAIR_ANCHORS, GS_ERR_UNSUPPORTED, "superani: pair %llu has %llu anchors, more than 2^26", (unsigned long long)p,
                       (unsigned long long)pa[p - sp0]);
        }
        // blocks of pairs sized to the anchors and the seeds they hold
        for (uint64_t p0 = sp0; p0 < sp1;) {
            uint64_t p1 = p0, na = 0, nseeds = 0;
            std::vector<uint64_t> aoff{0}, soff;
            while (p1 < sp1) {
                const uint64_t sq = qoff[pq[p1] + 1] - qoff[pq[p1]] + 1, sr = roff[pr[p1] + 1] - roff[pr[p1]] + 1;
                if (p1 > p0 && (na + pa[p1 - sp0] > cap_anchors || nseeds + sq + sr > AN_BLOCK_SEEDS)) break;
                soff.push_back(nseeds); soff.push_back(nseeds + sq);
                na += pa[p1 - sp0]; nseeds += sq + sr;
                aoff.push_back(na);
                p1++;
            }
            const uint64_t np = p1 - p0, s0 = first_slice[p0 - sp0], s1 = first_slice[p1 - sp0];
            GS_REQUIRE(na < (1ull << 32), GS_ERR_UNSUPPORTED, "superani: block too large");
            if ((rc = daoff.alloc(8 * (np + 1))) || (rc = dsoff.alloc(8 * 2 * np)) || (rc = d_nch.alloc(4 * np)) || (rc = d_mat.alloc(nseeds)) || (rc = d_diff.alloc(4 * nseeds)))
                return rc;
            GS_HIP_CHECK(hipMemcpyAsync(daoff.p, aoff.data(), 8 * (np + 1), hipMemcpyHostToDevice, c->stream));
            GS_HIP_CHECK(hipMemcpyAsync(dsoff.p, soff.data(), 8 * 2 * np, hipMemcpyHostToDevice, c->stream));
            GS_HIP_CHECK(hipMemsetAsync(d_nch.p, 0, 4 * np, c->stream));
            GS_HIP_CHECK(hipMemsetAsync(d_mat.p, 0, nseeds, c->stream));
            GS_HIP_CHECK(hipMemsetAsync(d_diff.p, 0, 4 * nseeds, c->stream));
            std::vector<uint32_t> sbase(std::max<uint64_t>(s1 - s0, 1), 0);
            if (na) {
                uint32_t run = 0;
                for (uint64_t s = s0; s < s1; s++) { sbase[s - s0] = run; run += scnt[s]; }
                if ((rc = d_rctg.alloc(4 * na)) || (rc = d_rpos.alloc(4 * na)) || (rc = d_qctg.alloc(4 * na)) || (rc = d_qpos.alloc(4 * na)) || (rc = d_str.alloc(4 * na)) ||
                    (rc = d_ridx.alloc(4 * na)) || (rc = d_qidx.alloc(4 * na)) || (rc = d_f.alloc(4 * na)) || (rc = d_pred.alloc(4 * na)) || (rc = d_root.alloc(4 * na)) ||
                    (rc = d_best.alloc(8 * na)))
                    return rc;
                GS_HIP_CHECK(hipMemcpyAsync(dslb.p, sbase.data(), 4 * (s1 - s0), hipMemcpyHostToDevice, c->stream));
                GS_HIP_CHECK(hipMemsetAsync(d_best.p, 0, 8 * na, c->stream));
                const AniAnchorsOut ao{d_rctg.as<uint32_t>(), d_rpos.as<uint32_t>(), d_qctg.as<uint32_t>(), d_qpos.as<uint32_t>(), d_str.as<uint32_t>(), d_ridx.as<uint32_t>(),
                                       d_qidx.as<uint32_t>()};
                {
                    ProfScope ps(c, FAM_HAMMING);
                    hipLaunchKernelGGL(k_ani_anchors<true>, dim3((uint32_t)(s1 - s0)), dim3(64), 0, c->stream, Q, qoff_dev, dqk.as<uint64_t>(), R, roff_dev, drk.as<uint64_t>(),
                                       pq_dev, pr_dev, dsl.as<AniSlice>() + s0, (uint32_t *)nullptr, dslb.as<uint32_t>(), ao);
                    GS_HIP_CHECK(hipGetLastError());
                }
                const AniAnchors an{ao.rctg, ao.rpos, ao.qctg, ao.qpos, ao.strand};
                if ((rc = ani_chain_block(c, an, daoff.as<uint64_t>(), np, na, d_pair, d_tiles, d_seg, d_segn, d_f.as<int32_t>(), d_pred.as<uint32_t>(), d_root.as<uint32_t>(),
                                          nullptr)))
                    return rc;
                const dim3 grid((uint32_t)((na + 255) / 256)), blk(256);
                hipLaunchKernelGGL(k_ani_ends, grid, blk, 0, c->stream, d_pair.as<uint32_t>(), daoff.as<uint64_t>(), d_f.as<int32_t>(), d_root.as<uint32_t>(), na,
                                   d_best.as<unsigned long long>());
                hipLaunchKernelGGL(k_ani_mark, dim3((uint32_t)std::min<uint64_t>(na, (uint64_t)c->n_cu * 32)), dim3(64), 0, c->stream, d_pair.as<uint32_t>(),
                                   daoff.as<uint64_t>(), dsoff.as<uint64_t>(), d_seg.as<uint32_t>(), d_segn.as<uint32_t>(), d_pred.as<uint32_t>(), d_root.as<uint32_t>(),
                                   d_qidx.as<uint32_t>(), d_ridx.as<uint32_t>(), d_best.as<unsigned long long>(), d_mat.as<uint8_t>(), d_diff.as<int32_t>(),
                                   d_nch.as<uint32_t>());
                GS_HIP_CHECK(hipGetLastError());
            }
            hipLaunchKernelGGL(k_ani_sides, dim3((uint32_t)(2 * np)), dim3(64), 0, c->stream, Q, qoff_dev, R, roff_dev, pq_dev, pr_dev, p0, daoff.as<uint64_t>(),
                               dsoff.as<uint64_t>(), d_mat.as<uint8_t>(), d_diff.as<int32_t>(), d_nch.as<uint32_t>(), k, out_dev);
            GS_HIP_CHECK(hipGetLastError());
            GS_HIP_CHECK(stream_wait(c));         // the host lists above must outlive their copies
            p0 = p1;
        }
        sp0 = sp1;
    }
    return GS_OK;
}

}  // namespace gs

extern "C" {

int gs_ani_sketch_batch(gs_ctx *c, uint32_t k, uint32_t cc, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                        const uint64_t *genome_rec_off, uint64_t n_genomes, uint32_t **seeds_out, uint64_t *off_out)
{
    using namespace gs;
    int rc = ani_check(k, cc);
    if (rc) return rc;
    GS_REQUIRE(c && seeds_out && off_out && genome_rec_off && (n_rec == 0 || (rec_start && rec_len)) && (seq_bytes == 0 || seq), GS_ERR_INVALID, "null argument");
    *seeds_out = nullptr;
    GS_CTX_LOCK(c);
    PoolBuf dseq(c, SL_ANIB_SEQ), drs(c, SL_ANIB_REC_START), drl(c, SL_ANIB_REC_LEN), dgo(c, SL_ANIB_GOFF);
    const size_t padded = (size_t)round_up(seq_bytes, 8) + 16;
    if ((rc = dseq.alloc(padded)) || (rc = drs.alloc(8 * n_rec)) || (rc = drl.alloc(8 * n_rec)) || (rc = dgo.alloc(8 * (n_genomes + 1)))) return rc;
    const size_t tail = round_up(seq_bytes, 8) >= 8 ? (size_t)round_up(seq_bytes, 8) - 8 : 0;      // the walkers read whole 8-byte words
    GS_HIP_CHECK(hipMemsetAsync((uint8_t *)dseq.p + tail, 0, padded - tail, c->stream));
    if (seq_bytes) GS_HIP_CHECK(hipMemcpyAsync(dseq.p, seq, seq_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_rec) {
        GS_HIP_CHECK(hipMemcpyAsync(drs.p, rec_start, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(drl.p, rec_len, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
    }
    GS_HIP_CHECK(hipMemcpyAsync(dgo.p, genome_rec_off, 8 * (n_genomes + 1), hipMemcpyHostToDevice, c->stream));
    std::vector<uint64_t> counts;
    std::vector<uint32_t> flat;
    if ((rc = ani_seed_core(c, k, cc, dseq.as<uint8_t>(), seq_bytes, rec_start, rec_len, n_rec, genome_rec_off, n_genomes, drs.as<uint64_t>(), drl.as<uint64_t>(),
                            dgo.as<uint64_t>(), counts, &flat, 0, nullptr)))
        return rc;
    off_out[0] = 0;
    for (uint64_t g = 0; g < n_genomes; g++) off_out[g + 1] = off_out[g] + counts[g];
    uint32_t *h = (uint32_t *)malloc(std::max<size_t>(4 * flat.size(), 16));
    GS_REQUIRE(h, GS_ERR_INVALID, "out of host memory (%zu seeds)", flat.size() / 4);
    if (!flat.empty()) memcpy(h, flat.data(), 4 * flat.size());
    *seeds_out = h;
    return GS_OK;
}

int gs_ani_sketch_batch_dev(gs_ctx *c, uint32_t k, uint32_t cc, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev,
                            uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint32_t cap, uint32_t *seeds_out_dev, uint32_t *count_out_dev)
{
    using namespace gs;
    int rc = ani_check(k, cc);
    if (rc) return rc;
    GS_REQUIRE(c && genome_rec_off_dev && (n_genomes == 0 || count_out_dev) && (n_rec == 0 || (seq_dev && rec_start_dev && rec_len_dev)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(cap == 0 || seeds_out_dev, GS_ERR_INVALID, "null seeds_out_dev");
    if (n_genomes == 0) return GS_OK;
    GS_CTX_LOCK(c);
    std::vector<uint64_t> rs(std::max<uint64_t>(n_rec, 1)), rl(std::max<uint64_t>(n_rec, 1)), go(n_genomes + 1);
    if (n_rec) {
        GS_HIP_CHECK(hipMemcpyAsync(rs.data(), rec_start_dev, 8 * n_rec, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(rl.data(), rec_len_dev, 8 * n_rec, hipMemcpyDeviceToHost, c->stream));
    }
    GS_HIP_CHECK(hipMemcpyAsync(go.data(), genome_rec_off_dev, 8 * (n_genomes + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    std::vector<uint64_t> counts;
    if ((rc = ani_seed_core(c, k, cc, (const uint8_t *)seq_dev, seq_bytes, rs.data(), rl.data(), n_rec, go.data(), n_genomes, rec_start_dev, rec_len_dev, genome_rec_off_dev,
                            counts, nullptr, cap, seeds_out_dev)))
        return rc;
    std::vector<uint32_t> c32(n_genomes);
    uint64_t worst = 0, worst_g = 0;
    for (uint64_t g = 0; g < n_genomes; g++) { c32[g] = (uint32_t)counts[g]; if (counts[g] > worst) { worst = counts[g]; worst_g = g; } }
    GS_HIP_CHECK(hipMemcpyAsync(count_out_dev, c32.data(), 4 * n_genomes, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    GS_REQUIRE(worst <= cap, GS_ERR_INVALID, "genome %llu has %llu seeds, more than cap = %u (counts hold the true sizes)", (unsigned long long)worst_g,
               (unsigned long long)worst, cap);
    return GS_OK;
}

int gs_ani_pairs_dev(gs_ctx *c, uint32_t k, const uint32_t *q_seeds_dev, const uint64_t *q_off_dev, uint64_t nq, const uint32_t *r_seeds_dev, const uint64_t *r_off_dev,
                     uint64_t nr, const uint32_t *pair_q_dev, const uint32_t *pair_r_dev, uint64_t n_pairs, uint64_t *out_dev, uint64_t max_block_anchors)
{
    using namespace gs;
    int rc = ani_check(k, 1);
    if (rc) return rc;
    GS_REQUIRE(c && q_off_dev && r_off_dev && (n_pairs == 0 || (pair_q_dev && pair_r_dev && out_dev)), GS_ERR_INVALID, "null argument");
    if (n_pairs == 0) return GS_OK;
    GS_CTX_LOCK(c);
    std::vector<uint64_t> qo(nq + 1), ro(nr + 1);
    std::vector<uint32_t> pq(n_pairs), pr(n_pairs);
    GS_HIP_CHECK(hipMemcpyAsync(qo.data(), q_off_dev, 8 * (nq + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(ro.data(), r_off_dev, 8 * (nr + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(pq.data(), pair_q_dev, 4 * n_pairs, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(pr.data(), pair_r_dev, 4 * n_pairs, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    return ani_pairs_impl(c, k, (const uint4 *)q_seeds_dev, q_off_dev, qo.data(), nq, (const uint4 *)r_seeds_dev, r_off_dev, ro.data(), nr, pair_q_dev, pair_r_dev, pq.data(),
                          pr.data(), n_pairs, max_block_anchors, out_dev);
}

int gs_ani_pairs(gs_ctx *c, uint32_t k, const uint32_t *q_seeds, const uint64_t *q_off, uint64_t nq, const uint32_t *r_seeds, const uint64_t *r_off, uint64_t nr,
                 const uint32_t *pair_q, const uint32_t *pair_r, uint64_t n_pairs, uint64_t *out, uint64_t max_block_anchors)
{
    using namespace gs;
    int rc = ani_check(k, 1);
    if (rc) return rc;
    GS_REQUIRE(c && q_off && r_off && (n_pairs == 0 || (pair_q && pair_r && out)), GS_ERR_INVALID, "null argument");
    if (n_pairs == 0) return GS_OK;
    GS_REQUIRE((q_off[nq] == 0 || q_seeds) && (r_off[nr] == 0 || r_seeds), GS_ERR_INVALID, "null seeds");
    GS_CTX_LOCK(c);
    PoolBuf dq(c, SL_ANIP_Q), dqo(c, SL_ANIP_QOFF), dr(c, SL_ANIP_R), dro(c, SL_ANIP_ROFF), dpq(c, SL_ANIP_PQ), dpr(c, SL_ANIP_PR), dout(c, SL_ANIP_OUT);
    if ((rc = dq.alloc(16 * q_off[nq])) || (rc = dqo.alloc(8 * (nq + 1))) || (rc = dr.alloc(16 * r_off[nr])) || (rc = dro.alloc(8 * (nr + 1))) ||
        (rc = dpq.alloc(4 * n_pairs)) || (rc = dpr.alloc(4 * n_pairs)) || (rc = dout.alloc(64 * n_pairs)))
        return rc;
    if (q_off[nq]) GS_HIP_CHECK(hipMemcpyAsync(dq.p, q_seeds, 16 * q_off[nq], hipMemcpyHostToDevice, c->stream));
    if (r_off[nr]) GS_HIP_CHECK(hipMemcpyAsync(dr.p, r_seeds, 16 * r_off[nr], hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dqo.p, q_off, 8 * (nq + 1), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dro.p, r_off, 8 * (nr + 1), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dpq.p, pair_q, 4 * n_pairs, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dpr.p, pair_r, 4 * n_pairs, hipMemcpyHostToDevice, c->stream));
    if ((rc = ani_pairs_impl(c, k, dq.as<uint4>(), dqo.as<uint64_t>(), q_off, nq, dr.as<uint4>(), dro.as<uint64_t>(), r_off, nr, dpq.as<uint32_t>(), dpr.as<uint32_t>(), pair_q,
                             pair_r, n_pairs, max_block_anchors, dout.as<uint64_t>())))
        return rc;
    GS_HIP_CHECK(hipMemcpyAsync(out, dout.p, 64 * n_pairs, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

int gs_ani_chain_dev(gs_ctx *c, const uint32_t *rcontig_dev, const uint32_t *rpos_dev, const uint32_t *qcontig_dev, const uint32_t *qpos_dev, const uint32_t *strand_dev,
                     const uint64_t *off_dev, uint64_t n_pairs, int32_t *f_out_dev, uint32_t *pred_out_dev, uint32_t *root_out_dev)
{
    using namespace gs;
    GS_REQUIRE(c && off_dev, GS_ERR_INVALID, "null argument");
    if (n_pairs == 0) return GS_OK;
    GS_CTX_LOCK(c);
    std::vector<uint64_t> off(n_pairs + 1);
    GS_HIP_CHECK(hipMemcpyAsync(off.data(), off_dev, 8 * (n_pairs + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    GS_REQUIRE(off[0] == 0, GS_ERR_INVALID, "superani: offsets must start at 0");
    for (uint64_t p = 0; p < n_pairs; p++) {
        GS_REQUIRE(off[p + 1] >= off[p], GS_ERR_INVALID, "superani: offsets decrease at pair %llu", (unsigned long long)p);
        GS_REQUIRE(off[p + 1] - off[p] <= GS_ANI_MAX_PAIR_ANCHORS, GS_ERR_UNSUPPORTED, "superani: pair %llu has more than 2^26 anchors", (unsigned long long)p);
    }
    const uint64_t n = off[n_pairs];
    if (n == 0) return GS_OK;
    GS_REQUIRE(n < (1ull << 32), GS_ERR_UNSUPPORTED, "superani: 2^32 anchors or more in one call");
    GS_REQUIRE(rcontig_dev && rpos_dev && qcontig_dev && qpos_dev && strand_dev && f_out_dev && pred_out_dev && root_out_dev, GS_ERR_INVALID, "null argument");
    PoolBuf d_pair(c, SL_ANI_A_PAIR), d_tiles(c, SL_ANI_SEG_TILES), d_seg(c, SL_ANI_SEG_START), d_segn(c, SL_ANI_SEG_N);
    const AniAnchors an{rcontig_dev, rpos_dev, qcontig_dev, qpos_dev, strand_dev};
    uint32_t bad = 0;
    int rc = ani_chain_block(c, an, off_dev, n_pairs, n, d_pair, d_tiles, d_seg, d_segn, f_out_dev, pred_out_dev, root_out_dev, &bad);
    if (rc) return rc;
    GS_REQUIRE(!bad, GS_ERR_INVALID, "superani: the anchors of a pair must be in order of (r contig, r position)");
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

int gs_ani_estimate(const uint64_t *counts, const uint64_t *bases_q, const uint64_t *bases_r, uint64_t n_pairs, uint32_t k, float *out)
{
    GS_REQUIRE(k >= 1 && (n_pairs == 0 || (counts && bases_q && bases_r && out)), GS_ERR_INVALID, "bad argument");
    const double e = 1.0 / (double)k;
    for (uint64_t p = 0; p < n_pairs; p++) {
        const uint64_t *r = counts + 8 * p;
        double ani = 0.0;
        if (r[3]) { const double share = (double)r[2] / (double)r[3]; ani = ::pow(share, e); }
        const double afq = bases_q[p] ? (double)r[4] / (double)bases_q[p] : 0.0, afr = bases_r[p] ? (double)r[7] / (double)bases_r[p] : 0.0;
        if ((afq > afr ? afq : afr) < GS_ANI_MIN_AF) ani = 0.0;
        out[3 * p] = (float)ani; out[3 * p + 1] = (float)afq; out[3 * p + 2] = (float)afr;
    }
    return GS_OK;
}

}  // extern "C"
