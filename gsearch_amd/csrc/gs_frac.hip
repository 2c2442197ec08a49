// gs_frac.hip — superaai (binaux/src/bin/superaai.rs of the reference): FracMinHash / bottom-k sketches of proteomes and the AAI of every
// query x reference pair (SPEC.md 9). Upstream re-reads and re-sketches both files of every pair inside its par_iter (superaai.rs:115-156);
// here each file is sketched once and the all-pairs step runs on the device.
//
//   k_frac_hash      one workgroup per stretch of FR_TASK windows of one record: a k-byte window slides through registers (one to four u64),
//                    MurmurHash3_x64_128 (seed 42), hashes <= the genome's threshold collected in LDS, one global atomic per workgroup to
//                    place them in the genome's candidate region. A genome is spread over as many workgroups as it has stretches.
//   k_frac_seg_sort  one workgroup per genome of <= FR_SORT candidates: bitonic sort in LDS, duplicates dropped, the bottom `num` written back.
//                    Longer segments go through radix_sort_u64 / run_length_encode_u64 (gs_radix.hip), one genome at a time.
//   k_frac_pairs     one workgroup per (query, tile of references): the query's sketch in LDS (or read from global memory when longer), each
//                    wavefront walks one reference's first min(b, num) values 64 at a time; a binary search gives each value's rank in the query,
//                    a ballot / popcount prefix the common values before it, and so its rank in the union (SPEC 9 fact b).
// No float atomics: candidate slots come from integer atomics, and their order is erased by the sort.
#include <charconv>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"

namespace gs {
int ingest_records_dev(gs_ctx *c, bool aa, bool contiguous, const void *text_dev, uint64_t n_bytes, const uint64_t *seq_begin, const uint64_t *seq_end,
                       uint64_t n_rec, void *out_dev, uint64_t out_base0, uint64_t *rec_start_out, uint64_t *rec_len_out, uint64_t *out_end, bool raw);

constexpr uint32_t FR_T = 256;                  // hash kernel: threads per workgroup
constexpr uint32_t FR_PER = 16;                 // consecutive windows per thread
constexpr uint32_t FR_TASK = FR_T * FR_PER;     // windows per workgroup (never more survivors than LDS slots)
constexpr uint32_t FR_SORT = 8192;              // candidates a segment may have to be sorted in LDS (64 KB)
constexpr uint32_t FR_SORT_T = 1024;
constexpr uint32_t FP_T = 512;                  // pair kernel: threads per workgroup
constexpr uint32_t FP_RT = 128;                 // references per workgroup
constexpr uint32_t FP_LDS = 8192;               // query values kept in LDS; a longer query is searched in global memory

struct FracTask { uint64_t pos; uint32_t n, genome; };     // windows [pos, pos + n) of one record (byte offsets of their first byte)

// slide one byte into a k-byte window held little-endian in NW words (bytes past k stay zero)
template <int NW> __device__ __forceinline__ void frac_slide(uint64_t (&w)[NW], uint32_t top_shift, uint64_t b)
{
#pragma unroll
    for (int j = 0; j < NW - 1; j++) w[j] = (w[j] >> 8) | (w[j + 1] << 56);
    w[NW - 1] = (w[NW - 1] >> 8) | (b << top_shift);
}

template <int NW>
__global__ __launch_bounds__(FR_T) void k_frac_hash(const uint8_t *__restrict__ seq, const FracTask *__restrict__ tasks, uint32_t k,
                                                    const uint64_t *__restrict__ thr, const uint64_t *__restrict__ cand_off, const uint64_t *__restrict__ cap,
                                                    unsigned long long *__restrict__ cnt, uint64_t *__restrict__ cand)
{
    __shared__ uint64_t s_buf[FR_TASK];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const FracTask t = tasks[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t th = thr[t.genome];
    const uint32_t w0 = threadIdx.x * FR_PER, top = 8 * ((k - 1) & 7);
    const bool any = w0 < t.n;
    const uint8_t *p = seq + t.pos + w0;
    uint64_t w[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) w[j] = 0;
    if (any)
        for (uint32_t i = 0; i + 1 < k; i++) frac_slide<NW>(w, top, p[i]);
    const uint64_t lt = (1ull << lane) - 1;
    for (uint32_t i = 0; i < FR_PER; i++) {
        const bool valid = w0 + i < t.n;
        bool keep = false;
        uint64_t h = 0;
        if (valid) {
            frac_slide<NW>(w, top, p[i + k - 1]);
            h = mm3_h1_4(w[0], NW > 1 ? w[NW > 1 ? 1 : 0] : 0, NW > 2 ? w[NW > 2 ? 2 : 0] : 0, NW > 3 ? w[NW > 3 ? 3 : 0] : 0, k);
            keep = h <= th;
        }
        const uint64_t bal = __ballot(keep);
        if (bal) {
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)bal) - 1;
            uint32_t base = 0;
            if (lane == lead) base = atomicAdd(&s_n, (uint32_t)__popcll(bal));
            base = __shfl(base, lead);
            if (keep) s_buf[base + (uint32_t)__popcll(bal & lt)] = h;
        }
    }
    __syncthreads();
    const uint32_t n = s_n;
    if (n == 0) return;
    if (threadIdx.x == 0) s_base = atomicAdd(&cnt[t.genome], (unsigned long long)n);
    __syncthreads();
    const uint64_t base = s_base, cp = cap[t.genome], off = cand_off[t.genome];
    for (uint32_t i = threadIdx.x; i < n; i += FR_T)
        if (base + i < cp) cand[off + base + i] = s_buf[i];          // an overflowing genome is counted in full and redone with its exact size
}

// genome g = sel[blockIdx.x]: its n <= FR_SORT candidates sorted in LDS, the distinct values' count to distinct[g], the first `num` of them
// (all when num == 0) written back ascending to the start of its region
__global__ __launch_bounds__(FR_SORT_T) void k_frac_seg_sort(uint64_t *__restrict__ cand, const uint64_t *__restrict__ cand_off,
                                                             const unsigned long long *__restrict__ cnt, const uint32_t *__restrict__ sel, uint32_t num,
                                                             uint32_t *__restrict__ distinct)
{
    __shared__ uint64_t s[FR_SORT];
    __shared__ uint32_t s_wc[FR_SORT_T / 64];
    const uint32_t g = sel[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t n = (uint32_t)cnt[g];
    uint64_t *seg = cand + cand_off[g];
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (uint32_t i = tid; i < np2; i += FR_SORT_T) s[i] = i < n ? seg[i] : ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= np2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = tid; i < np2 / 2; i += FR_SORT_T) {
                const uint32_t lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                const uint64_t a = s[lo], b = s[hi];
                if ((a > b) == ((lo & size) == 0)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    uint32_t run = 0;
    const uint64_t lt = (1ull << lane) - 1;
    for (uint32_t c0 = 0; c0 < n; c0 += FR_SORT_T) {
        const uint32_t i = c0 + tid;
        const bool head = i < n && (i == 0 || s[i] != s[i - 1]);
        const uint64_t bal = __ballot(head);
        if (lane == 0) s_wc[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t pre = run, tot = 0;
        for (uint32_t w = 0; w < FR_SORT_T / 64; w++) { if (w < wv) pre += s_wc[w]; tot += s_wc[w]; }
        pre += (uint32_t)__popcll(bal & lt);
        if (head && (num == 0 || pre < num)) seg[pre] = s[i];
        run += tot;
        __syncthreads();
    }
    if (tid == 0) distinct[g] = run;
}

// copy n[j] values from srcs[j] to dst + dst_off[j], one workgroup per job
__global__ __launch_bounds__(256) void k_frac_gather(const uint64_t *const *__restrict__ srcs, uint64_t *__restrict__ dst, const uint64_t *__restrict__ dst_off,
                                                     const uint32_t *__restrict__ n)
{
    const uint32_t j = blockIdx.x, m = n[j];
    const uint64_t *a = srcs[j];
    uint64_t *b = dst + dst_off[j];
    for (uint32_t i = threadIdx.x; i < m; i += 256) b[i] = a[i];
}
// queue the copies of one round's finished genomes as one gather launch: (source, destination offset, count) per genome
struct FracCopies {
    std::vector<const uint64_t *> src; std::vector<uint64_t> dst; std::vector<uint32_t> n;
    void add(const uint64_t *s, uint64_t d, uint64_t m) { if (m) { src.push_back(s); dst.push_back(d); n.push_back((uint32_t)m); } }
    int launch(gs_ctx *c, uint64_t *dst_base)
    {
        if (src.empty()) return GS_OK;
        PoolBuf ds(c, SL_FRAC_COPY_SRC), dd(c, SL_FRAC_COPY_DST), dn(c, SL_FRAC_COPY_N);
        int rc;
        const size_t m = src.size();
        if ((rc = ds.alloc(8 * m)) || (rc = dd.alloc(8 * m)) || (rc = dn.alloc(4 * m))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(ds.p, src.data(), 8 * m, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(dd.p, dst.data(), 8 * m, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(dn.p, n.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_frac_gather, dim3((uint32_t)m), dim3(256), 0, c->stream, (const uint64_t *const *)ds.p, dst_base, dd.as<uint64_t>(), dn.as<uint32_t>());
        GS_HIP_CHECK(hipGetLastError());
        GS_HIP_CHECK(stream_wait(c));                 // the host arrays above are pageable: they must outlive the copies
        src.clear(); dst.clear(); n.clear();
        return GS_OK;
    }
};

// SPEC 9 similarity of query q against every reference of the workgroup's tile. Sketches: ascending, distinct.
__global__ __launch_bounds__(FP_T) void k_frac_pairs(const uint64_t *__restrict__ Q, const uint64_t *__restrict__ q_off, const uint64_t *__restrict__ R,
                                                     const uint64_t *__restrict__ r_off, uint64_t nr, uint64_t n_tiles, uint32_t num, uint32_t lds_cap,
                                                     double *__restrict__ sim, uint32_t *__restrict__ common_out, uint32_t *__restrict__ union_out)
{
    extern __shared__ uint64_t sA[];
    const uint64_t q = blockIdx.x / n_tiles, tile = blockIdx.x % n_tiles;
    const uint64_t a0 = q_off[q], a = q_off[q + 1] - a0;
    const uint64_t *A = Q + a0;
    if (a <= lds_cap) {
        for (uint64_t i = threadIdx.x; i < a; i += FP_T) sA[i] = A[i];
        __syncthreads();
        A = sA;
    }
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t lt = (1ull << lane) - 1;
    const uint64_t r_end = (tile + 1) * FP_RT < nr ? (tile + 1) * FP_RT : nr;
    for (uint64_t r = tile * FP_RT + wv; r < r_end; r += FP_T / 64) {
        const uint64_t b0 = r_off[r], b = r_off[r + 1] - b0;
        const uint64_t *B = R + b0;
        const bool full = num == 0 || (a < num && b < num);               // |A n B| in full is needed only then (fact a)
        const uint64_t jmax = num && b > num ? num : b;                   // union rank >= rank in B (fact b)
        uint64_t c = 0, counted = 0, lo = 0;
        for (uint64_t j0 = 0; j0 < jmax; j0 += 64) {
            const uint64_t j = j0 + lane;
            const bool valid = j < jmax;
            const uint64_t x = valid ? B[j] : 0;
            uint64_t L = lo, H = a;
            if (valid)
                while (L < H) { const uint64_t m = (L + H) >> 1; if (A[m] < x) L = m + 1; else H = m; }
            const bool found = valid && L < a && A[L] == x;
            const uint64_t bal = __ballot(found);
            const uint64_t rank = L + j - (c + (uint64_t)__popcll(bal & lt));  // union values below x
            counted += (uint64_t)__popcll(__ballot(found && (num == 0 || rank < num)));
            c += (uint64_t)__popcll(bal);
            const uint32_t last = (uint32_t)(jmax - 1 - j0 < 63 ? jmax - 1 - j0 : 63);
            lo = __shfl(L, last);
            if (!full && __shfl(rank, last) >= num) break;
        }
        const uint64_t u = full ? (num && a + b - c > num ? num : a + b - c) : num;
        if (lane == 0) {
            const uint64_t o = q * nr + r;
            sim[o] = (double)counted / (double)(u > 1 ? u : 1);
            if (common_out) common_out[o] = (uint32_t)counted;
            if (union_out) union_out[o] = (uint32_t)u;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// The sketches of n_genomes genomes whose residues are on the device (seq_dev; record r = residues [rec_start[r], rec_start[r] + rec_len[r]),
// HOST arrays; genome g = records [goff[g], goff[g+1])). `emit(g, src_dev, n)` is called for every genome once its n values sit ascending at
// src_dev, a device pointer valid until `round_end()` returns, which is called after each round's emits.
// Threshold of a genome: max_hash (all of S is needed: num == 0, or few windows), or - with num > 0 - a tighter one under which about
// 1.25 num + 64 windows are expected. That one is speculation: a genome with fewer than num distinct values under it is redone with an 8 x
// larger threshold (max_hash at most). A genome whose candidates overflow its slots is counted in full and redone with exactly that many.
template <class Emit, class RoundEnd>
static int frac_sketch_core(gs_ctx *c, uint32_t k, uint32_t scaled, uint32_t num, const uint8_t *seq_dev, const uint64_t *rec_start, const uint64_t *rec_len,
                            uint64_t n_rec, const uint64_t *goff, uint64_t ng, Emit &&emit, RoundEnd &&round_end)
{
    const uint64_t max_hash = frac_max_hash(scaled), eff = max_hash ? max_hash : ~0ull;
    std::vector<uint64_t> W(ng, 0);
    for (uint64_t g = 0; g < ng; g++)
        for (uint64_t r = goff[g]; r < goff[g + 1]; r++) W[g] += rec_len[r] >= k ? rec_len[r] - k + 1 : 0;
    std::vector<uint64_t> thr(ng, eff), cap(ng, 0), off(ng + 1, 0);
    std::vector<uint8_t> todo(ng, 0);
    const double two64 = 18446744073709551616.0;
    for (uint64_t g = 0; g < ng; g++) {
        if (num == 0 && max_hash == 0) { emit(g, nullptr, 0); continue; }     // no filter and no bound: the sketch is empty
        if (W[g] == 0) { emit(g, nullptr, 0); continue; }
        todo[g] = 1;
        if (num) {
            const double target = 1.25 * num + 64.0;
            if ((double)W[g] > target) {
                const double t = target / (double)W[g] * two64;
                if (t < (double)eff) thr[g] = (uint64_t)t;
            }
        }
    }
    PoolBuf dcand(c, SL_FRAC_CAND), dthr(c, SL_FRAC_THR), doff(c, SL_FRAC_OFF), dcap(c, SL_FRAC_CAP), dcnt(c, SL_FRAC_CNT), dtask(c, SL_FRAC_TASK), dsel(c, SL_FRAC_SEL), ddist(c, SL_FRAC_DIST);
    PoolBuf dalt(c, SL_FRAC_ALT), dlen(c, SL_FRAC_LEN), dpos(c, SL_FRAC_POS), drs(c, SL_FRAC_RADIX), dnr(c, SL_FRAC_NRUNS);
    std::vector<unsigned long long> cnt(ng);
    std::vector<uint32_t> dist(ng);
    std::vector<uint8_t> overflow(ng, 0);
    int rc;
    for (int round = 0;; round++) {
        GS_REQUIRE(round < 64, GS_ERR_INVALID, "frac sketch: no progress after 64 rounds");
        std::vector<uint64_t> act;
        for (uint64_t g = 0; g < ng; g++) if (todo[g]) act.push_back(g);
        if (act.empty()) break;
        uint64_t tot = 0;
        for (uint64_t g : act) {
            if (!overflow[g]) {
                const double e = thr[g] == ~0ull ? (double)W[g] : (double)W[g] * ((double)thr[g] / two64);
                cap[g] = std::min<uint64_t>(W[g], (uint64_t)(1.25 * e) + 1024);
            }
            off[g] = tot; tot += cap[g];
        }
        std::vector<FracTask> tasks;
        for (uint64_t g : act)
            for (uint64_t r = goff[g]; r < goff[g + 1]; r++) {
                if (rec_len[r] < k) continue;
                const uint64_t nw = rec_len[r] - k + 1;
                for (uint64_t w = 0; w < nw; w += FR_TASK) tasks.push_back({rec_start[r] + w, (uint32_t)std::min<uint64_t>(FR_TASK, nw - w), (uint32_t)g});
            }
        GS_REQUIRE(tasks.size() < (1ull << 31), GS_ERR_UNSUPPORTED, "frac sketch: batch too large");
        if ((rc = dcand.alloc(8 * tot)) || (rc = dthr.alloc(8 * ng)) || (rc = doff.alloc(8 * ng)) || (rc = dcap.alloc(8 * ng)) || (rc = dcnt.alloc(8 * ng)) ||
            (rc = dtask.alloc(sizeof(FracTask) * tasks.size())) || (rc = ddist.alloc(4 * ng)))
            return rc;
        GS_HIP_CHECK(hipMemcpyAsync(dthr.p, thr.data(), 8 * ng, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(doff.p, off.data(), 8 * ng, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(dcap.p, cap.data(), 8 * ng, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(dtask.p, tasks.data(), sizeof(FracTask) * tasks.size(), hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemsetAsync(dcnt.p, 0, 8 * ng, c->stream));
        {
            ProfScope ps(c, FAM_SKETCH);
            const dim3 grid((uint32_t)tasks.size()), blk(FR_T);
            const FracTask *tk = dtask.as<FracTask>();
            auto *cn = dcnt.as<unsigned long long>();
            if (k <= 8) hipLaunchKernelGGL(k_frac_hash<1>, grid, blk, 0, c->stream, seq_dev, tk, k, dthr.as<uint64_t>(), doff.as<uint64_t>(), dcap.as<uint64_t>(), cn, dcand.as<uint64_t>());
            else if (k <= 16) hipLaunchKernelGGL(k_frac_hash<2>, grid, blk, 0, c->stream, seq_dev, tk, k, dthr.as<uint64_t>(), doff.as<uint64_t>(), dcap.as<uint64_t>(), cn, dcand.as<uint64_t>());
            else if (k <= 24) hipLaunchKernelGGL(k_frac_hash<3>, grid, blk, 0, c->stream, seq_dev, tk, k, dthr.as<uint64_t>(), doff.as<uint64_t>(), dcap.as<uint64_t>(), cn, dcand.as<uint64_t>());
            else hipLaunchKernelGGL(k_frac_hash<4>, grid, blk, 0, c->stream, seq_dev, tk, k, dthr.as<uint64_t>(), doff.as<uint64_t>(), dcap.as<uint64_t>(), cn, dcand.as<uint64_t>());
            GS_HIP_CHECK(hipGetLastError());
        }
        GS_HIP_CHECK(hipMemcpyAsync(cnt.data(), dcnt.p, 8 * ng, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(stream_wait(c));
        std::vector<uint32_t> small;
        std::vector<uint64_t> large;
        uint64_t large_max = 0;
        for (uint64_t g : act) {
            overflow[g] = cnt[g] > cap[g];
            if (overflow[g]) { cap[g] = cnt[g]; continue; }
            if (cnt[g] <= FR_SORT) small.push_back((uint32_t)g); else { large.push_back(g); large_max = std::max<uint64_t>(large_max, cnt[g]); }
        }
        if (!small.empty()) {
            if ((rc = dsel.alloc(4 * small.size()))) return rc;
            GS_HIP_CHECK(hipMemcpyAsync(dsel.p, small.data(), 4 * small.size(), hipMemcpyHostToDevice, c->stream));
            ProfScope ps(c, FAM_SKETCH);
            hipLaunchKernelGGL(k_frac_seg_sort, dim3((uint32_t)small.size()), dim3(FR_SORT_T), 0, c->stream, dcand.as<uint64_t>(), doff.as<uint64_t>(),
                               (const unsigned long long *)dcnt.p, dsel.as<uint32_t>(), num, ddist.as<uint32_t>());
            GS_HIP_CHECK(hipGetLastError());
        }
        if (!large.empty()) {
            GS_REQUIRE(large_max < (1ull << 32), GS_ERR_UNSUPPORTED, "frac sketch: more than 2^32 candidates in one genome");
            if ((rc = dalt.alloc(8 * large_max)) || (rc = dlen.alloc(4 * large_max)) || (rc = dpos.alloc(4 * large_max)) || (rc = drs.alloc(radix_scratch_bytes(large_max))))
                return rc;
            for (uint64_t g : large) {
                uint64_t *seg = dcand.as<uint64_t>() + off[g], *sorted = nullptr;
                const uint64_t n = cnt[g];
                if ((rc = radix_sort_u64(c, seg, dalt.as<uint64_t>(), n, 64, drs.p, &sorted))) return rc;
                uint64_t *uniq = sorted == seg ? dalt.as<uint64_t>() : seg;
                if ((rc = run_length_encode_u64(c, sorted, n, uniq, dlen.as<uint32_t>(), ddist.as<uint32_t>() + g, dpos.as<uint32_t>(), drs.p))) return rc;
                const uint64_t keep = num ? std::min<uint64_t>(num, n) : n;        // (at most the distinct count is used)
                if (uniq != seg) GS_HIP_CHECK(hipMemcpyAsync(seg, uniq, 8 * keep, hipMemcpyDeviceToDevice, c->stream));
            }
        }
        GS_HIP_CHECK(hipMemcpyAsync(dist.data(), ddist.p, 4 * ng, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(stream_wait(c));
        for (uint64_t g : act) {
            if (overflow[g]) continue;
            if (num && dist[g] < num && thr[g] < eff) {         // speculation failed: fewer than num distinct values under a threshold below max_hash
                thr[g] = thr[g] > eff / 8 ? eff : std::max<uint64_t>(thr[g] * 8, 1);
                continue;
            }
            todo[g] = 0;
            if ((rc = emit(g, dcand.as<uint64_t>() + off[g], num ? std::min<uint64_t>(num, dist[g]) : dist[g]))) return rc;
        }
        if ((rc = round_end())) return rc;
    }
    return GS_OK;
}

int frac_check_k(uint32_t k)
{
    GS_REQUIRE(k >= 1, GS_ERR_INVALID, "k must be >= 1");
    GS_REQUIRE(k <= GS_FRAC_KMAX, GS_ERR_UNSUPPORTED, "k = %u: only 1 <= k <= %u is supported", k, (unsigned)GS_FRAC_KMAX);
    return GS_OK;
}

// residues on the device -> library-allocated host CSR (values ascending, off_out[ng + 1])
int frac_sketch_to_host(gs_ctx *c, uint32_t k, uint32_t scaled, uint32_t num, const uint8_t *seq_dev, const uint64_t *rec_start, const uint64_t *rec_len,
                        uint64_t n_rec, const uint64_t *goff, uint64_t ng, std::vector<std::vector<uint64_t>> &rows)
{
    int rc = frac_check_k(k);
    if (rc) return rc;
    rows.assign(ng, {});
    FracCopies cp;
    std::vector<uint64_t> done;
    uint64_t tot = 0;
    PoolBuf dst(c, SL_FRAC_HOST_ROWS);
    auto emit = [&](uint64_t g, const uint64_t *src, uint64_t n) -> int {
        rows[g].resize(n);
        if (n) { cp.add(src, tot, n); done.push_back(g); tot += n; }
        return GS_OK;
    };
    auto round_end = [&]() -> int {
        int r2;
        if (tot == 0) return GS_OK;
        if ((r2 = dst.alloc(8 * tot)) || (r2 = cp.launch(c, dst.as<uint64_t>()))) return r2;
        std::vector<uint64_t> h(tot);
        GS_HIP_CHECK(hipMemcpyAsync(h.data(), dst.p, 8 * tot, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(stream_wait(c));
        uint64_t o = 0;
        for (uint64_t g : done) { memcpy(rows[g].data(), h.data() + o, 8 * rows[g].size()); o += rows[g].size(); }
        done.clear(); tot = 0;
        return GS_OK;
    };
    return frac_sketch_core(c, k, scaled, num, seq_dev, rec_start, rec_len, n_rec, goff, ng, emit, round_end);
}

static int rows_to_csr(const std::vector<std::vector<uint64_t>> &rows, uint64_t **hash_out, uint64_t *off_out)
{
    uint64_t tot = 0;
    off_out[0] = 0;
    for (size_t g = 0; g < rows.size(); g++) { tot += rows[g].size(); off_out[g + 1] = tot; }
    uint64_t *h = (uint64_t *)malloc(8 * std::max<uint64_t>(tot, 1));
    GS_REQUIRE(h, GS_ERR_INVALID, "out of host memory (%llu values)", (unsigned long long)tot);
    for (size_t g = 0; g < rows.size(); g++) if (!rows[g].empty()) memcpy(h + off_out[g], rows[g].data(), 8 * rows[g].size());
    *hash_out = h;
    return GS_OK;
}

static int check_sorted_csr(const uint64_t *v, const uint64_t *off, uint64_t n, const char *what)
{
    GS_REQUIRE(off[0] == 0, GS_ERR_INVALID, "%s: offsets must start at 0", what);
    for (uint64_t i = 0; i < n; i++) {
        GS_REQUIRE(off[i + 1] >= off[i] && off[i + 1] - off[i] < (1ull << 32), GS_ERR_INVALID, "%s: bad offsets at %llu", what, (unsigned long long)i);
        for (uint64_t j = off[i] + 1; j < off[i + 1]; j++)
            GS_REQUIRE(v[j - 1] < v[j], GS_ERR_INVALID, "%s: sketch %llu is not strictly ascending", what, (unsigned long long)i);
    }
    return GS_OK;
}

static int frac_pairs_launch(gs_ctx *c, uint32_t num, const uint64_t *Q, const uint64_t *q_off, uint64_t nq, uint64_t max_a, const uint64_t *R,
                             const uint64_t *r_off, uint64_t nr, double *sim, uint32_t *common, uint32_t *uni)
{
    if (nq == 0 || nr == 0) return GS_OK;
    const uint64_t n_tiles = (nr + FP_RT - 1) / FP_RT;
    GS_REQUIRE(nq * n_tiles < (1ull << 31), GS_ERR_UNSUPPORTED, "frac similarity: %llu x %llu pairs in one call", (unsigned long long)nq, (unsigned long long)nr);
    const uint32_t lds_cap = (uint32_t)std::min<uint64_t>(max_a, FP_LDS);
    ProfScope ps(c, FAM_HAMMING);
    hipLaunchKernelGGL(k_frac_pairs, dim3((uint32_t)(nq * n_tiles)), dim3(FP_T), 8 * std::max<uint32_t>(lds_cap, 1), c->stream, Q, q_off, R, r_off, nr, n_tiles, num,
                       lds_cap, sim, common, uni);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

}  // namespace gs

extern "C" {

uint64_t gs_frac_max_hash(uint32_t scaled) { return gs::frac_max_hash(scaled); }

double gs_aai(double sim, uint32_t k)
{
    const double two_s = 2.0 * sim, one_s = 1.0 + sim;
    return 1.0 + ::log(two_s / one_s) / (double)k;
}

int gs_frac_sketch_batch(gs_ctx *c, uint32_t k, uint32_t scaled, uint32_t num, const void *text, uint64_t n_bytes, const uint64_t *rec_begin,
                         const uint64_t *rec_end, uint64_t n_rec, const uint64_t *genome_rec_off, uint64_t n_genomes, uint64_t **hash_out, uint64_t *off_out)
{
    int rc = gs::frac_check_k(k);
    if (rc) return rc;
    GS_REQUIRE(c && hash_out && off_out && genome_rec_off && (n_rec == 0 || (rec_begin && rec_end)) && (n_bytes == 0 || text), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(genome_rec_off[0] == 0 && genome_rec_off[n_genomes] == n_rec, GS_ERR_INVALID, "genome_rec_off must run from 0 to n_rec");
    for (uint64_t g = 0; g < n_genomes; g++) GS_REQUIRE(genome_rec_off[g] <= genome_rec_off[g + 1], GS_ERR_INVALID, "genome_rec_off must not decrease");
    for (uint64_t r = 0; r < n_rec; r++) GS_REQUIRE(rec_begin[r] <= rec_end[r] && rec_end[r] <= n_bytes, GS_ERR_INVALID, "record %llu outside the text", (unsigned long long)r);
    *hash_out = nullptr;
    GS_CTX_LOCK(c);
    gs::PoolBuf dtext(c, gs::SL_FRACB_TEXT), dres(c, gs::SL_FRACB_RESIDUES);
    if ((rc = dtext.alloc(n_bytes + 64)) || (rc = dres.alloc(n_bytes + 64))) return rc;
    if (n_bytes) GS_HIP_CHECK(hipMemcpyAsync(dtext.p, text, n_bytes, hipMemcpyHostToDevice, c->stream));
    std::vector<uint64_t> rs(std::max<uint64_t>(n_rec, 1), 0), rl(std::max<uint64_t>(n_rec, 1), 0);
    if ((rc = gs::ingest_records_dev(c, true, false, dtext.p, n_bytes, rec_begin, rec_end, n_rec, dres.p, 0, rs.data(), rl.data(), nullptr, true))) return rc;
    std::vector<std::vector<uint64_t>> rows;
    if ((rc = gs::frac_sketch_to_host(c, k, scaled, num, dres.as<uint8_t>(), rs.data(), rl.data(), n_rec, genome_rec_off, n_genomes, rows))) return rc;
    return gs::rows_to_csr(rows, hash_out, off_out);
}

int gs_frac_sketch_batch_dev(gs_ctx *c, uint32_t k, uint32_t scaled, uint32_t num, const void *seq_dev, uint64_t n_bytes, const uint64_t *rec_start_dev,
                             const uint64_t *rec_len_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint32_t cap,
                             uint64_t *hash_out_dev, uint32_t *count_out_dev)
{
    int rc = gs::frac_check_k(k);
    if (rc) return rc;
    GS_REQUIRE(c && genome_rec_off_dev && (n_genomes == 0 || count_out_dev) && (n_rec == 0 || (seq_dev && rec_start_dev && rec_len_dev)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(cap == 0 || hash_out_dev, GS_ERR_INVALID, "null hash_out_dev");
    if (n_genomes == 0) return GS_OK;
    GS_CTX_LOCK(c);
    std::vector<uint64_t> rs(std::max<uint64_t>(n_rec, 1)), rl(std::max<uint64_t>(n_rec, 1)), go(n_genomes + 1);
    if (n_rec) {
        GS_HIP_CHECK(hipMemcpyAsync(rs.data(), rec_start_dev, 8 * n_rec, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(rl.data(), rec_len_dev, 8 * n_rec, hipMemcpyDeviceToHost, c->stream));
    }
    GS_HIP_CHECK(hipMemcpyAsync(go.data(), genome_rec_off_dev, 8 * (n_genomes + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(gs::stream_wait(c));
    GS_REQUIRE(go[0] == 0 && go[n_genomes] == n_rec, GS_ERR_INVALID, "genome_rec_off must run from 0 to n_rec");
    for (uint64_t g = 0; g < n_genomes; g++) GS_REQUIRE(go[g] <= go[g + 1], GS_ERR_INVALID, "genome_rec_off must not decrease");
    for (uint64_t r = 0; r < n_rec; r++) GS_REQUIRE(rs[r] + rl[r] >= rs[r] && rs[r] + rl[r] <= n_bytes, GS_ERR_INVALID, "record %llu outside the sequence", (unsigned long long)r);
    std::vector<uint32_t> counts(n_genomes, 0);
    uint64_t worst = 0, worst_g = 0;
    gs::FracCopies cp;
    auto emit = [&](uint64_t g, const uint64_t *src, uint64_t n) -> int {
        counts[g] = (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull);
        if (n > worst) { worst = n; worst_g = g; }
        cp.add(src, g * (uint64_t)cap, std::min<uint64_t>(n, cap));      // never more than cap values into a row
        return GS_OK;
    };
    auto round_end = [&]() -> int { return cp.launch(c, hash_out_dev); };
    if ((rc = gs::frac_sketch_core(c, k, scaled, num, (const uint8_t *)seq_dev, rs.data(), rl.data(), n_rec, go.data(), n_genomes, emit, round_end))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(count_out_dev, counts.data(), 4 * n_genomes, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(gs::stream_wait(c));
    GS_REQUIRE(worst <= cap, GS_ERR_INVALID, "genome %llu has %llu values, more than cap = %u (counts hold the true sizes)", (unsigned long long)worst_g,
               (unsigned long long)worst, cap);
    return GS_OK;
}

int gs_frac_similarity_qxc(gs_ctx *c, uint32_t num, const uint64_t *Q, const uint64_t *q_off, uint64_t nq, const uint64_t *R, const uint64_t *r_off, uint64_t nr,
                           double *sim_out, uint32_t *common_out, uint32_t *union_out)
{
    GS_REQUIRE(c && q_off && r_off && (nq == 0 || nr == 0 || sim_out), GS_ERR_INVALID, "null argument");
    int rc;
    if ((rc = gs::check_sorted_csr(Q, q_off, nq, "Q")) || (rc = gs::check_sorted_csr(R, r_off, nr, "R"))) return rc;
    if (nq == 0 || nr == 0) return GS_OK;
    GS_CTX_LOCK(c);
    uint64_t max_a = 0;
    for (uint64_t i = 0; i < nq; i++) max_a = std::max<uint64_t>(max_a, q_off[i + 1] - q_off[i]);
    const uint64_t nqv = q_off[nq], nrv = r_off[nr], np = nq * nr;
    gs::PoolBuf dq(c, gs::SL_FRACS_Q), dqo(c, gs::SL_FRACS_QOFF), dr(c, gs::SL_FRACS_R), dro(c, gs::SL_FRACS_ROFF), ds(c, gs::SL_FRACS_SIM), dc(c, gs::SL_FRACS_COMMON), du(c, gs::SL_FRACS_UNION);
    if ((rc = dq.alloc(8 * nqv)) || (rc = dqo.alloc(8 * (nq + 1))) || (rc = dr.alloc(8 * nrv)) || (rc = dro.alloc(8 * (nr + 1))) || (rc = ds.alloc(8 * np)) ||
        (common_out && (rc = dc.alloc(4 * np))) || (union_out && (rc = du.alloc(4 * np))))
        return rc;
    if (nqv) GS_HIP_CHECK(hipMemcpyAsync(dq.p, Q, 8 * nqv, hipMemcpyHostToDevice, c->stream));
    if (nrv) GS_HIP_CHECK(hipMemcpyAsync(dr.p, R, 8 * nrv, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dqo.p, q_off, 8 * (nq + 1), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dro.p, r_off, 8 * (nr + 1), hipMemcpyHostToDevice, c->stream));
    if ((rc = gs::frac_pairs_launch(c, num, dq.as<uint64_t>(), dqo.as<uint64_t>(), nq, max_a, dr.as<uint64_t>(), dro.as<uint64_t>(), nr, ds.as<double>(),
                                    common_out ? dc.as<uint32_t>() : nullptr, union_out ? du.as<uint32_t>() : nullptr)))
        return rc;
    GS_HIP_CHECK(hipMemcpyAsync(sim_out, ds.p, 8 * np, hipMemcpyDeviceToHost, c->stream));
    if (common_out) GS_HIP_CHECK(hipMemcpyAsync(common_out, dc.p, 4 * np, hipMemcpyDeviceToHost, c->stream));
    if (union_out) GS_HIP_CHECK(hipMemcpyAsync(union_out, du.p, 4 * np, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(gs::stream_wait(c));
    return GS_OK;
}

int gs_frac_similarity_qxc_dev(gs_ctx *c, uint32_t num, const uint64_t *Q_dev, const uint64_t *q_off_dev, uint64_t nq, const uint64_t *R_dev, const uint64_t *r_off_dev,
                               uint64_t nr, double *sim_out_dev, uint32_t *common_out_dev, uint32_t *union_out_dev)
{
    GS_REQUIRE(c && q_off_dev && r_off_dev && (nq == 0 || nr == 0 || sim_out_dev), GS_ERR_INVALID, "null argument");
    if (nq == 0 || nr == 0) return GS_OK;
    GS_CTX_LOCK(c);
    std::vector<uint64_t> qo(nq + 1);       // the longest query decides whether queries are read from LDS
    GS_HIP_CHECK(hipMemcpyAsync(qo.data(), q_off_dev, 8 * (nq + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(gs::stream_wait(c));
    uint64_t max_a = 0;
    for (uint64_t i = 0; i < nq; i++) max_a = std::max<uint64_t>(max_a, qo[i + 1] - qo[i]);
    return gs::frac_pairs_launch(c, num, Q_dev, q_off_dev, nq, max_a, R_dev, r_off_dev, nr, sim_out_dev, common_out_dev, union_out_dev);
}

/* superaai.rs:97-113,159-165: `q\tr\t{sim}\t{aai}` per pair, query-major, joined by '\n' with no trailing newline; f64 as Rust's Display
 * (shortest round-trip digits, fixed notation: std::to_chars without precision) */
int gs_superaai_write(const char *out_path, const char *const *q_paths, uint64_t nq, const char *const *r_paths, uint64_t nr, const double *sim, uint32_t k)
{
    GS_REQUIRE(out_path && (nq == 0 || q_paths) && (nr == 0 || r_paths) && (nq == 0 || nr == 0 || sim), GS_ERR_INVALID, "null argument");
    FILE *f = fopen(out_path, "wb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot create %s", out_path);
    std::string line;
    char num[2][400];
    bool first = true, ok = true;
    for (uint64_t i = 0; i < nq && ok; i++)
        for (uint64_t j = 0; j < nr && ok; j++) {
            const double s = sim[i * nr + j], a = gs_aai(s, k);
            auto r0 = std::to_chars(num[0], num[0] + sizeof num[0] - 1, s, std::chars_format::fixed);
            auto r1 = std::to_chars(num[1], num[1] + sizeof num[1] - 1, a, std::chars_format::fixed);
            *r0.ptr = 0; *r1.ptr = 0;
            line.clear();
            if (!first) line += '\n';
            first = false;
            line += q_paths[i]; line += '\t'; line += r_paths[j]; line += '\t'; line += num[0]; line += '\t'; line += num[1];
            ok = fwrite(line.data(), 1, line.size(), f) == line.size();
        }
    ok = (fclose(f) == 0) && ok;
    GS_REQUIRE(ok, GS_ERR_IO, "write to %s failed", out_path);
    return GS_OK;
}

}  // extern "C"
