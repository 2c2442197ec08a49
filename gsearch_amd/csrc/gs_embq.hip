// gs_embq.hip — the quality of an embedding by neighbourhood conservation (SPEC.md 8.1; upstream's get_quality_estimate_from_edge_length, embed.rs:68-70):
// how much of every row of the k-NN graph lies among the kq nearest points of its node in the embedded space. Exact: all n x n pairs of positions are
// evaluated, none is stored, nothing is approximated. Squared distances are f32 sums in one pinned order (no fused multiply-add: -ffp-contract=off) and are
// compared as their u32 bit patterns, which is their order because they are >= +0 or +inf and never NaN. No atomics outside the finiteness flag.
//
//  * k_embq_finite : one thread per coordinate; a NaN or an infinity raises the flag.
//  * k_embq_edge   : one thread per slot; e2[i][t] = d2(i, ids[i][t]), +0 in an unused slot.
//  * k_embq_count  : THE all-pairs kernel, used by the rank pass and by every radius pass. One thread per row keeps the row's coordinates, K thresholds
//                    and K counters in registers; the points stream through LDS in tiles of GS_EMBQ_TILE_P, every lane reads the same point (a
//                    broadcast, no bank conflict) and counts d2 < threshold. The row itself is counted like any point (d2 = +0) and taken out afterwards.
//  * rank pass     : thresholds = e2, GS_EMBQ_RANK_K slots per launch; k_embq_rank_finish takes the row itself out and marks the unused slots.
//  * radius        : the kq_eff-th smallest d2 of a row, by bracketing its bit pattern from the top: a pass counts the points below the three bounds that
//                    split the open range into four (k_embq_count, K = 3) and k_embq_radius_step appends two bits. 16 passes, no histogram, no list.
//  * blocks        : a launch takes at most GS_EMBQ_MAXQ rows against at most GS_EMBQ_MAXP points (environment, read at every call; unset: all); the counts of the
//                    point blocks add up in the output array (the first block writes, the later ones add: nothing depends on what the array held).
//  * memory        : this unit touches nothing the other units share: its temporaries are allocations of the call (DevBuf, which gs_debug_mem_fill
//                    poisons like any other), its stage times lie in a table of its own, and the context, the scratch pool and their headers are as
//                    they were before it existed.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"

#define GS_EMBQ_RANK_K 8                  // thresholds a lane of the rank pass keeps in registers: knbn slots are taken 8 at a time
#define GS_EMBQ_RADIX_BITS 2              // bits of the radius a bracketing pass decides (3 thresholds in registers); divides 32

namespace gs {

constexpr uint32_t EQ_TQ = GS_EMBQ_TILE_Q, EQ_TP = GS_EMBQ_TILE_P;
constexpr int EQ_RK = GS_EMBQ_RANK_K, EQ_RB = GS_EMBQ_RADIX_BITS, EQ_DIG = (1 << EQ_RB) - 1, EQ_PASSES = 32 / EQ_RB;
static_assert(32 % EQ_RB == 0 && 2 + EQ_PASSES + 2 == GS_EMBQ_TIMES, "the radius passes cover the 32 bits and every stage has its time slot");
enum { EQ_T_EDGE = 0, EQ_T_RANK = 1, EQ_T_RADIUS = 2, EQ_T_FINISH = 2 + EQ_PASSES, EQ_T_SUMMARY = 3 + EQ_PASSES };

__global__ __launch_bounds__(256) void k_embq_finite(const float *__restrict__ y, uint64_t len, uint32_t *__restrict__ err)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < len && (__float_as_uint(y[s]) & 0x7f800000u) == 0x7f800000u) atomicOr(err, 1u);
}

// SPEC 8.1 d2: the squares are never -0, so the sum from +0 is the sum that starts at the first square
template <int D>
__device__ __forceinline__ float embq_d2(const float (&a)[D], const float *__restrict__ b)
{
    float df = a[0] - b[0];
    float s = df * df;
#pragma unroll
    for (int t = 1; t < D; t++) { df = a[t] - b[t]; s = s + df * df; }
    return s;
}

template <int D>
__global__ __launch_bounds__(256) void k_embq_edge(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ cnt, const float *__restrict__ y, uint64_t n,
                                                   uint32_t knbn, float *__restrict__ e2)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n * knbn) return;
    const uint64_t i = s / knbn;
    const uint32_t t = (uint32_t)(s - i * knbn);
    float v = 0.0f;
    if (t < cnt[i]) {
        float yi[D];
#pragma unroll
        for (int u = 0; u < D; u++) yi[u] = y[i * D + u];
        v = embq_d2<D>(yi, y + ids[s] * D);
    }
    e2[s] = v;
}

// out[i * stride + t0 + k] (+)= #{ j in [p0, p1) : bits(d2(i, j)) < thr[i * stride + t0 + k] } for the rows i in [q0, q1) and k < kk <= K
template <int D, int K>
__global__ __launch_bounds__(EQ_TQ) void k_embq_count(const float *__restrict__ y, uint64_t q0, uint64_t q1, uint64_t p0, uint64_t p1,
                                                      const uint32_t *__restrict__ thr, uint32_t stride, uint32_t t0, uint32_t kk, uint32_t *__restrict__ out,
                                                      int add)
{
    __shared__ float pts[EQ_TP * D];
    const uint64_t i = q0 + (uint64_t)blockIdx.x * EQ_TQ + threadIdx.x;
    const bool live = i < q1;
    float yi[D];
    uint32_t th[K], c[K];
#pragma unroll
    for (int t = 0; t < D; t++) yi[t] = live ? y[i * D + t] : 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) { th[k] = live && (uint32_t)k < kk ? thr[i * stride + t0 + k] : 0u; c[k] = 0; }   // a bound of 0 counts nothing
    for (uint64_t base = p0; base < p1; base += EQ_TP) {
        const uint32_t np = p1 - base < EQ_TP ? (uint32_t)(p1 - base) : EQ_TP;
        __syncthreads();                             // the tile before has been read by every wave
        for (uint32_t s = threadIdx.x; s < np * D; s += EQ_TQ) pts[s] = y[base * D + s];
        __syncthreads();
#pragma unroll 4
        for (uint32_t j = 0; j < np; j++) {
            const uint32_t b = __float_as_uint(embq_d2<D>(yi, pts + j * D));
#pragma unroll
            for (int k = 0; k < K; k++) c[k] += b < th[k] ? 1u : 0u;
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < K; k++)
        if ((uint32_t)k < kk) {
            const uint64_t o = i * stride + t0 + k;
            out[o] = add ? out[o] + c[k] : c[k];
        }
}

// the counts include the row itself wherever +0 < e2; an unused slot holds 0xFFFFFFFF
__global__ __launch_bounds__(256) void k_embq_rank_finish(const uint32_t *__restrict__ cnt, const float *__restrict__ e2, uint64_t n, uint32_t knbn,
                                                          uint32_t *__restrict__ rank)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n * knbn) return;
    const uint64_t i = s / knbn;
    rank[s] = (uint32_t)(s - i * knbn) < cnt[i] ? rank[s] - (__float_as_uint(e2[s]) != 0u ? 1u : 0u) : 0xFFFFFFFFu;
}

// digit k of the bits at `shift` below `prefix`: every pattern <= prefix | k << shift | (the bits under shift all set), as a strict bound
__device__ __forceinline__ uint32_t embq_bound(uint32_t prefix, uint32_t k, uint32_t shift) { return (prefix | (k << shift) | ((1u << shift) - 1u)) + 1u; }

__global__ __launch_bounds__(256) void k_embq_radius_init(uint64_t n, uint32_t *__restrict__ prefix, uint32_t *__restrict__ thr)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    prefix[i] = 0;
    for (uint32_t k = 0; k < (uint32_t)EQ_DIG; k++) thr[i * EQ_DIG + k] = embq_bound(0, k, 32 - EQ_RB);
}
// the digit at `shift` of row i's radius is the first whose bound has kq_eff other points below it (the row itself lies below every bound), the last
// digit if none has; then the bounds of the next pass
__global__ __launch_bounds__(256) void k_embq_radius_step(uint64_t n, uint32_t shift, uint32_t kq_eff, const uint32_t *__restrict__ below,
                                                          uint32_t *__restrict__ prefix, uint32_t *__restrict__ thr)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k = 0;
    while (k < (uint32_t)EQ_DIG && below[i * EQ_DIG + k] - 1u < kq_eff) k++;
    const uint32_t p = prefix[i] | (k << shift);
    prefix[i] = p;
    if (shift)
        for (k = 0; k < (uint32_t)EQ_DIG; k++) thr[i * EQ_DIG + k] = embq_bound(p, k, shift - EQ_RB);
}

static inline uint32_t nblk(uint64_t n, uint32_t b = 256) { return (uint32_t)((n + b - 1) / b); }

// rows and points per launch of k_embq_count; read at every call, so that a test reaches several blocks of both at a few hundred nodes
static void embq_blocks(uint64_t *maxq, uint64_t *maxp)
{
    const char *q = getenv("GS_EMBQ_MAXQ"), *p = getenv("GS_EMBQ_MAXP");
    const uint64_t vq = q && *q ? strtoull(q, nullptr, 10) : 0, vp = p && *p ? strtoull(p, nullptr, 10) : 0;
    *maxq = vq ? vq : (uint64_t)1 << 31;          // by default one launch per pass: a second, smaller launch would run behind the first at low occupancy
    *maxp = vp ? vp : (uint64_t)1 << 31;
}

template <int D, int K>
static void count_launch(gs_ctx *c, const float *y, uint64_t n, const uint32_t *thr, uint32_t stride, uint32_t t0, uint32_t kk, uint32_t *out)
{
    uint64_t maxq, maxp;
    embq_blocks(&maxq, &maxp);
    for (uint64_t p0 = 0; p0 < n; p0 += maxp)
        for (uint64_t q0 = 0; q0 < n; q0 += maxq) {
            const uint64_t q1 = std::min(n, q0 + maxq), p1 = std::min(n, p0 + maxp);
            hipLaunchKernelGGL((k_embq_count<D, K>), dim3(nblk(q1 - q0, EQ_TQ)), dim3(EQ_TQ), 0, c->stream, y, q0, q1, p0, p1, thr, stride, t0, kk, out, p0 ? 1 : 0);
        }
}
template <int K>
static void count_pass(gs_ctx *c, uint32_t D, const float *y, uint64_t n, const uint32_t *thr, uint32_t stride, uint32_t t0, uint32_t kk, uint32_t *out)
{
    switch (D) {
    case 1: count_launch<1, K>(c, y, n, thr, stride, t0, kk, out); break;
    case 2: count_launch<2, K>(c, y, n, thr, stride, t0, kk, out); break;
    case 3: count_launch<3, K>(c, y, n, thr, stride, t0, kk, out); break;
    default: count_launch<4, K>(c, y, n, thr, stride, t0, kk, out); break;
    }
}

// the stage times of every context's last call (gs_embed_quality_last_ms); an entry outlives its context, 160 bytes each
struct StageTimes { double ms[GS_EMBQ_TIMES]; };
static std::mutex embq_times_mu;
static std::map<const gs_ctx *, StageTimes> embq_times;
static double *embq_ms_of(const gs_ctx *c)             // (std::map: the address stays valid while other entries come)
{
    std::lock_guard<std::mutex> g(embq_times_mu);
    return embq_times[c].ms;
}

namespace {
// stream events around the stages of a call; read() after the stream has been waited for
struct StageClock {
    gs_ctx *c; double *ms_out;
    hipEvent_t ev[GS_EMBQ_TIMES + 2] = {};
    int stage[GS_EMBQ_TIMES + 2], n = 0;
    StageClock(gs_ctx *ctx, double *out) : c(ctx), ms_out(out) {}
    ~StageClock() { for (int i = 0; i < n; i++) (void)hipEventDestroy(ev[i]); }
    void mark(int next_stage)                   // the stage that begins here; -1 closes the last one
    {
        if (n > (int)GS_EMBQ_TIMES || hipEventCreate(&ev[n]) != hipSuccess) return;
        (void)hipEventRecord(ev[n], c->stream);
        stage[n++] = next_stage;
    }
    void read()
    {
        for (int i = 0; i + 1 < n; i++) {
            float ms = 0.0f;
            if (stage[i] >= 0 && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) ms_out[stage[i]] += (double)ms;
        }
    }
};
}  // namespace

static int quality_args(uint64_t n, uint32_t knbn, uint32_t dim, uint32_t kq)
{
    GS_REQUIRE(knbn >= 1 && knbn <= (uint32_t)KNN_MAX, GS_ERR_INVALID, "knbn must be in 1..%d", (int)KNN_MAX);
    GS_REQUIRE(n < ((uint64_t)1 << 31) && n * knbn < ((uint64_t)1 << 31), GS_ERR_UNSUPPORTED, "graph of %llu x %u entries: at most 2^31", (unsigned long long)n, knbn);
    GS_REQUIRE(n >= 2, GS_ERR_INVALID, "the quality of an embedding needs at least two nodes");
    GS_REQUIRE(kq >= 1, GS_ERR_INVALID, "kq must be at least 1");
    GS_REQUIRE(dim >= 1 && dim <= GS_EMBED_DIM_MAX, GS_ERR_INVALID, "embedding dim must be in 1..%u", (unsigned)GS_EMBED_DIM_MAX);
    return GS_OK;
}

// SPEC 8.1 on a validated device graph and device positions: rank, e2 (n x knbn) and rad2 (n), each optional, all on the device. Waits for the stream
// once (the finiteness flag) before the passes and once at the end.
static int quality_dev(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const uint32_t *cnt, const float *y, uint32_t D, uint32_t kq, uint32_t *rank,
                       float *e2, float *rad2)
{
    int rc;
    const uint64_t nk = n * knbn;
    const uint32_t kq_eff = (uint32_t)std::min<uint64_t>(kq, n - 1);
    double *times = embq_ms_of(c);
    for (uint32_t s = 0; s < GS_EMBQ_TIMES; s++) times[s] = 0.0;
    DevBuf flag, se2, thr, below;
    if ((rc = flag.alloc(16))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(flag.p, 0, 16, c->stream));
    hipLaunchKernelGGL(k_embq_finite, dim3(nblk(n * D)), dim3(256), 0, c->stream, y, n * D, flag.as<uint32_t>());
    GS_HIP_CHECK(hipGetLastError());
    uint32_t err = 0;
    GS_HIP_CHECK(hipMemcpyAsync(&err, flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    GS_REQUIRE(!err, GS_ERR_INVALID, "a coordinate is NaN or infinite");
    StageClock clk(c, times);
    if (rank || e2) {
        if (!e2) { if ((rc = se2.alloc(4 * nk))) return rc; e2 = se2.as<float>(); }
        clk.mark(EQ_T_EDGE);
        switch (D) {
        case 1: hipLaunchKernelGGL(k_embq_edge<1>, dim3(nblk(nk)), dim3(256), 0, c->stream, ids, cnt, y, n, knbn, e2); break;
        case 2: hipLaunchKernelGGL(k_embq_edge<2>, dim3(nblk(nk)), dim3(256), 0, c->stream, ids, cnt, y, n, knbn, e2); break;
        case 3: hipLaunchKernelGGL(k_embq_edge<3>, dim3(nblk(nk)), dim3(256), 0, c->stream, ids, cnt, y, n, knbn, e2); break;
        default: hipLaunchKernelGGL(k_embq_edge<4>, dim3(nblk(nk)), dim3(256), 0, c->stream, ids, cnt, y, n, knbn, e2); break;
        }
        GS_HIP_CHECK(hipGetLastError());
    }
    if (rank) {
        clk.mark(EQ_T_RANK);
        for (uint32_t t0 = 0; t0 < knbn; t0 += EQ_RK)
            count_pass<EQ_RK>(c, D, y, n, (const uint32_t *)e2, knbn, t0, std::min<uint32_t>(EQ_RK, knbn - t0), rank);
        clk.mark(EQ_T_FINISH);
        hipLaunchKernelGGL(k_embq_rank_finish, dim3(nblk(nk)), dim3(256), 0, c->stream, cnt, e2, n, knbn, rank);
        GS_HIP_CHECK(hipGetLastError());
    }
    if (rad2) {
        if ((rc = thr.alloc(4 * n * EQ_DIG)) || (rc = below.alloc(4 * n * EQ_DIG))) return rc;
        uint32_t *prefix = (uint32_t *)rad2;                 // the radius is built in place: its bit pattern, from the top
        clk.mark(-1);
        hipLaunchKernelGGL(k_embq_radius_init, dim3(nblk(n)), dim3(256), 0, c->stream, n, prefix, thr.as<uint32_t>());
        for (int pass = 0; pass < EQ_PASSES; pass++) {
            clk.mark(EQ_T_RADIUS + pass);
            count_pass<EQ_DIG>(c, D, y, n, thr.as<uint32_t>(), EQ_DIG, 0, EQ_DIG, below.as<uint32_t>());
            hipLaunchKernelGGL(k_embq_radius_step, dim3(nblk(n)), dim3(256), 0, c->stream, n, (uint32_t)(32 - EQ_RB * (pass + 1)), kq_eff, below.as<uint32_t>(), prefix,
                               thr.as<uint32_t>());
        }
        GS_HIP_CHECK(hipGetLastError());
    }
    clk.mark(-1);
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    clk.read();
    return GS_OK;
}

static const double EQ_Q[7] = {0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99};
static void quantiles(std::vector<double> &v, double *q)
{
    std::sort(v.begin(), v.end());
    const uint64_t N = v.size();
    for (int k = 0; k < 7; k++) q[k] = N ? v[(uint64_t)(EQ_Q[k] * (double)(N - 1))] : NAN;
}

// SPEC 8.1 "Summary", in f64 from the three arrays
static void summarise(uint64_t n, uint32_t knbn, uint32_t kq_eff, const uint32_t *cnt, const uint32_t *rank, const float *e2, const float *rad2,
                      gs_embed_quality_summary *out, uint64_t *hist)
{
    gs_embed_quality_summary s;
    memset(&s, 0, sizeof(s));
    s.n = n; s.knbn = knbn; s.kq_eff = kq_eff;
    if (hist) for (uint32_t b = 0; b <= knbn; b++) hist[b] = 0;
    std::vector<double> edge, radius, ratio;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t c = cnt[i];
        if (!c) continue;
        uint32_t ci = 0;
        float emax2 = 0.0f;
        for (uint32_t t = 0; t < c; t++) {
            if (rank[i * knbn + t] < kq_eff) ci++;
            emax2 = std::max(emax2, e2[i * knbn + t]);
        }
        s.n_rows++; s.n_edges += c; s.n_conserved += ci;
        if (!ci) s.n_nomatch++;
        if (hist) hist[ci]++;
        const double a = (double)emax2, b = (double)rad2[i];
        edge.push_back(std::sqrt(a));
        radius.push_back(std::sqrt(b));
        ratio.push_back((a == 0.0 && b == 0.0) || (std::isinf(a) && std::isinf(b)) ? 1.0 : (b == 0.0 ? (double)INFINITY : std::sqrt(a / b)));
    }
    s.mean_conserved = s.n_rows > s.n_nomatch ? (double)s.n_conserved / (double)(s.n_rows - s.n_nomatch) : 0.0;
    s.frac_conserved = s.n_edges ? (double)s.n_conserved / (double)s.n_edges : (double)NAN;
    quantiles(edge, s.q_edge);
    quantiles(radius, s.q_radius);
    quantiles(ratio, s.q_ratio);
    *out = s;
}

int embed_quality_graph(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *dids, const float *ddist, const uint32_t *dcnt, const float *pos, uint32_t dim,
                        uint32_t kq, gs_embed_quality_summary *summary, uint64_t *hist_out, uint32_t *rank_out, float *e2_out, float *rad2_out)
{
    (void)ddist;
    int rc;
    if ((rc = quality_args(n, knbn, dim, kq))) return rc;
    const uint64_t nk = n * knbn;
    DevBuf dpos, drank, de2, drad;
    if ((rc = dpos.alloc(4 * n * dim)) || (rc = drank.alloc(4 * nk)) || (rc = de2.alloc(4 * nk)) || (rc = drad.alloc(4 * n))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dpos.p, pos, 4 * n * dim, hipMemcpyHostToDevice, c->stream));
    if ((rc = quality_dev(c, n, knbn, dids, dcnt, dpos.as<float>(), dim, kq, drank.as<uint32_t>(), de2.as<float>(), drad.as<float>()))) return rc;
    std::vector<uint32_t> hc(n), hrank(rank_out ? 0 : nk);
    std::vector<float> he2(e2_out ? 0 : nk), hrad(rad2_out ? 0 : n);
    uint32_t *rk = rank_out ? rank_out : hrank.data();
    float *e2 = e2_out ? e2_out : he2.data(), *rad = rad2_out ? rad2_out : hrad.data();
    GS_HIP_CHECK(hipMemcpyAsync(hc.data(), dcnt, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(rk, drank.p, 4 * nk, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(e2, de2.p, 4 * nk, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(rad, drad.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    summarise(n, knbn, (uint32_t)std::min<uint64_t>(kq, n - 1), hc.data(), rk, e2, rad, summary, hist_out);
    embq_ms_of(c)[EQ_T_SUMMARY] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GS_OK;
}

}  // namespace gs

extern "C" {

int gs_embed_quality(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *count, const float *pos, uint32_t dim,
                     uint32_t kq, gs_embed_quality_summary *summary_out, uint64_t *hist_out, uint32_t *rank_out, float *e2_out, float *rad2_out)
{
    GS_REQUIRE(c, GS_ERR_INVALID, "null context");
    int rc;
    if ((rc = gs::quality_args(n, knbn, dim, kq))) return rc;
    GS_REQUIRE(ids && dist && count && pos && summary_out, GS_ERR_INVALID, "null argument");
    GS_CTX_LOCK(c);
    gs::DevBuf a, b, d;
    if ((rc = a.alloc(8 * n * knbn)) || (rc = b.alloc(4 * n * knbn)) || (rc = d.alloc(4 * n))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(a.p, ids, 8 * n * knbn, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(b.p, dist, 4 * n * knbn, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(d.p, count, 4 * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = gs::embed_validate(c, n, knbn, a.as<uint64_t>(), b.as<float>(), d.as<uint32_t>()))) return rc;
    return gs::embed_quality_graph(c, n, knbn, a.as<uint64_t>(), b.as<float>(), d.as<uint32_t>(), pos, dim, kq, summary_out, hist_out, rank_out, e2_out, rad2_out);
}

int gs_embed_quality_dev(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids_dev, const float *dist_dev, const uint32_t *count_dev, const float *pos_dev,
                         uint32_t dim, uint32_t kq, uint32_t *rank_out_dev, float *e2_out_dev, float *rad2_out_dev)
{
    GS_REQUIRE(c, GS_ERR_INVALID, "null context");
    int rc;
    if ((rc = gs::quality_args(n, knbn, dim, kq))) return rc;
    GS_REQUIRE(ids_dev && dist_dev && count_dev && pos_dev, GS_ERR_INVALID, "null argument");
    GS_CTX_LOCK(c);
    if ((rc = gs::embed_validate(c, n, knbn, ids_dev, dist_dev, count_dev))) return rc;
    return gs::quality_dev(c, n, knbn, ids_dev, count_dev, pos_dev, dim, kq, rank_out_dev, e2_out_dev, rad2_out_dev);
}

int gs_embed_quality_last_ms(gs_ctx *c, double *ms_out)
{
    GS_REQUIRE(c && ms_out, GS_ERR_INVALID, "null argument");
    GS_CTX_LOCK(c);
    memcpy(ms_out, gs::embq_ms_of(c), sizeof(double) * GS_EMBQ_TIMES);
    return GS_OK;
}

}  // extern "C"
