// gs_embed.hip — upstream's `ann` subcommand (src/utils/embed.rs of the reference): statistics of the k-NN graph and a UMAP-like 2-D embedding
// of it, bit-exact and reproducible (SPEC.md 8; constants in gs_spec.hpp). No float atomics anywhere: every sum has one pinned order.
//
//  * k_embed_check : one thread per row; the input rules of SPEC 8 (ids < n, no self, no repeat, distances >= 0 and ascending).
//  * k_embed_memb  : calibration, one thread per row in f64: rho, sigma by bisection, memberships p (SPEC 2 EXP).
//  * k_embed_occ   : k-occurrence by integer atomics (the count does not depend on their order).
//  * adjacency     : (target << 32 | source) keys through the stable radix sort; per node its range of sources (k_embed_deg), the offsets
//                    (k_embed_scan, one workgroup), then k_embed_fill writes (node u32, weight f32): the own row in row order, then the sources
//                    whose row holds the node and that its own row does not hold, ascending. Nodes longer than L_H go to a list (heavy).
//  * epochs        : Jacobi steps between two position buffers. k_embed_light sums a node's attraction-then-negative sequence in one thread;
//                    k_embed_heavy gives a heavy node one wavefront: lane l sums entries l, l+64, ..., and the 64 partials fold by a fixed halving tree.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"

namespace gs {

constexpr uint32_t EMB_LH = GS_EMBED_LIGHT;
enum { EMB_BAD_COUNT = 1, EMB_BAD_ID = 2, EMB_BAD_SELF = 4, EMB_BAD_REPEAT = 8, EMB_BAD_DIST = 16 };

__global__ __launch_bounds__(256) void k_embed_check(const uint64_t *__restrict__ ids, const float *__restrict__ dist, const uint32_t *__restrict__ cnt,
                                                     uint64_t n, uint32_t knbn, uint32_t *__restrict__ err)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i];
    if (c > knbn) { atomicOr(err, (uint32_t)EMB_BAD_COUNT); return; }
    const uint64_t *row = ids + i * knbn;
    const float *d = dist + i * knbn;
    uint32_t bad = 0;
    for (uint32_t t = 0; t < c; t++) {
        const uint64_t j = row[t];
        if (j >= n) bad |= EMB_BAD_ID;
        if (j == i) bad |= EMB_BAD_SELF;
        if (!(d[t] >= 0.0f) || (t > 0 && d[t] < d[t - 1])) bad |= EMB_BAD_DIST;
        for (uint32_t u = 0; u < t; u++) if (row[u] == j) bad |= EMB_BAD_REPEAT;
    }
    if (bad) atomicOr(err, bad);
}

// SPEC 8 calibration of row i (f64): memb[i][t] for t < count, 0 beyond
__global__ __launch_bounds__(256) void k_embed_memb(const float *__restrict__ dist, const uint32_t *__restrict__ cnt, uint64_t n, uint32_t knbn, float *__restrict__ memb)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i];
    const float *d = dist + i * knbn;
    float *p = memb + i * knbn;
    for (uint32_t t = c; t < knbn; t++) p[t] = 0.0f;
    if (c == 0) return;
    if (c == 1) { p[0] = 1.0f; return; }
    double rho = 0.0;
    for (uint32_t t = 0; t < c; t++) if (d[t] > 0.0f) { rho = (double)d[t]; break; }
    const double target = spec_ln((double)c) / spec_ln(2.0);
    double lo = 0.0, hi = 0.0, mid = 1.0;
    bool hi_inf = true;
    for (int it = 0; it < GS_EMBED_BISECT; it++) {
        double ps = 0.0;
        for (uint32_t t = 0; t < c; t++) {
            const double dd = (double)d[t] - rho;
            ps = ps + (dd > 0.0 ? spec_exp(-(dd / mid)) : 1.0);
        }
        if (fabs(ps - target) < GS_EMBED_TOL) break;
        if (ps > target) { hi = mid; hi_inf = false; mid = (lo + hi) / 2.0; }
        else { lo = mid; mid = hi_inf ? mid * 2.0 : (lo + hi) / 2.0; }
    }
    double mean = 0.0;
    for (uint32_t t = 0; t < c; t++) mean = mean + (double)d[t];
    mean = mean / (double)c;
    if (mid < GS_EMBED_MIN_SCALE * mean) mid = GS_EMBED_MIN_SCALE * mean;
    for (uint32_t t = 0; t < c; t++) {
        const double dd = (double)d[t] - rho;
        p[t] = (float)(dd > 0.0 ? spec_exp(-(dd / mid)) : 1.0);
    }
}

__global__ __launch_bounds__(256) void k_embed_occ(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ cnt, uint64_t n, uint32_t knbn, uint32_t *__restrict__ occ)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (uint32_t t = 0; t < cnt[i]; t++) atomicAdd(&occ[ids[i * knbn + t]], 1u);
}

// the first and the last kept distance of every row (rows with count 0: +inf, not read)
__global__ __launch_bounds__(256) void k_embed_ends(const float *__restrict__ dist, const uint32_t *__restrict__ cnt, uint64_t n, uint32_t knbn, float *__restrict__ ends)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i];
    ends[2 * i] = c ? dist[i * knbn] : INFINITY;
    ends[2 * i + 1] = c ? dist[i * knbn + c - 1] : INFINITY;
}

// one key per slot: (target << 32 | source) for kept entries, (n << 32) (after every target) for the unused ones
__global__ __launch_bounds__(256) void k_embed_keys(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ cnt, uint64_t n, uint32_t knbn, uint64_t *__restrict__ keys)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n * knbn) return;
    const uint64_t i = s / knbn;
    const uint32_t t = (uint32_t)(s - i * knbn);
    keys[s] = t < cnt[i] ? (ids[s] << 32) | i : n << 32;
}

__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t *a, uint64_t len, uint64_t key)
{
    uint64_t lo = 0, hi = len;
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (a[m] < key) lo = m + 1; else hi = m; }
    return lo;
}
// slot of node j in row i, or -1
__device__ __forceinline__ int row_slot(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ cnt, uint32_t knbn, uint64_t i, uint64_t j)
{
    const uint64_t *row = ids + i * knbn;
    for (uint32_t t = 0; t < cnt[i]; t++) if (row[t] == j) return (int)t;
    return -1;
}

// per node: its range of sorted reverse keys, and the length of its adjacency; heavy nodes are listed (in any order: each is written by one wave)
__global__ __launch_bounds__(256) void k_embed_deg(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ cnt, uint64_t n, uint32_t knbn,
                                                   const uint64_t *__restrict__ sorted, uint64_t *__restrict__ range, uint32_t *__restrict__ deg,
                                                   uint32_t *__restrict__ heavy, uint32_t *__restrict__ n_heavy)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t nk = n * knbn;
    const uint64_t b = lower_bound_u64(sorted, nk, j << 32), e = lower_bound_u64(sorted, nk, (j + 1) << 32);
    range[2 * j] = b; range[2 * j + 1] = e;
    uint32_t d = cnt[j];
    for (uint64_t k = b; k < e; k++) if (row_slot(ids, cnt, knbn, j, (uint32_t)sorted[k]) < 0) d++;
    deg[j] = d;
    if (d > EMB_LH) heavy[atomicAdd(n_heavy, 1u)] = (uint32_t)j;
}

// off[0..n] = exclusive prefix sum of deg (one workgroup: lanes take contiguous stretches)
__global__ __launch_bounds__(1024) void k_embed_scan(const uint32_t *__restrict__ deg, uint64_t n, uint64_t *__restrict__ off)
{
    __shared__ uint64_t part[1024];
    const uint64_t per = (n + 1023) / 1024, b = (uint64_t)threadIdx.x * per, e = b + per < n ? b + per : n;
    uint64_t s = 0;
    for (uint64_t i = b; i < e; i++) s += deg[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    s = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t i = b; i < e; i++) { off[i] = s; s += deg[i]; }
    if (threadIdx.x == 1023) off[n] = part[1023];
}

// CSR of node i: own row (row order), then the reverse-only sources ascending; weight (p_ij + p_ji) - p_ij p_ji; Wsum[i] in adjacency order
__global__ __launch_bounds__(256) void k_embed_fill(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ cnt, const float *__restrict__ memb, uint64_t n,
                                                    uint32_t knbn, const uint64_t *__restrict__ sorted, const uint64_t *__restrict__ range,
                                                    const uint64_t *__restrict__ off, uint32_t *__restrict__ adj, float *__restrict__ w, float *__restrict__ Wsum)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t o = off[i];
    float W = 0.0f;
    for (uint32_t t = 0; t < cnt[i]; t++) {
        const uint64_t j = ids[i * knbn + t];
        const float pij = memb[i * knbn + t];
        const int u = row_slot(ids, cnt, knbn, j, i);
        const float pji = u < 0 ? 0.0f : memb[j * knbn + u];
        const float x = (pij + pji) - pij * pji;
        adj[o] = (uint32_t)j; w[o] = x; o++;
        W = W + x;
    }
    for (uint64_t k = range[2 * i]; k < range[2 * i + 1]; k++) {
        const uint64_t s = (uint32_t)sorted[k];
        if (row_slot(ids, cnt, knbn, i, s) >= 0) continue;
        const float pij = 0.0f, pji = memb[s * knbn + row_slot(ids, cnt, knbn, s, i)];
        const float x = (pij + pji) - pij * pji;
        adj[o] = (uint32_t)s; w[o] = x; o++;
        W = W + x;
    }
    Wsum[i] = W;
}

__global__ __launch_bounds__(256) void k_embed_init(uint64_t n, uint32_t dim, uint64_t seed, float *__restrict__ y)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n * dim) return;
    const uint64_t i = s / dim;
    y[s] = embed_init_coord(seed, i, dim, (uint32_t)(s - i * dim));
}

__device__ __forceinline__ float emb_clamp(float x) { return x > GS_EMBED_CLAMP ? GS_EMBED_CLAMP : (x < -GS_EMBED_CLAMP ? -GS_EMBED_CLAMP : x); }

// entry k of node i's combined sequence (k < deg: attraction to adjacency entry b + k; else negative sample k - deg) added into acc
template <int D>
__device__ __forceinline__ void emb_term(const float *__restrict__ y, const float (&yi)[D], const uint32_t *__restrict__ adj, const float *__restrict__ w,
                                         uint64_t b, uint32_t deg, uint32_t k, uint64_t i, uint64_t n, uint32_t S, float g2, uint64_t ekey, float (&acc)[D])
{
    uint64_t j;
    float wk = 0.0f;
    const bool att = k < deg;
    if (att) { j = adj[b + k]; wk = w[b + k]; }
    else {
        j = embed_neg(ekey, i, S, k - deg, n);
        if (j == i) return;
    }
    float diff[D];
#pragma unroll
    for (int t = 0; t < D; t++) diff[t] = yi[t] - y[j * D + t];
    float d2 = diff[0] * diff[0];
#pragma unroll
    for (int t = 1; t < D; t++) d2 = d2 + diff[t] * diff[t];
    const float c = att ? (-2.0f * wk) / (1.0f + d2) : g2 / ((GS_EMBED_EPS + d2) * (1.0f + d2));
#pragma unroll
    for (int t = 0; t < D; t++) acc[t] = acc[t] + emb_clamp(c * diff[t]);
}

template <int D>
__global__ __launch_bounds__(256) void k_embed_light(const float *__restrict__ y, float *__restrict__ yn, const uint64_t *__restrict__ off, const uint32_t *__restrict__ adj,
                                                     const float *__restrict__ w, const float *__restrict__ Wsum, uint64_t n, uint32_t S, float rate, float lr_e, uint64_t ekey)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = off[i];
    const uint32_t deg = (uint32_t)(off[i + 1] - b);
    if (deg > EMB_LH) return;
    float yi[D], acc[D];
#pragma unroll
    for (int t = 0; t < D; t++) { yi[t] = y[i * D + t]; acc[t] = 0.0f; }
    const float g2 = 2.0f * ((rate * Wsum[i]) / (float)S);
    for (uint32_t k = 0; k < deg + S; k++) emb_term<D>(y, yi, adj, w, b, deg, k, i, n, S, g2, ekey, acc);
#pragma unroll
    for (int t = 0; t < D; t++) yn[i * D + t] = yi[t] + lr_e * acc[t];
}

template <int D>
__global__ __launch_bounds__(256) void k_embed_heavy(const float *__restrict__ y, float *__restrict__ yn, const uint64_t *__restrict__ off, const uint32_t *__restrict__ adj,
                                                     const float *__restrict__ w, const float *__restrict__ Wsum, const uint32_t *__restrict__ heavy, uint32_t nh, uint64_t n,
                                                     uint32_t S, float rate, float lr_e, uint64_t ekey)
{
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= nh) return;                  // whole wavefronts leave together
    const uint64_t i = heavy[h], b = off[i];
    const uint32_t deg = (uint32_t)(off[i + 1] - b);
    float yi[D], acc[D];
#pragma unroll
    for (int t = 0; t < D; t++) { yi[t] = y[i * D + t]; acc[t] = 0.0f; }
    const float g2 = 2.0f * ((rate * Wsum[i]) / (float)S);
    for (uint32_t k = lane; k < deg + S; k += 64) emb_term<D>(y, yi, adj, w, b, deg, k, i, n, S, g2, ekey, acc);
#pragma unroll
    for (uint32_t o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int t = 0; t < D; t++) acc[t] = acc[t] + __shfl_down(acc[t], o, 64);
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < D; t++) yn[i * D + t] = yi[t] + lr_e * acc[t];
    }
}

static inline uint32_t nblk(uint64_t n, uint32_t b = 256) { return (uint32_t)((n + b - 1) / b); }

static int embed_check_params(const gs_embed_params *p)
{
    GS_REQUIRE(p->dim >= 1 && p->dim <= GS_EMBED_DIM_MAX, GS_ERR_INVALID, "embedding dim must be in 1..%u", (unsigned)GS_EMBED_DIM_MAX);
    GS_REQUIRE(p->neg_samples >= 1 && p->neg_samples <= 65535, GS_ERR_INVALID, "neg_samples must be in 1..65535");
    GS_REQUIRE(p->neg_rate >= 0.0f && p->lr >= 0.0f && std::isfinite(p->neg_rate) && std::isfinite(p->lr), GS_ERR_INVALID, "neg_rate and lr must be finite and >= 0");
    return GS_OK;
}
static int graph_args(uint64_t n, uint32_t knbn)
{
    GS_REQUIRE(knbn >= 1 && knbn <= (uint32_t)KNN_MAX, GS_ERR_INVALID, "knbn must be in 1..%d", (int)KNN_MAX);
    GS_REQUIRE(n < ((uint64_t)1 << 31) && n * knbn < ((uint64_t)1 << 31), GS_ERR_UNSUPPORTED, "graph of %llu x %u entries: at most 2^31", (unsigned long long)n, knbn);
    return GS_OK;
}
// the input rules of SPEC 8 on device arrays (waits for the stream)
int embed_validate(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *cnt)
{
    PoolBuf e(c, SL_EMB_FLAG);
    int rc;
    if ((rc = e.alloc(16))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(e.p, 0, 16, c->stream));
    hipLaunchKernelGGL(k_embed_check, dim3(nblk(n)), dim3(256), 0, c->stream, ids, dist, cnt, n, knbn, e.as<uint32_t>());
    GS_HIP_CHECK(hipGetLastError());
    uint32_t err = 0;
    GS_HIP_CHECK(hipMemcpyAsync(&err, e.p, 4, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    GS_REQUIRE(!(err & EMB_BAD_COUNT), GS_ERR_INVALID, "a row count exceeds knbn");
    GS_REQUIRE(!(err & EMB_BAD_ID), GS_ERR_INVALID, "a neighbour id is not a node number < n");
    GS_REQUIRE(!(err & EMB_BAD_SELF), GS_ERR_INVALID, "a row holds its own node");
    GS_REQUIRE(!(err & EMB_BAD_REPEAT), GS_ERR_INVALID, "a row holds a node twice");
    GS_REQUIRE(!(err & EMB_BAD_DIST), GS_ERR_INVALID, "a distance is NaN, negative or smaller than the one before it");
    return GS_OK;
}

// SPEC 8 on a validated device graph: positions (n x dim) to pos (device); init (device, optional) replaces the seeded draw; memb (device, optional).
// Waits for the stream once before the epochs (the number of heavy nodes sizes their launch) and once at the end.
static int embed_graph_dev(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *cnt, const gs_embed_params *p,
                    const float *init, float *pos, float *memb_out)
{
    const uint32_t D = p->dim;
    int rc;
    PoolBuf pm(c, SL_EMB_PM), keys(c, SL_EMB_KEYS), alt(c, SL_EMB_ALT), rs(c, SL_EMB_RADIX), range(c, SL_EMB_RANGE), deg(c, SL_EMB_DEG), off(c, SL_EMB_OFF), adj(c, SL_EMB_ADJ), w(c, SL_EMB_W), W(c, SL_EMB_WSUM), heavy(c, SL_EMB_HEAVY), y0(c, SL_EMB_Y0),
        y1(c, SL_EMB_Y1), nh(c, SL_EMB_FLAG);
    const uint64_t nk = n * knbn;
    if ((rc = nh.alloc(16)) || (rc = keys.alloc(8 * nk)) || (rc = alt.alloc(8 * nk)) || (rc = rs.alloc(radix_scratch_bytes(nk))) || (rc = range.alloc(16 * n)) ||
        (rc = deg.alloc(4 * n)) || (rc = off.alloc(8 * (n + 1))) || (rc = adj.alloc(8 * nk)) || (rc = w.alloc(8 * nk)) || (rc = W.alloc(4 * n)) ||
        (rc = heavy.alloc(4 * n)) || (rc = y0.alloc(4 * n * D)) || (rc = y1.alloc(4 * n * D)))
        return rc;
    float *mb = memb_out;
    if (!mb) { if ((rc = pm.alloc(4 * nk))) return rc; mb = pm.as<float>(); }
    hipLaunchKernelGGL(k_embed_memb, dim3(nblk(n)), dim3(256), 0, c->stream, dist, cnt, n, knbn, mb);
    hipLaunchKernelGGL(k_embed_keys, dim3(nblk(nk)), dim3(256), 0, c->stream, ids, cnt, n, knbn, keys.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    int endbit = 32;
    while (endbit < 64 && (n >> (endbit - 32))) endbit++;
    uint64_t *sorted = nullptr;
    if ((rc = radix_sort_u64(c, keys.as<uint64_t>(), alt.as<uint64_t>(), nk, endbit, rs.p, &sorted))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(nh.p, 0, 4, c->stream));
    hipLaunchKernelGGL(k_embed_deg, dim3(nblk(n)), dim3(256), 0, c->stream, ids, cnt, n, knbn, sorted, range.as<uint64_t>(), deg.as<uint32_t>(),
                       heavy.as<uint32_t>(), nh.as<uint32_t>());
    hipLaunchKernelGGL(k_embed_scan, dim3(1), dim3(1024), 0, c->stream, deg.as<uint32_t>(), n, off.as<uint64_t>());
    hipLaunchKernelGGL(k_embed_fill, dim3(nblk(n)), dim3(256), 0, c->stream, ids, cnt, mb, n, knbn, sorted, range.as<uint64_t>(), off.as<uint64_t>(),
                       adj.as<uint32_t>(), w.as<float>(), W.as<float>());
    if (init) GS_HIP_CHECK(hipMemcpyAsync(y0.p, init, 4 * n * D, hipMemcpyDeviceToDevice, c->stream));
    else hipLaunchKernelGGL(k_embed_init, dim3(nblk(n * D)), dim3(256), 0, c->stream, n, D, p->seed, y0.as<float>());
    GS_HIP_CHECK(hipGetLastError());
    uint32_t n_heavy = 0;
    GS_HIP_CHECK(hipMemcpyAsync(&n_heavy, nh.p, 4, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    float *ya = y0.as<float>(), *yb = y1.as<float>();
    const uint32_t E = p->epochs, S = p->neg_samples;
    for (uint32_t e = 0; e < E; e++) {
        const float lr_e = p->lr * ((float)(E - e) / (float)E);
        const uint64_t ekey = embed_epoch_key(p->seed, e);
#define GS_EMBED_EPOCH(DD)                                                                                                                                   \
    hipLaunchKernelGGL(k_embed_light<DD>, dim3(nblk(n)), dim3(256), 0, c->stream, ya, yb, off.as<uint64_t>(), adj.as<uint32_t>(), w.as<float>(), W.as<float>(), \
                       n, S, p->neg_rate, lr_e, ekey);                                                                                                        \
    if (n_heavy)                                                                                                                                             \
        hipLaunchKernelGGL(k_embed_heavy<DD>, dim3((n_heavy + 3) / 4), dim3(256), 0, c->stream, ya, yb, off.as<uint64_t>(), adj.as<uint32_t>(), w.as<float>(), \
                           W.as<float>(), heavy.as<uint32_t>(), n_heavy, n, S, p->neg_rate, lr_e, ekey);
        switch (D) {
        case 1: GS_EMBED_EPOCH(1) break;
        case 2: GS_EMBED_EPOCH(2) break;
        case 3: GS_EMBED_EPOCH(3) break;
        default: GS_EMBED_EPOCH(4) break;
        }
#undef GS_EMBED_EPOCH
        GS_HIP_CHECK(hipGetLastError());
        std::swap(ya, yb);
    }
    GS_HIP_CHECK(hipMemcpyAsync(pos, ya, 4 * n * D, hipMemcpyDeviceToDevice, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

// k-occurrence on the device, the rest of SPEC 8's statistics on the host from occ, counts and each row's first / last distance
int knn_stats_dev(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *cnt, gs_knn_stats *st, uint32_t *occ_out,
                  uint64_t *hist_out)
{
    int rc;
    PoolBuf docc(c, SL_KST_OCC), dends(c, SL_KST_ENDS);
    if ((rc = docc.alloc(4 * n)) || (rc = dends.alloc(8 * n))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(docc.p, 0, 4 * n, c->stream));
    hipLaunchKernelGGL(k_embed_occ, dim3(nblk(n)), dim3(256), 0, c->stream, ids, cnt, n, knbn, docc.as<uint32_t>());
    hipLaunchKernelGGL(k_embed_ends, dim3(nblk(n)), dim3(256), 0, c->stream, dist, cnt, n, knbn, dends.as<float>());
    GS_HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> occ(n), hc(n);
    std::vector<float> ends(2 * n);
    GS_HIP_CHECK(hipMemcpyAsync(occ.data(), docc.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(hc.data(), cnt, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(ends.data(), dends.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    gs_knn_stats s;
    memset(&s, 0, sizeof(s));
    s.n = n; s.knbn = knbn;
    std::vector<float> first, last;
    for (uint64_t i = 0; i < n; i++) {
        s.n_edges += hc[i];
        if (hc[i] == 0) s.n_empty++;
        else { first.push_back(ends[2 * i]); last.push_back(ends[2 * i + 1]); }
        s.max_occ = std::max(s.max_occ, occ[i]);
    }
    const double mean = n ? (double)s.n_edges / (double)n : 0.0;
    double m2 = 0.0, m3 = 0.0;
    for (uint64_t i = 0; i < n; i++) { const double dv = (double)occ[i] - mean; m2 = m2 + dv * dv; m3 = m3 + (dv * dv) * dv; }
    s.occ_mean = mean;
    s.occ_std = n ? std::sqrt(m2 / (double)n) : 0.0;
    s.occ_skew = s.occ_std > 0.0 ? (m3 / (double)n) / (s.occ_std * s.occ_std * s.occ_std) : 0.0;
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    const uint64_t nh = std::min<uint64_t>(n, GS_EMBED_HUBS);
    std::partial_sort(order.begin(), order.begin() + nh, order.end(), [&](uint32_t a, uint32_t b) { return occ[a] != occ[b] ? occ[a] > occ[b] : a < b; });
    for (uint32_t h = 0; h < GS_EMBED_HUBS; h++) { s.hub_ids[h] = h < nh ? order[h] : ~(uint64_t)0; s.hub_occ[h] = h < nh ? occ[order[h]] : 0; }
    std::sort(first.begin(), first.end());
    std::sort(last.begin(), last.end());
    static const double Q[7] = {0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99};
    for (int q = 0; q < 7; q++) {
        const uint64_t N = first.size();
        const uint64_t k = N ? (uint64_t)(Q[q] * (double)(N - 1)) : 0;
        s.q_first[q] = N ? first[k] : NAN;
        s.q_last[q] = N ? last[k] : NAN;
    }
    *st = s;
    if (occ_out) memcpy(occ_out, occ.data(), 4 * n);
    if (hist_out) {
        for (uint32_t b = 0; b <= GS_EMBED_HIST_BINS; b++) hist_out[b] = 0;
        for (uint64_t i = 0; i < n; i++) hist_out[std::min<uint32_t>(occ[i], GS_EMBED_HIST_BINS)]++;
    }
    return GS_OK;
}

// a caller's graph (host or device arrays) in pooled device buffers 94-96, validated
static int graph_in(gs_ctx *c, bool on_dev, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *cnt, const uint64_t **dids,
                    const float **ddist, const uint32_t **dcnt)
{
    int rc;
    if (on_dev) { *dids = ids; *ddist = dist; *dcnt = cnt; }
    else {
        PoolBuf a(c, SL_EMBIN_IDS), b(c, SL_EMBIN_DIST), d(c, SL_EMBIN_COUNT);
        if ((rc = a.alloc(8 * n * knbn)) || (rc = b.alloc(4 * n * knbn)) || (rc = d.alloc(4 * n))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(a.p, ids, 8 * n * knbn, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(b.p, dist, 4 * n * knbn, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(d.p, cnt, 4 * n, hipMemcpyHostToDevice, c->stream));
        *dids = a.as<uint64_t>(); *ddist = b.as<float>(); *dcnt = d.as<uint32_t>();
    }
    return embed_validate(c, n, knbn, *dids, *ddist, *dcnt);
}

// host or device caller arrays around embed_graph_dev (the graph already in device buffers)
int embed_common(gs_ctx *c, bool on_dev, uint64_t n, uint32_t knbn, const uint64_t *dids, const float *ddist, const uint32_t *dcnt, const gs_embed_params *prm,
                 const float *init, float *pos_out, float *memb_out)
{
    const gs_embed_params p = prm ? *prm : gs_embed_params_default();
    int rc;
    if ((rc = embed_check_params(&p))) return rc;
    const uint64_t D = p.dim;
    PoolBuf dinit(c, SL_EMB_INIT), dpos(c, SL_EMB_POS), dmemb(c, SL_EMB_MEMB);
    const float *ip = init;
    float *pp = pos_out, *mp = memb_out;
    if (!on_dev) {
        if (init) {
            if ((rc = dinit.alloc(4 * n * D))) return rc;
            GS_HIP_CHECK(hipMemcpyAsync(dinit.p, init, 4 * n * D, hipMemcpyHostToDevice, c->stream));
            ip = dinit.as<float>();
        }
        if ((rc = dpos.alloc(4 * n * D))) return rc;
        pp = dpos.as<float>();
        if (memb_out) { if ((rc = dmemb.alloc(4 * n * knbn))) return rc; mp = dmemb.as<float>(); }
    }
    if ((rc = embed_graph_dev(c, n, knbn, dids, ddist, dcnt, &p, ip, pp, mp))) return rc;
    if (!on_dev) {
        GS_HIP_CHECK(hipMemcpyAsync(pos_out, pp, 4 * n * D, hipMemcpyDeviceToHost, c->stream));
        if (memb_out) GS_HIP_CHECK(hipMemcpyAsync(memb_out, mp, 4 * n * knbn, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    return GS_OK;
}

static int embed_knn_graph_common(gs_ctx *c, bool on_dev, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *cnt,
                                  const gs_embed_params *prm, const float *init, float *pos_out, float *memb_out)
{
    GS_REQUIRE(c, GS_ERR_INVALID, "null context");
    int rc;
    if ((rc = graph_args(n, knbn))) return rc;
    if (n == 0) return GS_OK;
    GS_REQUIRE(ids && dist && cnt && pos_out, GS_ERR_INVALID, "null argument");
    GS_CTX_LOCK(c);
    const uint64_t *dids; const float *ddist; const uint32_t *dcnt;
    if ((rc = graph_in(c, on_dev, n, knbn, ids, dist, cnt, &dids, &ddist, &dcnt))) return rc;
    return embed_common(c, on_dev, n, knbn, dids, ddist, dcnt, prm, init, pos_out, memb_out);
}

}  // namespace gs

extern "C" {

gs_embed_params gs_embed_params_default(void)
{
    gs_embed_params p;
    p.dim = GS_EMBED_DIM; p.epochs = GS_EMBED_EPOCHS; p.neg_samples = GS_EMBED_NEG; p.neg_rate = GS_EMBED_NEG_RATE; p.lr = GS_EMBED_LR; p.seed = GS_EMBED_SEED;
    return p;
}
int gs_embed_knn_graph(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *count, const gs_embed_params *prm,
                       const float *init, float *pos_out, float *memb_out)
{
    return gs::embed_knn_graph_common(c, false, n, knbn, ids, dist, count, prm, init, pos_out, memb_out);
}
int gs_embed_knn_graph_dev(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids_dev, const float *dist_dev, const uint32_t *count_dev,
                           const gs_embed_params *prm, const float *init_dev, float *pos_out_dev, float *memb_out_dev)
{
    return gs::embed_knn_graph_common(c, true, n, knbn, ids_dev, dist_dev, count_dev, prm, init_dev, pos_out_dev, memb_out_dev);
}
int gs_knn_graph_stats(gs_ctx *c, uint64_t n, uint32_t knbn, const uint64_t *ids, const float *dist, const uint32_t *count, gs_knn_stats *stats_out,
                       uint32_t *occ_out, uint64_t *hist_out)
{
    GS_REQUIRE(c, GS_ERR_INVALID, "null context");
    int rc;
    if ((rc = gs::graph_args(n, knbn))) return rc;
    GS_REQUIRE(ids && dist && count && stats_out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n > 0, GS_ERR_INVALID, "statistics of an empty graph");
    GS_CTX_LOCK(c);
    const uint64_t *dids; const float *ddist; const uint32_t *dcnt;
    if ((rc = gs::graph_in(c, false, n, knbn, ids, dist, count, &dids, &ddist, &dcnt))) return rc;
    return gs::knn_stats_dev(c, n, knbn, dids, ddist, dcnt, stats_out, occ_out, hist_out);
}

}  // extern "C"
