// gs_derep.hip — derep: clusters of the database at a distance cut (SPEC.md 18).
//
// Nodes u != v are linked iff their mismatch count is <= c_max. Both answers come from ONE pass over the 16-bit count matrix, block of rows by block
// of rows (cluster_rows = dense_counts, gs_index.hip); a block is consumed while it is in memory and no edge is ever stored.
//   components (single linkage)   k_derep_union    a workgroup per row unites the row's node with every linked column in a forest parent[n]
//                                 k_derep_flatten  parent[x] = root(x), after every block: paths are one hop when the next block starts
//   greedy representatives        rows in rank order (priority descending, node number ascending); per block
//                                 k_derep_cover    per row the best (count, rank) over the linked representatives of EARLIER blocks, and the row's
//                                                  bit mask of linked members earlier in the block
//                                 k_derep_resolve  one wavefront walks the block's rows in order: an uncovered row whose mask meets no representative
//                                                  of the block is one
//                                 k_derep_assign   a row that is none takes the smallest (count, rank) of its cover and the block's representatives
//                                                  its mask names
// The union contract. parent[x] is changed only by an agent-scope atomicCAS(&parent[x], x, y) with y < x: a root is hooked under a smaller node of
// the other tree, once per launch at most. There is no path compression inside k_derep_union, so during a launch a word holds one of two values and
// a read that is stale (a CU's L1 is never refreshed, an XCD's L2 not from another XCD) can only say "still a root": every value read is an ancestor.
// A stale root costs a failed CAS, never a wrong "same tree"; after a failed CAS the walk goes on from the value the CAS returned, so termination
// rests on the atomics alone (node numbers fall strictly). The root of a tree is the smallest node of its component: the label.
#include <algorithm>
#include <numeric>
#include <vector>
#include "gs_internal.hpp"
#include "gs_countrow.hpp"

namespace gs {
namespace {

constexpr int DT = 256;                  // threads per workgroup of the row kernels
constexpr int DW = DT / 64;              // waves per workgroup
constexpr int DU = 4;                    // 16-byte loads in flight per lane in k_derep_cover
constexpr int RG = 8;                    // rows whose masks k_derep_resolve loads ahead of the serial walk
constexpr uint32_t MAX_BLOCK = 4096;     // rows per block at most: the resolve wave holds the block's representatives in two words per lane
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t NOKEY = ~(uint64_t)0;

__device__ __forceinline__ uint32_t ld_parent(const uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of x as far as this reader can see: an ancestor of x in any case
__device__ __forceinline__ uint32_t find_root(const uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = ld_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}
// one tree out of those of a and b; returns an ancestor of both
__device__ __forceinline__ uint32_t unite(uint32_t *parent, uint32_t a, uint32_t b, unsigned long long *stats)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return a;
        const uint32_t hi = max(a, b), lo = min(a, b);
        uint32_t seen = hi;
        const bool won = __hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef GS_DEREP_STATS
        atomicAdd(stats + (won ? 0 : 1), 1ull);
#endif
        if (won) return lo;
        a = seen; b = lo;                // hi had been hooked under `seen` < hi: on from what the CAS returned
    }
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v = min(v, (uint64_t)__shfl_xor((unsigned long long)v, d, 64));
    return v;
}

__global__ void __launch_bounds__(DT) k_derep_iota(uint32_t *__restrict__ a, uint32_t n)
{
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i < n) a[i] = i;
}

// row blockIdx.x of the block is node node0 + blockIdx.x. A wave keeps ru, an ancestor of the row's node; the roots of the linked columns of a step
// that differ from it are reduced over the wave (one union per distinct root, the smallest first). Pad columns >= n are never entries.
__global__ void __launch_bounds__(DT) k_derep_union(const uint16_t *__restrict__ slab, uint64_t ld, uint32_t n, uint32_t c_max, uint32_t node0, uint32_t *parent,
                                                    unsigned long long *stats)
{
    const uint32_t u = node0 + blockIdx.x, lane = threadIdx.x & 63;
    const uint4 *rv = (const uint4 *)(slab + (uint64_t)blockIdx.x * ld);
    const uint32_t nv = (n + 7) / 8;
    uint32_t ru = find_root(parent, u);
    for (uint32_t base = 0; base < nv; base += DT) {         // (uniform trip count: the wave votes below)
        const uint32_t v = base + threadIdx.x;
        const uint4 x = v < nv ? rv[v] : make_uint4(0, 0, 0, 0);
        uint32_t lm = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t j = v * 8 + e;
            if (v < nv && j < n && j != u && count16(x, e) <= c_max) lm |= 1u << e;
        }
        if (!__any(lm != 0)) continue;
#pragma unroll 1
        for (int e = 0; e < 8; e++) {
            uint32_t rj = (lm >> e) & 1 ? find_root(parent, v * 8 + e) : NONE;
            if (rj == ru) rj = NONE;
            while (__any(rj != NONE)) {
                const uint32_t mn = wave_min_u32(rj);
                uint32_t r = ru;
                if (lane == 0) r = unite(parent, ru, mn, stats);
                ru = __shfl(r, 0, 64);
                if (rj == mn || rj == ru) rj = NONE;
            }
        }
    }
}
__global__ void __launch_bounds__(DT) k_derep_flatten(uint32_t *parent, uint32_t n)
{
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = find_root(parent, i);                 // (another thread's store below is a root too: still an ancestor)
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Row r of the block is the node of rank q0 + r. reprank[j] = the rank of node j once it is a representative, NONE before; the launches of earlier
// blocks wrote it. cover[r] = min (count << 32 | rank) over the linked representatives of rank < q0, NOKEY if none. mask[r][W]: bit t = the node of
// rank q0 + t, t < r, is linked to the row's; W words (a multiple of 2), all of them written.
__global__ void __launch_bounds__(DT) k_derep_cover(const uint16_t *__restrict__ slab, uint64_t ld, uint32_t n, uint32_t c_max, const uint32_t *__restrict__ order,
                                                    uint32_t q0, const uint32_t *__restrict__ reprank, uint64_t *__restrict__ cover, uint32_t *__restrict__ mask, uint32_t W)
{
    __shared__ uint64_t lk[DW];
    const uint32_t r = blockIdx.x, u = order[q0 + r], lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint16_t *row = slab + (uint64_t)r * ld;
    const uint4 *rv = (const uint4 *)row;
    const uint32_t nv = (n + 7) / 8;
    uint64_t key = NOKEY;
    for (uint32_t v0 = threadIdx.x; v0 < nv; v0 += DU * DT) {
        uint4 x[DU];
#pragma unroll
        for (int i = 0; i < DU; i++) x[i] = v0 + i * DT < nv ? rv[v0 + i * DT] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
#pragma unroll
        for (int i = 0; i < DU; i++) {
            const uint32_t v = v0 + i * DT;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint32_t j = v * 8 + e, c = count16(x[i], e);
                if (v < nv && j < n && j != u && c <= c_max) {
                    const uint32_t rr = reprank[j];
                    if (rr < q0) key = min(key, ((uint64_t)c << 32) | rr);
                }
            }
        }
    }
    key = wave_min_u64(key);
    if (lane == 0) lk[w] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < DW; i++) key = min(key, lk[i]);
        cover[r] = key;
    }
    for (uint32_t t0 = w * 64; t0 < W * 32; t0 += DT) {      // (t0 is uniform in a wave, W * 32 a multiple of 64)
        const uint32_t t = t0 + lane;
        const bool linked = t < r && row[order[q0 + t]] <= c_max;
        const unsigned long long b = __ballot(linked);
        if (lane == 0) { mask[(uint64_t)r * W + t0 / 32] = (uint32_t)b; mask[(uint64_t)r * W + t0 / 32 + 1] = (uint32_t)(b >> 32); }
    }
}

// One wavefront. Lane l keeps words l and l + 64 of the block's representative mask. The masks of RG rows are loaded before the serial steps over them.
// A representative gets its rank into reprank and itself as its answer.
__global__ void __launch_bounds__(64) k_derep_resolve(const uint32_t *__restrict__ order, uint32_t q0, uint32_t nb, const uint64_t *__restrict__ cover,
                                                      const uint32_t *__restrict__ mask, uint32_t W, uint32_t *__restrict__ reprank, uint32_t *__restrict__ brep,
                                                      uint32_t *__restrict__ out_node, uint16_t *__restrict__ out_count)
{
    const uint32_t lane = threadIdx.x;
    uint32_t rm0 = 0, rm1 = 0;
    for (uint32_t r0 = 0; r0 < nb; r0 += RG) {
        uint32_t m0[RG], m1[RG];
        bool cov[RG];
#pragma unroll
        for (int g = 0; g < RG; g++) {
            const uint32_t r = r0 + g;
            m0[g] = r < nb && lane < W ? mask[(uint64_t)r * W + lane] : 0;
            m1[g] = r < nb && lane + 64 < W ? mask[(uint64_t)r * W + 64 + lane] : 0;
            cov[g] = r < nb ? cover[r] != NOKEY : true;
        }
#pragma unroll
        for (int g = 0; g < RG; g++) {
            const uint32_t r = r0 + g;
            if (r >= nb || cov[g]) continue;                 // (uniform)
            if (__any(((m0[g] & rm0) | (m1[g] & rm1)) != 0)) continue;
            if (lane == ((r >> 5) & 63)) {
                if ((r >> 5) < 64) rm0 |= 1u << (r & 31);
                else rm1 |= 1u << (r & 31);
            }
            if (lane == 0) {
                const uint32_t u = order[q0 + r];
                reprank[u] = q0 + r;
                out_node[u] = u;
                out_count[u] = 0;
            }
        }
    }
    if (lane < W) brep[lane] = rm0;
    if (lane + 64 < W) brep[lane + 64] = rm1;
}

// a wave per row: a row that is no representative takes the smallest (count, rank) of its cover and the block's representatives its mask names
__global__ void __launch_bounds__(DT) k_derep_assign(const uint16_t *__restrict__ slab, uint64_t ld, const uint32_t *__restrict__ order, uint32_t q0, uint32_t nb,
                                                     const uint64_t *__restrict__ cover, const uint32_t *__restrict__ mask, uint32_t W, const uint32_t *__restrict__ brep,
                                                     uint32_t *__restrict__ out_node, uint16_t *__restrict__ out_count)
{
    const uint32_t lane = threadIdx.x & 63, r = blockIdx.x * DW + (threadIdx.x >> 6);
    if (r >= nb) return;
    if ((brep[r >> 5] >> (r & 31)) & 1) return;
    const uint16_t *row = slab + (uint64_t)r * ld;
    uint64_t key = cover[r];
    for (uint32_t wd = lane; wd < W; wd += 64) {
        uint32_t bits = mask[(uint64_t)r * W + wd] & brep[wd];
        while (bits) {
            const uint32_t t = wd * 32 + (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1;
            key = min(key, ((uint64_t)row[order[q0 + t]] << 32) | (q0 + t));
        }
    }
    key = wave_min_u64(key);
    if (lane == 0) {
        const uint32_t u = order[q0 + r];
        out_node[u] = order[(uint32_t)key];
        out_count[u] = (uint16_t)(key >> 32);
    }
}

inline dim3 grid_for(uint64_t items) { return dim3((uint32_t)((items + DT - 1) / DT)); }

// equal blocks of at most max_rows rows (every block streams the whole database once: a short last one costs almost as much as a full one)
inline uint64_t block_rows(const ClusterSource &src)
{
    const uint64_t cap = std::min<uint64_t>(src.max_rows, MAX_BLOCK), parts = (src.n + cap - 1) / cap;
    return (src.n + parts - 1) / parts;
}

// cluster[v] = the label / representative of node v -> the info fields
void fill_info(const uint64_t *cluster, uint64_t n, uint32_t c_max, gs_derep_info *info)
{
    std::vector<uint32_t> size(n, 0);
    for (uint64_t i = 0; i < n; i++) size[cluster[i]]++;
    info->n_clusters = info->n_singletons = info->largest = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!size[i]) continue;
        info->n_clusters++;
        info->n_singletons += size[i] == 1;
        info->largest = std::max<uint64_t>(info->largest, size[i]);
    }
    info->c_max = c_max; info->reserved = 0;
}

#ifdef GS_DEREP_STATS
void print_stats(gs_ctx *c, const unsigned long long *dstats)
{
    unsigned long long h[2] = {0, 0};
    if (hipMemcpyAsync(h, dstats, 16, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess)
        fprintf(stderr, "[GS_DEREP] CAS: %llu successful, %llu failed\n", h[0], h[1]);
}
#endif

}  // namespace

int components_nodes(gs_ctx *c, const ClusterSource &src, uint32_t c_max, uint64_t *label, gs_derep_info *info)
{
    const uint64_t n = src.n;
    GS_REQUIRE(n < 0xFFFFFFFFull, GS_ERR_UNSUPPORTED, "derep needs fewer than 2^32 - 1 nodes");
    PoolBuf nodes(c, SL_DR_ORDER), parent(c, SL_DR_STATE), acc(c, SL_DR_ACC);
    int rc;
    if ((rc = nodes.alloc(4 * n)) || (rc = parent.alloc(4 * n)) || (rc = acc.alloc(16))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(acc.p, 0, 16, c->stream));
    hipLaunchKernelGGL(k_derep_iota, grid_for(n), dim3(DT), 0, c->stream, nodes.as<uint32_t>(), (uint32_t)n);
    hipLaunchKernelGGL(k_derep_iota, grid_for(n), dim3(DT), 0, c->stream, parent.as<uint32_t>(), (uint32_t)n);
    GS_HIP_CHECK(hipGetLastError());
    const uint64_t bq = block_rows(src);
    for (uint64_t q0 = 0; q0 < n; q0 += bq) {
        const uint64_t nb = std::min(bq, n - q0);
        const uint16_t *slab = nullptr;
        if ((rc = cluster_rows(src.ix, nodes.as<uint32_t>() + q0, nb, &slab))) return rc;
        ProfScope ps(c, FAM_SEARCH);
        hipLaunchKernelGGL(k_derep_union, dim3((uint32_t)nb), dim3(DT), 0, c->stream, slab, src.ld, (uint32_t)n, c_max, (uint32_t)q0, parent.as<uint32_t>(),
                           acc.as<unsigned long long>());
        hipLaunchKernelGGL(k_derep_flatten, grid_for(n), dim3(DT), 0, c->stream, parent.as<uint32_t>(), (uint32_t)n);
        GS_HIP_CHECK(hipGetLastError());
    }
    std::vector<uint32_t> h(n);
    GS_HIP_CHECK(hipMemcpyAsync(h.data(), parent.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
#ifdef GS_DEREP_STATS
    print_stats(c, acc.as<unsigned long long>());
#endif
    for (uint64_t i = 0; i < n; i++) label[i] = h[i];
    fill_info(label, n, c_max, info);
    return GS_OK;
}

int derep_nodes(gs_ctx *c, const ClusterSource &src, uint32_t c_max, const uint64_t *priority, uint64_t *rep_node, uint16_t *rep_count, gs_derep_info *info)
{
    const uint64_t n = src.n;
    GS_REQUIRE(n < 0xFFFFFFFFull, GS_ERR_UNSUPPORTED, "derep needs fewer than 2^32 - 1 nodes");
    // rank order: priority descending, node number ascending (a stable sort of the node numbers)
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (priority) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return priority[a] > priority[b]; });
    const uint64_t bq = block_rows(src);
    const uint32_t W = (uint32_t)(round_up(bq, 64) / 32);
    PoolBuf dorder(c, SL_DR_ORDER), reprank(c, SL_DR_STATE), cover(c, SL_DR_COVER), mask(c, SL_DR_MASK), brep(c, SL_DR_BREP), onode(c, SL_DR_OUT_NODE),
        ocnt(c, SL_DR_OUT_COUNT);
    int rc;
    if ((rc = dorder.alloc(4 * n)) || (rc = reprank.alloc(4 * n)) || (rc = cover.alloc(8 * bq)) || (rc = mask.alloc(4 * bq * W)) || (rc = brep.alloc(4 * (size_t)W)) ||
        (rc = onode.alloc(4 * n)) || (rc = ocnt.alloc(2 * n))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dorder.p, order.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemsetAsync(reprank.p, 0xFF, 4 * n, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));       // (`order` is pageable and goes out of scope on every return below)
    for (uint64_t q0 = 0; q0 < n; q0 += bq) {
        const uint64_t nb = std::min(bq, n - q0);
        const uint16_t *slab = nullptr;
        if ((rc = cluster_rows(src.ix, dorder.as<uint32_t>() + q0, nb, &slab))) return rc;
        ProfScope ps(c, FAM_SEARCH);
        hipLaunchKernelGGL(k_derep_cover, dim3((uint32_t)nb), dim3(DT), 0, c->stream, slab, src.ld, (uint32_t)n, c_max, dorder.as<uint32_t>(), (uint32_t)q0,
                           reprank.as<uint32_t>(), cover.as<uint64_t>(), mask.as<uint32_t>(), W);
        hipLaunchKernelGGL(k_derep_resolve, dim3(1), dim3(64), 0, c->stream, dorder.as<uint32_t>(), (uint32_t)q0, (uint32_t)nb, cover.as<uint64_t>(),
                           mask.as<uint32_t>(), W, reprank.as<uint32_t>(), brep.as<uint32_t>(), onode.as<uint32_t>(), ocnt.as<uint16_t>());
        hipLaunchKernelGGL(k_derep_assign, dim3((uint32_t)((nb + DW - 1) / DW)), dim3(DT), 0, c->stream, slab, src.ld, dorder.as<uint32_t>(), (uint32_t)q0, (uint32_t)nb,
                           cover.as<uint64_t>(), mask.as<uint32_t>(), W, brep.as<uint32_t>(), onode.as<uint32_t>(), ocnt.as<uint16_t>());
        GS_HIP_CHECK(hipGetLastError());
    }
    std::vector<uint32_t> h(n);
    GS_HIP_CHECK(hipMemcpyAsync(h.data(), onode.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(rep_count, ocnt.p, 2 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < n; i++) rep_node[i] = h[i];
    fill_info(rep_node, n, c_max, info);
    return GS_OK;
}

}  // namespace gs
