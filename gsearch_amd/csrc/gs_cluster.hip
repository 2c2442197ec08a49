// gs_cluster.hip — hnswcore: a coreset of an index's nodes, k-medoids on it, every node to its nearest centre (SPEC.md 10).
//
// All distances are rows of the 16-bit count matrix: a block of candidate rows (coreset points, medoids) against every node, produced by the
// index's dense producer (cluster_rows = dense_counts, gs_index.hip). The kernels here reduce such blocks:
//   k_colmin          per node (column) the smallest (count, position) over the block's rows, folded into a running pair kept across blocks
//   k_colmin_out      the running pairs as outputs: position, count, the candidate's node number, histogram of the positions, sum of the counts
//   k_core_*          round 1 of the sampling (hash compare against d0 / D) and the ordered compaction of the coreset
//   k_gather_cols     P[block rows, :] = slab[:, C]
//   k_row_totals      per coreset point j the weighted cost of the members of its cluster to j: the kernel that runs once per k-medoid iteration
//   k_init_medoids / k_assign / k_update_medoids     the rest of the Voronoi iteration
// Every value is an integer and every sum a u64 of weight x count, so the order of the adds (waves, atomics on counters) changes nothing.
#include <chrono>
#include <cmath>
#include <numeric>
#include "gs_internal.hpp"
#include "gs_countrow.hpp"
#include "gs_spec.hpp"

namespace gs {
namespace {

constexpr int CT = 256;                  // threads per workgroup
constexpr int CW = CT / 64;              // waves per workgroup
constexpr int CU = 4;                    // 16-byte loads in flight per lane in k_colmin
constexpr int UR = 4;                    // rows of P per wave in k_row_totals: the weights and labels of a step are loaded once for all of them
constexpr int IT = 1024;                 // threads of k_init_medoids (one workgroup)
constexpr uint64_t NOKEY = ~(uint64_t)0;
constexpr uint32_t CHOSEN = 0xFFFFFFFFu; // dmin of a coreset point that is a medoid already (a count is at most 65535)

__global__ void __launch_bounds__(CT) k_gather_rows(const uint4 *__restrict__ data, uint64_t stride16, const uint32_t *__restrict__ nodes, uint4 *__restrict__ out)
{
    const uint4 *s = data + (uint64_t)nodes[blockIdx.x] * stride16;
    uint4 *d = out + (uint64_t)blockIdx.x * stride16;
    for (uint64_t v = threadIdx.x; v < stride16; v += CT) d[v] = s[v];
}

// best[j] = min(best[j], min over the nb rows r of (slab[r][j] << 32 | pos0 + r)): the smallest count, ties to the smallest position. A workgroup owns
// 512 columns: lane l of every wave holds columns 8 l .. 8 l + 7 of them (one 16-byte load per row), wave w takes rows w, w + CW, ...; the waves' pairs
// meet in LDS and wave 0 folds them into the pair kept from earlier blocks. A column has one owner: no atomics.
__global__ void __launch_bounds__(CT) k_colmin(const uint16_t *__restrict__ slab, uint64_t ld, uint32_t nb, uint32_t n, uint32_t pos0, uint64_t *__restrict__ best)
{
    __shared__ uint64_t L[CW - 1][8][64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t nv = ld / 8, v = (uint64_t)blockIdx.x * 64 + lane;
    uint64_t key[8];
#pragma unroll
    for (int e = 0; e < 8; e++) key[e] = NOKEY;
    if (v < nv) {
        const uint4 *col = (const uint4 *)slab + v;
        for (uint32_t r0 = w; r0 < nb; r0 += CW * CU) {
            uint4 x[CU];
#pragma unroll
            for (int u = 0; u < CU; u++) x[u] = r0 + u * CW < nb ? col[(uint64_t)(r0 + u * CW) * nv] : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < CU; u++) {
                const uint32_t r = r0 + u * CW;
                if (r < nb) {
#pragma unroll
                    for (int e = 0; e < 8; e++) key[e] = min(key[e], ((uint64_t)count16(x[u], e) << 32) | (pos0 + r));
                }
            }
        }
    }
    if (w) {
#pragma unroll
        for (int e = 0; e < 8; e++) L[w - 1][e][lane] = key[e];
    }
    __syncthreads();
    if (w == 0 && v < nv) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
#pragma unroll
            for (int o = 0; o < CW - 1; o++) key[e] = min(key[e], L[o][e][lane]);
            const uint64_t j = v * 8 + e;
            if (j < n) best[j] = min(best[j], key[e]);
        }
    }
}

// sum of one u64 per thread over the workgroup, in thread 0
template <int NW>
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t *lds)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NW; i++) t += lds[i];
    return t;
}
// the smallest (key, idx) pair of the workgroup, in every thread
template <int NW>
__device__ __forceinline__ void block_argmin(uint64_t &key, uint32_t &idx, uint64_t *lk, uint32_t *li)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint64_t ok = __shfl_down(key, d, 64);
        const uint32_t oi = __shfl_down(idx, d, 64);
        if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
    __syncthreads();                     // (the readers of an earlier call are done with lk / li)
    if ((threadIdx.x & 63) == 0) { lk[threadIdx.x >> 6] = key; li[threadIdx.x >> 6] = idx; }
    __syncthreads();
    key = lk[0]; idx = li[0];
    for (int i = 1; i < NW; i++) {
        const uint64_t ok = lk[i];
        const uint32_t oi = li[i];
        if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
}

// the running pairs as outputs; every output is optional. cand: the node numbers of the candidates (for `node`); hist: += 1 at each node's position;
// sum: += the counts
__global__ void __launch_bounds__(CT) k_colmin_out(const uint64_t *__restrict__ best, uint32_t n, const uint32_t *__restrict__ cand, uint32_t *__restrict__ arg,
                                                   uint16_t *__restrict__ cnt, uint64_t *__restrict__ node, uint32_t *__restrict__ hist, unsigned long long *__restrict__ sum)
{
    __shared__ uint64_t lds[CW];
    const uint32_t i = blockIdx.x * CT + threadIdx.x;
    uint64_t c = 0;
    if (i < n) {
        const uint64_t key = best[i];
        const uint32_t pos = (uint32_t)key;
        c = key >> 32;
        if (arg) arg[i] = pos;
        if (cnt) cnt[i] = (uint16_t)c;
        if (node) node[i] = cand[pos];
        if (hist) atomicAdd(&hist[pos], 1u);
    }
    if (sum) {
        const uint64_t t = block_sum<CW>(c, lds);
        if (threadIdx.x == 0 && t) atomicAdd(sum, (unsigned long long)t);
    }
}

// node i is in the coreset: a member of round 0, or drawn in round 1 with probability t1 d0(i) / D (d0 = the count in its running pair)
__device__ __forceinline__ bool in_core(uint32_t i, const uint8_t *in0, const uint64_t *best, uint64_t seed, uint64_t D, uint64_t t1)
{
    return in0[i] || cluster_keep1(cluster_hash(seed, 1, i), D, t1, (uint32_t)(best[i] >> 32));
}
__global__ void __launch_bounds__(CT) k_core_count(const uint8_t *__restrict__ in0, const uint64_t *__restrict__ best, uint32_t n, uint64_t seed,
                                                   const unsigned long long *__restrict__ D, uint64_t t1, uint32_t *__restrict__ blockcnt)
{
    __shared__ uint32_t wsum[CW];
    const uint32_t i = blockIdx.x * CT + threadIdx.x;
    uint32_t tot;
    block_excl_scan<CW>(i < n && in_core(i, in0, best, seed, *D, t1), wsum, tot);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = tot;
}
// blockcnt[0 .. nblk) -> its exclusive prefix in place, the total in blockcnt[nblk]; one workgroup
__global__ void __launch_bounds__(CT) k_core_scan(uint32_t *__restrict__ blockcnt, uint32_t nblk)
{
    __shared__ uint32_t wsum[2][CW];
    uint32_t run = 0, par = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += CT, par ^= 1) {
        const uint32_t b = b0 + threadIdx.x, v = b < nblk ? blockcnt[b] : 0;
        uint32_t tot;
        const uint32_t pre = block_excl_scan<CW>(v, wsum[par], tot);
        if (b < nblk) blockcnt[b] = run + pre;
        run += tot;
    }
    if (threadIdx.x == 0) blockcnt[nblk] = run;
}
__global__ void __launch_bounds__(CT) k_core_write(const uint8_t *__restrict__ in0, const uint64_t *__restrict__ best, uint32_t n, uint64_t seed,
                                                   const unsigned long long *__restrict__ D, uint64_t t1, const uint32_t *__restrict__ blockoff, uint32_t *__restrict__ core)
{
    __shared__ uint32_t wsum[CW];
    const uint32_t i = blockIdx.x * CT + threadIdx.x;
    const bool in = i < n && in_core(i, in0, best, seed, *D, t1);
    uint32_t tot;
    const uint32_t pre = block_excl_scan<CW>(in, wsum, tot);
    if (in) core[blockoff[blockIdx.x] + pre] = i;
}

// P[row0 + r][j] = slab[r][core[j]] for the nb rows of a block (blockIdx.y = r); the pad columns p .. pld - 1 are written as 0
__global__ void __launch_bounds__(CT) k_gather_cols(const uint16_t *__restrict__ slab, uint64_t ld, const uint32_t *__restrict__ core, uint32_t p, uint16_t *__restrict__ P,
                                                    uint64_t pld, uint32_t row0)
{
    const uint32_t j = blockIdx.x * CT + threadIdx.x, r = blockIdx.y;
    if (j < pld) P[(uint64_t)(row0 + r) * pld + j] = j < p ? slab[(uint64_t)r * ld + core[j]] : (uint16_t)0;
}

// tot[j] = sum over the i with lab[i] == lab[j] of w[i] P[i][j], read as P[j][i] (P is symmetric): a wave owns UR rows and streams them contiguously,
// 16 bytes per lane and row and step; the 8 weights and labels of a step come once (from L2: 8 p bytes in all) for the UR rows. w and lab hold pld
// entries; the pad entries of w and of every row of P are 0. No atomics.
__global__ void __launch_bounds__(CT) k_row_totals(const uint16_t *__restrict__ P, uint64_t pld, uint32_t p, const uint32_t *__restrict__ w, const uint32_t *__restrict__ lab,
                                                   unsigned long long *__restrict__ tot)
{
    const uint32_t lane = threadIdx.x & 63, j0 = (blockIdx.x * CW + (threadIdx.x >> 6)) * UR;
    if (j0 >= p) return;
    const uint32_t nv = (uint32_t)(pld / 8);
    const uint4 *row[UR];
    uint32_t lj[UR];
    uint64_t acc[UR];
#pragma unroll
    for (int u = 0; u < UR; u++) {
        const uint32_t j = min(j0 + u, p - 1);
        row[u] = (const uint4 *)(P + (uint64_t)j * pld);
        lj[u] = lab[j];
        acc[u] = 0;
    }
    for (uint32_t v = lane; v < nv; v += 64) {
        uint4 x[UR];
#pragma unroll
        for (int u = 0; u < UR; u++) x[u] = row[u][v];
        const uint4 wa = ((const uint4 *)w)[2 * v], wb = ((const uint4 *)w)[2 * v + 1], la = ((const uint4 *)lab)[2 * v], lb = ((const uint4 *)lab)[2 * v + 1];
        const uint32_t wi[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w}, li[8] = {la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w};
#pragma unroll
        for (int e = 0; e < 8; e++) {
#pragma unroll
            for (int u = 0; u < UR; u++) acc[u] += li[e] == lj[u] ? (uint64_t)wi[e] * count16(x[u], e) : 0;
        }
    }
#pragma unroll
    for (int u = 0; u < UR; u++) {
        uint64_t a = acc[u];
#pragma unroll
        for (int d = 32; d; d >>= 1) a += __shfl_down(a, d, 64);
        if (lane == 0 && j0 + u < p) tot[j0 + u] = a;
    }
}

// the k initial medoids, one workgroup: med[0] = argmin (tot[j], j); then the unchosen j of largest w[j] dmin[j] (ties: the smallest j), dmin = the count
// to the nearest medoid so far, read from the row of the medoid chosen last
__global__ void __launch_bounds__(IT) k_init_medoids(const uint16_t *__restrict__ P, uint64_t pld, uint32_t p, const uint32_t *__restrict__ w,
                                                     const unsigned long long *__restrict__ tot, uint32_t k, uint32_t *__restrict__ med, uint32_t *__restrict__ dmin)
{
    __shared__ uint64_t lk[IT / 64];
    __shared__ uint32_t li[IT / 64];
    uint64_t key = NOKEY;
    uint32_t idx = CHOSEN;
    for (uint32_t j = threadIdx.x; j < p; j += IT) {
        dmin[j] = 65535;                 // (every count is <= m <= 65535)
        if (tot[j] < key) { key = tot[j]; idx = j; }
    }
    block_argmin<IT / 64>(key, idx, lk, li);
    if (threadIdx.x == 0) med[0] = idx;
    for (uint32_t c = 1; c < k; c++) {
        const uint16_t *row = P + (uint64_t)idx * pld;
        const uint32_t last = idx;
        key = NOKEY; idx = CHOSEN;
        for (uint32_t j = threadIdx.x; j < p; j += IT) {     // (a thread meets the same j in every round: dmin needs no barrier)
            uint32_t d = dmin[j];
            if (j == last) d = CHOSEN;
            else if (d != CHOSEN) d = min(d, (uint32_t)row[j]);
            dmin[j] = d;
            // largest w dmin first: the complement of (w dmin + 1), 0 is left to the chosen ones
            const uint64_t kk = d == CHOSEN ? NOKEY : ~((uint64_t)w[j] * d + 1);
            if (kk < key) { key = kk; idx = j; }
        }
        block_argmin<IT / 64>(key, idx, lk, li);
        if (threadIdx.x == 0) med[c] = idx;
    }
}

// lab[i] = the t minimising (P[med_t][i], t), a medoid to itself; cost += w[i] x that count
__global__ void __launch_bounds__(CT) k_assign(const uint16_t *__restrict__ P, uint64_t pld, uint32_t p, const uint32_t *__restrict__ med, uint32_t k,
                                               const uint32_t *__restrict__ w, uint32_t *__restrict__ lab, unsigned long long *__restrict__ cost)
{
    __shared__ uint64_t lds[CW];
    const uint32_t i = blockIdx.x * CT + threadIdx.x;
    uint64_t term = 0;
    if (i < p) {
        uint32_t bc = 0xFFFFFFFFu, bt = 0;
        bool self = false;
        for (uint32_t t = 0; t < k; t++) {
            const uint32_t mt = med[t], c = P[(uint64_t)mt * pld + i];
            if (mt == i) { bc = c; bt = t; self = true; }
            else if (!self && c < bc) { bc = c; bt = t; }
        }
        lab[i] = bt;
        term = (uint64_t)w[i] * bc;
    }
    const uint64_t t = block_sum<CW>(term, lds);
    if (threadIdx.x == 0 && t) atomicAdd(cost, (unsigned long long)t);
}

// workgroup t: newmed[t] = the j of cluster t minimising (tot[j], j); *moved |= 1 when it is not med[t]
__global__ void __launch_bounds__(CT) k_update_medoids(const unsigned long long *__restrict__ tot, const uint32_t *__restrict__ lab, uint32_t p, const uint32_t *__restrict__ med,
                                                       uint32_t *__restrict__ newmed, uint32_t *__restrict__ moved)
{
    __shared__ uint64_t lk[CW];
    __shared__ uint32_t li[CW];
    const uint32_t t = blockIdx.x;
    uint64_t key = NOKEY;
    uint32_t idx = CHOSEN;
    for (uint32_t j = threadIdx.x; j < p; j += CT)
        if (lab[j] == t && (idx == CHOSEN || tot[j] < key)) { key = tot[j]; idx = j; }
    block_argmin<CW>(key, idx, lk, li);
    if (threadIdx.x == 0) {
        newmed[t] = idx;
        if (idx != med[t]) atomicOr(moved, 1u);
    }
}

inline dim3 grid_for(uint64_t items) { return dim3((uint32_t)((items + CT - 1) / CT)); }

// GS_CLUSTER_VERBOSE=1: the time of every stage (the stream is drained at each boundary) on stderr
struct StageClock {
    gs_ctx *c; bool on; std::chrono::steady_clock::time_point t0;
    explicit StageClock(gs_ctx *ctx) : c(ctx), on(getenv("GS_CLUSTER_VERBOSE") != nullptr) { if (on) { (void)hipStreamSynchronize(c->stream); t0 = std::chrono::steady_clock::now(); } }
    double lap()
    {
        (void)hipStreamSynchronize(c->stream);
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

// the two events around the update kernel of a verbose run
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// The candidates cand_dev[0 .. nc) (device node numbers) against every node, block by block: best[i] = the smallest (count, position) of node i.
// P != null: also P[position][:] = the counts to the nodes core[0 .. p) (the candidates ARE the coreset then).
int nearest_pass(gs_ctx *c, const ClusterSource &src, const uint32_t *cand_dev, uint64_t nc, uint64_t *best, uint16_t *P, uint64_t pld, const uint32_t *core, uint32_t p)
{
    GS_HIP_CHECK(hipMemsetAsync(best, 0xFF, 8 * src.n, c->stream));
    // equal blocks: every block streams the whole database once, a short last one costs almost as much as a full one
    const uint64_t parts = (nc + src.max_rows - 1) / src.max_rows, bq = (nc + parts - 1) / parts;
    for (uint64_t q0 = 0; q0 < nc; q0 += bq) {
        const uint64_t nb = std::min(bq, nc - q0);
        const uint16_t *slab = nullptr;
        int rc = cluster_rows(src.ix, cand_dev + q0, nb, &slab);
        if (rc) return rc;
        hipLaunchKernelGGL(k_colmin, dim3((uint32_t)((src.ld / 8 + 63) / 64)), dim3(CT), 0, c->stream, slab, src.ld, (uint32_t)nb, (uint32_t)src.n, (uint32_t)q0, best);
        if (P) hipLaunchKernelGGL(k_gather_cols, dim3((uint32_t)((pld + CT - 1) / CT), (uint32_t)nb), dim3(CT), 0, c->stream, slab, src.ld, core, p, P, pld, (uint32_t)q0);
        GS_HIP_CHECK(hipGetLastError());
    }
    return GS_OK;
}

}  // namespace

int gather_rows(gs_ctx *c, const void *data, uint64_t stride, const uint32_t *nodes_dev, uint64_t nb, void *out)
{
    GS_REQUIRE(stride % 16 == 0 && nb <= 0x7FFFFFFFull, GS_ERR_INVALID, "gather_rows: bad shape");
    if (nb == 0) return GS_OK;
    hipLaunchKernelGGL(k_gather_rows, dim3((uint32_t)nb), dim3(CT), 0, c->stream, (const uint4 *)data, stride / 16, nodes_dev, (uint4 *)out);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

int nearest_of_nodes(gs_ctx *c, const ClusterSource &src, const uint64_t *cand, uint64_t nc, uint32_t *arg_out, uint16_t *count_out)
{
    GS_REQUIRE(nc >= 1 && nc <= 0xFFFFFFFFull, GS_ERR_INVALID, "nearest_of needs between 1 and 2^32 - 1 candidates");
    GS_REQUIRE(src.n < ((uint64_t)1 << 32), GS_ERR_UNSUPPORTED, "nearest_of needs fewer than 2^32 nodes");
    std::vector<uint32_t> nodes(nc);
    for (uint64_t i = 0; i < nc; i++) {
        GS_REQUIRE(cand[i] < src.n, GS_ERR_INVALID, "candidate %llu is node %llu of %llu", (unsigned long long)i, (unsigned long long)cand[i], (unsigned long long)src.n);
        nodes[i] = (uint32_t)cand[i];
    }
    PoolBuf dn(c, SL_CL_NODES), best(c, SL_CL_BEST), darg(c, SL_CL_OUT_ARG), dcnt(c, SL_CL_OUT_COUNT);
    int rc;
    if ((rc = dn.alloc(4 * nc)) || (rc = best.alloc(8 * src.n)) || (rc = darg.alloc(4 * src.n)) || (rc = dcnt.alloc(2 * src.n))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dn.p, nodes.data(), 4 * nc, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));    // (`nodes` is pageable and goes out of scope on every return below)
    if ((rc = nearest_pass(c, src, dn.as<uint32_t>(), nc, best.as<uint64_t>(), nullptr, 0, nullptr, 0))) return rc;
    hipLaunchKernelGGL(k_colmin_out, grid_for(src.n), dim3(CT), 0, c->stream, best.as<uint64_t>(), (uint32_t)src.n, (const uint32_t *)nullptr, darg.as<uint32_t>(),
                       dcnt.as<uint16_t>(), (uint64_t *)nullptr, (uint32_t *)nullptr, (unsigned long long *)nullptr);
    GS_HIP_CHECK(hipGetLastError());
    GS_HIP_CHECK(hipMemcpyAsync(arg_out, darg.p, 4 * src.n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(count_out, dcnt.p, 2 * src.n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int cluster_nodes(gs_ctx *c, const ClusterSource &src, const gs_cluster_params *prm, uint64_t *centre_node, uint16_t *centre_count, uint64_t *medoids,
                  uint64_t *sizes, uint64_t *core_nodes, uint64_t *core_weight, uint64_t core_cap, gs_cluster_info *info)
{
    const uint64_t n = src.n, k = prm->n_cluster, seed = prm->seed;
    GS_REQUIRE(k <= n, GS_ERR_INVALID, "n_cluster %llu exceeds the %llu nodes", (unsigned long long)k, (unsigned long long)n);
    GS_REQUIRE(prm->fraction > 0.0 && prm->fraction <= 1.0, GS_ERR_INVALID, "fraction must be in (0, 1]");      // (false for NaN)
    GS_REQUIRE(prm->max_iter >= 1, GS_ERR_INVALID, "max_iter must be at least 1");
    GS_REQUIRE(n < ((uint64_t)1 << 32) && n * src.m < ((uint64_t)1 << 40), GS_ERR_UNSUPPORTED, "the sampling needs nb_point x m < 2^40");
    StageClock clk(c);
    int rc;

    // round 0 on the host: it reads nothing but the hashes
    const uint64_t t = std::min<uint64_t>(n, std::max<uint64_t>(std::max<uint64_t>(k, 1), (uint64_t)std::ceil(prm->fraction * (double)n)));
    const uint64_t t0 = (t + 1) / 2, t1 = t - t0, nfirst = std::max<uint64_t>(k, 1);
    std::vector<uint64_t> h0(n);
    std::vector<uint8_t> in0(n);
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; i++) { h0[i] = cluster_hash(seed, 0, i); in0[i] = cluster_keep0(h0[i], n, t0); }
    std::iota(order.begin(), order.end(), 0u);
    std::partial_sort(order.begin(), order.begin() + nfirst, order.end(), [&](uint32_t a, uint32_t b) { return h0[a] != h0[b] ? h0[a] < h0[b] : a < b; });
    for (uint64_t i = 0; i < nfirst; i++) in0[order[i]] = 1;
    std::vector<uint32_t> s0;
    for (uint64_t i = 0; i < n; i++) if (in0[i]) s0.push_back((uint32_t)i);

    const uint32_t nblk = (uint32_t)((n + CT - 1) / CT);
    PoolBuf dn(c, SL_CL_NODES), best(c, SL_CL_BEST), din0(c, SL_CL_IN0), blocks(c, SL_CL_BLOCKS), core(c, SL_CL_CORE), acc(c, SL_CL_ACC);
    PoolBuf onode(c, SL_CL_OUT_NODE), ocnt(c, SL_CL_OUT_COUNT);
    if ((rc = dn.alloc(4 * std::max<uint64_t>(s0.size(), k))) || (rc = best.alloc(8 * n)) || (rc = din0.alloc(n)) || (rc = blocks.alloc(4 * ((size_t)nblk + 1))) ||
        (rc = core.alloc(4 * n)) || (rc = acc.alloc(32)) || (rc = onode.alloc(8 * n)) || (rc = ocnt.alloc(2 * n))) return rc;
    unsigned long long *dD = acc.as<unsigned long long>(), *dcost = dD + 1, *dall = dD + 2;
    uint32_t *dmoved = (uint32_t *)(dD + 3);
    GS_HIP_CHECK(hipMemsetAsync(acc.p, 0, 32, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dn.p, s0.data(), 4 * s0.size(), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(din0.p, in0.data(), n, hipMemcpyHostToDevice, c->stream));
    // d0 and D, round 1, the coreset in node order
    if ((rc = nearest_pass(c, src, dn.as<uint32_t>(), s0.size(), best.as<uint64_t>(), nullptr, 0, nullptr, 0))) return rc;
    hipLaunchKernelGGL(k_colmin_out, grid_for(n), dim3(CT), 0, c->stream, best.as<uint64_t>(), (uint32_t)n, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                       (uint16_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, dD);
    hipLaunchKernelGGL(k_core_count, dim3(nblk), dim3(CT), 0, c->stream, din0.as<uint8_t>(), best.as<uint64_t>(), (uint32_t)n, seed, dD, t1, blocks.as<uint32_t>());
    hipLaunchKernelGGL(k_core_scan, dim3(1), dim3(CT), 0, c->stream, blocks.as<uint32_t>(), nblk);
    hipLaunchKernelGGL(k_core_write, dim3(nblk), dim3(CT), 0, c->stream, din0.as<uint8_t>(), best.as<uint64_t>(), (uint32_t)n, seed, dD, t1, blocks.as<uint32_t>(),
                       core.as<uint32_t>());
    GS_HIP_CHECK(hipGetLastError());
    uint32_t p = 0;
    GS_HIP_CHECK(hipMemcpyAsync(&p, blocks.as<uint32_t>() + nblk, 4, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (clk.on) fprintf(stderr, "[GS_CLUSTER] round 0: %zu rows, coreset p = %u: %.2f ms\n", s0.size(), p, clk.lap());
    info->n_core = p;
    GS_REQUIRE((!core_nodes && !core_weight) || core_cap >= p, GS_ERR_INVALID, "the coreset has %u points, core_cap is %llu", p, (unsigned long long)core_cap);

    // nearest coreset point of every node, the weights, and P (one pass over the coreset's rows feeds all three)
    const uint64_t pld = round_up(p, 8);
    PoolBuf dw(c, SL_CL_WEIGHT), dlab(c, SL_CL_LABEL), dP(c, SL_CL_P), dtot(c, SL_CL_TOT), dmed(c, SL_CL_MED), ddmin(c, SL_CL_DMIN);
    if ((rc = dw.alloc(4 * std::max<uint64_t>(pld, k)))) return rc;
    if (k && ((rc = dlab.alloc(4 * pld)) || (rc = dP.alloc(2 * (size_t)p * pld)) || (rc = dtot.alloc(8 * (size_t)p)) || (rc = dmed.alloc(8 * k)) || (rc = ddmin.alloc(4 * (size_t)p))))
        return rc;
    GS_HIP_CHECK(hipMemsetAsync(dw.p, 0, 4 * pld, c->stream));
    if ((rc = nearest_pass(c, src, core.as<uint32_t>(), p, best.as<uint64_t>(), k ? dP.as<uint16_t>() : nullptr, pld, core.as<uint32_t>(), p))) return rc;
    hipLaunchKernelGGL(k_colmin_out, grid_for(n), dim3(CT), 0, c->stream, best.as<uint64_t>(), (uint32_t)n, core.as<uint32_t>(), (uint32_t *)nullptr, ocnt.as<uint16_t>(),
                       onode.as<uint64_t>(), dw.as<uint32_t>(), dall);
    GS_HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> hcore(p), hw(p);
    GS_HIP_CHECK(hipMemcpyAsync(hcore.data(), core.p, 4 * (size_t)p, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(hw.data(), dw.p, 4 * (size_t)p, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (clk.on) fprintf(stderr, "[GS_CLUSTER] coreset pass: %u rows (nearest, weights%s): %.2f ms\n", p, k ? ", P" : "", clk.lap());
    for (uint32_t i = 0; i < p; i++) {
        if (core_nodes) core_nodes[i] = hcore[i];
        if (core_weight) core_weight[i] = hw[i];
    }
    info->iterations = 0; info->converged = 1; info->cost_core = 0;

    if (k) {
        uint32_t *med = dmed.as<uint32_t>(), *newmed = med + k;
        GS_HIP_CHECK(hipMemsetAsync(dlab.p, 0, 4 * pld, c->stream));     // one cluster: the totals of the first medoid
        const dim3 gtot((p + CW * UR - 1) / (CW * UR));
        hipLaunchKernelGGL(k_row_totals, gtot, dim3(CT), 0, c->stream, dP.as<uint16_t>(), pld, p, dw.as<uint32_t>(), dlab.as<uint32_t>(), dtot.as<unsigned long long>());
        hipLaunchKernelGGL(k_init_medoids, dim3(1), dim3(IT), 0, c->stream, dP.as<uint16_t>(), pld, p, dw.as<uint32_t>(), dtot.as<unsigned long long>(), (uint32_t)k, med,
                           ddmin.as<uint32_t>());
        GS_HIP_CHECK(hipGetLastError());
        if (clk.on) fprintf(stderr, "[GS_CLUSTER] initial medoids (k = %llu): %.2f ms\n", (unsigned long long)k, clk.lap());
        EventPair ev;
        if (clk.on) { GS_HIP_CHECK(hipEventCreate(&ev.a)); GS_HIP_CHECK(hipEventCreate(&ev.b)); }
        info->converged = 0;
        while (info->iterations < prm->max_iter) {
            GS_HIP_CHECK(hipMemsetAsync(dcost, 0, 8, c->stream));
            GS_HIP_CHECK(hipMemsetAsync(dmoved, 0, 4, c->stream));
            hipLaunchKernelGGL(k_assign, grid_for(p), dim3(CT), 0, c->stream, dP.as<uint16_t>(), pld, p, med, (uint32_t)k, dw.as<uint32_t>(), dlab.as<uint32_t>(), dcost);
            if (clk.on) GS_HIP_CHECK(hipEventRecord(ev.a, c->stream));
            hipLaunchKernelGGL(k_row_totals, gtot, dim3(CT), 0, c->stream, dP.as<uint16_t>(), pld, p, dw.as<uint32_t>(), dlab.as<uint32_t>(), dtot.as<unsigned long long>());
            if (clk.on) GS_HIP_CHECK(hipEventRecord(ev.b, c->stream));
            hipLaunchKernelGGL(k_update_medoids, dim3((uint32_t)k), dim3(CT), 0, c->stream, dtot.as<unsigned long long>(), dlab.as<uint32_t>(), p, med, newmed, dmoved);
            GS_HIP_CHECK(hipGetLastError());
            unsigned long long hacc[4];
            GS_HIP_CHECK(hipMemcpyAsync(hacc, acc.p, 32, hipMemcpyDeviceToHost, c->stream));
            GS_HIP_CHECK(hipStreamSynchronize(c->stream));
            info->iterations++;
            info->cost_core = hacc[1];
            const bool moved = (uint32_t)hacc[3] != 0;
            if (clk.on) {
                float ums = 0;
                GS_HIP_CHECK(hipEventElapsedTime(&ums, ev.a, ev.b));
                const double bytes = 2.0 * p * pld;
                fprintf(stderr, "[GS_CLUSTER] iteration %u: %.3f ms, update kernel %.3f ms = %.1f MB of P at %.2f TB/s, cost %llu%s\n", info->iterations, clk.lap(), ums,
                        bytes / 1e6, bytes / (ums * 1e-3) / 1e12, hacc[1], moved ? "" : " (converged)");
            }
            if (!moved) { info->converged = 1; break; }
            std::swap(med, newmed);
        }
        // the medoids by ascending node number (the coreset is in node order), then every node to its nearest one
        std::vector<uint32_t> hmed(k);
        GS_HIP_CHECK(hipMemcpyAsync(hmed.data(), med, 4 * k, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        std::sort(hmed.begin(), hmed.end());
        for (uint64_t i = 0; i < k; i++) { hmed[i] = hcore[hmed[i]]; medoids[i] = hmed[i]; }
        GS_HIP_CHECK(hipMemcpyAsync(dn.p, hmed.data(), 4 * k, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemsetAsync(dw.p, 0, 4 * k, c->stream));
        GS_HIP_CHECK(hipMemsetAsync(dall, 0, 8, c->stream));
        if ((rc = nearest_pass(c, src, dn.as<uint32_t>(), k, best.as<uint64_t>(), nullptr, 0, nullptr, 0))) return rc;
        hipLaunchKernelGGL(k_colmin_out, grid_for(n), dim3(CT), 0, c->stream, best.as<uint64_t>(), (uint32_t)n, dn.as<uint32_t>(), (uint32_t *)nullptr, ocnt.as<uint16_t>(),
                           onode.as<uint64_t>(), dw.as<uint32_t>(), dall);
        GS_HIP_CHECK(hipGetLastError());
        std::vector<uint32_t> hs(k);
        GS_HIP_CHECK(hipMemcpyAsync(hs.data(), dw.p, 4 * k, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < k; i++) sizes[i] = hs[i];
        if (clk.on) fprintf(stderr, "[GS_CLUSTER] final dispatch: %llu rows: %.2f ms\n", (unsigned long long)k, clk.lap());
    }
    unsigned long long hall = 0;
    GS_HIP_CHECK(hipMemcpyAsync(centre_node, onode.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(centre_count, ocnt.p, 2 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(&hall, dall, 8, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    info->cost_all = hall;
    return GS_OK;
}

}  // namespace gs

extern "C" gs_cluster_params gs_cluster_params_default(void)
{
    gs_cluster_params p;
    p.n_cluster = 0; p.fraction = 0.1; p.max_iter = 15; p.seed = 0x5eed;
    return p;
}
