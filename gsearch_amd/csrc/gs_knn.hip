// gs_knn.hip — exact k nearest nodes from rows of the 16-bit count matrix.
//
// gs_index_exact_search / gs_index_knn_graph produce a block of count rows with dense_counts (match-join or compare tile kernel, gs_index.hip)
// and hand it here. One workgroup owns one row of n counts (leading dimension ld, a multiple of 8; the pad columns are never read as
// entries) and selects its k smallest (count, node) keys among the entries with count <= c_max, node != the excluded diagonal node:
//   pass 1: 256-bin LDS histogram of the count's high byte            -> the bin b1 that holds the k-th entry
//   pass 2: 256-bin LDS histogram of the low byte of entries in b1    -> the exact k-th count t, and `need` = how many entries equal to t are kept
//   pass 3: every entry below t plus the first `need` entries equal to t in node order, placed by a block-wide prefix sum (no atomics: the set of
//           kept ties is the first ones by node number, the tie rule of the search)
//   sort  : bitonic sort of the <= 1024 keys in LDS, then the row's knbn answers (unused slots: UINT64_MAX / +inf)
// A row is read three times, 16 bytes per lane and load. Histogram adds are merged per lane over runs of equal bins first: at s = 18000 most
// counts of unrelated genomes share one high byte, and 64 lanes adding to one LDS word serialise.
#include "gs_internal.hpp"
#include "gs_countrow.hpp"

namespace gs {
namespace {

constexpr int KT = 256;                  // threads per workgroup = histogram bins
constexpr int KW = KT / 64;              // waves per workgroup
constexpr int KU = 4;                    // 16-byte loads in flight per lane in the histogram passes

struct KnnLds {
    uint32_t hist[256];
    uint32_t wsum[2][KW];
    uint32_t sel[4];
    uint64_t keys[KNN_MAX];
};

// histogram of bin(c) over the row's entries that pass `keep`; adds of equal consecutive bins of a lane are merged
template <class Keep, class Bin>
__device__ __forceinline__ void row_hist(const uint4 *rv, uint32_t nv, uint32_t n, uint32_t *hist, Keep keep, Bin bin)
{
    uint32_t cur = 0, run = 0;
    for (uint32_t v0 = threadIdx.x; v0 < nv; v0 += KU * KT) {
        uint4 x[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) x[u] = v0 + u * KT < nv ? rv[v0 + u * KT] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const uint32_t v = v0 + u * KT;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint32_t j = v * 8 + e, c = count16(x[u], e);
                if (v < nv && j < n && keep(j, c)) {
                    const uint32_t b = bin(c);
                    if (run && b != cur) { atomicAdd(&hist[cur], run); run = 0; }
                    cur = b; run++;
                }
            }
        }
    }
    if (run) atomicAdd(&hist[cur], run);
}

__global__ void __launch_bounds__(KT) k_knn_select(const uint16_t *__restrict__ mat, uint64_t ld, uint32_t n, uint32_t knbn, uint32_t c_max, uint64_t diag0,
                                                   uint32_t m, uint64_t *__restrict__ ids, float *__restrict__ dist, uint32_t *__restrict__ count)
{
    __shared__ KnnLds L;
    const uint32_t tid = threadIdx.x, r = blockIdx.x;
    const uint4 *rv = (const uint4 *)(mat + (uint64_t)r * ld);
    const uint32_t nv = (n + 7) / 8;
    const uint32_t excl = diag0 == ~(uint64_t)0 ? 0xFFFFFFFFu : (uint32_t)(diag0 + r);
    auto eligible = [&](uint32_t j, uint32_t c) { return c <= c_max && j != excl; };

    // pass 1: high byte
    L.hist[tid] = 0;
    __syncthreads();
    row_hist(rv, nv, n, L.hist, eligible, [](uint32_t c) { return c >> 8; });
    __syncthreads();
    uint32_t h = L.hist[tid], tot;
    uint32_t ex = block_excl_scan<KW>(h, L.wsum[0], tot);
    uint32_t K, t, n_less;
    if (tot <= knbn) {                   // every eligible entry is kept: all of them count as "below t"
        K = tot; t = c_max + 1; n_less = tot;
    } else {
        K = knbn;
        if (ex < K && ex + h >= K) { L.sel[0] = tid; L.sel[1] = ex; }
        L.hist[tid] = 0;                 // (every thread read its own bin before the scan's barrier)
        __syncthreads();
        const uint32_t b1 = L.sel[0], before1 = L.sel[1];
        // pass 2: low byte inside bin b1
        row_hist(rv, nv, n, L.hist, [&](uint32_t j, uint32_t c) { return eligible(j, c) && (c >> 8) == b1; }, [](uint32_t c) { return c & 0xFFu; });
        __syncthreads();
        h = L.hist[tid];
        ex = block_excl_scan<KW>(h, L.wsum[1], tot);
        const uint32_t K2 = K - before1;
        if (ex < K2 && ex + h >= K2) { L.sel[2] = (b1 << 8) | tid; L.sel[3] = before1 + ex; }
        __syncthreads();
        t = L.sel[2]; n_less = L.sel[3];
    }
    const uint32_t need = K - n_less;    // entries equal to t that are kept (the first ones in node order)

    // pass 3: ordered compaction, one 16-byte load per lane and step (lane order = node order), the next step's load in flight
    uint32_t run_less = 0, run_eq = 0, par = 1;       // (wsum[0] may still be read by the pass-1 scan when pass 2 was skipped)
    uint4 x = tid < nv ? rv[tid] : make_uint4(0, 0, 0, 0);
    for (uint32_t base = 0; base < nv; base += KT) {
        const uint32_t v = base + tid;
        const uint4 nxt = v + KT < nv ? rv[v + KT] : make_uint4(0, 0, 0, 0);
        uint32_t less = 0, eq = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t j = v * 8 + e, c = count16(x, e);
            const bool el = v < nv && j < n && eligible(j, c);
            less += el && c < t;
            eq += el && c == t;
        }
        uint32_t btot;                   // (per step at most 2048 of each: the two 16-bit halves do not carry into each other)
        const uint32_t pre = block_excl_scan<KW>(less | (eq << 16), L.wsum[par], btot);
        par ^= 1;
        if (less | eq) {
            uint32_t pl = run_less + (pre & 0xFFFFu), pe = run_eq + (pre >> 16);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint32_t j = v * 8 + e, c = count16(x, e);
                if (!(j < n && eligible(j, c))) continue;
                const uint64_t key = ((uint64_t)c << 32) | j;
                if (c < t) { if (pl < n_less) L.keys[pl] = key; pl++; }
                else if (c == t) { if (pe < need) L.keys[n_less + pe] = key; pe++; }
            }
        }
        run_less += btot & 0xFFFFu; run_eq += btot >> 16;
        if (run_less >= n_less && run_eq >= need) break;          // (uniform: block totals)
        x = nxt;
    }

    // sort the K keys (ascending (count, node)); pad to a power of two with keys that sort last
    uint32_t P = 1;
    while (P < K) P <<= 1;
    for (uint32_t i = K + tid; i < P; i += KT) L.keys[i] = ~(uint64_t)0;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += KT) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t a = L.keys[i], b = L.keys[l];
                    if ((a > b) == ((i & k) == 0)) { L.keys[i] = b; L.keys[l] = a; }
                }
            }
            __syncthreads();
        }
    const uint64_t o = (uint64_t)r * knbn;
    for (uint32_t i = tid; i < knbn; i += KT) {
        if (i < K) {
            const uint64_t key = L.keys[i];
            ids[o + i] = (uint32_t)key;
            dist[o + i] = (float)(uint32_t)(key >> 32) / (float)m;
        } else {
            ids[o + i] = ~(uint64_t)0;
            dist[o + i] = INFINITY;
        }
    }
    if (tid == 0) count[r] = K;
}

}  // namespace

int knn_select(gs_ctx *c, const uint16_t *mat, uint64_t ld, uint64_t nrows, uint64_t n, uint32_t knbn, uint32_t c_max, uint64_t diag0, uint32_t m,
               uint64_t *ids, float *dist, uint32_t *count)
{
    GS_REQUIRE(knbn >= 1 && knbn <= (uint32_t)KNN_MAX, GS_ERR_INVALID, "knbn must be in 1..%d", (int)KNN_MAX);
    GS_REQUIRE(ld % 8 == 0 && ld >= n && n < 0xFFFFFFFFull && c_max <= 65535, GS_ERR_INVALID, "knn_select: bad row shape");
    GS_REQUIRE(((uintptr_t)mat & 15) == 0, GS_ERR_INVALID, "knn_select: count rows must be 16-byte aligned");
    if (nrows == 0) return GS_OK;
    GS_REQUIRE(nrows <= 0x7FFFFFFFull, GS_ERR_INVALID, "knn_select: too many rows in one launch");
    ProfScope ps(c, FAM_SEARCH);
    hipLaunchKernelGGL(k_knn_select, dim3((uint32_t)nrows), dim3(KT), 0, c->stream, mat, ld, (uint32_t)n, knbn, c_max, diag0, m, ids, dist, count);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

}  // namespace gs
