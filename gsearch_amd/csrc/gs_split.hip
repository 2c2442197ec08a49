// gs_split.hip — split databases (SPEC.md 17 items 12-18): the queries stay on the device while the pieces of a database pass under
// them one at a time. A piece answers the listed query rows (gs_index_parallel_search_dev on the gathered rows) and its answers are merged IN PLACE
// into the running lists of those rows, so that after the last piece the lists are what one search of the whole database would have been merged to.
//
//   k_check_rows        the row list is strictly ascending and below nq (one flag word, read before anything else is queued)
//   k_gather_row_bytes  the listed query rows one after the other, for rows that are no multiple of 16 bytes (gather_rows of gs_cluster.hip otherwise)
//   k_topk_reset        empty running lists
//   k_topk_merge_rows   one wavefront per listed row: both lists into LDS, every entry's output rank = its own index + a binary search in the other list
#include <cmath>
#include "gs_internal.hpp"

namespace gs {
namespace {

constexpr int MR_T = 64;                      // one wavefront per listed row
constexpr uint32_t MR_KMAX = KNN_MAX;         // the limit of gs_index_exact_search: 3 lists of 12 bytes per entry are 36 KB of LDS there
constexpr uint64_t NOID = ~(uint64_t)0;
constexpr uint32_t INF_BITS = 0x7F800000u;

__global__ void __launch_bounds__(256) k_check_rows(const uint32_t *__restrict__ rows, uint64_t nr, uint64_t nq, uint32_t *__restrict__ flag)
{
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nr; r += (uint64_t)gridDim.x * blockDim.x)
        if (rows[r] >= nq || (r > 0 && rows[r - 1] >= rows[r])) *flag = 1u;       // every writer writes the same word
}

__global__ void __launch_bounds__(256) k_gather_row_bytes(const uint8_t *__restrict__ data, uint64_t rowbytes, const uint32_t *__restrict__ rows, uint8_t *__restrict__ out)
{
    const uint8_t *s = data + (uint64_t)rows[blockIdx.x] * rowbytes;
    uint8_t *d = out + (uint64_t)blockIdx.x * rowbytes;
    for (uint64_t b = threadIdx.x; b < rowbytes; b += blockDim.x) d[b] = s[b];
}

__global__ void __launch_bounds__(256) k_topk_reset(uint64_t nq, uint32_t knbn, uint64_t *__restrict__ ids, float *__restrict__ dist, uint32_t *__restrict__ count,
                                                    uint64_t *__restrict__ evals)
{
    const uint64_t n = nq * knbn;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        ids[i] = NOID; dist[i] = INFINITY;
        if (i < nq) { count[i] = 0; if (evals) evals[i] = 0; }
    }
}

// (distance bits, id) ascending; distances are non-negative floats, so their bit patterns order like the values
__device__ __forceinline__ bool key_less(uint32_t d0, uint64_t i0, uint32_t d1, uint64_t i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

// Row q = rows[r] (r itself without a list). R = the first min(run_count[q], knbn) entries of the running list, A = the first min(a_count[r], knbn)
// answers of the piece with id_offset added. A search orders equal distances by node number, which need not be the order of the ids: A is first put
// in (distance, id) order - an entry that has an equal-distance neighbour finds its run by two binary searches on the distance and its place by
// counting the smaller ids of that run, everybody else keeps its index. Then every entry knows its rank in the merge without looking at more than
// log2(knbn) entries of the other list: an entry of R goes behind the entries of A that are smaller, an entry of A behind those of R that are
// smaller OR EQUAL (on a full tie the running entry goes first), so the two counts of a pair (r, a) never both include or both exclude the other and
// the ranks are a permutation. Everything is in LDS before the first store: the merge is in place.
__global__ void __launch_bounds__(MR_T) k_topk_merge_rows(const uint32_t *__restrict__ rows, uint32_t knbn, uint64_t id_offset, const uint64_t *__restrict__ a_ids,
                                                          const float *__restrict__ a_dist, const uint32_t *__restrict__ a_count, const uint64_t *__restrict__ a_evals,
                                                          uint64_t *__restrict__ run_ids, float *__restrict__ run_dist, uint32_t *__restrict__ run_count,
                                                          uint64_t *__restrict__ run_evals)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mr[];
    uint64_t *rid = (uint64_t *)s_mr, *aid = rid + knbn, *bid = aid + knbn;          // R, A as the search left it, A in (distance, id) order
    uint32_t *rd = (uint32_t *)(bid + knbn), *ad = rd + knbn, *bd = ad + knbn;
    const uint64_t r = blockIdx.x, q = rows ? rows[r] : r;
    const uint32_t lane = threadIdx.x;
    const uint32_t nR = min(run_count[q], knbn), nA = min(a_count[r], knbn);
    for (uint32_t t = lane; t < nR; t += MR_T) { rid[t] = run_ids[q * knbn + t]; rd[t] = __float_as_uint(run_dist[q * knbn + t]); }
    for (uint32_t t = lane; t < nA; t += MR_T) { aid[t] = a_ids[r * knbn + t] + id_offset; ad[t] = __float_as_uint(a_dist[r * knbn + t]); }
    __syncthreads();
    for (uint32_t t = lane; t < nA; t += MR_T) {
        const uint32_t d = ad[t]; const uint64_t id = aid[t];
        uint32_t pos = t;
        if ((t > 0 && ad[t - 1] == d) || (t + 1 < nA && ad[t + 1] == d)) {
            uint32_t lo = 0, hi = t;                                               // first entry of the run: the first index whose distance is >= d
            while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (ad[mid] < d) lo = mid + 1; else hi = mid; }
            const uint32_t first = lo;
            lo = t + 1; hi = nA;                                                    // one past its last entry: the first index whose distance is > d
            while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (ad[mid] <= d) lo = mid + 1; else hi = mid; }
            pos = first;
            for (uint32_t u = first; u < lo; u++) pos += aid[u] < id || (aid[u] == id && u < t);
        }
        bid[pos] = id; bd[pos] = d;
    }
    __syncthreads();
    const uint32_t total = min(nR + nA, knbn);
    for (uint32_t t = lane; t < nR; t += MR_T) {
        const uint32_t d = rd[t]; const uint64_t id = rid[t];
        uint32_t lo = 0, hi = nA;                                                   // entries of A below (d, id)
        while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (key_less(bd[mid], bid[mid], d, id)) lo = mid + 1; else hi = mid; }
        const uint32_t rank = t + lo;
        if (rank < knbn) { run_ids[q * knbn + rank] = id; run_dist[q * knbn + rank] = __uint_as_float(d); }
    }
    for (uint32_t t = lane; t < nA; t += MR_T) {
        const uint32_t d = bd[t]; const uint64_t id = bid[t];
        uint32_t lo = 0, hi = nR;                                                   // entries of R not above (d, id)
        while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (!key_less(d, id, rd[mid], rid[mid])) lo = mid + 1; else hi = mid; }
        const uint32_t rank = t + lo;
        if (rank < knbn) { run_ids[q * knbn + rank] = id; run_dist[q * knbn + rank] = __uint_as_float(d); }
    }
    for (uint32_t t = total + lane; t < knbn; t += MR_T) { run_ids[q * knbn + t] = NOID; run_dist[q * knbn + t] = __uint_as_float(INF_BITS); }
    if (lane == 0) {
        run_count[q] = total;
        if (run_evals) run_evals[q] += a_evals[r];
    }
}

// rows_dev[0 .. nr): strictly ascending and below nq. Waits for the stream once (the flag).
int check_rows_dev(gs_ctx *c, const uint32_t *rows_dev, uint64_t nr, uint64_t nq)
{
    PoolBuf flag(c, SL_SPLIT_FLAG);
    int rc;
    if ((rc = flag.alloc(4))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(flag.p, 0, 4, c->stream));
    hipLaunchKernelGGL(k_check_rows, dim3((uint32_t)std::min<uint64_t>((nr + 255) / 256, 1024)), dim3(256), 0, c->stream, rows_dev, nr, nq, flag.as<uint32_t>());
    GS_HIP_CHECK(hipGetLastError());
    uint32_t bad = 0;
    GS_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    GS_REQUIRE(bad == 0, GS_ERR_INVALID, "gs_index_search_merge_dev: the rows must be strictly ascending and below nq = %llu", (unsigned long long)nq);
    return GS_OK;
}

// the device form behind both entry points: the caller holds the context lock and has checked the arguments and the row list
int search_merge_dev(gs_index *piece, gs_ctx *c, size_t rowbytes, const void *queries_dev, const uint32_t *rows_dev, uint64_t nr, uint32_t knbn, uint32_t ef,
                     uint64_t id_offset, uint64_t *run_ids, float *run_dist, uint32_t *run_count, uint64_t *run_evals)
{
    PoolBuf qrows(c, SL_SPLIT_QROWS), ids(c, SL_SPLIT_IDS), dist(c, SL_SPLIT_DIST), count(c, SL_SPLIT_COUNT), evals(c, SL_SPLIT_EVALS);
    int rc;
    const void *q = queries_dev;
    if (rows_dev) {
        if ((rc = qrows.alloc(rowbytes * nr))) return rc;
        if (rowbytes % 16 == 0 && (uintptr_t)queries_dev % 16 == 0) {
            if ((rc = gather_rows(c, queries_dev, rowbytes, rows_dev, nr, qrows.p))) return rc;
        } else {
            hipLaunchKernelGGL(k_gather_row_bytes, dim3((uint32_t)nr), dim3(256), 0, c->stream, (const uint8_t *)queries_dev, (uint64_t)rowbytes, rows_dev, qrows.as<uint8_t>());
            GS_HIP_CHECK(hipGetLastError());
        }
        q = qrows.p;
    }
    if ((rc = ids.alloc(8 * nr * knbn)) || (rc = dist.alloc(4 * nr * knbn)) || (rc = count.alloc(4 * nr)) || (rc = evals.alloc(8 * nr))) return rc;
    if ((rc = gs_index_parallel_search_dev(piece, q, nr, knbn, ef, ids.as<uint64_t>(), dist.as<float>(), count.as<uint32_t>(), evals.as<uint64_t>()))) return rc;
    hipLaunchKernelGGL(k_topk_merge_rows, dim3((uint32_t)nr), dim3(MR_T), (size_t)36 * knbn, c->stream, rows_dev, knbn, id_offset, ids.as<uint64_t>(), dist.as<float>(),
                       count.as<uint32_t>(), evals.as<uint64_t>(), run_ids, run_dist, run_count, run_evals);
    GS_HIP_CHECK(hipGetLastError());
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int check_merge_args(gs_index *piece, uint64_t nq, uint64_t nr, bool listed, uint32_t knbn, uint32_t ef, size_t *rowbytes)
{
    GS_REQUIRE(piece, GS_ERR_INVALID, "null index");
    GS_REQUIRE(knbn >= 1 && ef >= 1, GS_ERR_INVALID, "knbn and ef must be positive");
    GS_REQUIRE(knbn <= MR_KMAX, GS_ERR_UNSUPPORTED, "gs_index_search_merge: knbn %u exceeds %u", knbn, MR_KMAX);
    GS_REQUIRE(nq <= 0x7FFFFFFFull, GS_ERR_UNSUPPORTED, "gs_index_search_merge: more than 2^31 - 1 queries in one call");
    GS_REQUIRE(!listed || nr <= nq, GS_ERR_INVALID, "gs_index_search_merge: %llu rows listed of %llu queries (the rows must be strictly ascending and below nq)",
               (unsigned long long)nr, (unsigned long long)nq);
    gs_index_params prm;
    int rc = gs_index_get_params(piece, &prm);
    if (rc) return rc;
    *rowbytes = (size_t)prm.m * kind_bytes(prm.kind);
    return GS_OK;
}

}  // namespace
}  // namespace gs

extern "C" {

int gs_topk_reset_dev(gs_ctx *c, uint64_t nq, uint32_t knbn, uint64_t *run_ids_dev, float *run_dist_dev, uint32_t *run_count_dev, uint64_t *run_evals_dev)
{
    GS_REQUIRE(c && knbn >= 1, GS_ERR_INVALID, "gs_topk_reset_dev: bad argument");
    if (nq == 0) return GS_OK;
    GS_REQUIRE(run_ids_dev && run_dist_dev && run_count_dev, GS_ERR_INVALID, "gs_topk_reset_dev: null argument");
    GS_CTX_LOCK(c);
    hipLaunchKernelGGL(gs::k_topk_reset, dim3((uint32_t)std::min<uint64_t>((nq * knbn + 255) / 256, 4096)), dim3(256), 0, c->stream, nq, knbn, run_ids_dev, run_dist_dev,
                       run_count_dev, run_evals_dev);
    GS_HIP_CHECK(hipGetLastError());
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_index_search_merge_dev(gs_index *piece, const void *queries_dev, uint64_t nq, const uint32_t *rows_dev, uint64_t nr, uint32_t knbn, uint32_t ef, uint64_t id_offset,
                              uint64_t *run_ids_dev, float *run_dist_dev, uint32_t *run_count_dev, uint64_t *run_evals_dev)
{
    size_t rowbytes = 0;
    int rc = gs::check_merge_args(piece, nq, nr, rows_dev != nullptr, knbn, ef, &rowbytes);
    if (rc) return rc;
    if (!rows_dev) nr = nq;
    if (nr == 0) return GS_OK;
    GS_REQUIRE(queries_dev && run_ids_dev && run_dist_dev && run_count_dev, GS_ERR_INVALID, "gs_index_search_merge_dev: null argument");
    gs_ctx *c = gs::index_ctx(piece);
    GS_CTX_LOCK(c);
    if (rows_dev && (rc = gs::check_rows_dev(c, rows_dev, nr, nq))) return rc;
    return gs::search_merge_dev(piece, c, rowbytes, queries_dev, rows_dev, nr, knbn, ef, id_offset, run_ids_dev, run_dist_dev, run_count_dev, run_evals_dev);
}

/* the host-pointer twin: the listed rows of the queries and of the running lists are gathered on the host, merged on the device as nr rows of their own,
 * and scattered back; a row that is not listed is neither read nor written */
int gs_index_search_merge(gs_index *piece, const void *queries, uint64_t nq, const uint32_t *rows, uint64_t nr, uint32_t knbn, uint32_t ef, uint64_t id_offset,
                          uint64_t *run_ids, float *run_dist, uint32_t *run_count, uint64_t *run_evals)
{
    size_t rowbytes = 0;
    int rc = gs::check_merge_args(piece, nq, nr, rows != nullptr, knbn, ef, &rowbytes);
    if (rc) return rc;
    if (!rows) nr = nq;
    if (nr == 0) return GS_OK;
    GS_REQUIRE(queries && run_ids && run_dist && run_count, GS_ERR_INVALID, "gs_index_search_merge: null argument");
    if (rows)
        for (uint64_t r = 0; r < nr; r++)
            GS_REQUIRE(rows[r] < nq && (r == 0 || rows[r - 1] < rows[r]), GS_ERR_INVALID, "gs_index_search_merge: the rows must be strictly ascending and below nq = %llu (row %llu is %u)",
                       (unsigned long long)nq, (unsigned long long)r, rows[r]);
    auto at = [&](uint64_t r) -> uint64_t { return rows ? rows[r] : r; };
    std::vector<uint8_t> hq(rowbytes * nr);
    std::vector<uint64_t> hids(nr * knbn), hev(nr, 0);
    std::vector<float> hdist(nr * knbn);
    std::vector<uint32_t> hcnt(nr);
    for (uint64_t r = 0; r < nr; r++) {
        const uint64_t q = at(r);
        std::copy_n((const uint8_t *)queries + q * rowbytes, rowbytes, hq.begin() + r * rowbytes);
        std::copy_n(run_ids + q * knbn, knbn, hids.begin() + r * knbn);
        std::copy_n(run_dist + q * knbn, knbn, hdist.begin() + r * knbn);
        hcnt[r] = run_count[q];
        if (run_evals) hev[r] = run_evals[q];
    }
    gs_ctx *c = gs::index_ctx(piece);
    GS_CTX_LOCK(c);
    gs::PoolBuf dq(c, gs::SL_SPLITB_QUERIES), dids(c, gs::SL_SPLITB_RUN_IDS), ddist(c, gs::SL_SPLITB_RUN_DIST), dcnt(c, gs::SL_SPLITB_RUN_COUNT), dev(c, gs::SL_SPLITB_RUN_EVALS);
    if ((rc = dq.alloc(hq.size())) || (rc = dids.alloc(8 * nr * knbn)) || (rc = ddist.alloc(4 * nr * knbn)) || (rc = dcnt.alloc(4 * nr)) || (rc = dev.alloc(8 * nr))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dq.p, hq.data(), hq.size(), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dids.p, hids.data(), 8 * nr * knbn, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(ddist.p, hdist.data(), 4 * nr * knbn, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dcnt.p, hcnt.data(), 4 * nr, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dev.p, hev.data(), 8 * nr, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if ((rc = gs::search_merge_dev(piece, c, rowbytes, dq.p, nullptr, nr, knbn, ef, id_offset, dids.as<uint64_t>(), ddist.as<float>(), dcnt.as<uint32_t>(), dev.as<uint64_t>())))
        return rc;
    GS_HIP_CHECK(hipMemcpyAsync(hids.data(), dids.p, 8 * nr * knbn, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(hdist.data(), ddist.p, 4 * nr * knbn, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(hcnt.data(), dcnt.p, 4 * nr, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(hev.data(), dev.p, 8 * nr, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (uint64_t r = 0; r < nr; r++) {
        const uint64_t q = at(r);
        std::copy_n(hids.begin() + r * knbn, knbn, run_ids + q * knbn);
        std::copy_n(hdist.begin() + r * knbn, knbn, run_dist + q * knbn);
        run_count[q] = hcnt[r];
        if (run_evals) run_evals[q] = hev[r];
    }
    return GS_OK;
}

}  // extern "C"
