// gs_hmh.hip — cardinality and all-pairs similarity of HyperMinHash sketches (hypermash, /root/reference/src/bin/hypermash.rs:253-275;
// the `hyperminhash` crate's Sketch::cardinality / similarity). Arithmetic: SPEC.md 7, constants in gs_spec.hpp.
//
//  * k_hmh_card   : one workgroup per sketch; empty-register count and the register sum as an exact integer (units of 2^-51), rounded once.
//  * k_hmh_cn     : Q x R tile kernel (128 x 128 pairs per workgroup, 8 x 8 per lane, K-chunks of 32 registers through LDS) for
//                   C = #{a == b != 0} and the both-empty count; an empty register is staged as a sentinel of its side (Q: 2^16, R: 2^17),
//                   so one compare per register pair gives C, and the both-empty count comes from two 32-bit masks per row and chunk.
//  * k_hmh_finish : per pair: the C == 0 / empty-sketch rules and the closed form of the expected collisions (max card > 2^19).
//  * k_hmh_pvec + k_hmh_small : the small-set branch (both cards <= 2^19). X = sum over 65536 terms of P(n) P(m') is a dot product of two
//                   vectors P(card) built once per small sketch: an f64 GEMM over the small rows, the similarity written in its epilogue.
#include <algorithm>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"

namespace gs {

constexpr uint32_t HM = GS_HMH_M;

__global__ __launch_bounds__(256) void k_hmh_card(const uint16_t *__restrict__ sigs, uint64_t n, uint64_t *__restrict__ card)
{
    __shared__ uint64_t s_hi[256], s_lo[256];
    __shared__ uint32_t s_ez[256];
    const uint64_t g = blockIdx.x;
    if (g >= n) return;
    const uint16_t *row = sigs + g * (uint64_t)HM;
    uint64_t s = 0;
    uint32_t ez = 0;
    for (uint32_t i = threadIdx.x; i < HM; i += 256) {
        const uint32_t lz = (uint32_t)row[i] >> GS_HMH_R;            // 0 (empty) .. 51
        ez += lz == 0;
        s += (uint64_t)1 << (51 - lz);                               // 2^-lz in units of 2^-51; 64 registers per lane: < 2^57
    }
    s_hi[threadIdx.x] = s >> 32; s_lo[threadIdx.x] = s & 0xFFFFFFFFull; s_ez[threadIdx.x] = ez;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { s_hi[threadIdx.x] += s_hi[threadIdx.x + o]; s_lo[threadIdx.x] += s_lo[threadIdx.x + o]; s_ez[threadIdx.x] += s_ez[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // total = hi * 2^32 + lo (hi < 2^34, lo < 2^41) as 128 bits
        const uint64_t hi = s_hi[0], lo = s_lo[0];
        const uint64_t l = lo + (hi << 32);
        const uint64_t h = (hi >> 32) + (l < lo ? 1 : 0);
        card[g] = hmh_card(s_ez[0], h, l);
    }
}

constexpr int CT = 128;        // tile edge (pairs)
constexpr int CK = 32;         // registers per K-chunk
constexpr int CP = CK + 1;     // LDS row pitch (words)
// out[q * ld + r] = C | N << 16 for q < nq, r < nr
__global__ __launch_bounds__(256) void k_hmh_cn(const uint16_t *__restrict__ Q, uint64_t nq, const uint16_t *__restrict__ R, uint64_t nr,
                                                uint32_t *__restrict__ out, uint64_t ld)
{
    __shared__ uint32_t sq[CT * CP], sr[CT * CP];
    __shared__ uint32_t mq[CT], mr[CT];
    const uint64_t q0 = (uint64_t)blockIdx.x * CT, r0 = (uint64_t)blockIdx.y * CT;
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    // low 16 bits: C so far; high 16 bits: both-empty count so far (each <= 16384)
    uint32_t cnt[8][8];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) cnt[i][j] = 0;
    for (uint32_t k0 = 0; k0 < HM; k0 += CK) {
        // staging: 128 rows x 32 registers per side = 512 x 16 B; lane handles 2 + 2, four lanes per row
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const uint16_t *src = side ? R : Q;
            const uint64_t base = side ? r0 : q0, lim = side ? nr : nq;
            uint32_t *dst = side ? sr : sq, *msk = side ? mr : mq;
            const uint32_t sent = side ? 0x20000u : 0x10000u;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t idx = threadIdx.x + 256 * h, row = idx >> 2, part = idx & 3;
                const uint64_t gr = base + row < lim ? base + row : lim - 1;          // clamped rows: results discarded
                const uint4 v = *(const uint4 *)(src + gr * HM + k0 + part * 8);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t m8 = 0;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t a = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                    dst[row * CP + part * 8 + e] = a ? a : sent;
                    m8 |= (uint32_t)(a == 0) << e;
                }
                uint32_t m32 = m8 << (8 * part);
                m32 |= __shfl_xor(m32, 1);
                m32 |= __shfl_xor(m32, 2);
                if (part == 0) msk[row] = m32;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < CK; kk++) {
            uint32_t a[8], b[8];
#pragma unroll
            for (int i = 0; i < 8; i++) { a[i] = sq[(ty + 16 * i) * CP + kk]; b[i] = sr[(tx + 16 * i) * CP + kk]; }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 8; j++) cnt[i][j] += a[i] == b[j] ? 1u : 0u;
        }
        {
            uint32_t a[8], b[8];
#pragma unroll
            for (int i = 0; i < 8; i++) { a[i] = mq[ty + 16 * i]; b[i] = mr[tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 8; j++) cnt[i][j] += (uint32_t)__popc(a[i] & b[j]) << 16;
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t q = q0 + ty + 16 * i;
        if (q >= nq) continue;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t r = r0 + tx + 16 * j;
            if (r >= nr) continue;
            const uint32_t C = cnt[i][j] & 0xFFFFu, both = cnt[i][j] >> 16;
            out[q * ld + r] = C | ((HM - both) << 16);
        }
    }
}

// the pairs the small-set GEMM does not take: C == 0, an empty sketch (card 0), or max card > 2^19
__global__ void k_hmh_finish(const uint32_t *__restrict__ cn, uint64_t nq, uint64_t nr, const uint64_t *__restrict__ cq, const uint64_t *__restrict__ cr,
                             double *__restrict__ sim)
{
    const uint64_t total = nq * nr;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = t / nr, r = t - q * nr;
        const uint32_t v = cn[t], C = v & 0xFFFFu, N = v >> 16;
        const uint64_t a = cq[q], b = cr[r];
        if (C == 0 || a == 0 || b == 0) { sim[t] = 0.0; continue; }
        const double n = (double)(a > b ? a : b), mn = (double)(a > b ? b : a);
        if (!(n > GS_HMH_SMALL)) continue;                           // small-set branch: k_hmh_small
        sim[t] = hmh_sim_from(C, N, hmh_ec_closed(n, mn));
    }
}

// P(card)[t] = (1 - b2)^card - (1 - b1)^card for the 65536 terms t of the small-set sum, one vector per listed sketch
__global__ void k_hmh_pvec(const uint64_t *__restrict__ card, const uint32_t *__restrict__ list, uint32_t n, double *__restrict__ out)
{
    const uint64_t total = (uint64_t)n * GS_HMH_NP;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)(x / GS_HMH_NP), t = (uint32_t)(x % GS_HMH_NP);
        const double c = (double)card[list[s]];
        double b1, b2;
        hmh_b(t, b1, b2);
        out[x] = pow(1.0 - b2, c) - pow(1.0 - b1, c);
    }
}

// X for every (listed query, listed reference) pair = PQ[i] . PR[j] (64 x 64 pairs per workgroup, 4 x 4 per lane, K-chunks of 32 terms
// through LDS), then ec = X + 0.5 / p and the similarity of the pair
constexpr int ST = 64, SK = 32, SP = SK + 1;
__global__ __launch_bounds__(256) void k_hmh_small(const double *__restrict__ PQ, const uint32_t *__restrict__ lq, uint32_t nlq, const double *__restrict__ PR,
                                                   const uint32_t *__restrict__ lr, uint32_t nlr, const uint32_t *__restrict__ cn, uint64_t ld,
                                                   double *__restrict__ sim)
{
    __shared__ double sa[ST * SP], sb[ST * SP];
    const uint32_t i0 = blockIdx.x * ST, j0 = blockIdx.y * ST;
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    for (uint32_t k0 = 0; k0 < GS_HMH_NP; k0 += SK) {
        // 64 rows x 32 terms per side = 2048 doubles: 8 per lane and side
#pragma unroll
        for (int h = 0; h < 8; h++) {
            const uint32_t idx = threadIdx.x + 256 * h, row = idx >> 5, col = idx & 31;
            const uint32_t ra = i0 + row < nlq ? i0 + row : nlq - 1, rb = j0 + row < nlr ? j0 + row : nlr - 1;
            sa[row * SP + col] = PQ[(uint64_t)ra * GS_HMH_NP + k0 + col];
            sb[row * SP + col] = PR[(uint64_t)rb * GS_HMH_NP + k0 + col];
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < SK; kk++) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[i] = sa[(ty + 16 * i) * SP + kk]; b[i] = sb[(tx + 16 * i) * SP + kk]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i0 + ty + 16 * i >= nlq) continue;
        const uint64_t q = lq[i0 + ty + 16 * i];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j0 + tx + 16 * j >= nlr) continue;
            const uint64_t r = lr[j0 + tx + 16 * j];
            const uint32_t v = cn[q * ld + r], C = v & 0xFFFFu, N = v >> 16;
            if (C == 0) continue;                                         // (k_hmh_finish wrote 0)
            sim[q * ld + r] = hmh_sim_from(C, N, acc[i][j] + 0.5 / (double)GS_HMH_P);
        }
    }
}

int hmh_cardinality_dev(gs_ctx *c, const uint16_t *sigs, uint64_t n, uint64_t *card)
{
    if (n == 0) return GS_OK;
    for (uint64_t g0 = 0; g0 < n; g0 += 1u << 30) {
        const uint64_t ng = std::min<uint64_t>(n - g0, 1u << 30);
        hipLaunchKernelGGL(k_hmh_card, dim3((uint32_t)ng), dim3(256), 0, c->stream, sigs + g0 * HM, ng, card + g0);
        GS_HIP_CHECK(hipGetLastError());
    }
    return GS_OK;
}

// pairs of query rows [qa, qb) x all references: rows of `sim` (ld = nr) and of the C | N matrix (`cn`, row qa first)
static int hmh_similarity_dev(gs_ctx *c, const uint16_t *Q, uint64_t nq, const uint16_t *R, uint64_t nr, double *sim)
{
    int rc;
    PoolBuf cq(c, SL_HMH_CARD_Q), cr(c, SL_HMH_CARD_R), cnb(c, SL_HMH_NB), pq(c, SL_HMH_PACK_Q), pr(c, SL_HMH_PACK_R), lst(c, SL_HMH_LIST);
    if ((rc = cq.alloc(8 * nq)) || (rc = cr.alloc(8 * nr))) return rc;
    if ((rc = hmh_cardinality_dev(c, Q, nq, cq.as<uint64_t>())) || (rc = hmh_cardinality_dev(c, R, nr, cr.as<uint64_t>()))) return rc;
    // which sketches take the small-set branch with which: card in [1, 2^19]
    std::vector<uint64_t> hq(nq), hr(nr);
    GS_HIP_CHECK(hipMemcpyAsync(hq.data(), cq.p, 8 * nq, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(hr.data(), cr.p, 8 * nr, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> sq_all, sr_all;
    for (uint64_t i = 0; i < nq; i++) if (hq[i] && !((double)hq[i] > GS_HMH_SMALL)) sq_all.push_back((uint32_t)i);
    for (uint64_t i = 0; i < nr; i++) if (hr[i] && !((double)hr[i] > GS_HMH_SMALL)) sr_all.push_back((uint32_t)i);
    // query rows per pass: the C | N matrix of a pass stays under 1 GB
    const uint64_t qpass = std::max<uint64_t>(CT, ((uint64_t)1 << 28) / std::max<uint64_t>(nr, 1) / CT * CT);
    // small sketches per P-vector block: 2048 x 512 kB = 1 GB per side
    constexpr uint32_t PB = 2048;
    if ((rc = cnb.alloc(4 * std::min(qpass, nq) * nr))) return rc;
    if (!sq_all.empty() && !sr_all.empty()) {
        if ((rc = pq.alloc((size_t)8 * GS_HMH_NP * std::min<size_t>(PB, sq_all.size()))) || (rc = pr.alloc((size_t)8 * GS_HMH_NP * std::min<size_t>(PB, sr_all.size()))) ||
            (rc = lst.alloc(4 * (sq_all.size() + sr_all.size())))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(lst.p, sq_all.data(), 4 * sq_all.size(), hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(lst.as<uint32_t>() + sq_all.size(), sr_all.data(), 4 * sr_all.size(), hipMemcpyHostToDevice, c->stream));
    }
    const uint32_t *dlq = lst.as<uint32_t>(), *dlr = lst.as<uint32_t>() + sq_all.size();
    size_t s_lo = 0;                                                     // first small query row of the pass
    for (uint64_t qa = 0; qa < nq; qa += qpass) {
        const uint64_t qn = std::min(qpass, nq - qa);
        {
            ProfScope ps(c, FAM_HAMMING);
            hipLaunchKernelGGL(k_hmh_cn, dim3((uint32_t)((qn + CT - 1) / CT), (uint32_t)((nr + CT - 1) / CT)), dim3(256), 0, c->stream, Q + qa * HM, qn, R, nr,
                               cnb.as<uint32_t>(), nr);
            GS_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_hmh_finish, dim3((uint32_t)std::min<uint64_t>((qn * nr + 255) / 256, 1u << 16)), dim3(256), 0, c->stream, cnb.as<uint32_t>(), qn, nr,
                           cq.as<uint64_t>() + qa, cr.as<uint64_t>(), sim + qa * nr);
        GS_HIP_CHECK(hipGetLastError());
        size_t s_hi = s_lo;
        while (s_hi < sq_all.size() && sq_all[s_hi] < qa + qn) s_hi++;
        if (sr_all.empty()) { s_lo = s_hi; continue; }
        for (size_t a0 = s_lo; a0 < s_hi; a0 += PB) {
            const uint32_t na = (uint32_t)std::min<size_t>(PB, s_hi - a0);
            hipLaunchKernelGGL(k_hmh_pvec, dim3(8192), dim3(256), 0, c->stream, cq.as<uint64_t>(), dlq + a0, na, pq.as<double>());
            GS_HIP_CHECK(hipGetLastError());
            // (rows of the pass: the lists hold absolute query numbers, the C | N matrix and `sim` are offset to the pass)
            std::vector<uint32_t> rel(sq_all.begin() + a0, sq_all.begin() + a0 + na);
            for (auto &x : rel) x -= (uint32_t)qa;
            PoolBuf lrel(c, SL_HMH_LIST_REL);
            if ((rc = lrel.alloc(4 * (size_t)na))) return rc;
            GS_HIP_CHECK(hipMemcpyAsync(lrel.p, rel.data(), 4 * (size_t)na, hipMemcpyHostToDevice, c->stream));
            for (size_t b0 = 0; b0 < sr_all.size(); b0 += PB) {
                const uint32_t nb = (uint32_t)std::min<size_t>(PB, sr_all.size() - b0);
                hipLaunchKernelGGL(k_hmh_pvec, dim3(8192), dim3(256), 0, c->stream, cr.as<uint64_t>(), dlr + b0, nb, pr.as<double>());
                GS_HIP_CHECK(hipGetLastError());
                ProfScope ps(c, FAM_HAMMING);
                hipLaunchKernelGGL(k_hmh_small, dim3((na + ST - 1) / ST, (nb + ST - 1) / ST), dim3(256), 0, c->stream, pq.as<double>(), lrel.as<uint32_t>(), na,
                                   pr.as<double>(), dlr + b0, nb, cnb.as<uint32_t>(), nr, sim + qa * nr);
                GS_HIP_CHECK(hipGetLastError());
            }
            // (lrel's lease ends with this iteration and the next block takes SL_HMH_LIST_REL again and rewrites it: wait for this block's kernels first)
            GS_HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        s_lo = s_hi;
        // (the C | N buffer is rewritten by the next pass: stream order keeps it safe)
    }
    return GS_OK;
}

}  // namespace gs

extern "C" {

int gs_hmh_cardinality_dev(gs_ctx *c, const uint16_t *sigs_dev, uint64_t n, uint64_t *card_out_dev)
{
    GS_REQUIRE(c && (n == 0 || (sigs_dev && card_out_dev)), GS_ERR_INVALID, "null argument");
    GS_CTX_LOCK(c);
    return gs::hmh_cardinality_dev(c, sigs_dev, n, card_out_dev);
}

int gs_hmh_cardinality(gs_ctx *c, const uint16_t *sigs, uint64_t n, uint64_t *card_out)
{
    GS_REQUIRE(c && (n == 0 || (sigs && card_out)), GS_ERR_INVALID, "null argument");
    GS_CTX_LOCK(c);
    if (n == 0) return GS_OK;
    int rc;
    gs::PoolBuf ds(c, gs::SL_HMHC_SIGS), dc(c, gs::SL_HMHC_CARD);
    if ((rc = ds.alloc((size_t)2 * GS_HMH_M * n)) || (rc = dc.alloc(8 * n))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(ds.p, sigs, (size_t)2 * GS_HMH_M * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = gs::hmh_cardinality_dev(c, ds.as<uint16_t>(), n, dc.as<uint64_t>()))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(card_out, dc.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_hmh_similarity_qxc_dev(gs_ctx *c, const uint16_t *Q_dev, uint64_t nq, const uint16_t *R_dev, uint64_t nr, double *sim_out_dev)
{
    GS_REQUIRE(c && (nq == 0 || nr == 0 || (Q_dev && R_dev && sim_out_dev)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(nq < ((uint64_t)1 << 31) && nr < (uint64_t)65535 * 128, GS_ERR_INVALID, "too many sketches in one call");
    GS_CTX_LOCK(c);
    if (nq == 0 || nr == 0) return GS_OK;
    return gs::hmh_similarity_dev(c, Q_dev, nq, R_dev, nr, sim_out_dev);
}

int gs_hmh_similarity_qxc(gs_ctx *c, const uint16_t *Q, uint64_t nq, const uint16_t *R, uint64_t nr, double *sim_out)
{
    GS_REQUIRE(c && (nq == 0 || nr == 0 || (Q && R && sim_out)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(nq < ((uint64_t)1 << 31) && nr < (uint64_t)65535 * 128, GS_ERR_INVALID, "too many sketches in one call");
    GS_CTX_LOCK(c);
    if (nq == 0 || nr == 0) return GS_OK;
    int rc;
    gs::PoolBuf dq(c, gs::SL_HMHS_Q), dr(c, gs::SL_HMHS_R), ds(c, gs::SL_HMHS_SIM);
    if ((rc = dq.alloc((size_t)2 * GS_HMH_M * nq)) || (rc = dr.alloc((size_t)2 * GS_HMH_M * nr)) || (rc = ds.alloc((size_t)8 * nq * nr))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(dq.p, Q, (size_t)2 * GS_HMH_M * nq, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(dr.p, R, (size_t)2 * GS_HMH_M * nr, hipMemcpyHostToDevice, c->stream));
    if ((rc = gs::hmh_similarity_dev(c, dq.as<uint16_t>(), nq, dr.as<uint16_t>(), nr, ds.as<double>()))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(sim_out, ds.p, (size_t)8 * nq * nr, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GS_OK;
}

double gs_hmh_distance(double sim, int k)
{
    return 1.0 - pow(2.0 * sim / (1.0 + sim), 1.0 / (double)k);
}

}  // extern "C"
