// gs_hmm_hits.hip — best hits become sketcher records (SPEC 13.8): the [n_genomes][n_prof] matrix gs_hmm_best_hits_dev leaves, optionally with the spans
// a trace, the envelopes or the alignments of its pairs give, -> the chosen residues back to back in (genome, profile) order with the descriptors
// gs_sketch_batch_dev reads. Three steps on the device:
//   k_hit_spans   one thread per (genome, profile): hit or not, where its residues start in the source and how many they are; what is wrong goes to one word
//   k_gene_scan   the library's one-workgroup prefix sum (gs_gene.hip) over the hit flags and over the lengths; the two totals -> ONE read-back
//   k_hit_copy    one wavefront per hit: its descriptors, then its residues byte by byte (any alignment of source and destination; the volume is a few
//                 hundred residues a hit next to a profile search)
// Nothing is written to the caller's arrays before the counts, the spans and the capacities have been checked. The host form is the same rules in plain C++.
#include "gs_internal.hpp"
#include "gs_spec.hpp"

namespace gs {

__global__ void k_gene_scan(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ total);      // gs_gene.hip

enum : uint32_t { HIT_BAD_REC = 1, HIT_BAD_SPAN = 2, HIT_MANY_ITEMS = 4 };

// pair h of the matrix -> 0: no hit; 1: a hit of *len residues from byte *src of the source; otherwise the HIT_ bit of what is wrong with it
GS_HD uint32_t hit_span(uint64_t h, const uint32_t *best_rec, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *n_item,
                        const int32_t *item, uint32_t item_words, uint32_t max_item, uint64_t *src, uint64_t *len, uint32_t *bad)
{
    *src = 0; *len = 0; *bad = 0;
    const uint32_t r = best_rec[h];
    if (r == GS_HMM_NO_HIT) return 0;
    if (r >= n_rec) { *bad = HIT_BAD_REC; return 0; }
    const uint64_t L = rec_len[r];
    uint64_t a = 0, b = L;
    const uint32_t ni = n_item ? n_item[h] : 0;
    if (ni > max_item) { *bad = HIT_MANY_ITEMS; return 0; }
    if (ni) {
        const int64_t i_from = item[(h * max_item) * item_words], i_to = item[(h * max_item + ni - 1) * item_words + 1];
        if (i_from < 1 || i_to < i_from - 1 || (uint64_t)i_to > L) { *bad = HIT_BAD_SPAN; return 0; }
        a = (uint64_t)(i_from - 1); b = (uint64_t)i_to;
    }
    *src = rec_start[r] + a; *len = b - a;
    return 1;
}

__global__ __launch_bounds__(256) void k_hit_spans(const uint32_t *__restrict__ best_rec, uint64_t n, const uint64_t *__restrict__ rec_start,
                                                   const uint64_t *__restrict__ rec_len, uint64_t n_rec, const uint32_t *__restrict__ n_item,
                                                   const int32_t *__restrict__ item, uint32_t item_words, uint32_t max_item, uint64_t *__restrict__ flag,
                                                   uint64_t *__restrict__ len, uint64_t *__restrict__ src, uint32_t *__restrict__ err)
{
    const uint64_t h = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n) return;
    uint64_t s, l;
    uint32_t bad;
    flag[h] = hit_span(h, best_rec, rec_start, rec_len, n_rec, n_item, item, item_words, max_item, &s, &l, &bad);
    len[h] = l; src[h] = s;
    if (bad) atomicOr(err, bad);
}

// pos[0..n]: hits in front of pair h (pos[n] = all of them), off[0..n]: their residues. One wavefront a pair; a pair without a hit writes nothing but, as
// the first of its genome, the genome's offset.
enum { HIT_COPY_WAVES = 4 };
__global__ __launch_bounds__(64 * HIT_COPY_WAVES) void k_hit_copy(uint64_t n, uint64_t n_prof, const uint64_t *__restrict__ pos, const uint64_t *__restrict__ off,
                                                                  const uint64_t *__restrict__ len, const uint64_t *__restrict__ src, const uint8_t *__restrict__ aa,
                                                                  uint8_t *__restrict__ out_aa, uint64_t *__restrict__ out_start, uint64_t *__restrict__ out_len,
                                                                  uint64_t *__restrict__ out_goff)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t h = (uint64_t)blockIdx.x * HIT_COPY_WAVES + (threadIdx.x >> 6); h < n; h += (uint64_t)gridDim.x * HIT_COPY_WAVES) {
        const uint64_t j = pos[h];
        if (lane == 0) {
            if (h % n_prof == 0) out_goff[h / n_prof] = j;
            if (h == n - 1) out_goff[n / n_prof] = pos[n];
        }
        if (pos[h + 1] == j) continue;
        const uint64_t o = off[h], l = len[h];
        if (lane == 0) { out_start[j] = o; out_len[j] = l; }
        const uint8_t *from = aa + src[h];
        for (uint64_t i = lane; i < l; i += 64) out_aa[o + i] = from[i];
    }
}

static int hit_check_args(const void *best_rec, uint64_t n_genomes, uint64_t n_prof, const void *aa, const void *rec_start, const void *rec_len, uint64_t n_rec,
                          const void *n_item, const void *item, uint32_t item_words, uint32_t max_item, const void *out_aa, const void *out_start,
                          const void *out_len, const void *out_goff, const uint64_t *n_out)
{
    GS_REQUIRE(n_out && out_goff, GS_ERR_INVALID, "hit records: null argument");
    GS_REQUIRE(n_genomes == 0 || n_prof == 0 || best_rec, GS_ERR_INVALID, "hit records: null argument");
    GS_REQUIRE(n_rec == 0 || (aa && rec_start && rec_len), GS_ERR_INVALID, "hit records: null argument");
    GS_REQUIRE(n_rec < (1ull << 32), GS_ERR_UNSUPPORTED, "hit records: 2^32 records or more in one call");
    GS_REQUIRE(n_prof < (1ull << 32) && n_genomes < (1ull << 32) && n_genomes * n_prof < (1ull << 32), GS_ERR_UNSUPPORTED, "hit records: 2^32 (genome, profile) pairs or more");
    GS_REQUIRE((n_item == nullptr) == (item == nullptr), GS_ERR_INVALID, "hit records: n_item and item go together");
    GS_REQUIRE(!n_item || (item_words >= 2 && max_item >= 1), GS_ERR_INVALID, "hit records: spans need item_words >= 2 and max_item >= 1");
    return GS_OK;
}

static int hit_report(uint32_t err, uint32_t max_item)
{
    GS_REQUIRE(!(err & HIT_MANY_ITEMS), GS_ERR_INVALID, "hit records: a hit has more than max_item = %u items: run again with room", max_item);
    GS_REQUIRE(!(err & HIT_BAD_REC), GS_ERR_INVALID, "hit records: a best record that is neither GS_HMM_NO_HIT nor below n_rec");
    GS_REQUIRE(!(err & HIT_BAD_SPAN), GS_ERR_INVALID, "hit records: a span outside its record");
    return GS_OK;
}

static int hit_check_caps(const uint64_t n_out[2], uint64_t cap_rec, uint64_t cap_aa, const void *out_aa, const void *out_start, const void *out_len)
{
    GS_REQUIRE(n_out[0] <= cap_rec && n_out[1] <= cap_aa, GS_ERR_INVALID, "hit records: %llu records of %llu residues, room for %llu and %llu",
               (unsigned long long)n_out[0], (unsigned long long)n_out[1], (unsigned long long)cap_rec, (unsigned long long)cap_aa);
    GS_REQUIRE((n_out[0] == 0 || (out_start && out_len)) && (n_out[1] == 0 || out_aa), GS_ERR_INVALID, "hit records: null output");
    return GS_OK;
}

}  // namespace gs

extern "C" {

int gs_hmm_hit_records_dev(gs_ctx *c, const uint32_t *best_rec_dev, uint64_t n_genomes, uint64_t n_prof, const uint8_t *aa_dev, const uint64_t *rec_start_dev,
                           const uint64_t *rec_len_dev, uint64_t n_rec, const uint32_t *n_item_dev, const int32_t *item_dev, uint32_t item_words, uint32_t max_item,
                           uint64_t cap_rec, uint64_t cap_aa, uint8_t *out_aa_dev, uint64_t *out_start_dev, uint64_t *out_len_dev, uint64_t *out_genome_off_dev,
                           uint64_t n_out[2])
{
    using namespace gs;
    GS_REQUIRE(c, GS_ERR_INVALID, "hit records: null context");
    int rc = hit_check_args(best_rec_dev, n_genomes, n_prof, aa_dev, rec_start_dev, rec_len_dev, n_rec, n_item_dev, item_dev, item_words, max_item, out_aa_dev,
                            out_start_dev, out_len_dev, out_genome_off_dev, n_out);
    if (rc) return rc;
    GS_CTX_LOCK(c);
    const uint64_t n = n_genomes * n_prof;
    if (n == 0) {
        n_out[0] = n_out[1] = 0;
        GS_HIP_CHECK(hipMemsetAsync(out_genome_off_dev, 0, 8 * (n_genomes + 1), c->stream));
        GS_HIP_CHECK(stream_wait(c));
        return GS_OK;
    }
    PoolBuf flag(c, SL_HMMH_FLAG), len(c, SL_HMMH_LEN), src(c, SL_HMMH_SRC), pos(c, SL_HMMH_POS), off(c, SL_HMMH_OFF), meta(c, SL_HMMH_META);
    if ((rc = flag.alloc(8 * n)) || (rc = len.alloc(8 * n)) || (rc = src.alloc(8 * n)) || (rc = pos.alloc(8 * (n + 1))) || (rc = off.alloc(8 * (n + 1))) ||
        (rc = meta.alloc(8 * 3)))
        return rc;
    uint64_t *m = meta.as<uint64_t>();                      // hits, residues, what is wrong
    uint64_t got[3];
    {
        ProfScope ps(c, FAM_SEARCH);
        GS_HIP_CHECK(hipMemsetAsync(m, 0, 8 * 3, c->stream));
        hipLaunchKernelGGL(k_hit_spans, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, best_rec_dev, n, rec_start_dev, rec_len_dev, n_rec, n_item_dev,
                           item_dev, item_words, max_item, flag.as<uint64_t>(), len.as<uint64_t>(), src.as<uint64_t>(), (uint32_t *)(m + 2));
        hipLaunchKernelGGL(k_gene_scan, dim3(1), dim3(1024), 0, c->stream, flag.as<uint64_t>(), n, pos.as<uint64_t>(), m);
        hipLaunchKernelGGL(k_gene_scan, dim3(1), dim3(1024), 0, c->stream, len.as<uint64_t>(), n, off.as<uint64_t>(), m + 1);
        GS_HIP_CHECK(hipGetLastError());
    }
    GS_HIP_CHECK(hipMemcpyAsync(got, m, 8 * 3, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    if ((rc = hit_report((uint32_t)got[2], max_item))) return rc;
    n_out[0] = got[0]; n_out[1] = got[1];
    if ((rc = hit_check_caps(n_out, cap_rec, cap_aa, out_aa_dev, out_start_dev, out_len_dev))) return rc;
    {
        ProfScope ps(c, FAM_SEARCH);
        const uint64_t blocks = std::min<uint64_t>((n + HIT_COPY_WAVES - 1) / HIT_COPY_WAVES, 1u << 20);
        hipLaunchKernelGGL(k_hit_copy, dim3((uint32_t)blocks), dim3(64 * HIT_COPY_WAVES), 0, c->stream, n, n_prof, pos.as<uint64_t>(), off.as<uint64_t>(),
                           len.as<uint64_t>(), src.as<uint64_t>(), aa_dev, out_aa_dev, out_start_dev, out_len_dev, out_genome_off_dev);
        GS_HIP_CHECK(hipGetLastError());
    }
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

int gs_hmm_hit_records(gs_ctx *c, const uint32_t *best_rec, uint64_t n_genomes, uint64_t n_prof, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len,
                       uint64_t n_rec, const uint32_t *n_item, const int32_t *item, uint32_t item_words, uint32_t max_item, uint64_t cap_rec, uint64_t cap_aa,
                       uint8_t *out_aa, uint64_t *out_start, uint64_t *out_len, uint64_t *out_genome_off, uint64_t n_out[2])
{
    using namespace gs;
    (void)c;                                                // the host form launches nothing: the context may be NULL
    int rc = hit_check_args(best_rec, n_genomes, n_prof, aa, rec_start, rec_len, n_rec, n_item, item, item_words, max_item, out_aa, out_start, out_len,
                            out_genome_off, n_out);
    if (rc) return rc;
    const uint64_t n = n_genomes * n_prof;
    uint64_t s, l, cnt[2] = {0, 0};
    uint32_t bad, err = 0;
    for (uint64_t h = 0; h < n; h++) {
        cnt[0] += hit_span(h, best_rec, rec_start, rec_len, n_rec, n_item, item, item_words, max_item, &s, &l, &bad);
        cnt[1] += l; err |= bad;
    }
    if ((rc = hit_report(err, max_item))) return rc;
    n_out[0] = cnt[0]; n_out[1] = cnt[1];
    if ((rc = hit_check_caps(n_out, cap_rec, cap_aa, out_aa, out_start, out_len))) return rc;
    uint64_t j = 0, o = 0;
    for (uint64_t h = 0; h < n; h++) {
        if (h % n_prof == 0) out_genome_off[h / n_prof] = j;
        if (!hit_span(h, best_rec, rec_start, rec_len, n_rec, n_item, item, item_words, max_item, &s, &l, &bad)) continue;
        out_start[j] = o; out_len[j] = l;
        std::copy(aa + s, aa + s + l, out_aa + o);
        j++; o += l;
    }
    for (uint64_t g = n ? n_genomes : 0; g <= n_genomes; g++) out_genome_off[g] = j;
    return GS_OK;
}

}  // extern "C"
