// gs_gene.hip — SPEC 15: a self-trained gene caller on the packed records of gs_orf.hip. Every genome learns in-frame dicodon statistics from its own long
// ORFs, every ORF's candidate starts are scored with them, and a maximal-weight chain of nearly non-overlapping genes is chosen per record on both strands.
// It is the self-trained kind of Prodigal / GeneMarkS, not FragGeneScanRs ("Known limitations (genes)"). All integer arithmetic.
//
// Passes of a call (gene_run), the ORF descriptors coming from the tile passes of gs_orf.hip (orf_count / orf_emit without residues):
//   k_gene_hexamers    background: per (genome, slice) a 16 KiB LDS table of the forward hexamers, flushed to both strands' counts with global integer adds
//   per round:
//   k_gene_iv_*        the training intervals: round 1 the long ORFs, later the genes of the round before (one slot per ORF, n = 0 = not used)
//   k_gene_dicodons    per 256 intervals an LDS table of in-frame dicodons, flushed per genome
//   k_gene_tables      one workgroup per genome: Nb, Nc, the 4096 scores, {Nc, trained}
//   k_gene_score       one wavefront per ORF: trips of 256 codons from the 3' end, four codons a lane, a prefix sum with a carried total, max / arg-max
//   k_gene_cand_*      candidates numbered in ORF order (a prefix sum over blocks of 4096 ORFs), keyed by (record, end, strand), sorted (gs_radix.hip), gathered
//   k_gene_rec_coff, k_gene_k   the candidates of every record and k(i) by binary search
//   k_gene_chain       one wavefront per record: the lanes stage 64 candidates, lane 0 carries the recurrence, then walks back
//   after the last round: two prefix sums, ONE read-back of the counts, k_gene_emit (descriptors, residues), k_gene_rec_goff
// The only atomics are integer adds and ors, which commute: nothing depends on scheduling.
#include <string.h>
#include <vector>
#include "gs_internal.hpp"
#include "gs_spec.hpp"
#include "gs_orf.hpp"

namespace gs {

enum { GENE_ERR_REC = 1, GENE_ERR_GOFF = 2, GENE_ERR_IV = 4, GENE_ERR_BIG = 8, GENE_ERR_TABLE = 16, GENE_ERR_ORF = 32 };
enum { GENE_META_ERR = 0, GENE_META_N_CAND = 1, GENE_META_N_GENE = 2, GENE_META_N_AA = 3, GENE_META_WORDS = 8 };
constexpr uint32_t GENE_SLICES = 64;          // workgroups that share a genome's hexamers
constexpr uint32_t GENE_CHUNK = 4096;         // hexamer positions a workgroup takes at a time
constexpr uint32_t GENE_IV_BLOCK = 256;       // intervals per workgroup of k_gene_dicodons
constexpr uint32_t GENE_TRIP = 256;           // codons per trip of k_gene_score: four a lane
constexpr uint32_t GENE_SCAN_BLOCK = 4096;    // values per workgroup of the many-workgroup prefix sum
constexpr uint32_t GENE_NONE = 0xFFFFFFFFu;
constexpr int GENE_CI_BITS = 29;              // low bits of a sort key: the candidate's number in ORF order
static_assert(GS_ORF_TILE < 256, "(tiles * 192 + end) * 2 + strand stays below 2^35 with fewer than 2^26 tiles");

__constant__ char gene_letters[2][65] = {GS_ORF_TABLE_11, GS_ORF_TABLE_4};

struct GeneIn { const uint8_t *seq; const uint64_t *rs, *rl, *goff; uint64_t n_rec, n_genomes, seq_bases; };
// a candidate gene in (record, end, strand) order
struct GeneCand { uint64_t begin, end; int64_t score; uint32_t rec, flags, orf, n_aa; };

GS_HD bool gene_rec_ok(uint64_t s, uint64_t l, uint64_t seq_bases) { return l <= seq_bases && s <= seq_bases - l; }
// the six bases at absolute base g (all inside a record, so every byte that is read holds one of them)
GS_HD uint32_t gene_hexamer_at(const uint8_t *__restrict__ seq, uint64_t g)
{
    const uint64_t by = g >> 2;
    const uint32_t o = (uint32_t)g & 3u;
    uint32_t v = ((uint32_t)seq[by] << 16) | ((uint32_t)seq[by + 1] << 8);
    if (o == 3) v |= seq[by + 2];
    return (v >> (12 - 2 * o)) & 0xFFFu;
}
GS_HD uint32_t gene_codon_at(const uint8_t *__restrict__ seq, uint64_t g)
{
    const uint32_t o = (uint32_t)g & 3u;
    uint32_t v = (uint32_t)seq[g >> 2] << 8;
    if (o >= 2) v |= seq[(g >> 2) + 1];
    return (v >> (10 - 2 * o)) & 63u;
}
// the last g with goff[g] <= rec (goff[0] = 0 is checked elsewhere; every index read lies in [0, n_genomes))
GS_HD uint64_t gene_genome_of(const uint64_t *__restrict__ goff, uint64_t n_genomes, uint64_t rec)
{
    uint64_t lo = 0, hi = n_genomes;
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (goff[mid] <= rec) lo = mid; else hi = mid; }
    return lo;
}
GS_HD bool gene_goff_ok(const uint64_t *__restrict__ goff, uint64_t n_genomes, uint64_t n_rec, uint64_t g)
{
    const uint64_t r0 = goff[g], r1 = goff[g + 1];
    return r0 <= r1 && r1 <= n_rec && (g != 0 || r0 == 0) && (g + 1 != n_genomes || r1 == n_rec);
}
// SPEC 15 "Start of an ORF", shared by the kernel and the host form: the codon u places from the 3' end (u = n - 1 - j)
GS_HD uint32_t gene_codon_u(const uint8_t *__restrict__ seq, uint64_t rec_base, uint64_t begin, uint64_t n, bool rev, uint64_t u)
{
    return rev ? orf_rev_codon(gene_codon_at(seq, rec_base + begin + 3 * u)) : gene_codon_at(seq, rec_base + begin + 3 * (n - 1 - u));
}
// is (s, u) better than (bs, bu): the larger score, among equals the smaller j = the larger u
GS_HD bool gene_better(bool have, int64_t s, uint64_t u, bool bhave, int64_t bs, uint64_t bu) { return have && (!bhave || s > bs || (s == bs && u > bu)); }
GS_HD uint32_t gene_flags(bool rev, bool open5, bool open3, bool have, uint32_t type, int64_t score, int64_t min_score)
{
    return (rev ? GS_GENE_STRAND : 0u) | (open3 ? GS_GENE_OPEN3 : 0u) | (open5 ? GS_GENE_OPEN5 : 0u) |
           (have ? GS_GENE_HAS_START | (type << GS_GENE_TYPE_SHIFT) | (score >= min_score ? GS_GENE_CANDIDATE : 0u) : 0u);
}
GS_HD bool gene_orf_ok(const gs_orf &d, uint64_t n, uint64_t n_rec, const uint64_t *rs, const uint64_t *rl, uint64_t seq_bases)
{
    if (d.rec >= n_rec || d.strand > 1 || n == 0) return false;
    const uint64_t L = rl[d.rec];
    return gene_rec_ok(rs[d.rec], L, seq_bases) && n <= L / 3 && d.begin <= L - 3 * n;
}

// ---- background -----------------------------------------------------------------------------------------------------------------------------------------------
// grid (genome, slice): the chunks of GENE_CHUNK hexamer positions of the genome's records are dealt round the slices
__global__ __launch_bounds__(256) void k_gene_hexamers(const GeneIn in, uint64_t *__restrict__ bg, uint32_t *__restrict__ err)
{
    __shared__ uint32_t tab[4096];
    const uint64_t g = blockIdx.x;
    const uint32_t s = blockIdx.y, tid = threadIdx.x;
    for (uint32_t i = tid; i < 4096; i += 256) tab[i] = 0;
    if (!gene_goff_ok(in.goff, in.n_genomes, in.n_rec, g)) {           // (the same in every thread)
        if (s == 0 && tid == 0) atomicOr(err, GENE_ERR_GOFF);
        return;
    }
    __syncthreads();
    const uint64_t r0 = in.goff[g], r1 = in.goff[g + 1];
    uint64_t chunk_base = 0;
    bool bad = false;
    for (uint64_t r = r0; r < r1; r++) {
        const uint64_t st = in.rs[r], L = in.rl[r];
        if (!gene_rec_ok(st, L, in.seq_bases)) { bad = true; continue; }
        const uint64_t npos = L >= 6 ? L - 5 : 0, nch = (npos + GENE_CHUNK - 1) / GENE_CHUNK;
        for (uint64_t ch = (s + GENE_SLICES - chunk_base % GENE_SLICES) % GENE_SLICES; ch < nch; ch += GENE_SLICES) {
            const uint64_t pe = (ch + 1) * GENE_CHUNK < npos ? (ch + 1) * GENE_CHUNK : npos;
            for (uint64_t p = ch * GENE_CHUNK + tid; p < pe; p += 256) atomicAdd(&tab[gene_hexamer_at(in.seq, st + p)], 1u);
        }
        chunk_base += nch;
    }
    if (bad && s == 0 && tid == 0) atomicOr(err, GENE_ERR_REC);
    __syncthreads();
    unsigned long long *out = (unsigned long long *)bg + g * 4096;
    for (uint32_t i = tid; i < 4096; i += 256) {
        const uint32_t v = tab[i];
        if (v) { atomicAdd(&out[i], (unsigned long long)v); atomicAdd(&out[gene_rev_hexamer(i)], (unsigned long long)v); }
    }
}

// ---- training -------------------------------------------------------------------------------------------------------------------------------------------------
// one slot per ORF, in ORF order (= record order): round 1 the ORFs of train_min_aa codons and more
__global__ __launch_bounds__(256) void k_gene_iv_orfs(const gs_orf *__restrict__ orf, const uint64_t *__restrict__ olen, uint64_t n_orf, uint32_t train_min_aa,
                                                      gs_gene_interval *__restrict__ iv)
{
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_orf) return;
    const gs_orf d = orf[o];
    const uint64_t n = olen[o];
    iv[o] = gs_gene_interval{d.begin, n >= train_min_aa ? n : 0, d.rec, d.strand};
}
// later rounds: the chosen genes from the start codon to the last sense codon (the slots were reset by k_gene_iv_orfs with train_min_aa = 2^32 - 1)
__global__ __launch_bounds__(256) void k_gene_iv_genes(const GeneCand *__restrict__ cand, const uint8_t *__restrict__ chosen, const uint64_t *__restrict__ meta,
                                                       const gs_orf *__restrict__ orf, gs_gene_interval *__restrict__ iv)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= meta[GENE_META_N_CAND] || !chosen[i]) return;
    const GeneCand c = cand[i];
    const bool rev = c.flags & GS_GENE_STRAND;
    iv[c.orf].begin = rev ? orf[c.orf].begin : c.begin;
    iv[c.orf].n = c.n_aa;
}

__global__ __launch_bounds__(256) void k_gene_dicodons(const GeneIn in, const gs_gene_interval *__restrict__ iv, uint64_t n_iv, uint64_t *__restrict__ cod,
                                                       uint32_t *__restrict__ err)
{
    __shared__ uint32_t tab[4096];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t b0 = (uint64_t)blockIdx.x * GENE_IV_BLOCK, b1 = b0 + GENE_IV_BLOCK < n_iv ? b0 + GENE_IV_BLOCK : n_iv;
    uint64_t i = b0;
    while (i < b1) {                                                   // runs of intervals of one genome; i is the same in every thread
        const uint64_t rec = iv[i].rec;
        const uint64_t g = gene_genome_of(in.goff, in.n_genomes, rec < in.n_rec ? rec : 0);
        const uint64_t rlo = in.goff[g], rhi = in.goff[g + 1];
        if (rec >= in.n_rec || rec < rlo || rec >= rhi) {
            if (tid == 0) atomicOr(err, GENE_ERR_IV);
            i++;
            continue;
        }
        uint64_t a = i, b = b1;                                        // iv[a].rec < rhi; the first interval of another genome (the list is in record order)
        while (b - a > 1) { const uint64_t m = a + (b - a) / 2; if (iv[m].rec < rhi) a = m; else b = m; }
        const uint64_t e = b;
        for (uint32_t t = tid; t < 4096; t += 256) tab[t] = 0;
        __syncthreads();
        for (uint64_t k = i + wave; k < e; k += 4) {
            const gs_gene_interval v = iv[k];
            bool ok = v.rec >= rlo && v.rec < rhi && v.rec < in.n_rec && v.strand <= 1 && (k == 0 || iv[k - 1].rec <= v.rec);
            uint64_t st = 0;
            if (ok) {
                const uint64_t L = in.rl[v.rec];
                st = in.rs[v.rec];
                ok = gene_rec_ok(st, L, in.seq_bases) && v.n <= L / 3 && v.begin <= L - 3 * v.n;
            }
            if (!ok || v.n >= GS_GENE_MAX_INTERVAL) {
                if (lane == 0) atomicOr(err, ok ? GENE_ERR_BIG : GENE_ERR_IV);
                continue;
            }
            // forward codons t and t + 1 of the interval; on the reverse strand the second is read first
            for (uint64_t t = lane; t + 1 < v.n; t += 64) {
                const uint32_t f0 = gene_codon_at(in.seq, st + v.begin + 3 * t), f1 = gene_codon_at(in.seq, st + v.begin + 3 * t + 3);
                atomicAdd(&tab[v.strand ? 64 * orf_rev_codon(f1) + orf_rev_codon(f0) : 64 * f0 + f1], 1u);
            }
        }
        __syncthreads();
        unsigned long long *out = (unsigned long long *)cod + g * 4096;
        for (uint32_t t = tid; t < 4096; t += 256) { const uint32_t v = tab[t]; if (v) atomicAdd(&out[t], (unsigned long long)v); }
        __syncthreads();
        i = e;
    }
}

// one workgroup per genome
__global__ __launch_bounds__(256) void k_gene_tables(const uint64_t *__restrict__ bg, const uint64_t *__restrict__ cod, uint32_t min_train_codons,
                                                     int32_t *__restrict__ tables, uint64_t *__restrict__ info, uint32_t *__restrict__ err)
{
    __shared__ uint64_t red[2][256];
    const uint64_t g = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint64_t *b = bg + g * 4096, *c = cod + g * 4096;
    uint64_t sb = 0, sc = 0;
    for (uint32_t h = tid; h < 4096; h += 256) { sb += b[h] + 1; sc += c[h]; }
    red[0][tid] = sb; red[1][tid] = sc;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    const uint64_t Nb = red[0][0], Nc = red[1][0];
    const bool big = Nb > GS_GENE_MAX_NB || Nc + GS_GENE_PRIOR > GS_GENE_MAX_NC_A;
    if (tid == 0) {
        if (big) atomicOr(err, GENE_ERR_BIG);
        info[2 * g] = Nc;
        info[2 * g + 1] = Nc >= min_train_codons ? GS_GENE_TRAINED : 0;
    }
    for (uint32_t h = tid; h < 4096; h += 256) tables[g * 4096 + h] = big ? 0 : gene_table_entry(c[h], b[h] + 1, Nc, Nb);
}

__global__ __launch_bounds__(256) void k_gene_check_tables(const int32_t *__restrict__ tables, uint64_t n, uint32_t *__restrict__ err)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (tables[i] > GS_GENE_S_LIMIT || tables[i] < -GS_GENE_S_LIMIT)) atomicOr(err, GENE_ERR_TABLE);
}

// ---- scoring --------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t gene_shfl_up(int64_t x, uint32_t o) { return (int64_t)__shfl_up((unsigned long long)x, o); }
__device__ __forceinline__ int64_t gene_shfl_xor(int64_t x, uint32_t o) { return (int64_t)__shfl_xor((unsigned long long)x, o); }

// One wavefront per ORF. With u = n - 1 - j the place of a codon counted from the 3' end, T(u) = sum of x(u') over 1 <= u' <= u, x(u) = S[64 c(u) + c(u - 1)]:
// a prefix sum in u. A trip takes 256 places, lane l the four from u0 + 4 l on; the total of the trips before is carried. info (optional): per genome
// {Nc, trained} - an ORF of an untrained genome is no candidate.
__global__ __launch_bounds__(256) void k_gene_score(const GeneIn in, const int32_t *__restrict__ tables, const uint64_t *__restrict__ info, const gs_orf *__restrict__ orf,
                                                    const uint64_t *__restrict__ olen, uint64_t n_orf, uint32_t min_aa, int64_t min_score, uint64_t *__restrict__ best_j,
                                                    int64_t *__restrict__ score, uint32_t *__restrict__ flags, uint32_t *__restrict__ err)
{
    const uint64_t o = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (o >= n_orf) return;
    const gs_orf d = orf[o];
    const uint64_t n = olen[o];
    bool ok = gene_orf_ok(d, n, in.n_rec, in.rs, in.rl, in.seq_bases);
    uint64_t g = 0;
    if (ok) {
        g = gene_genome_of(in.goff, in.n_genomes, d.rec);
        ok = d.rec >= in.goff[g] && d.rec < in.goff[g + 1];
    }
    if (!ok) {
        if (lane == 0) { atomicOr(err, GENE_ERR_ORF); best_j[o] = GS_GENE_NO_START; score[o] = 0; flags[o] = 0; }
        return;
    }
    const int32_t *__restrict__ S = tables + g * 4096;
    const uint64_t base = in.rs[d.rec], L = in.rl[d.rec];
    const bool rev = d.strand != 0, low_open = d.begin < 3, high_open = d.begin + 3 * n + 3 > L;
    const bool open5 = rev ? high_open : low_open, open3 = rev ? low_open : high_open;
    int64_t carry = 0, bs = 0;
    uint64_t bu = 0;
    uint32_t btype = 0;
    bool bhave = false;
    for (uint64_t u0 = 0; u0 < n; u0 += GENE_TRIP) {
        const uint64_t ub = u0 + 4 * lane;
        uint32_t c[5];
#pragma unroll
        for (uint32_t r = 0; r < 5; r++) {
            const uint64_t u = ub + r - 1;                               // (ub = 0, r = 0: the place before the first; not read)
            c[r] = (ub + r >= 1 && u < n) ? gene_codon_u(in.seq, base, d.begin, n, rev, u) : 0;
        }
        int64_t p[4], run = 0;
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint64_t u = ub + r;
            run += (u >= 1 && u < n) ? S[64 * c[r + 1] + c[r]] : 0;
            p[r] = run;
        }
        int64_t incl = run;
        for (uint32_t k = 1; k < 64; k <<= 1) { const int64_t y = gene_shfl_up(incl, k); if (lane >= k) incl += y; }
        const int64_t before = carry + incl - run;
        // this lane's best candidate start
        int64_t ls = 0; uint64_t lu = 0; uint32_t lt = 0; bool lh = false;
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint64_t u = ub + r;
            if (u >= n) continue;
            const int64_t T = before + p[r];
            const int type = gene_start_type(c[r + 1]);
            const bool edge = open5 && u == n - 1, start = type >= 0 && u + 1 >= min_aa;
            if (!edge && !start) continue;
            const int64_t s = edge ? T : T + gene_start_bonus(type);
            const uint32_t t = edge ? (type == 0 ? 0u : GS_GENE_TYPE_EDGE) : (uint32_t)type;
            if (gene_better(true, s, u, lh, ls, lu)) { ls = s; lu = u; lt = t; lh = true; }
        }
        for (uint32_t k = 32; k > 0; k >>= 1) {
            const int64_t ys = gene_shfl_xor(ls, k);
            const uint64_t yu = (uint64_t)gene_shfl_xor((int64_t)lu, k);
            const uint32_t yt = __shfl_xor(lt, k);
            const bool yh = __shfl_xor((int)lh, k) != 0;
            if (gene_better(yh, ys, yu, lh, ls, lu)) { ls = ys; lu = yu; lt = yt; lh = yh; }
        }
        if (gene_better(lh, ls, lu, bhave, bs, bu)) { bs = ls; bu = lu; btype = lt; bhave = true; }
        carry += (int64_t)__shfl((unsigned long long)incl, 63);
    }
    if (lane == 0) {
        const bool trained = !info || (info[2 * g + 1] & GS_GENE_TRAINED);
        best_j[o] = bhave ? n - 1 - bu : GS_GENE_NO_START;
        score[o] = bhave ? bs : 0;
        flags[o] = gene_flags(rev, open5, open3, bhave, btype, bs, trained ? min_score : INT64_MAX);
    }
}

// ---- candidates -----------------------------------------------------------------------------------------------------------------------------------------------
// exclusive prefix sums of n values by ONE workgroup (lanes take contiguous stretches, as k_orf_rec_tiles): out[0..n], out[n] = the total, also to *total
__global__ __launch_bounds__(1024) void k_gene_scan(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ total)
{
    __shared__ uint64_t part[1024];
    const uint64_t per = (n + 1023) / 1024, b0 = (uint64_t)threadIdx.x * per, b = b0 < n ? b0 : n, e = b + per < n ? b + per : n;
    uint64_t sum = 0;
    for (uint64_t i = b; i < e; i++) sum += in[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t i = b; i < e; i++) { const uint64_t v = in[i]; out[i] = run; run += v; }
    if (threadIdx.x == 1023) { out[n] = part[1023]; if (total) *total = part[1023]; }
}
// The same over many workgroups, for columns of millions of values (one per ORF): the sums of blocks of GENE_SCAN_BLOCK values, k_gene_scan over those
// sums, then every block scans its values 256 at a time (coalesced) from its offset. out[n] = the total is written by the last block.
__global__ __launch_bounds__(256) void k_gene_block_sums(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t red[256];
    const uint64_t b0 = (uint64_t)blockIdx.x * GENE_SCAN_BLOCK;
    uint64_t x = 0;
    for (uint32_t i = threadIdx.x; i < GENE_SCAN_BLOCK; i += 256) x += b0 + i < n ? in[b0 + i] : 0;
    red[threadIdx.x] = x;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void k_gene_block_scan(const uint64_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ offs, uint64_t *__restrict__ out)
{
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t b0 = (uint64_t)blockIdx.x * GENE_SCAN_BLOCK;
    uint64_t carry = offs[blockIdx.x];
    for (uint32_t step = 0; step < GENE_SCAN_BLOCK / 256; step++) {
        const uint64_t i = b0 + 256 * step + tid, v = i < n ? in[i] : 0;
        uint64_t incl = v;
        for (uint32_t k = 1; k < 64; k <<= 1) { const uint64_t y = __shfl_up((unsigned long long)incl, k); if (lane >= k) incl += y; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t woff = 0, tot = 0;
        for (uint32_t w = 0; w < 4; w++) { if (w < wave) woff += wsum[w]; tot += wsum[w]; }
        if (i < n) out[i] = carry + woff + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0 && b0 + GENE_SCAN_BLOCK >= n) out[n] = carry;
}
__global__ __launch_bounds__(256) void k_gene_cand_flag(const uint32_t *__restrict__ flags, uint64_t n_orf, uint64_t *__restrict__ v)
{
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < n_orf) v[o] = (flags[o] & GS_GENE_CANDIDATE) ? 1 : 0;
}
// the gene of ORF (d, n) that starts at codon j: forward coordinates, the stop codon included where there is one
GS_HD void gene_coords(const gs_orf &d, uint64_t n, uint64_t j, uint32_t fl, uint64_t *begin, uint64_t *end)
{
    const uint64_t stop = (fl & GS_GENE_OPEN3) ? 0 : 3;
    if (fl & GS_GENE_STRAND) { *begin = d.begin - stop; *end = d.begin + 3 * n - 3 * j; }
    else { *begin = d.begin + 3 * j; *end = d.begin + 3 * n + stop; }
}
__global__ __launch_bounds__(256) void k_gene_cand_keys(const gs_orf *__restrict__ orf, const uint64_t *__restrict__ olen, const uint64_t *__restrict__ best_j,
                                                        const uint32_t *__restrict__ flags, const uint64_t *__restrict__ cidx, const uint64_t *__restrict__ rtoff,
                                                        uint64_t n_orf, uint64_t *__restrict__ keys, uint32_t *__restrict__ cand_orf)
{
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_orf || !(flags[o] & GS_GENE_CANDIDATE)) return;
    const gs_orf d = orf[o];
    uint64_t b, e;
    gene_coords(d, olen[o], best_j[o], flags[o], &b, &e);
    const uint64_t ci = cidx[o];
    keys[ci] = (((rtoff[d.rec] * GS_ORF_TILE + e) * 2 + d.strand) << GENE_CI_BITS) | ci;
    cand_orf[ci] = (uint32_t)o;
}
__global__ __launch_bounds__(256) void k_gene_cand_gather(const uint64_t *__restrict__ sorted, const uint32_t *__restrict__ cand_orf, const gs_orf *__restrict__ orf,
                                                          const uint64_t *__restrict__ olen, const uint64_t *__restrict__ best_j, const int64_t *__restrict__ score,
                                                          const uint32_t *__restrict__ flags, uint64_t n_cand, GeneCand *__restrict__ cand)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cand) return;
    const uint32_t o = cand_orf[sorted[i] & (((uint64_t)1 << GENE_CI_BITS) - 1)];
    const gs_orf d = orf[o];
    GeneCand c;
    gene_coords(d, olen[o], best_j[o], flags[o], &c.begin, &c.end);
    c.score = score[o]; c.rec = d.rec; c.flags = flags[o] & (GS_GENE_STRAND | (3u << GS_GENE_TYPE_SHIFT) | GS_GENE_OPEN3); c.orf = o;
    c.n_aa = (uint32_t)(olen[o] - best_j[o]);
    cand[i] = c;
}
// coff[r] = the sorted candidates in front of record r, coff[n_rec] = all. With t = the tiles in front of r, the key parts of r lie in [384 t + 2, 384 t' + 1],
// t' = the tiles in front of r + 1 (1 <= end <= L <= 192 tiles(r)): a gene that ends at the high edge of a record of 192 k bases has the key part 384 t' or
// 384 t' + 1, so the bisection is for the first key part ABOVE 384 t + 1, not the first at or above 384 t
__global__ __launch_bounds__(256) void k_gene_rec_coff(const uint64_t *__restrict__ sorted, uint64_t n_cand, const uint64_t *__restrict__ rtoff, uint64_t n_rec,
                                                       uint64_t *__restrict__ coff)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_rec) return;
    const uint64_t want = (rtoff[r] * GS_ORF_TILE * 2 + 2) << GENE_CI_BITS;
    uint64_t lo = 0, hi = n_cand;                                      // the first i with sorted[i] >= want
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (sorted[mid] < want) lo = mid + 1; else hi = mid; }
    coff[r] = r == n_rec ? n_cand : lo;
}
// k(i): the candidates m < i of the record with end_m <= begin_i + max_overlap (the ends ascend, so they are a prefix)
__global__ __launch_bounds__(256) void k_gene_k(const GeneCand *__restrict__ cand, uint64_t n_cand, const uint64_t *__restrict__ coff, uint32_t max_overlap,
                                                uint32_t *__restrict__ kk)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t first = coff[cand[i].rec], lim = cand[i].begin + max_overlap;
    uint64_t lo = first, hi = i;                                       // the first m with end_m > lim
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (cand[mid].end <= lim) lo = mid + 1; else hi = mid; }
    kk[i] = (uint32_t)(lo - first);
}
// One wavefront per record. f_i = score_i + P_k(i), P_k = max(0, max f_m over m < k): pm[i] / pa[i] hold the running maximum over m <= i and the smallest m
// that reaches it (GENE_NONE while it is 0). The recurrence is serial: the lanes stage 64 candidates' (score, k) in LDS, lane 0 carries it.
__global__ __launch_bounds__(64) void k_gene_chain(const GeneCand *__restrict__ cand, const uint32_t *__restrict__ kk, const uint64_t *__restrict__ coff,
                                                   int64_t *pm, uint32_t *pa, uint32_t *pred, uint8_t *chosen)
{
    __shared__ int64_t s_score[64];
    __shared__ uint32_t s_k[64];
    const uint64_t r = blockIdx.x, first = coff[r], cnt = coff[r + 1] - first;
    const uint32_t lane = threadIdx.x;
    int64_t run = 0, bestf = 0;
    uint32_t runarg = GENE_NONE, besti = GENE_NONE;
    for (uint64_t i0 = 0; i0 < cnt; i0 += 64) {
        if (i0 + lane < cnt) { s_score[lane] = cand[first + i0 + lane].score; s_k[lane] = kk[first + i0 + lane]; }
        __syncthreads();
        if (lane == 0) {
            const uint32_t m = cnt - i0 < 64 ? (uint32_t)(cnt - i0) : 64u;
            for (uint32_t t = 0; t < m; t++) {
                const uint64_t i = i0 + t;
                const uint32_t k = s_k[t];
                const int64_t P = k ? pm[first + k - 1] : 0;
                const uint32_t arg = k ? pa[first + k - 1] : GENE_NONE;
                const int64_t f = s_score[t] + P;
                pred[first + i] = P > 0 ? arg : GENE_NONE;
                if (f > run) { run = f; runarg = (uint32_t)i; }
                pm[first + i] = run; pa[first + i] = runarg;
                if (besti == GENE_NONE || f > bestf) { bestf = f; besti = (uint32_t)i; }
            }
        }
        __syncthreads();
    }
    if (lane == 0)
        for (uint32_t i = besti; i != GENE_NONE; i = pred[first + i]) chosen[first + i] = 1;
}
__global__ __launch_bounds__(256) void k_gene_chosen_cols(const GeneCand *__restrict__ cand, const uint8_t *__restrict__ chosen, uint64_t n_cand, uint64_t *__restrict__ v_gene,
                                                          uint64_t *__restrict__ v_aa)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cand) return;
    v_gene[i] = chosen[i] ? 1 : 0;
    v_aa[i] = chosen[i] ? cand[i].n_aa : 0;
}
// one wavefront per candidate: a chosen one writes its descriptor and its residues, the lanes stride over the codons
__global__ __launch_bounds__(256) void k_gene_emit(const GeneIn in, const GeneCand *__restrict__ cand, const uint8_t *__restrict__ chosen, const uint64_t *__restrict__ goff_scan,
                                                   const uint64_t *__restrict__ aoff_scan, uint64_t n_cand, uint32_t table_ix, gs_gene *__restrict__ gene, uint8_t *__restrict__ aa,
                                                   uint64_t *__restrict__ aa_start, uint64_t *__restrict__ aa_len)
{
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n_cand || !chosen[i]) return;
    const GeneCand c = cand[i];
    const uint64_t gi = goff_scan[i], ao = aoff_scan[i], base = in.rs[c.rec];
    if (lane == 0) {
        gene[gi] = gs_gene{c.begin, c.end, c.score, c.rec, c.flags};
        aa_start[gi] = ao; aa_len[gi] = c.n_aa;
    }
    const bool rev = c.flags & GS_GENE_STRAND, edge = ((c.flags >> GS_GENE_TYPE_SHIFT) & 3u) == GS_GENE_TYPE_EDGE;
    const char *letters = gene_letters[table_ix];
    for (uint64_t t = lane; t < c.n_aa; t += 64) {
        const uint32_t f = gene_codon_at(in.seq, base + (rev ? c.end - 3 - 3 * t : c.begin + 3 * t));
        aa[ao + t] = (t == 0 && !edge) ? (uint8_t)'M' : (uint8_t)letters[rev ? orf_rev_codon(f) : f];
    }
}
__global__ __launch_bounds__(256) void k_gene_rec_goff(const uint64_t *__restrict__ coff, const uint64_t *__restrict__ goff_scan, uint64_t n_rec, uint64_t *__restrict__ rec_gene_off)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= n_rec) rec_gene_off[r] = goff_scan[coff[r]];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------
static int gene_check_params(const gs_gene_params *prm, uint64_t n_rec, uint64_t n_genomes)
{
    GS_REQUIRE(prm, GS_ERR_INVALID, "gene: null parameters");
    GS_REQUIRE(prm->min_aa != 0, GS_ERR_INVALID, "gene: min_aa = 0");
    GS_REQUIRE((uint64_t)prm->max_overlap < 3ull * prm->min_aa, GS_ERR_INVALID, "gene: max_overlap %u is not below 3 * min_aa = %llu (SPEC 15: adjacent compatibility would not imply pairwise)",
               prm->max_overlap, 3ull * prm->min_aa);
    GS_REQUIRE(prm->rounds >= 1, GS_ERR_INVALID, "gene: rounds = 0");
    GS_REQUIRE(prm->flags == 0, GS_ERR_UNSUPPORTED, "gene: flags %u", prm->flags);
    GS_REQUIRE(prm->table == 11 || prm->table == 4, GS_ERR_UNSUPPORTED, "gene: translation table %u (11 and 4 are there)", prm->table);
    GS_REQUIRE(n_rec < (1ull << 32) && n_genomes < (1ull << 32), GS_ERR_UNSUPPORTED, "gene: 2^32 records or genomes or more in one call");
    GS_REQUIRE(n_genomes >= 1 || n_rec == 0, GS_ERR_INVALID, "gene: records without a genome");
    return GS_OK;
}
static int gene_report(uint32_t err)
{
    GS_REQUIRE(!(err & GENE_ERR_GOFF), GS_ERR_INVALID, "gene: genome_rec_off does not ascend from 0 to n_rec");
    GS_REQUIRE(!(err & GENE_ERR_REC), GS_ERR_INVALID, "gene: a record does not lie inside seq");
    GS_REQUIRE(!(err & GENE_ERR_IV), GS_ERR_INVALID, "gene: a training interval lies outside its record, is out of record order or has a strand above 1");
    GS_REQUIRE(!(err & GENE_ERR_ORF), GS_ERR_INVALID, "gene: an ORF lies outside its record, has no codon or a strand above 1");
    GS_REQUIRE(!(err & GENE_ERR_TABLE), GS_ERR_INVALID, "gene: a table entry outside +-%d", GS_GENE_S_LIMIT);
    GS_REQUIRE(!(err & GENE_ERR_BIG), GS_ERR_UNSUPPORTED,
               "gene: a genome of more than 2^30 hexamer positions or 2^32 - 4096 training dicodons, or an interval of 2^24 codons or more (a product would leave 64 bits)");
    return GS_OK;
}
static inline dim3 gene_grid(uint64_t n, uint32_t per) { return dim3((uint32_t)((n + per - 1) / per ? (n + per - 1) / per : 1)); }

struct GeneTrainWork {
    PoolBuf bg, cod, meta;
    explicit GeneTrainWork(gs_ctx *c) : bg(c, SL_GENE_BG), cod(c, SL_GENE_COD), meta(c, SL_GENE_META) {}
    uint32_t *err() const { return meta.as<uint32_t>(); }
    int alloc(gs_ctx *c, uint64_t n_genomes)
    {
        int rc;
        if ((rc = bg.alloc(8 * 4096 * n_genomes)) || (rc = cod.alloc(8 * 4096 * n_genomes)) || (rc = meta.alloc(8 * GENE_META_WORDS))) return rc;
        GS_HIP_CHECK(hipMemsetAsync(meta.p, 0, 8 * GENE_META_WORDS, c->stream));
        return GS_OK;
    }
};
static int gene_background(gs_ctx *c, const GeneIn &in, GeneTrainWork &w)
{
    if (in.n_genomes == 0) return GS_OK;
    GS_REQUIRE(in.n_genomes < (1ull << 31), GS_ERR_UNSUPPORTED, "gene: genomes");
    GS_HIP_CHECK(hipMemsetAsync(w.bg.p, 0, 8 * 4096 * in.n_genomes, c->stream));
    hipLaunchKernelGGL(k_gene_hexamers, dim3((uint32_t)in.n_genomes, GENE_SLICES), dim3(256), 0, c->stream, in, w.bg.as<uint64_t>(), w.err());
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}
// intervals -> counts -> tables and info, queued
static int gene_train_queue(gs_ctx *c, const GeneIn &in, GeneTrainWork &w, const gs_gene_params *prm, const gs_gene_interval *iv, uint64_t n_iv, int32_t *tables, uint64_t *info)
{
    if (in.n_genomes == 0) return GS_OK;
    GS_REQUIRE(n_iv < (1ull << 39), GS_ERR_UNSUPPORTED, "gene: intervals");
    GS_HIP_CHECK(hipMemsetAsync(w.cod.p, 0, 8 * 4096 * in.n_genomes, c->stream));
    if (n_iv) hipLaunchKernelGGL(k_gene_dicodons, gene_grid(n_iv, GENE_IV_BLOCK), dim3(256), 0, c->stream, in, iv, n_iv, w.cod.as<uint64_t>(), w.err());
    hipLaunchKernelGGL(k_gene_tables, dim3((uint32_t)in.n_genomes), dim3(256), 0, c->stream, w.bg.as<uint64_t>(), w.cod.as<uint64_t>(), prm->min_train_codons, tables, info, w.err());
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}
static int gene_read_meta(gs_ctx *c, const PoolBuf &meta, uint64_t h[GENE_META_WORDS])
{
    GS_HIP_CHECK(hipMemcpyAsync(h, meta.p, 8 * GENE_META_WORDS, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    return gene_report((uint32_t)h[GENE_META_ERR]);
}
static int gene_score_queue(gs_ctx *c, const GeneIn &in, const gs_gene_params *prm, const int32_t *tables, const uint64_t *info, const gs_orf *orf, const uint64_t *olen,
                            uint64_t n_orf, uint64_t *best_j, int64_t *score, uint32_t *flags, uint32_t *err)
{
    GS_REQUIRE(n_orf < (1ull << 33), GS_ERR_UNSUPPORTED, "gene: ORFs");
    if (n_orf)
        hipLaunchKernelGGL(k_gene_score, gene_grid(n_orf, 4), dim3(256), 0, c->stream, in, tables, info, orf, olen, n_orf, prm->min_aa, (int64_t)prm->min_score, best_j, score, flags,
                           err);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

// exclusive prefix sums of in[0..n) into out[0..n], the total to *total: one workgroup for a short column, else block sums, their scan, block scans
static int gene_scan_queue(gs_ctx *c, const uint64_t *in, uint64_t n, uint64_t *out, uint64_t *total, PoolBuf &sums, PoolBuf &offs)
{
    if (n <= GENE_SCAN_BLOCK) {
        hipLaunchKernelGGL(k_gene_scan, dim3(1), dim3(1024), 0, c->stream, in, n, out, total);
    } else {
        const uint64_t nb = (n + GENE_SCAN_BLOCK - 1) / GENE_SCAN_BLOCK;
        int rc;
        if ((rc = sums.alloc(8 * nb)) || (rc = offs.alloc(8 * (nb + 1)))) return rc;
        hipLaunchKernelGGL(k_gene_block_sums, dim3((uint32_t)nb), dim3(256), 0, c->stream, in, n, sums.as<uint64_t>());
        hipLaunchKernelGGL(k_gene_scan, dim3(1), dim3(1024), 0, c->stream, sums.as<uint64_t>(), nb, offs.as<uint64_t>(), total);
        hipLaunchKernelGGL(k_gene_block_scan, dim3((uint32_t)nb), dim3(256), 0, c->stream, in, n, offs.as<uint64_t>(), out);
    }
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}

struct GeneCallWork {
    PoolBuf orf, olen, ostart, ooff, tables, iv, best_j, score, flags, col0, col1, scan0, scan1, keys, alt, radix, cand_orf, cand, coff, kk, pm, pa, pred, chosen, sums, offs;
    explicit GeneCallWork(gs_ctx *c)
        : orf(c, SL_GENE_ORF), olen(c, SL_GENE_ORF_LEN), ostart(c, SL_GENE_ORF_START), ooff(c, SL_GENE_ORF_OFF), tables(c, SL_GENE_TABLES), iv(c, SL_GENE_IV),
          best_j(c, SL_GENE_BEST_J), score(c, SL_GENE_SCORE), flags(c, SL_GENE_FLAGS), col0(c, SL_GENE_COL0), col1(c, SL_GENE_COL1), scan0(c, SL_GENE_SCAN0),
          scan1(c, SL_GENE_SCAN1), keys(c, SL_GENE_KEYS), alt(c, SL_GENE_KEYS_ALT), radix(c, SL_GENE_RADIX), cand_orf(c, SL_GENE_CAND_ORF), cand(c, SL_GENE_CAND),
          coff(c, SL_GENE_REC_CAND), kk(c, SL_GENE_K), pm(c, SL_GENE_PMAX), pa(c, SL_GENE_PARG), pred(c, SL_GENE_PRED), chosen(c, SL_GENE_CHOSEN),
          sums(c, SL_GENE_SCAN_SUMS), offs(c, SL_GENE_SCAN_OFFS) {}
};

static int gene_check_outputs(uint64_t cap_gene, uint64_t cap_aa, const void *o0, const void *o1, const void *o2, const void *o3, const void *o4, bool *count_only)
{
    const int given = (o0 != nullptr) + (o1 != nullptr) + (o2 != nullptr) + (o3 != nullptr) + (o4 != nullptr);
    GS_REQUIRE(given == 0 || given == 5, GS_ERR_INVALID, "gene: all five gene outputs or none (%d given)", given);
    GS_REQUIRE(given == 5 || (cap_gene == 0 && cap_aa == 0), GS_ERR_INVALID, "gene: capacities without outputs");
    *count_only = given == 0;
    return GS_OK;
}

// The whole pipeline on device memory. The emission is a second step (gene_emit) so that the host form can size its staging by the counts.
struct GeneRun {
    OrfWork ow; GeneTrainWork tw; GeneCallWork w;
    GeneIn in{}; uint64_t n_orf = 0, n_cand = 0; uint32_t table_ix = 0;
    explicit GeneRun(gs_ctx *c) : ow(c), tw(c), w(c) {}
};
static int gene_run(gs_ctx *c, const gs_gene_params *prm, GeneRun &R, uint64_t seq_bytes, uint64_t *info, int32_t *tables_out, uint64_t n_out[2])
{
    const GeneIn &in = R.in;
    GeneCallWork &w = R.w;
    int rc;
    n_out[0] = n_out[1] = 0;
    gs_orf_params op{prm->min_aa, 0, prm->table, 0};
    uint64_t on[3];
    if ((rc = orf_count(c, &op, in.seq, seq_bytes, in.rs, in.rl, in.n_rec, R.ow, on))) return rc;
    const uint64_t n_orf = R.n_orf = on[0];
    GS_REQUIRE(n_orf < (1ull << 32), GS_ERR_UNSUPPORTED, "gene: 2^32 ORFs or more in one call");
    R.table_ix = prm->table == 11 ? 0 : 1;
    if ((rc = w.orf.alloc(sizeof(gs_orf) * n_orf)) || (rc = w.olen.alloc(8 * n_orf)) || (rc = w.ostart.alloc(8 * n_orf)) || (rc = w.ooff.alloc(8 * (in.n_rec + 1))) ||
        (rc = w.tables.alloc(4 * 4096 * in.n_genomes)) || (rc = w.iv.alloc(sizeof(gs_gene_interval) * n_orf)) || (rc = w.best_j.alloc(8 * n_orf)) ||
        (rc = w.score.alloc(8 * n_orf)) || (rc = w.flags.alloc(4 * n_orf)) || (rc = w.col0.alloc(8 * n_orf)) || (rc = w.scan0.alloc(8 * (n_orf + 1))) ||
        (rc = w.coff.alloc(8 * (in.n_rec + 1))) || (rc = R.tw.alloc(c, in.n_genomes)))
        return rc;
    if ((rc = orf_emit(c, in.n_rec, R.ow, w.orf.as<gs_orf>(), nullptr, w.ostart.as<uint64_t>(), w.olen.as<uint64_t>(), w.ooff.as<uint64_t>()))) return rc;
    if ((rc = gene_background(c, in, R.tw))) return rc;
    int32_t *tables = tables_out ? tables_out : w.tables.as<int32_t>();
    uint64_t *meta = R.tw.meta.as<uint64_t>();
    const gs_orf *orf = w.orf.as<gs_orf>();
    const uint64_t *olen = w.olen.as<uint64_t>();
    for (uint32_t round = 1; round <= prm->rounds; round++) {
        gs_gene_interval *iv = w.iv.as<gs_gene_interval>();
        if (n_orf) {
            hipLaunchKernelGGL(k_gene_iv_orfs, gene_grid(n_orf, 256), dim3(256), 0, c->stream, orf, olen, n_orf, round == 1 ? prm->train_min_aa : 0xFFFFFFFFu, iv);
            if (round > 1 && R.n_cand)
                hipLaunchKernelGGL(k_gene_iv_genes, gene_grid(R.n_cand, 256), dim3(256), 0, c->stream, w.cand.as<GeneCand>(), w.chosen.as<uint8_t>(), meta, orf, iv);
        }
        if ((rc = gene_train_queue(c, in, R.tw, prm, iv, n_orf, tables, info))) return rc;
        if ((rc = gene_score_queue(c, in, prm, tables, info, orf, olen, n_orf, w.best_j.as<uint64_t>(), w.score.as<int64_t>(), w.flags.as<uint32_t>(), R.tw.err()))) return rc;
        if (n_orf) hipLaunchKernelGGL(k_gene_cand_flag, gene_grid(n_orf, 256), dim3(256), 0, c->stream, w.flags.as<uint32_t>(), n_orf, w.col0.as<uint64_t>());
        if ((rc = gene_scan_queue(c, w.col0.as<uint64_t>(), n_orf, w.scan0.as<uint64_t>(), meta + GENE_META_N_CAND, w.sums, w.offs))) return rc;
        uint64_t h[GENE_META_WORDS];
        if ((rc = gene_read_meta(c, R.tw.meta, h))) return rc;
        const uint64_t n_cand = R.n_cand = h[GENE_META_N_CAND];
        GS_REQUIRE(n_cand < (1ull << GENE_CI_BITS), GS_ERR_UNSUPPORTED, "gene: 2^29 candidate genes or more in one call");
        if ((rc = w.keys.alloc(8 * n_cand)) || (rc = w.alt.alloc(8 * n_cand)) || (rc = w.radix.alloc(radix_scratch_bytes(n_cand))) || (rc = w.cand_orf.alloc(4 * n_cand)) ||
            (rc = w.cand.alloc(sizeof(GeneCand) * n_cand)) || (rc = w.kk.alloc(4 * n_cand)) || (rc = w.pm.alloc(8 * n_cand)) || (rc = w.pa.alloc(4 * n_cand)) ||
            (rc = w.pred.alloc(4 * n_cand)) || (rc = w.chosen.alloc(n_cand)))
            return rc;
        uint64_t *sorted = w.keys.as<uint64_t>();
        if (n_cand) {
            hipLaunchKernelGGL(k_gene_cand_keys, gene_grid(n_orf, 256), dim3(256), 0, c->stream, orf, olen, w.best_j.as<uint64_t>(), w.flags.as<uint32_t>(), w.scan0.as<uint64_t>(),
                               R.ow.a.rtoff, n_orf, w.keys.as<uint64_t>(), w.cand_orf.as<uint32_t>());
            GS_HIP_CHECK(hipGetLastError());
            if ((rc = radix_sort_u64(c, w.keys.as<uint64_t>(), w.alt.as<uint64_t>(), n_cand, 64, w.radix.p, &sorted))) return rc;
            hipLaunchKernelGGL(k_gene_cand_gather, gene_grid(n_cand, 256), dim3(256), 0, c->stream, sorted, w.cand_orf.as<uint32_t>(), orf, olen, w.best_j.as<uint64_t>(),
                               w.score.as<int64_t>(), w.flags.as<uint32_t>(), n_cand, w.cand.as<GeneCand>());
        }
        hipLaunchKernelGGL(k_gene_rec_coff, gene_grid(in.n_rec + 1, 256), dim3(256), 0, c->stream, sorted, n_cand, R.ow.a.rtoff, in.n_rec, w.coff.as<uint64_t>());
        if (n_cand) {
            GS_HIP_CHECK(hipMemsetAsync(w.chosen.p, 0, n_cand, c->stream));
            hipLaunchKernelGGL(k_gene_k, gene_grid(n_cand, 256), dim3(256), 0, c->stream, w.cand.as<GeneCand>(), n_cand, w.coff.as<uint64_t>(), prm->max_overlap, w.kk.as<uint32_t>());
            hipLaunchKernelGGL(k_gene_chain, dim3((uint32_t)in.n_rec), dim3(64), 0, c->stream, w.cand.as<GeneCand>(), w.kk.as<uint32_t>(), w.coff.as<uint64_t>(), w.pm.as<int64_t>(),
                               w.pa.as<uint32_t>(), w.pred.as<uint32_t>(), w.chosen.as<uint8_t>());
        }
        GS_HIP_CHECK(hipGetLastError());
    }
    // the counts of the last round's choice
    const uint64_t n_cand = R.n_cand;
    if ((rc = w.col0.alloc(8 * n_cand)) || (rc = w.col1.alloc(8 * n_cand)) || (rc = w.scan0.alloc(8 * (n_cand + 1))) || (rc = w.scan1.alloc(8 * (n_cand + 1)))) return rc;
    if (n_cand)
        hipLaunchKernelGGL(k_gene_chosen_cols, gene_grid(n_cand, 256), dim3(256), 0, c->stream, w.cand.as<GeneCand>(), w.chosen.as<uint8_t>(), n_cand, w.col0.as<uint64_t>(),
                           w.col1.as<uint64_t>());
    GS_HIP_CHECK(hipGetLastError());
    if ((rc = gene_scan_queue(c, w.col0.as<uint64_t>(), n_cand, w.scan0.as<uint64_t>(), meta + GENE_META_N_GENE, w.sums, w.offs)) ||
        (rc = gene_scan_queue(c, w.col1.as<uint64_t>(), n_cand, w.scan1.as<uint64_t>(), meta + GENE_META_N_AA, w.sums, w.offs)))
        return rc;
    uint64_t h[GENE_META_WORDS];
    if ((rc = gene_read_meta(c, R.tw.meta, h))) return rc;
    n_out[0] = h[GENE_META_N_GENE]; n_out[1] = h[GENE_META_N_AA];
    return GS_OK;
}
// queued behind gene_run; nothing is waited for
static int gene_emit(gs_ctx *c, GeneRun &R, gs_gene *gene, uint8_t *aa, uint64_t *aa_start, uint64_t *aa_len, uint64_t *rec_gene_off)
{
    GeneCallWork &w = R.w;
    if (R.n_cand)
        hipLaunchKernelGGL(k_gene_emit, gene_grid(R.n_cand, 4), dim3(256), 0, c->stream, R.in, w.cand.as<GeneCand>(), w.chosen.as<uint8_t>(), w.scan0.as<uint64_t>(),
                           w.scan1.as<uint64_t>(), R.n_cand, R.table_ix, gene, aa, aa_start, aa_len);
    hipLaunchKernelGGL(k_gene_rec_goff, gene_grid(R.in.n_rec + 1, 256), dim3(256), 0, c->stream, w.coff.as<uint64_t>(), w.scan0.as<uint64_t>(), R.in.n_rec, rec_gene_off);
    GS_HIP_CHECK(hipGetLastError());
    return GS_OK;
}
static int gene_check_caps(const uint64_t n_out[2], uint64_t cap_gene, uint64_t cap_aa)
{
    GS_REQUIRE(n_out[0] <= cap_gene && n_out[1] <= cap_aa, GS_ERR_INVALID, "gene: %llu genes of %llu residues do not fit capacities of %llu and %llu",
               (unsigned long long)n_out[0], (unsigned long long)n_out[1], (unsigned long long)cap_gene, (unsigned long long)cap_aa);
    return GS_OK;
}

}  // namespace gs

gs_gene_params gs_gene_params_default(void)
{
    gs_gene_params p;
    p.min_aa = GS_ORF_MIN_AA; p.table = 11; p.train_min_aa = GS_GENE_TRAIN_MIN_AA; p.min_train_codons = GS_GENE_MIN_TRAIN_CODONS; p.min_score = GS_GENE_MIN_SCORE;
    p.max_overlap = GS_GENE_MAX_OVERLAP; p.rounds = GS_GENE_ROUNDS; p.flags = 0;
    return p;
}
uint32_t gs_gene_log2_q16(uint64_t x) { return gs::gene_log2_q16(x); }

int gs_gene_train_dev(gs_ctx *c, const gs_gene_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                      const uint64_t *genome_rec_off_dev, uint64_t n_genomes, const gs_gene_interval *iv_dev, uint64_t n_iv, int32_t *tables_out_dev, uint64_t *info_out_dev)
{
    using namespace gs;
    GS_REQUIRE(c, GS_ERR_INVALID, "null argument");
    int rc;
    if ((rc = gene_check_params(prm, n_rec, n_genomes))) return rc;
    GS_REQUIRE(genome_rec_off_dev && (n_rec == 0 || (rec_start_dev && rec_len_dev)) && (n_iv == 0 || iv_dev), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n_genomes == 0 || (tables_out_dev && info_out_dev), GS_ERR_INVALID, "null output");
    GS_REQUIRE(seq_dev || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_REQUIRE(seq_bytes < (1ull << 61), GS_ERR_UNSUPPORTED, "gene: seq_bytes");
    GS_CTX_LOCK(c);
    GeneTrainWork w(c);
    if ((rc = w.alloc(c, n_genomes))) return rc;
    const GeneIn in{(const uint8_t *)seq_dev, rec_start_dev, rec_len_dev, genome_rec_off_dev, n_rec, n_genomes, 4 * seq_bytes};
    if ((rc = gene_background(c, in, w)) || (rc = gene_train_queue(c, in, w, prm, iv_dev, n_iv, tables_out_dev, info_out_dev))) return rc;
    uint64_t h[GENE_META_WORDS];
    return gene_read_meta(c, w.meta, h);
}

int gs_gene_score_dev(gs_ctx *c, const gs_gene_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                      const uint64_t *genome_rec_off_dev, uint64_t n_genomes, const int32_t *tables_dev, const gs_orf *orf_dev, const uint64_t *orf_len_dev, uint64_t n_orf,
                      uint64_t *best_j_out_dev, int64_t *score_out_dev, uint32_t *flags_out_dev)
{
    using namespace gs;
    GS_REQUIRE(c, GS_ERR_INVALID, "null argument");
    int rc;
    if ((rc = gene_check_params(prm, n_rec, n_genomes))) return rc;
    GS_REQUIRE(genome_rec_off_dev && (n_rec == 0 || (rec_start_dev && rec_len_dev)) && (n_genomes == 0 || tables_dev), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n_orf == 0 || (orf_dev && orf_len_dev && best_j_out_dev && score_out_dev && flags_out_dev), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n_orf == 0 || n_genomes != 0, GS_ERR_INVALID, "gene: ORFs without a genome");
    GS_REQUIRE(seq_dev || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_REQUIRE(seq_bytes < (1ull << 61), GS_ERR_UNSUPPORTED, "gene: seq_bytes");
    GS_CTX_LOCK(c);
    PoolBuf meta(c, SL_GENE_META);
    if ((rc = meta.alloc(8 * GENE_META_WORDS))) return rc;
    GS_HIP_CHECK(hipMemsetAsync(meta.p, 0, 8 * GENE_META_WORDS, c->stream));
    const GeneIn in{(const uint8_t *)seq_dev, rec_start_dev, rec_len_dev, genome_rec_off_dev, n_rec, n_genomes, 4 * seq_bytes};
    if (n_genomes) hipLaunchKernelGGL(k_gene_check_tables, gene_grid(4096 * n_genomes, 256), dim3(256), 0, c->stream, tables_dev, 4096 * n_genomes, meta.as<uint32_t>());
    if ((rc = gene_score_queue(c, in, prm, tables_dev, nullptr, orf_dev, orf_len_dev, n_orf, best_j_out_dev, score_out_dev, flags_out_dev, meta.as<uint32_t>()))) return rc;
    uint64_t h[GENE_META_WORDS];
    return gene_read_meta(c, meta, h);
}

int gs_gene_call_dev(gs_ctx *c, const gs_gene_params *prm, const void *seq_dev, uint64_t seq_bytes, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                     const uint64_t *genome_rec_off_dev, uint64_t n_genomes, uint64_t cap_gene, uint64_t cap_aa, gs_gene *gene_out_dev, uint8_t *aa_out_dev,
                     uint64_t *aa_start_out_dev, uint64_t *aa_len_out_dev, uint64_t *rec_gene_off_out_dev, uint64_t *info_out_dev, int32_t *tables_out_dev, uint64_t n_out[2])
{
    using namespace gs;
    GS_REQUIRE(c && n_out, GS_ERR_INVALID, "null argument");
    int rc;
    bool count_only;
    if ((rc = gene_check_params(prm, n_rec, n_genomes)) ||
        (rc = gene_check_outputs(cap_gene, cap_aa, gene_out_dev, aa_out_dev, aa_start_out_dev, aa_len_out_dev, rec_gene_off_out_dev, &count_only)))
        return rc;
    GS_REQUIRE(genome_rec_off_dev && (n_rec == 0 || (rec_start_dev && rec_len_dev)) && (n_genomes == 0 || info_out_dev), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(seq_dev || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_CTX_LOCK(c);
    GeneRun R(c);
    R.in = GeneIn{(const uint8_t *)seq_dev, rec_start_dev, rec_len_dev, genome_rec_off_dev, n_rec, n_genomes, 4 * seq_bytes};
    if ((rc = gene_run(c, prm, R, seq_bytes, info_out_dev, tables_out_dev, n_out))) return rc;
    if (count_only) return GS_OK;
    if ((rc = gene_check_caps(n_out, cap_gene, cap_aa))) return rc;
    return gene_emit(c, R, gene_out_dev, aa_out_dev, aa_start_out_dev, aa_len_out_dev, rec_gene_off_out_dev);
}

int gs_gene_call(gs_ctx *c, const gs_gene_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec,
                 const uint64_t *genome_rec_off, uint64_t n_genomes, uint64_t cap_gene, uint64_t cap_aa, gs_gene *gene_out, uint8_t *aa_out, uint64_t *aa_start_out,
                 uint64_t *aa_len_out, uint64_t *rec_gene_off_out, uint64_t *info_out, int32_t *tables_out, uint64_t n_out[2])
{
    using namespace gs;
    GS_REQUIRE(c && n_out, GS_ERR_INVALID, "null argument");
    int rc;
    bool count_only;
    if ((rc = gene_check_params(prm, n_rec, n_genomes)) || (rc = gene_check_outputs(cap_gene, cap_aa, gene_out, aa_out, aa_start_out, aa_len_out, rec_gene_off_out, &count_only)))
        return rc;
    GS_REQUIRE(genome_rec_off && (n_rec == 0 || (rec_start && rec_len)) && (n_genomes == 0 || info_out), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(seq || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_CTX_LOCK(c);
    PoolBuf d_seq(c, SL_GENEB_SEQ), d_rs(c, SL_GENEB_REC_START), d_rl(c, SL_GENEB_REC_LEN), d_goff(c, SL_GENEB_GOFF), d_info(c, SL_GENEB_INFO), d_tab(c, SL_GENEB_TABLES);
    if ((rc = d_seq.alloc(seq_bytes)) || (rc = d_rs.alloc(8 * n_rec)) || (rc = d_rl.alloc(8 * n_rec)) || (rc = d_goff.alloc(8 * (n_genomes + 1))) ||
        (rc = d_info.alloc(16 * n_genomes)) || (rc = d_tab.alloc(4 * 4096 * n_genomes)))
        return rc;
    if (seq_bytes) GS_HIP_CHECK(hipMemcpyAsync(d_seq.p, seq, seq_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_rec) {
        GS_HIP_CHECK(hipMemcpyAsync(d_rs.p, rec_start, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(d_rl.p, rec_len, 8 * n_rec, hipMemcpyHostToDevice, c->stream));
    }
    GS_HIP_CHECK(hipMemcpyAsync(d_goff.p, genome_rec_off, 8 * (n_genomes + 1), hipMemcpyHostToDevice, c->stream));
    GeneRun R(c);
    R.in = GeneIn{d_seq.as<uint8_t>(), d_rs.as<uint64_t>(), d_rl.as<uint64_t>(), d_goff.as<uint64_t>(), n_rec, n_genomes, 4 * seq_bytes};
    if ((rc = gene_run(c, prm, R, seq_bytes, d_info.as<uint64_t>(), d_tab.as<int32_t>(), n_out))) return rc;
    if (n_genomes) {
        GS_HIP_CHECK(hipMemcpyAsync(info_out, d_info.p, 16 * n_genomes, hipMemcpyDeviceToHost, c->stream));
        if (tables_out) GS_HIP_CHECK(hipMemcpyAsync(tables_out, d_tab.p, 4 * 4096 * n_genomes, hipMemcpyDeviceToHost, c->stream));
    }
    if (count_only) { GS_HIP_CHECK(stream_wait(c)); return GS_OK; }
    if ((rc = gene_check_caps(n_out, cap_gene, cap_aa))) { (void)stream_wait(c); return rc; }
    const uint64_t ng = n_out[0], na = n_out[1];
    PoolBuf d_gene(c, SL_GENEB_GENE), d_aa(c, SL_GENEB_AA), d_as(c, SL_GENEB_AA_START), d_al(c, SL_GENEB_AA_LEN), d_off(c, SL_GENEB_REC_OFF);
    if ((rc = d_gene.alloc(sizeof(gs_gene) * ng)) || (rc = d_aa.alloc(na)) || (rc = d_as.alloc(8 * ng)) || (rc = d_al.alloc(8 * ng)) || (rc = d_off.alloc(8 * (n_rec + 1)))) return rc;
    if ((rc = gene_emit(c, R, d_gene.as<gs_gene>(), d_aa.as<uint8_t>(), d_as.as<uint64_t>(), d_al.as<uint64_t>(), d_off.as<uint64_t>()))) return rc;
    if (ng) {
        GS_HIP_CHECK(hipMemcpyAsync(gene_out, d_gene.p, sizeof(gs_gene) * ng, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(aa_start_out, d_as.p, 8 * ng, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(aa_len_out, d_al.p, 8 * ng, hipMemcpyDeviceToHost, c->stream));
    }
    if (na) GS_HIP_CHECK(hipMemcpyAsync(aa_out, d_aa.p, na, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(rec_gene_off_out, d_off.p, 8 * (n_rec + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

// ---- the stage entries on the host: the same definitions in plain loops, no device ------------------------------------------------------------------------------
static int gene_host_check(const gs_gene_params *prm, const void *seq, uint64_t seq_bytes, const uint64_t *rs, const uint64_t *rl, uint64_t n_rec, const uint64_t *goff,
                           uint64_t n_genomes)
{
    using namespace gs;
    int rc;
    if ((rc = gene_check_params(prm, n_rec, n_genomes))) return rc;
    GS_REQUIRE(goff && (n_rec == 0 || (rs && rl)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(seq || seq_bytes == 0, GS_ERR_INVALID, "null seq");
    GS_REQUIRE(seq_bytes < (1ull << 61), GS_ERR_UNSUPPORTED, "gene: seq_bytes");
    uint32_t err = 0;
    for (uint64_t g = 0; g < n_genomes; g++) if (!gene_goff_ok(goff, n_genomes, n_rec, g)) err |= GENE_ERR_GOFF;
    if (!err) for (uint64_t r = 0; r < n_rec; r++) if (!gene_rec_ok(rs[r], rl[r], 4 * seq_bytes)) err |= GENE_ERR_REC;
    return gene_report(err);
}

int gs_gene_train_host(const gs_gene_params *prm, const void *seq_v, uint64_t seq_bytes, const uint64_t *rs, const uint64_t *rl, uint64_t n_rec, const uint64_t *goff,
                       uint64_t n_genomes, const gs_gene_interval *iv, uint64_t n_iv, int32_t *tables_out, uint64_t *info_out)
{
    using namespace gs;
    int rc;
    if ((rc = gene_host_check(prm, seq_v, seq_bytes, rs, rl, n_rec, goff, n_genomes))) return rc;
    GS_REQUIRE((n_iv == 0 || iv) && (n_genomes == 0 || (tables_out && info_out)), GS_ERR_INVALID, "null argument");
    const uint8_t *seq = (const uint8_t *)seq_v;
    std::vector<uint64_t> bg(4096 * n_genomes, 0), cod(4096 * n_genomes, 0);
    uint32_t err = 0;
    for (uint64_t g = 0; g < n_genomes; g++)
        for (uint64_t r = goff[g]; r < goff[g + 1]; r++)
            for (uint64_t p = 0; p + 6 <= rl[r]; p++) {
                const uint32_t h = gene_hexamer_at(seq, rs[r] + p);
                bg[g * 4096 + h]++; bg[g * 4096 + gene_rev_hexamer(h)]++;
            }
    for (uint64_t k = 0; k < n_iv; k++) {
        const gs_gene_interval v = iv[k];
        if (v.rec >= n_rec || v.strand > 1 || (k != 0 && iv[k - 1].rec > v.rec) || v.n > rl[v.rec] / 3 || v.begin > rl[v.rec] - 3 * v.n) { err |= GENE_ERR_IV; continue; }
        if (v.n >= GS_GENE_MAX_INTERVAL) { err |= GENE_ERR_BIG; continue; }
        const uint64_t g = gene_genome_of(goff, n_genomes, v.rec);
        for (uint64_t t = 0; t + 1 < v.n; t++) {
            const uint32_t f0 = gene_codon_at(seq, rs[v.rec] + v.begin + 3 * t), f1 = gene_codon_at(seq, rs[v.rec] + v.begin + 3 * t + 3);
            cod[g * 4096 + (v.strand ? 64 * orf_rev_codon(f1) + orf_rev_codon(f0) : 64 * f0 + f1)]++;
        }
    }
    for (uint64_t g = 0; g < n_genomes; g++) {
        uint64_t Nb = 4096, Nc = 0;
        for (uint32_t h = 0; h < 4096; h++) { Nb += bg[g * 4096 + h]; Nc += cod[g * 4096 + h]; }
        if (Nb > GS_GENE_MAX_NB || Nc + GS_GENE_PRIOR > GS_GENE_MAX_NC_A) { err |= GENE_ERR_BIG; continue; }
        info_out[2 * g] = Nc;
        info_out[2 * g + 1] = Nc >= prm->min_train_codons ? GS_GENE_TRAINED : 0;
        for (uint32_t h = 0; h < 4096; h++) tables_out[g * 4096 + h] = gene_table_entry(cod[g * 4096 + h], bg[g * 4096 + h] + 1, Nc, Nb);
    }
    return gene_report(err);
}

int gs_gene_score_host(const gs_gene_params *prm, const void *seq_v, uint64_t seq_bytes, const uint64_t *rs, const uint64_t *rl, uint64_t n_rec, const uint64_t *goff,
                       uint64_t n_genomes, const int32_t *tables, const gs_orf *orf, const uint64_t *orf_len, uint64_t n_orf, uint64_t *best_j_out, int64_t *score_out,
                       uint32_t *flags_out)
{
    using namespace gs;
    int rc;
    if ((rc = gene_host_check(prm, seq_v, seq_bytes, rs, rl, n_rec, goff, n_genomes))) return rc;
    GS_REQUIRE((n_genomes == 0 || tables) && (n_orf == 0 || (orf && orf_len && best_j_out && score_out && flags_out)), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n_orf == 0 || n_genomes != 0, GS_ERR_INVALID, "gene: ORFs without a genome");
    const uint8_t *seq = (const uint8_t *)seq_v;
    uint32_t err = 0;
    for (uint64_t i = 0; i < 4096 * n_genomes; i++) if (tables[i] > GS_GENE_S_LIMIT || tables[i] < -GS_GENE_S_LIMIT) err |= GENE_ERR_TABLE;
    for (uint64_t o = 0; o < n_orf; o++) {
        const gs_orf d = orf[o];
        const uint64_t n = orf_len[o];
        best_j_out[o] = GS_GENE_NO_START; score_out[o] = 0; flags_out[o] = 0;
        if (!gene_orf_ok(d, n, n_rec, rs, rl, 4 * seq_bytes)) { err |= GENE_ERR_ORF; continue; }
        const int32_t *S = tables + gene_genome_of(goff, n_genomes, d.rec) * 4096;
        const uint64_t base = rs[d.rec], L = rl[d.rec];
        const bool rev = d.strand != 0, low_open = d.begin < 3, high_open = d.begin + 3 * n + 3 > L;
        const bool open5 = rev ? high_open : low_open, open3 = rev ? low_open : high_open;
        int64_t T = 0, bs = 0; uint64_t bu = 0; uint32_t bt = 0; bool have = false;
        uint32_t after = 0;
        for (uint64_t u = 0; u < n; u++) {
            const uint32_t cu = gene_codon_u(seq, base, d.begin, n, rev, u);
            if (u >= 1) T += S[64 * cu + after];
            after = cu;
            const int type = gene_start_type(cu);
            const bool edge = open5 && u == n - 1, start = type >= 0 && u + 1 >= prm->min_aa;
            if (!edge && !start) continue;
            const int64_t s = edge ? T : T + gene_start_bonus(type);
            if (gene_better(true, s, u, have, bs, bu)) { bs = s; bu = u; bt = edge ? (type == 0 ? 0u : GS_GENE_TYPE_EDGE) : (uint32_t)type; have = true; }
        }
        best_j_out[o] = have ? n - 1 - bu : GS_GENE_NO_START;
        score_out[o] = have ? bs : 0;
        flags_out[o] = gene_flags(rev, open5, open3, have, bt, bs, prm->min_score);
    }
    return gene_report(err);
}
