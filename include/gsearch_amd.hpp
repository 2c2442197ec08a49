// gsearch_amd.hpp — C++17 host-side mirror of the reference's operator interface for the sketch-and-query hot path,
// header-only over the C ABI (gsearch_amd.h). The reference is Rust; its extension points for this path are the traits
//   kmerutils::sketching::setsketchert::SeqSketcherT   (src/dna/dnasketch.rs:64-73, calls :336,357; dnarequest.rs:272,287)
//   anndists::dist::Distance / DistHamming             (src/dna/dnasketch.rs:72,139; src/bin/bindash.rs:93-99)
//   hnsw_rs::Hnsw                                      (src/dna/dnasketch.rs:139-141,159-160,435; src/dna/dnarequest.rs:353)
// The classes below keep their names, argument meaning and error behaviour (the reference panics / exits on internal
// failure, dnasketch.rs:228,285,380: here a gsearch::Error is thrown with the library's message).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <ostream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "gsearch_amd.h"

namespace gsearch {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error("gsearch_amd error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int rc) { if (rc != GS_OK) throw Error(rc, gs_last_error()); }
// debugging (not for production use): fill new device allocations and newly taken scratch with `byte` (0..255); -1 = off
inline void debug_mem_fill(int byte) { check(gs_debug_mem_fill(byte)); }

class Context {   // one per (process, GPU)
public:
    explicit Context(int device = 0, void *stream = nullptr) { check(gs_ctx_create(&h_, device, stream)); }
    ~Context() { gs_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    gs_ctx *get() const { return h_; }
    void sync() { check(gs_ctx_sync(h_)); }
    void release_scratch() { check(gs_ctx_release_scratch(h_)); }   // device scratch kept between calls
private:
    gs_ctx *h_ = nullptr;
};

enum class SketchAlgo : uint32_t { PROB3A = GS_ALGO_PROB3A, SUPER = GS_ALGO_SUPER, SUPER2 = GS_ALGO_SUPER2, HLL = GS_ALGO_HLL, OPTDENS = GS_ALGO_OPTDENS, REVOPTDENS = GS_ALGO_REVOPTDENS,
                                  HMH = GS_ALGO_HMH /* hypermash: sketch_size 16384, canonical DNA, u16 */ };
enum class DataType : uint32_t { DNA = GS_DATA_DNA, AA = GS_DATA_AA, DNA_FWD = GS_DATA_DNA_FWD /* bindash.rs:346-354: k <= 14, no reverse-complement minimum */ };

// kmerutils::sketcharg::SeqSketcherParams::new(kmer_size, sketch_size, algo, data_t)  (src/bin/gsearch.rs:258-263)
class SeqSketcherParams {
public:
    SeqSketcherParams(uint32_t kmer_size, uint32_t sketch_size, SketchAlgo algo, DataType data_t = DataType::DNA)
        : p_{kmer_size, sketch_size, (uint32_t)algo, (uint32_t)data_t} { check(gs_check_params(&p_)); }
    uint32_t get_kmer_size() const { return p_.k; }
    uint32_t get_sketch_size() const { return p_.sketch_size; }
    SketchAlgo get_algo() const { return (SketchAlgo)p_.algo; }
    int sig_kind() const { return gs_sig_kind(&p_); }
    const gs_sketch_params *raw() const { return &p_; }
private:
    gs_sketch_params p_;
};

template <class T> constexpr int kind_of()
{
    if (std::is_same<T, float>::value) return GS_KIND_F32;
    if (std::is_same<T, uint32_t>::value) return GS_KIND_U32;
    if (std::is_same<T, uint64_t>::value) return GS_KIND_U64;
    return GS_KIND_U16;
}

// A `Sequence` of the reference is a 2-bit packed record; here a record is ASCII (the glue packs like encode_and_add, dnafiles.rs:70-71)
using Record = std::string;

// SeqSketcherT<Kmer>: `Sig` is the signature element type of the (algo, k) dispatch (dnasketch.rs:499-642)
template <class Sig>
class SeqSketcher {
public:
    SeqSketcher(Context &ctx, const SeqSketcherParams &params) : ctx_(ctx), params_(params)
    {
        if (params_.sig_kind() != kind_of<Sig>()) throw Error(GS_ERR_INVALID, "Sig type does not match the (algo, k) dispatch of the reference");
    }
    // all sequences are ONE genome -> exactly one signature (assert at dnasketch.rs:359)
    std::vector<std::vector<Sig>> sketch_compressedkmer_seqs(const std::vector<const Record *> &vseq) const { return run(vseq, true); }
    // one signature per input sequence, in input order (assert at dnasketch.rs:338)
    std::vector<std::vector<Sig>> sketch_compressedkmer(const std::vector<const Record *> &vseq) const { return run(vseq, false); }
    // batch form: genomes = lists of records -> row-major (n_genomes x sketch_size)
    std::vector<Sig> sketch_genomes(const std::vector<std::vector<Record>> &genomes) const
    {
        std::vector<const Record *> recs; std::vector<uint64_t> goff{0};
        for (auto &g : genomes) { for (auto &r : g) recs.push_back(&r); goff.push_back(recs.size()); }
        return sketch_flat(recs, goff);
    }
private:
    std::vector<Sig> sketch_flat(const std::vector<const Record *> &recs, const std::vector<uint64_t> &goff) const
    {
        const bool aa = params_.raw()->data_t == GS_DATA_AA;
        std::vector<uint64_t> rs(recs.size()), rl(recs.size());
        uint64_t total = 0;
        for (auto *r : recs) total += r->size() + 4;
        std::vector<uint8_t> seq(aa ? total + 64 : total / 4 + 64, 0);
        uint64_t off = 0;
        for (size_t i = 0; i < recs.size(); i++) {
            const uint8_t *a = (const uint8_t *)recs[i]->data();
            rs[i] = off;
            if (aa) { rl[i] = gs_filter_aa(a, recs[i]->size(), seq.data() + off); off += rl[i]; }
            else { rl[i] = gs_pack_dna(a, recs[i]->size(), seq.data(), off); off += (rl[i] + 3) / 4 * 4; }
        }
        const uint64_t ng = goff.size() - 1, m = params_.get_sketch_size();
        std::vector<Sig> out(ng * m);
        check(gs_sketch_batch(ctx_.get(), params_.raw(), seq.data(), seq.size(), rs.data(), rl.data(), recs.size(), goff.data(), ng, out.data()));
        return out;
    }
    std::vector<std::vector<Sig>> run(const std::vector<const Record *> &vseq, bool one_genome) const
    {
        std::vector<uint64_t> goff;
        if (one_genome) goff = {0, vseq.size()};
        else for (uint64_t i = 0; i <= vseq.size(); i++) goff.push_back(i);
        std::vector<Sig> flat = sketch_flat(vseq, goff);
        const uint64_t m = params_.get_sketch_size();
        std::vector<std::vector<Sig>> out(goff.size() - 1);
        for (size_t g = 0; g < out.size(); g++) out[g].assign(flat.begin() + g * m, flat.begin() + (g + 1) * m);
        return out;
    }
    Context &ctx_;
    SeqSketcherParams params_;
};
// the names gsearch instantiates (dnasketch.rs:499-642)
template <class Sig = float> using OptDensHashSketch = SeqSketcher<Sig>;
template <class Sig = float> using RevOptDensHashSketch = SeqSketcher<Sig>;
template <class Sig = float> using SuperHashSketch = SeqSketcher<Sig>;
template <class Sig> using SuperHash2Sketch = SeqSketcher<Sig>;
template <class Sig> using ProbHash3aSketch = SeqSketcher<Sig>;

// anndists::dist::DistHamming: eval(a, b) = count(a[i] != b[i]) / len as f32
class DistHamming {
public:
    explicit DistHamming(Context &ctx) : ctx_(&ctx) {}
    template <class T> float eval(const std::vector<T> &va, const std::vector<T> &vb) const
    {
        if (va.size() != vb.size()) throw Error(GS_ERR_INVALID, "signature lengths differ");
        float d = 0;
        check(gs_hamming_qxc(ctx_->get(), kind_of<T>(), (uint32_t)va.size(), va.data(), 1, vb.data(), 1, &d));
        return d;
    }
    // Q (nq x m) against C (nc x m), row-major: the all-pairs loop of bindash.rs:120-157 in one call
    template <class T> std::vector<float> eval_qxc(const std::vector<T> &Q, uint64_t nq, const std::vector<T> &C, uint64_t nc, uint32_t m) const
    {
        std::vector<float> out(nq * nc);
        check(gs_hamming_qxc(ctx_->get(), kind_of<T>(), m, Q.data(), nq, C.data(), nc, out.data()));
        return out;
    }
    Context &context() const { return *ctx_; }
private:
    Context *ctx_;
};
// reformat.rs:80-86
inline double calculate_ani(double distance, int kmer, int model) { return gs_ani(distance, kmer, model); }

// hypermash (src/bin/hypermash.rs; hyperminhash::Sketch, SPEC 7): sketches of 16384 u16 registers (SeqSketcher<uint16_t> with SketchAlgo::HMH, or
// hmh_sketch_files with hypermash's reader rules), their cardinality, the similarity of every query x reference pair and the distance
inline std::vector<uint64_t> hmh_cardinality(Context &ctx, const std::vector<uint16_t> &sigs)
{
    std::vector<uint64_t> out(sigs.size() / GS_HMH_REGISTERS);
    check(gs_hmh_cardinality(ctx.get(), sigs.data(), out.size(), out.data()));
    return out;
}
inline std::vector<double> hmh_similarity_qxc(Context &ctx, const std::vector<uint16_t> &Q, const std::vector<uint16_t> &R)
{
    const uint64_t nq = Q.size() / GS_HMH_REGISTERS, nr = R.size() / GS_HMH_REGISTERS;
    std::vector<double> out(nq * nr);
    check(gs_hmh_similarity_qxc(ctx.get(), Q.data(), nq, R.data(), nr, out.data()));
    return out;
}
inline std::vector<uint16_t> hmh_sketch_files(Context &ctx, uint32_t k, const std::vector<std::string> &paths, uint32_t n_threads = 0)
{
    std::vector<const char *> p;
    for (const auto &x : paths) p.push_back(x.c_str());
    std::vector<uint16_t> out(paths.size() * GS_HMH_REGISTERS);
    check(gs_hmh_sketch_files(ctx.get(), k, p.data(), p.size(), n_threads, out.data(), nullptr, nullptr, nullptr));
    return out;
}
inline double hypermash_distance(double sim, int kmer) { return gs_hmh_distance(sim, kmer); }

// superaai (binaux/src/bin/superaai.rs; sourmash KmerMinHash, SPEC 9): FracMinHash / bottom-k sketches of proteome files (ascending u64 values per
// file), the similarity of every query x reference pair (query-major) and the AAI
struct FracSketches { std::vector<uint64_t> values, off; };        // file f: values[off[f] .. off[f+1])
inline FracSketches frac_sketch_files(Context &ctx, const std::vector<std::string> &paths, uint32_t k = 7, uint32_t scaled = 100, uint32_t num = 5120,
                                      uint32_t n_threads = 0)
{
    std::vector<const char *> p;
    for (const auto &x : paths) p.push_back(x.c_str());
    FracSketches out;
    out.off.resize(paths.size() + 1);
    uint64_t *h = nullptr;
    check(gs_frac_sketch_files(ctx.get(), k, scaled, num, p.data(), p.size(), n_threads, &h, out.off.data(), nullptr, nullptr, nullptr));
    out.values.assign(h, h + out.off.back());
    gs_host_free(h);
    return out;
}
inline std::vector<double> frac_similarity_qxc(Context &ctx, uint32_t num, const FracSketches &Q, const FracSketches &R)
{
    const uint64_t nq = Q.off.size() - 1, nr = R.off.size() - 1;
    std::vector<double> out(nq * nr);
    check(gs_frac_similarity_qxc(ctx.get(), num, Q.values.data(), Q.off.data(), nq, R.values.data(), R.off.data(), nr, out.data(), nullptr, nullptr));
    return out;
}
inline double aai(double sim, uint32_t k) { return gs_aai(sim, k); }

// superani (binaux/src/bin/superani.rs; SPEC 12): seeds of packed genomes (the layout of gs_sketch_batch), the eight integers of every listed pair and
// the closed form {ani, af_q, af_r}
struct AniSeeds { std::vector<uint32_t> seeds; std::vector<uint64_t> off; };        // genome g: 4 u32 per seed, seeds [off[g] .. off[g+1])
inline AniSeeds ani_sketch_batch(Context &ctx, const void *seq, uint64_t seq_bytes, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len,
                                 const std::vector<uint64_t> &genome_rec_off, uint32_t k = 16, uint32_t c = 30)
{
    AniSeeds out;
    out.off.resize(genome_rec_off.size());
    uint32_t *h = nullptr;
    check(gs_ani_sketch_batch(ctx.get(), k, c, seq, seq_bytes, rec_start.data(), rec_len.data(), rec_start.size(), genome_rec_off.data(), genome_rec_off.size() - 1, &h,
                              out.off.data()));
    out.seeds.assign(h, h + 4 * out.off.back());
    gs_host_free(h);
    return out;
}
inline std::vector<uint64_t> ani_pairs(Context &ctx, const AniSeeds &Q, const AniSeeds &R, const std::vector<uint32_t> &pair_q, const std::vector<uint32_t> &pair_r,
                                       uint32_t k = 16, uint64_t max_block_anchors = 0)
{
    std::vector<uint64_t> out(8 * pair_q.size());
    check(gs_ani_pairs(ctx.get(), k, Q.seeds.data(), Q.off.data(), Q.off.size() - 1, R.seeds.data(), R.off.data(), R.off.size() - 1, pair_q.data(), pair_r.data(),
                       pair_q.size(), out.data(), max_block_anchors));
    return out;
}
inline std::vector<float> ani_estimate(const std::vector<uint64_t> &counts, const std::vector<uint64_t> &bases_q, const std::vector<uint64_t> &bases_r, uint32_t k = 16)
{
    std::vector<float> out(3 * bases_q.size());
    check(gs_ani_estimate(counts.data(), bases_q.data(), bases_r.data(), bases_q.size(), k, out.data()));
    return out;
}

// hmmsearch (`hmmsearch_rs -f proteome.faa -m profile.HMM`; SPEC 13, 13.1): a set of HMMER3 profiles on the device, the raw Viterbi score (units of
// 2^-10 bit) of every record against every profile, the Forward score of the pairs above a Viterbi floor, and the best record per genome and profile
class HmmDb {
public:
    HmmDb(Context &ctx, const std::vector<std::string> &paths) : ctx_(&ctx)
    {
        std::vector<const char *> p;
        for (const auto &s : paths) p.push_back(s.c_str());
        check(gs_hmm_db_load(ctx.get(), p.data(), p.size(), &db_));
        uint64_t n = 0;
        check(gs_hmm_db_info(db_, &n, nullptr, 0));
        info_.resize(n);
        check(gs_hmm_db_info(db_, &n, info_.data(), n));
    }
    ~HmmDb() { gs_hmm_db_free(db_); }
    HmmDb(const HmmDb &) = delete;
    HmmDb &operator=(const HmmDb &) = delete;
    gs_hmm_db *get() const { return db_; }
    const std::vector<gs_hmm_info> &info() const { return info_; }
    // residues as gs_filter_aa leaves them; record r = aa[rec_start[r] .. + rec_len[r]) -> n_rec x n_prof scores, GS_HMM_NO_SCORE for an empty record
    std::vector<int32_t> search(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len) const
    {
        std::vector<int32_t> out(rec_start.size() * info_.size());
        check(gs_hmm_search(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), out.data()));
        return out;
    }
    // SPEC 13.1: the Viterbi matrix (as search() gives it) and the Forward raw score of the pairs whose Viterbi score reaches vit_floor[p] (units; an
    // empty vector: every pair that has a Viterbi score), GS_HMM_NO_SCORE for the others
    std::pair<std::vector<int32_t>, std::vector<int32_t>> search_forward(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len,
                                                                          const std::vector<int32_t> &vit_floor = {}) const
    {
        std::vector<int32_t> vit(rec_start.size() * info_.size()), fwd(vit.size());
        check(gs_hmm_search_forward(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), vit_floor.empty() ? nullptr : vit_floor.data(), vit.data(),
                                    fwd.data()));
        return {std::move(vit), std::move(fwd)};
    }
    // SPEC 13.3: the MSV raw score of every pair (ungapped diagonals; the prefilter's score)
    std::vector<int32_t> search_msv(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len) const
    {
        std::vector<int32_t> out(rec_start.size() * info_.size());
        check(gs_hmm_search_msv(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), out.data()));
        return out;
    }
    // SPEC 13.3: MSV of every pair, Viterbi of the pairs whose MSV score reaches msv_floor[p], and - forward = true - Forward behind vit_floor as
    // search_forward() runs it; GS_HMM_NO_SCORE for the pairs a floor left out. An empty floor vector: every pair that has the score in front
    struct Filtered { std::vector<int32_t> msv, vit, fwd; };
    Filtered search_filtered(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len, const std::vector<int32_t> &msv_floor = {},
                             bool forward = false, const std::vector<int32_t> &vit_floor = {}) const
    {
        const size_t n = rec_start.size() * info_.size();
        Filtered f{std::vector<int32_t>(n), std::vector<int32_t>(n), std::vector<int32_t>(forward ? n : 0)};
        check(gs_hmm_search_filtered(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), msv_floor.empty() ? nullptr : msv_floor.data(),
                                     vit_floor.empty() ? nullptr : vit_floor.data(), f.msv.data(), f.vit.data(), forward ? f.fwd.data() : nullptr));
        return f;
    }
    // SPEC 13.7: vf of every pair, the packed int16 Viterbi filter score: vf >= the Viterbi score, GS_HMM_VF_OVER where the int16 cells overflow
    std::vector<int32_t> search_vit16(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len) const
    {
        std::vector<int32_t> out(rec_start.size() * info_.size());
        check(gs_hmm_search_vit16(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), out.data()));
        return out;
    }
    // the int16 table of profile p, [GS_HMM_TABLE_ROWS][M + 1]
    std::vector<int16_t> tables16(uint64_t p) const
    {
        std::vector<int16_t> out((size_t)GS_HMM_TABLE_ROWS * (info_.at(p).M + 1));
        check(gs_hmm_db_tables16(db_, p, out.data(), out.size()));
        return out;
    }
    // SPEC 13.7: MSV of every pair (use_msv), vf of every pair or of the pairs at or above msv_floor[p], Viterbi of the pairs with vf >= vf_floor[p] and -
    // forward = true - Forward behind vit_floor; GS_HMM_NO_SCORE for the pairs a floor left out. An empty floor vector: every pair that has the score in front
    struct Staged { std::vector<int32_t> msv, vf, vit, fwd; };
    Staged search_staged(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len, const std::vector<int32_t> &vf_floor,
                         bool use_msv = false, const std::vector<int32_t> &msv_floor = {}, bool forward = false, const std::vector<int32_t> &vit_floor = {}) const
    {
        const size_t n = rec_start.size() * info_.size();
        Staged f{std::vector<int32_t>(use_msv ? n : 0), std::vector<int32_t>(n), std::vector<int32_t>(n), std::vector<int32_t>(forward ? n : 0)};
        check(gs_hmm_search_staged(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), use_msv ? 1 : 0, msv_floor.empty() ? nullptr : msv_floor.data(),
                                   vf_floor.empty() ? nullptr : vf_floor.data(), vit_floor.empty() ? nullptr : vit_floor.data(), use_msv ? f.msv.data() : nullptr,
                                   f.vf.data(), f.vit.data(), forward ? f.fwd.data() : nullptr));
        return f;
    }
    // SPEC 13.2: the domains of the Viterbi path of the pairs (pair_rec[j], pair_prof[j]), traced back on the device. raw[j] as search() gives it,
    // n_dom[j] the true number of domains, dom[(j * max_dom + d) * GS_HMM_DOM_WORDS ..] the first max_dom of them in sequence order (zeros behind them)
    struct Trace { std::vector<int32_t> raw; std::vector<uint32_t> n_dom; std::vector<int32_t> dom; };
    Trace trace(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len, const std::vector<uint32_t> &pair_rec,
                const std::vector<uint32_t> &pair_prof, uint32_t max_dom = 8, uint64_t max_block_cells = 0) const
    {
        Trace t{std::vector<int32_t>(pair_rec.size()), std::vector<uint32_t>(pair_rec.size()), std::vector<int32_t>(pair_rec.size() * max_dom * GS_HMM_DOM_WORDS)};
        check(gs_hmm_trace(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), pair_rec.data(), pair_prof.data(), pair_rec.size(), max_dom,
                           max_block_cells, t.raw.data(), t.n_dom.data(), t.dom.empty() ? nullptr : t.dom.data()));
        return t;
    }
    // SPEC 13.4: Forward and Backward raw scores and the posterior envelopes of the pairs. n_env[j] the true number of envelopes,
    // env[(j * max_env + d) * GS_HMM_ENV_WORDS ..] = i_from, i_to, env_raw, peak of the first max_env of them in sequence order (zeros behind them)
    struct Envelopes { std::vector<int32_t> fwd, bck; std::vector<uint32_t> n_env; std::vector<int32_t> env; };
    Envelopes envelopes(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len, const std::vector<uint32_t> &pair_rec,
                        const std::vector<uint32_t> &pair_prof, uint32_t max_env = 8, uint64_t max_block_rows = 0) const
    {
        const size_t n = pair_rec.size();
        Envelopes e{std::vector<int32_t>(n), std::vector<int32_t>(n), std::vector<uint32_t>(n), std::vector<int32_t>(n * max_env * GS_HMM_ENV_WORDS)};
        check(gs_hmm_envelopes(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), pair_rec.data(), pair_prof.data(), n, max_env, max_block_rows,
                               e.fwd.data(), e.bck.data(), e.n_env.data(), e.env.empty() ? nullptr : e.env.data(), nullptr, nullptr, nullptr));
        return e;
    }
    // SPEC 13.5: the null2 bias of the envelopes envelopes() listed for the same pairs and max_env. slot[(j * max_env + d) * GS_HMM_N2_WORDS ..] = corr,
    // dom_bias, seg_raw, mass; the corrected scores are env_raw - dom_bias and fwd[j] - seq_bias[j]
    struct Null2 { std::vector<int32_t> slot, seq_bias; };
    Null2 null2(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len, const std::vector<uint32_t> &pair_rec,
                const std::vector<uint32_t> &pair_prof, const Envelopes &e, uint32_t max_env = 8, uint64_t max_block_cells = 0) const
    {
        const size_t n = pair_rec.size();
        Null2 b{std::vector<int32_t>(n * max_env * GS_HMM_N2_WORDS), std::vector<int32_t>(n)};
        check(gs_hmm_null2(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), pair_rec.data(), pair_prof.data(), n, max_env, max_block_cells,
                           e.n_env.data(), e.env.empty() ? nullptr : e.env.data(), b.slot.empty() ? nullptr : b.slot.data(), b.seq_bias.data(), nullptr, nullptr, nullptr,
                           nullptr));
        return b;
    }
    // SPEC 13.6: the optimal-accuracy alignment of the envelopes envelopes() listed for the same pairs and max_env.
    // slot[(j * max_env + d) * GS_HMM_ALI_WORDS ..] = i_from, i_to, k_from, k_to, oa, n_match, n_ins, n_del; expected accuracy = oa / (65536 Ld)
    std::vector<int32_t> align(const uint8_t *aa, const std::vector<uint64_t> &rec_start, const std::vector<uint64_t> &rec_len, const std::vector<uint32_t> &pair_rec,
                               const std::vector<uint32_t> &pair_prof, const Envelopes &e, uint32_t max_env = 8, uint64_t max_block_cells = 0) const
    {
        const size_t n = pair_rec.size();
        std::vector<int32_t> slot(n * max_env * GS_HMM_ALI_WORDS);
        check(gs_hmm_align(ctx_->get(), db_, aa, rec_start.data(), rec_len.data(), rec_start.size(), pair_rec.data(), pair_prof.data(), n, max_env, max_block_cells,
                           e.n_env.data(), e.env.empty() ? nullptr : e.env.data(), slot.empty() ? nullptr : slot.data(), nullptr, nullptr));
        return slot;
    }
    // SPEC 13.8: the hits of a [n_genomes][n_prof] best-hit matrix as sketcher records, on the host: the chosen residues back to back in (genome, profile)
    // order, start / len against them, genome_off[g] the first hit of genome g. n_item / item (both empty: whole records): the spans of trace(),
    // envelopes() or align() over the matrix as a pair list, item_words the words of one of their slots, max_item the slots a pair
    struct HitRecords { std::vector<uint8_t> aa; std::vector<uint64_t> start, len, genome_off; };
    static HitRecords hit_records(const std::vector<uint32_t> &best_rec, uint64_t n_genomes, uint64_t n_prof, const uint8_t *aa, const std::vector<uint64_t> &rec_start,
                                  const std::vector<uint64_t> &rec_len, const std::vector<uint32_t> &n_item = {}, const std::vector<int32_t> &item = {},
                                  uint32_t item_words = GS_HMM_DOM_WORDS, uint32_t max_item = 8)
    {
        uint64_t room = 0, n_out[2] = {0, 0};
        for (uint32_t r : best_rec) room += r < rec_len.size() ? rec_len[r] : 0;
        HitRecords h{std::vector<uint8_t>(room + 8), std::vector<uint64_t>(best_rec.size()), std::vector<uint64_t>(best_rec.size()), std::vector<uint64_t>(n_genomes + 1)};
        check(gs_hmm_hit_records(nullptr, best_rec.data(), n_genomes, n_prof, aa, rec_start.data(), rec_len.data(), rec_start.size(), n_item.empty() ? nullptr : n_item.data(),
                                 item.empty() ? nullptr : item.data(), item_words, max_item, best_rec.size(), room, h.aa.data(), h.start.data(), h.len.data(),
                                 h.genome_off.data(), n_out));
        h.start.resize(n_out[0]); h.len.resize(n_out[0]); h.aa.resize(n_out[1]);
        return h;
    }
    // the floor of profile p for a Viterbi P-value of filter_p (HMMER's F2 = 1e-3): INT32_MIN + 1 without STATS LOCAL VITERBI
    int32_t viterbi_floor(size_t profile, double filter_p = 1e-3) const
    {
        int32_t f = INT32_MIN + 1;
        if (info_[profile].flags & GS_HMM_HAS_STATS) check(gs_hmm_viterbi_floor(info_[profile].mu, info_[profile].lambda, filter_p, &f));
        return f;
    }
    static double forward_evalue(double bits, double tau, double lambda, double n_targets) { return gs_hmm_forward_evalue(bits, tau, lambda, n_targets); }
    static double bits(int32_t raw) { return gs_hmm_bits(raw); }
    double evalue(size_t profile, int32_t raw, double n_targets) const
    {
        return gs_hmm_evalue(gs_hmm_bits(raw), info_[profile].mu, info_[profile].lambda, n_targets);
    }

private:
    Context *ctx_;
    gs_hmm_db *db_ = nullptr;
    std::vector<gs_hmm_info> info_;
};

// bigsig (binaux/src/bin/bigsig.rs; SPEC 11): a bit-sliced Bloom index of genomes - one colour per genome in the order added - and, for every read, the
// colour with the most k-mer hits and whether that many hits are significant. A genome or a read is a list of records (ASCII text); the mates of a
// pair are two records of one read.
struct BigsiHits { std::vector<uint32_t> n_kmers, best_colour, best_hits; std::vector<double> tail; std::vector<uint8_t> accept; };
struct BigsiTies {
    uint32_t max_ties;
    std::vector<uint32_t> n_kmers, best_hits, n_tied, tied, sig_colour; std::vector<double> tail; std::vector<uint8_t> verdict;      // verdict: GS_BIGSI_TOO_SHORT ..
};
class Bigsi {
public:
    // minimizer_len = m > 0: a minimizer index (SPEC 11.1) of window length k
    Bigsi(Context &ctx, uint32_t k, uint32_t num_hash, uint64_t bloom_size, uint64_t colour_capacity, DataType dt = DataType::DNA, uint32_t minimizer_len = 0)
        : ctx_(&ctx)
    {
        const gs_bigsi_params p{k, num_hash, bloom_size, (uint32_t)dt, 0, 0};
        if (minimizer_len) check(gs_bigsi_create_mini(ctx.get(), &p, minimizer_len, colour_capacity, &bx_));
        else check(gs_bigsi_create(ctx.get(), &p, colour_capacity, &bx_));
    }
    uint32_t minimizer_len() const { return gs_bigsi_minimizer_len(bx_); }
    Bigsi(Context &ctx, const std::string &path, uint64_t colour_capacity = 0) : ctx_(&ctx) { check(gs_bigsi_load(ctx.get(), path.c_str(), colour_capacity, &bx_)); }
    // host only, no context (SPEC 16.2): the fixed header of a .gsbx file; everything the loading constructor checks before it asks the device for memory
    static gs_bigsi_file_description describe(const std::string &path) { gs_bigsi_file_description d; check(gs_bigsi_describe(path.c_str(), &d)); return d; }
    static gs_bigsi_file_description verify(const std::string &path) { gs_bigsi_file_description d; check(gs_bigsi_verify(path.c_str(), &d)); return d; }
    ~Bigsi() { gs_bigsi_free(bx_); }
    Bigsi(const Bigsi &) = delete;
    Bigsi &operator=(const Bigsi &) = delete;
    gs_bigsi *get() const { return bx_; }
    gs_bigsi_desc info() const { gs_bigsi_desc d; check(gs_bigsi_info(bx_, &d)); return d; }
    // min_count >= 2: the coverage filter - within each colour only values seen that often are inserted
    void add_genomes(const std::vector<std::vector<std::string>> &genomes, const std::vector<std::string> &accessions = {}, uint32_t min_count = 1)
    {
        Text t(genomes);
        check(gs_bigsi_add_batch_min_count(bx_, t.text.data(), nullptr, 0, t.begin.data(), t.end.data(), t.begin.size(), t.off.data(), genomes.size(), min_count));
        if (!accessions.empty()) {
            names_.insert(names_.end(), accessions.begin(), accessions.end());
            std::vector<const char *> p;
            for (const auto &x : names_) p.push_back(x.c_str());
            check(gs_bigsi_set_accessions(bx_, p.data(), p.size()));
        }
    }
    std::vector<uint64_t> bits_set() const
    {
        std::vector<uint64_t> t(info().n_colours);
        check(gs_bigsi_bits_set(bx_, 0, t.size(), t.data(), nullptr));
        return t;
    }
    // quals: empty, or the quality string of every record; fp_correct: the threshold itself (bigsig passes 10^-p)
    BigsiHits identify(const std::vector<std::vector<std::string>> &reads, const std::vector<std::vector<std::string>> &quals = {}, uint32_t min_phred = 15,
                       uint32_t down_sample = 1, double fp_correct = 1e-3) const
    {
        Text t(reads), q(quals);
        const uint64_t n = reads.size();
        BigsiHits out{std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<double>(n), std::vector<uint8_t>(n)};
        check(gs_bigsi_query(bx_, t.text.data(), quals.empty() ? nullptr : q.text.data(), min_phred, t.begin.data(), t.end.data(), t.begin.size(), t.off.data(), n,
                             down_sample, out.n_kmers.data(), out.best_colour.data(), out.best_hits.data(), nullptr));
        if (n == 0) return out;
        void *d[5] = {};
        const size_t bytes[5] = {4 * n, 4 * n, 4 * n, 8 * n, n};
        for (int i = 0; i < 5; i++) check(gs_dev_alloc(ctx_->get(), bytes[i], &d[i]));
        check(gs_dev_upload(ctx_->get(), d[0], out.n_kmers.data(), 4 * n));
        check(gs_dev_upload(ctx_->get(), d[1], out.best_colour.data(), 4 * n));
        check(gs_dev_upload(ctx_->get(), d[2], out.best_hits.data(), 4 * n));
        check(gs_bigsi_classify_dev(bx_, n, (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], fp_correct, (double *)d[3], (uint8_t *)d[4]));
        check(gs_dev_download(ctx_->get(), out.tail.data(), d[3], 8 * n));
        check(gs_dev_download(ctx_->get(), out.accept.data(), d[4], n));
        for (int i = 0; i < 5; i++) check(gs_dev_free(ctx_->get(), d[i]));
        return out;
    }
    // SPEC 11.2: every colour that reaches the top count (tied: n_reads x max_ties, UINT32_MAX behind a list), the tail of the most significant one, the verdict
    BigsiTies identify_ties(const std::vector<std::vector<std::string>> &reads, const std::vector<std::vector<std::string>> &quals = {}, uint32_t min_phred = 15,
                            uint32_t down_sample = 1, double fp_correct = 1e-3, uint32_t max_ties = GS_BIGSI_DEFAULT_TIES) const
    {
        Text t(reads), q(quals);
        const uint64_t n = reads.size();
        BigsiTies out{max_ties, std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n * max_ties),
                      std::vector<uint32_t>(n), std::vector<double>(n), std::vector<uint8_t>(n)};
        check(gs_bigsi_query_ties(bx_, t.text.data(), quals.empty() ? nullptr : q.text.data(), min_phred, t.begin.data(), t.end.data(), t.begin.size(), t.off.data(), n,
                                  down_sample, max_ties, out.n_kmers.data(), out.best_hits.data(), out.n_tied.data(), out.tied.data(), out.sig_colour.data()));
        if (n == 0) return out;
        void *d[6] = {};
        const size_t bytes[6] = {4 * n, 4 * n, 4 * n, 4 * n, 8 * n, n};
        const uint32_t *src[4] = {out.n_kmers.data(), out.best_hits.data(), out.n_tied.data(), out.sig_colour.data()};
        for (int i = 0; i < 6; i++) check(gs_dev_alloc(ctx_->get(), bytes[i], &d[i]));
        for (int i = 0; i < 4; i++) check(gs_dev_upload(ctx_->get(), d[i], src[i], 4 * n));
        check(gs_bigsi_verdict_dev(bx_, n, (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], (const uint32_t *)d[3], fp_correct, (double *)d[4],
                                   (uint8_t *)d[5]));
        check(gs_dev_download(ctx_->get(), out.tail.data(), d[4], 8 * n));
        check(gs_dev_download(ctx_->get(), out.verdict.data(), d[5], n));
        for (int i = 0; i < 6; i++) check(gs_dev_free(ctx_->get(), d[i]));
        return out;
    }
    // the six-field `{prefix}_reads.txt` and `{prefix}_counts.txt`, with the accessions given to add_genomes
    void write_report(const std::string &prefix, const std::vector<std::string> &read_ids, const BigsiTies &r) const
    {
        std::vector<const char *> acc, ids;
        for (const auto &x : names_) acc.push_back(x.c_str());
        for (const auto &x : read_ids) ids.push_back(x.c_str());
        check(gs_bigsig_write_report(prefix.c_str(), acc.data(), acc.size(), ids.data(), ids.size(), r.max_ties, r.n_kmers.data(), r.best_hits.data(), r.n_tied.data(),
                                     r.tied.data(), r.verdict.data()));
    }
    void save(const std::string &path) const { check(gs_bigsi_save(bx_, path.c_str())); }

private:
    struct Text {   // records end to end, their bounds, and the record offsets of the groups
        std::string text; std::vector<uint64_t> begin, end, off{0};
        explicit Text(const std::vector<std::vector<std::string>> &groups)
        {
            for (const auto &g : groups) {
                for (const auto &r : g) { begin.push_back(text.size()); text += r; end.push_back(text.size()); }
                off.push_back(begin.size());
            }
        }
    };
    Context *ctx_; gs_bigsi *bx_ = nullptr; std::vector<std::string> names_;
};

// hnsw_rs::Neighbour{d_id, distance, p_id}: gsearch reads d_id (the DataId the point was inserted under: an index into its seqdict) and distance
// (answer.rs:42,55-57); p_id = PointId(layer, rank in layer)
struct PointId { uint8_t layer; int32_t rank; };
struct Neighbour { size_t d_id; float distance; PointId p_id{0xFF, -1}; float get_distance() const { return distance; } };

// (path, fasta id, sequence length) of one database / request item: what ReqAnswer::dump reads of
// utils::idsketch::ItemDict via get_id().get_path(), get_id().get_fasta_id(), get_len() (answer.rs:48-50,56,68-69)
struct ItemDict { std::string path, fasta_id; size_t len; };
using SeqDict = std::vector<ItemDict>;

// Rust's {:.5E} on an f32 (answer.rs:60): exact decimal expansion of the value rounded half-even to 5 decimals,
// exponent without padding and without '+': 6.07500E-1, 0.00000E0
inline std::string rust_5E(float x)
{
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.5E", (double)x);
    std::string s(buf);
    const size_t e = s.find('E');
    return s.substr(0, e) + "E" + std::to_string(std::stoi(s.substr(e + 1)));
}

// answer.rs:14-76 ReqAnswer: text record of one request. Only neighbours with distance < threshold are written; the
// header line is written when any neighbour has distance <= threshold (answer.rs:42 vs :55 - the two tests differ).
class ReqAnswer {
public:
    ReqAnswer(size_t rank, ItemDict req_item, const std::vector<Neighbour> &neighbours) : rank_(rank), req_item_(std::move(req_item)), neighbours_(neighbours) {}
    size_t dump(const SeqDict &seqdict, float threshold, std::ostream &out) const
    {
        bool has_match = false;
        for (auto &n : neighbours_) has_match |= n.distance <= threshold;
        size_t nb_match = 0;
        if (!has_match) return 0;
        out << "\n" << rank_ << "\t" << req_item_.path << "\tfasta_id:\t" << req_item_.fasta_id << "\tlength:\t" << req_item_.len;
        for (auto &n : neighbours_) {
            if (!(n.distance < threshold)) continue;
            nb_match++;
            const ItemDict &d = seqdict.at(n.d_id);
            out << "\nquery_id:\t" << req_item_.path << "\tdistance:\t" << rust_5E(n.distance) << "\tanswer_fasta_path\t" << d.path << "\t"
                << d.fasta_id << " \t answer_seq_len:\t " << d.len;
        }
        return nb_match;
    }
    const ItemDict &get_request_id() const { return req_item_; }
private:
    size_t rank_;
    ItemDict req_item_;
    const std::vector<Neighbour> &neighbours_;
};

// bindash.rs:93-99 compute_distance: j = 1 - d (f32); frac = 2j/(1+j) (f32); 1.0f64 - frac.powf(1/k as f32) as f64
inline double bindash_compute_distance(float hamming_distance, size_t kmer_size)
{
    const float j = 1.0f - hamming_distance;
    const float frac = 2.0f * j / (1.0f + j);
    return 1.0 - (double)std::pow(frac, 1.0f / (float)kmer_size);
}

// hnsw_rs' own dump on the host, no context (SPEC 16.1): get_hnsw_type (reloadhnsw.rs:13-38) - the description at the head of <basename>.hnsw.graph -,
// and everything gs_index_load_hnswrs checks before it touches the device
inline gs_hnswrs_description hnswrs_describe(const std::string &basename) { gs_hnswrs_description d; check(gs_hnswrs_describe(basename.c_str(), &d)); return d; }
inline gs_hnswrs_description hnswrs_verify(const std::string &basename) { gs_hnswrs_description d; check(gs_hnswrs_verify(basename.c_str(), &d)); return d; }

// hnsw_rs::Hnsw<T, DistHamming>
template <class T>
class Hnsw {
public:
    // Hnsw::new(max_nb_connection, max_elements, max_layer, ef_construction, dist_f)  (dnasketch.rs:139)
    Hnsw(uint32_t max_nb_connection, uint64_t max_elements, uint32_t max_layer, uint32_t ef_construction, const DistHamming &dist_f, uint64_t seed = 0)
        : ctx_(&dist_f.context())
    {
        prm_ = gs_index_params{kind_of<T>(), 0, max_nb_connection, max_elements, max_layer, ef_construction, 1.0, 0, 0, seed, 0};
    }
    ~Hnsw() { gs_index_destroy(h_); }
    Hnsw(const Hnsw &) = delete;
    Hnsw &operator=(const Hnsw &) = delete;
    void modify_level_scale(double f) { frozen(); prm_.scale_modify = f; }             // dnasketch.rs:141
    void set_extend_candidates(bool b) { frozen(); prm_.extend_candidates = b; }       // dnasketch.rs:159
    void set_keeping_pruned(bool b) { frozen(); prm_.keep_pruned = b; }                // dnasketch.rs:160
    size_t get_nb_point() const { return h_ ? gs_index_nb_point(h_) : 0; }
    // parallel_insert(&[(&Vec<T>, usize)]) (dnasketch.rs:429-435): any DataIds; searches return them as d_id
    void parallel_insert(const std::vector<std::pair<const std::vector<T> *, size_t>> &datas)
    {
        if (datas.empty()) return;
        const size_t m = datas[0].first->size();
        ensure(m);
        std::vector<T> flat(datas.size() * m);
        std::vector<uint64_t> ids(datas.size());
        for (size_t i = 0; i < datas.size(); i++) {
            if (datas[i].first->size() != m) throw Error(GS_ERR_INVALID, "signature length mismatch");
            ids[i] = datas[i].second;
            std::copy(datas[i].first->begin(), datas[i].first->end(), flat.begin() + i * m);
        }
        check(gs_index_parallel_insert_ids(h_, flat.data(), ids.data(), datas.size()));
    }
    // parallel_search(&[Vec<T>], knbn, ef) -> Vec<Vec<Neighbour>>, ascending distance (dnarequest.rs:353)
    std::vector<std::vector<Neighbour>> parallel_search(const std::vector<std::vector<T>> &datas, size_t knbn, size_t ef) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "search on an empty index");
        const size_t nq = datas.size(), m = prm_.m;
        std::vector<T> flat(nq * m);
        for (size_t i = 0; i < nq; i++) { if (datas[i].size() != m) throw Error(GS_ERR_INVALID, "signature length mismatch"); std::copy(datas[i].begin(), datas[i].end(), flat.begin() + i * m); }
        std::vector<uint64_t> ids(nq * knbn); std::vector<float> dist(nq * knbn); std::vector<uint32_t> cnt(nq);
        std::vector<uint8_t> pl(nq * knbn); std::vector<int32_t> pr(nq * knbn);
        check(gs_index_parallel_search_pid(h_, flat.data(), nq, (uint32_t)knbn, (uint32_t)ef, ids.data(), dist.data(), cnt.data(), nullptr, pl.data(), pr.data()));
        std::vector<std::vector<Neighbour>> out(nq);
        for (size_t i = 0; i < nq; i++)
            for (uint32_t j = 0; j < cnt[i]; j++) out[i].push_back(Neighbour{(size_t)ids[i * knbn + j], dist[i * knbn + j], PointId{pl[i * knbn + j], pr[i * knbn + j]}});
        return out;
    }
    // exact knbn nearest nodes by exhaustive DistHamming, distances <= max_dist (gs_index_exact_search); p_id is not filled
    std::vector<std::vector<Neighbour>> exact_search(const std::vector<std::vector<T>> &datas, size_t knbn, float max_dist = 1.0f) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "search on an empty index");
        const size_t nq = datas.size(), m = prm_.m;
        std::vector<T> flat(nq * m);
        for (size_t i = 0; i < nq; i++) { if (datas[i].size() != m) throw Error(GS_ERR_INVALID, "signature length mismatch"); std::copy(datas[i].begin(), datas[i].end(), flat.begin() + i * m); }
        std::vector<uint64_t> ids(nq * knbn); std::vector<float> dist(nq * knbn); std::vector<uint32_t> cnt(nq);
        check(gs_index_exact_search(h_, flat.data(), nq, (uint32_t)knbn, max_dist, ids.data(), dist.data(), cnt.data()));
        return lists(ids, dist, cnt, knbn);
    }
    // this index as one piece of a split database (gs_index_search_merge, SPEC 17 items 12-18): the answers of the listed queries (rows: ascending
    // positions in datas, nullptr = all), id_offset added, merged in place into their running lists under (distance, id). run_ids / run_dist:
    // datas.size() x knbn, run_count / run_evals: datas.size(); new_running_lists() makes the empty ones
    struct RunningLists { std::vector<uint64_t> ids; std::vector<float> dist; std::vector<uint32_t> count; std::vector<uint64_t> evals; };
    static RunningLists new_running_lists(size_t nq, size_t knbn)
    {
        return RunningLists{std::vector<uint64_t>(nq * knbn, UINT64_MAX), std::vector<float>(nq * knbn, INFINITY), std::vector<uint32_t>(nq, 0), std::vector<uint64_t>(nq, 0)};
    }
    void search_merge(const std::vector<std::vector<T>> &datas, size_t knbn, size_t ef, RunningLists &run, uint64_t id_offset = 0, const std::vector<uint32_t> *rows = nullptr) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "search on an empty index");
        const size_t nq = datas.size(), m = prm_.m;
        if (run.ids.size() != nq * knbn || run.dist.size() != nq * knbn || run.count.size() != nq || run.evals.size() != nq) throw Error(GS_ERR_INVALID, "running lists of another shape");
        if (rows && rows->empty()) return;
        std::vector<T> flat(nq * m);
        for (size_t i = 0; i < nq; i++) { if (datas[i].size() != m) throw Error(GS_ERR_INVALID, "signature length mismatch"); std::copy(datas[i].begin(), datas[i].end(), flat.begin() + i * m); }
        check(gs_index_search_merge(h_, flat.data(), nq, rows ? rows->data() : nullptr, rows ? rows->size() : 0, (uint32_t)knbn, (uint32_t)ef, id_offset, run.ids.data(),
                                    run.dist.data(), run.count.data(), run.evals.data()));
    }
    // hnsw2knn: the knbn nearest OTHER nodes of nodes [first, first + n) in insertion order, exact (gs_index_knn_graph)
    std::vector<std::vector<Neighbour>> knn_graph(size_t knbn, float max_dist = 1.0f, size_t first = 0, size_t n = SIZE_MAX) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "k-NN graph of an empty index");
        if (n == SIZE_MAX) n = get_nb_point() - std::min(first, get_nb_point());
        std::vector<uint64_t> ids(n * knbn); std::vector<float> dist(n * knbn); std::vector<uint32_t> cnt(n);
        check(gs_index_knn_graph(h_, (uint32_t)knbn, max_dist, first, n, ids.data(), dist.data(), cnt.data()));
        return lists(ids, dist, cnt, knbn);
    }
    // ann --embed (embed.rs:34-64): the exact self graph embedded (SPEC 8); nb_point x prm.dim positions, row-major, in node order
    std::vector<float> embed(size_t knbn = 8, const gs_embed_params *prm = nullptr, const std::vector<float> *init = nullptr, float max_dist = 1.0f) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "embedding of an empty index");
        const gs_embed_params p = prm ? *prm : gs_embed_params_default();
        std::vector<float> out(get_nb_point() * p.dim);
        if (init && init->size() != out.size()) throw Error(GS_ERR_INVALID, "initial positions must be nb_point x dim");
        check(gs_index_embed(h_, (uint32_t)knbn, max_dist, &p, init ? init->data() : nullptr, out.data()));
        return out;
    }
    // ann --stats (embed.rs:26-33): statistics of the exact self graph; occ / hist (optional) receive the k-occurrences and their histogram
    gs_knn_stats knn_graph_stats(size_t knbn = 8, float max_dist = 1.0f, std::vector<uint32_t> *occ = nullptr, std::vector<uint64_t> *hist = nullptr) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "statistics of an empty index");
        gs_knn_stats st;
        if (occ) occ->resize(get_nb_point());
        if (hist) hist->resize(65);
        check(gs_index_knn_graph_stats(h_, (uint32_t)knbn, max_dist, &st, occ ? occ->data() : nullptr, hist ? hist->data() : nullptr));
        return st;
    }
    // ann --embed's quality indicator (embed.rs:68-70; SPEC 8.1): how much of the exact self graph lies among the kq nearest points of each node at
    // the positions `pos` (nb_point x dim, node order, as embed() returns them); hist (optional): rows by their number of conserved edges
    gs_embed_quality_summary embed_quality(const std::vector<float> &pos, size_t dim = 2, size_t knbn = 8, size_t kq = 200, float max_dist = 1.0f,
                                           std::vector<uint64_t> *hist = nullptr) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "embedding quality of an empty index");
        if (pos.size() != get_nb_point() * dim) throw Error(GS_ERR_INVALID, "positions must be nb_point x dim");
        gs_embed_quality_summary s;
        if (hist) hist->resize(knbn + 1);
        check(gs_index_embed_quality(h_, (uint32_t)knbn, max_dist, pos.data(), (uint32_t)dim, (uint32_t)kq, &s, hist ? hist->data() : nullptr, nullptr, nullptr,
                                     nullptr));
        return s;
    }
    // hnswcore (SPEC 10): per node, in node order, the NODE NUMBER of its centre and the mismatch count to it; the medoids ascending (empty for
    // n_cluster = 0, where the coreset points are the centres) and how many nodes each received
    struct Clusters { std::vector<uint64_t> centre_node; std::vector<uint16_t> centre_count; std::vector<uint64_t> medoids, sizes; gs_cluster_info info; };
    Clusters cluster(const gs_cluster_params *prm = nullptr) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "clustering of an empty index");
        const gs_cluster_params p = prm ? *prm : gs_cluster_params_default();
        Clusters r;
        r.centre_node.resize(get_nb_point()); r.centre_count.resize(get_nb_point()); r.medoids.resize(p.n_cluster); r.sizes.resize(p.n_cluster);
        check(gs_index_cluster(h_, &p, r.centre_node.data(), r.centre_count.data(), r.medoids.data(), r.sizes.data(), nullptr, nullptr, 0, &r.info));
        return r;
    }
    // for every node the position in `nodes` (node numbers) that minimises (mismatch count, position), and that count (gs_index_nearest_of)
    std::pair<std::vector<uint32_t>, std::vector<uint16_t>> nearest_of(const std::vector<uint64_t> &nodes) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "nearest_of on an empty index");
        std::vector<uint32_t> arg(get_nb_point()); std::vector<uint16_t> cnt(get_nb_point());
        check(gs_index_nearest_of(h_, nodes.data(), nodes.size(), arg.data(), cnt.data()));
        return {std::move(arg), std::move(cnt)};
    }
    // derep (SPEC 18): clusters at a distance cut. components: per node the smallest NODE NUMBER of its connected component of the link graph
    struct Components { std::vector<uint64_t> label; gs_derep_info info; };
    Components components(float max_dist) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "components of an empty index");
        Components r;
        r.label.resize(get_nb_point());
        check(gs_index_components(h_, max_dist, r.label.data(), &r.info));
        return r;
    }
    // greedy representatives: per node the NODE NUMBER of its representative (itself for one) and the mismatch count to it; priority: empty = all
    // equal, otherwise one value per node, higher first
    struct Derep { std::vector<uint64_t> rep_node; std::vector<uint16_t> rep_count; gs_derep_info info; };
    Derep derep(float max_dist, const std::vector<uint64_t> &priority = {}) const
    {
        if (!h_) throw Error(GS_ERR_STATE, "derep of an empty index");
        if (!priority.empty() && priority.size() != get_nb_point()) throw Error(GS_ERR_INVALID, "one priority per node");
        Derep r;
        r.rep_node.resize(get_nb_point()); r.rep_count.resize(get_nb_point());
        check(gs_index_derep(h_, max_dist, priority.empty() ? nullptr : priority.data(), r.rep_node.data(), r.rep_count.data(), &r.info));
        return r;
    }
    void file_dump(const std::string &path) const { check(gs_index_save(h_, path.c_str())); }      // dumpload.rs:31 (own format)
    void debug_fill_scratch(int byte) { if (h_) check(gs_index_debug_fill_scratch(h_, byte)); }    // debugging (not for production use): gsearch_amd.h
private:
    void frozen() const { if (h_) throw Error(GS_ERR_STATE, "index parameters are frozen once the index holds points"); }
    void ensure(size_t m) { if (!h_) { prm_.m = (uint32_t)m; check(gs_index_create(ctx_->get(), &prm_, &h_)); } }
    static std::vector<std::vector<Neighbour>> lists(const std::vector<uint64_t> &ids, const std::vector<float> &dist, const std::vector<uint32_t> &cnt, size_t knbn)
    {
        std::vector<std::vector<Neighbour>> out(cnt.size());
        for (size_t i = 0; i < cnt.size(); i++)
            for (uint32_t j = 0; j < cnt[i]; j++) out[i].push_back(Neighbour{(size_t)ids[i * knbn + j], dist[i * knbn + j]});
        return out;
    }
    Context *ctx_;
    gs_index_params prm_;
    gs_index *h_ = nullptr;
};

}  // namespace gsearch
