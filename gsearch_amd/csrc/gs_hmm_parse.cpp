// gs_hmm_parse.cpp — the reader of HMMER3 profile text (SPEC 13 "Units", "Files") and the hmmsearch calls that touch no device. Plain C++, no HIP:
// built by g++ alone, so that a host program can link it without the GPU runtime (tests/host/loader_sweep.cpp does).
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <utility>
#include "gs_hmm_parse.hpp"

namespace gs {

static bool digits(const std::string &s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos; }
// one number of a file -> units (SPEC 13 "Units")
static bool hmm_file_units(const std::string &t, int32_t *out)
{
    if (t == "*") { *out = GS_HMM_STAR; return true; }
    const size_t dot = t.find('.');
    const std::string ip = t.substr(0, dot), fr = dot == std::string::npos ? "" : t.substr(dot + 1);
    if (!digits(ip) || ip.size() > 4 || (dot != std::string::npos && !digits(fr))) { set_error("hmm: not a number: '%s'", t.c_str()); return false; }
    if (fr.size() > 5) { set_error("hmm: more than 5 decimals: '%s'", t.c_str()); return false; }
    uint64_t d = strtoull(ip.c_str(), nullptr, 10) * 100000ull, f = 0;
    for (size_t i = 0; i < 5; i++) f = f * 10 + (i < fr.size() ? (uint64_t)(fr[i] - '0') : 0);
    d += f;
    if (d > GS_HMM_MAX_FILE_VALUE) { set_error("hmm: a value of 100 nats or more: '%s'", t.c_str()); return false; }
    *out = -(int32_t)((d * GS_HMM_UNIT_C + (1ull << (GS_HMM_UNIT_S - 1))) >> GS_HMM_UNIT_S);
    return true;
}
// a cutoff in bits as the file writes it -> units, rounded half up
static bool hmm_bits_units(const std::string &tok, int32_t *out)
{
    const bool neg = !tok.empty() && tok[0] == '-';
    const size_t b = tok.find_first_not_of("+-");
    const std::string t = b == std::string::npos ? "" : tok.substr(b);
    const size_t dot = t.find('.');
    const std::string ip = t.substr(0, dot), fr = dot == std::string::npos ? "" : t.substr(dot + 1);
    if (!digits(ip) || ip.size() > 6 || (!fr.empty() && !digits(fr)) || fr.size() > 5) { set_error("hmm: not a cutoff: '%s'", tok.c_str()); return false; }
    int64_t den = 1;
    for (size_t i = 0; i < fr.size(); i++) den *= 10;
    int64_t d = strtoll(ip.c_str(), nullptr, 10) * den + (fr.empty() ? 0 : strtoll(fr.c_str(), nullptr, 10));
    if (neg) d = -d;
    const int64_t num = 2 * d * 1024 + den, q = num / (2 * den);
    *out = (int32_t)(num % (2 * den) < 0 ? q - 1 : q);              // floor
    return true;
}

// a number of a header line (GA / TC / NC, STATS LOCAL): sign, digits, then optionally a point and digits; anything else is malformed
static bool hmm_header_number(const std::string &tok, double *out)
{
    const std::string t = tok.substr(!tok.empty() && (tok[0] == '+' || tok[0] == '-') ? 1 : 0);
    const size_t dot = t.find('.');
    const std::string ip = t.substr(0, dot), fr = dot == std::string::npos ? "" : t.substr(dot + 1);
    if (!digits(ip) || (!fr.empty() && !digits(fr))) { set_error("hmm: not a number: '%s'", tok.c_str()); return false; }
    *out = strtod(tok.c_str(), nullptr);
    return true;
}

struct HmmLines {      // the non-blank lines of a text, split at white space
    const char *p, *end;
    bool next(std::vector<std::string> &tok, std::string *raw = nullptr)
    {
        while (p < end) {
            const char *e = (const char *)memchr(p, '\n', (size_t)(end - p));
            if (!e) e = end;
            const char *a = p;
            p = e < end ? e + 1 : end;
            tok.clear();
            for (const char *c = a; c < e;) {
                while (c < e && (*c == ' ' || *c == '\t' || *c == '\r')) c++;
                const char *s = c;
                while (c < e && !(*c == ' ' || *c == '\t' || *c == '\r')) c++;
                if (c > s) tok.emplace_back(s, c);
            }
            if (!tok.empty()) { if (raw) raw->assign(a, e); return true; }
        }
        return false;
    }
    bool more() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) p++; return p < end; }
};

int hmm_parse_all(const char *text, size_t n, std::vector<HmmModel> &out)
{
    HmmLines in{text, text + n};
    std::vector<std::string> f;
    std::string raw;
    static const int32_t bg[20] = GS_HMM_BG_LIST;
    const size_t first = out.size();
#define HMM_LINE(what) GS_REQUIRE(in.next(f, &raw), GS_ERR_INVALID, "hmm: the text ends inside a model (%s)", what)
    while (in.more()) {
        HMM_LINE("header");
        GS_REQUIRE(raw.compare(0, 7, "HMMER3/") == 0, GS_ERR_INVALID, "hmm: not a HMMER3 profile: '%.40s'", raw.c_str());
        HmmModel m;
        memset(&m.info, 0, sizeof m.info);
        bool has_name = false, has_alph = false;
        std::string alph;
        for (;;) {
            HMM_LINE("header");
            if (f[0] == "HMM") break;
            if (f[0] == "STATS" && f.size() > 4 && f[1] == "LOCAL") {
                const int w = f[2] == "MSV" ? 0 : (f[2] == "VITERBI" ? 1 : (f[2] == "FORWARD" ? 2 : -1));
                if (w >= 0) {
                    if (!hmm_header_number(f[3], &m.stats[2 * w]) || !hmm_header_number(f[4], &m.stats[2 * w + 1])) return GS_ERR_INVALID;
                    m.has_stats |= 1u << w;
                    if (w == 1) { m.info.mu = m.stats[2]; m.info.lambda = m.stats[3]; m.info.flags |= GS_HMM_HAS_STATS; }
                }
            }
            if (f[0] == "NAME" && f.size() > 1) { snprintf(m.info.name, sizeof m.info.name, "%s", f[1].c_str()); has_name = true; }
            else if (f[0] == "ACC" && f.size() > 1) snprintf(m.info.acc, sizeof m.info.acc, "%s", f[1].c_str());
            else if (f[0] == "LENG" && f.size() > 1) {
                GS_REQUIRE(f[1].size() <= 9 && f[1].find_first_not_of("0123456789") == std::string::npos, GS_ERR_INVALID, "hmm: LENG '%s'", f[1].c_str());
                m.info.M = (uint32_t)strtoul(f[1].c_str(), nullptr, 10);
            } else if (f[0] == "ALPH" && f.size() > 1) {
                alph = f[1]; has_alph = true;
                for (char &ch : alph) if (ch >= 'A' && ch <= 'Z') ch = (char)(ch + 32);
            } else if ((f[0] == "GA" || f[0] == "TC" || f[0] == "NC") && f.size() > 2) {
                std::string a = f[1], b = f[2];
                while (!a.empty() && a.back() == ';') a.pop_back();
                while (!b.empty() && b.back() == ';') b.pop_back();
                double *dst = f[0] == "GA" ? m.info.ga : (f[0] == "TC" ? m.info.tc : m.info.nc);
                if (!hmm_header_number(a, &dst[0]) || !hmm_header_number(b, &dst[1])) return GS_ERR_INVALID;
                m.info.flags |= f[0] == "GA" ? GS_HMM_HAS_GA : (f[0] == "TC" ? GS_HMM_HAS_TC : GS_HMM_HAS_NC);
                if (f[0] == "GA" && !hmm_bits_units(a, &m.info.ga_units)) return GS_ERR_INVALID;
            }
        }
        GS_REQUIRE(has_name && has_alph && m.info.M >= 1, GS_ERR_INVALID, "hmm: NAME, LENG or ALPH missing");
        GS_REQUIRE(alph == "amino", GS_ERR_INVALID, "hmm: %s: ALPH %s (only amino)", m.info.name, alph.c_str());
        GS_REQUIRE(m.info.M <= GS_HMM_MAX_M, GS_ERR_UNSUPPORTED, "hmm: %s has %u nodes, more than %u", m.info.name, m.info.M, GS_HMM_MAX_M);
        const uint32_t M = m.info.M, W = M + 1;
        m.info.tbm = hmm_tbm(M);
        m.tab.assign((size_t)GS_HMM_TABLE_ROWS * W, 0);
        HMM_LINE("transition names");
        HMM_LINE("node 0");
        if (f[0] == "COMPO") HMM_LINE("node 0");
        int32_t u;
        auto emissions = [&](size_t skip, int32_t *col, uint32_t k) {          // 20 numbers from f[skip]; col: where the match scores of node k go
            for (int a = 0; a < 20; a++) {
                if (!hmm_file_units(f[skip + a], &u)) return false;
                if (col) col[(size_t)a * W + k] = u - bg[a];
            }
            return true;
        };
        for (uint32_t k = 0; k <= M; k++) {
            if (k > 0) {
                HMM_LINE("match emissions");
                GS_REQUIRE(f.size() >= 21 && f[0] == std::to_string(k), GS_ERR_INVALID, "hmm: %s: node %u expected, found '%.20s'", m.info.name, k, f[0].c_str());
                if (!emissions(1, m.tab.data(), k)) return GS_ERR_INVALID;
                HMM_LINE("insert emissions");
            }
            GS_REQUIRE(f.size() == 20, GS_ERR_INVALID, "hmm: %s: insert emissions of node %u: %zu fields", m.info.name, k, f.size());
            if (!emissions(0, nullptr, k)) return GS_ERR_INVALID;             // validated; insert emissions score 0 (SPEC 13)
            HMM_LINE("transitions");
            GS_REQUIRE(f.size() == 7, GS_ERR_INVALID, "hmm: %s: transitions of node %u: %zu fields", m.info.name, k, f.size());
            for (int t = 0; t < 7; t++) {
                if (!hmm_file_units(f[t], &u)) return GS_ERR_INVALID;
                m.tab[(size_t)(20 + t) * W + k] = u;
            }
        }
        HMM_LINE("//");
        GS_REQUIRE(f.size() == 1 && f[0] == "//", GS_ERR_INVALID, "hmm: %s: no // after node %u", m.info.name, M);
        out.push_back(std::move(m));
    }
#undef HMM_LINE
    GS_REQUIRE(out.size() > first, GS_ERR_INVALID, "hmm: no model in the text");
    return GS_OK;
}

uint16_t hmm_lse_entry(uint32_t j) { return (uint16_t)floor(1024.0 * log2(1.0 + exp2(-2.0 * (double)j / 1024.0)) + 0.5); }
uint32_t hmm_exp2_entry(uint32_t f) { return (uint32_t)floor(65536.0 * exp2(-(double)f / 1024.0) + 0.5); }

}  // namespace gs

extern "C" {

int gs_hmm_exp2_table(uint32_t *out, uint64_t cap)
{
    GS_REQUIRE(out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(cap >= GS_HMM_EXP2_N, GS_ERR_INVALID, "hmm: the table has %u entries, cap = %llu", GS_HMM_EXP2_N, (unsigned long long)cap);
    for (uint32_t f = 0; f < GS_HMM_EXP2_N; f++) out[f] = gs::hmm_exp2_entry(f);
    return GS_OK;
}

int gs_hmm_parse_mem(const void *text, uint64_t n_bytes, uint32_t model, gs_hmm_info *info_out, int32_t *tables_out, uint64_t cap_words, uint32_t *n_models_out)
{
    using namespace gs;
    GS_REQUIRE(text || n_bytes == 0, GS_ERR_INVALID, "null argument");
    std::vector<HmmModel> ms;
    int rc = hmm_parse_all((const char *)text, (size_t)n_bytes, ms);
    if (rc) return rc;
    if (n_models_out) *n_models_out = (uint32_t)ms.size();
    GS_REQUIRE(model < ms.size(), GS_ERR_INVALID, "hmm: model %u of %zu", model, ms.size());
    if (info_out) *info_out = ms[model].info;
    if (tables_out) {
        GS_REQUIRE(cap_words >= ms[model].tab.size(), GS_ERR_INVALID, "hmm: the table needs %zu words, cap_words = %llu", ms[model].tab.size(), (unsigned long long)cap_words);
        memcpy(tables_out, ms[model].tab.data(), 4 * ms[model].tab.size());
    }
    return GS_OK;
}

int gs_hmm_parse_stats_mem(const void *text, uint64_t n_bytes, uint32_t model, double out[6], uint32_t *has_out)
{
    using namespace gs;
    GS_REQUIRE((text || n_bytes == 0) && out && has_out, GS_ERR_INVALID, "null argument");
    std::vector<HmmModel> ms;
    int rc = hmm_parse_all((const char *)text, (size_t)n_bytes, ms);
    if (rc) return rc;
    GS_REQUIRE(model < ms.size(), GS_ERR_INVALID, "hmm: model %u of %zu", model, ms.size());
    for (int i = 0; i < 6; i++) out[i] = ms[model].stats[i];
    *has_out = ms[model].has_stats;
    return GS_OK;
}

int gs_hmm_specials(uint64_t L, uint32_t M, int32_t out[6])
{
    using namespace gs;
    GS_REQUIRE(out && L >= 1 && M >= 1, GS_ERR_INVALID, "bad argument");
    GS_REQUIRE(L <= GS_HMM_MAX_L && M <= GS_HMM_MAX_M, GS_ERR_UNSUPPORTED, "hmm: L = %llu, M = %u: larger than the limits", (unsigned long long)L, M);
    const HmmSpecials s = hmm_specials((uint32_t)L);
    out[0] = s.tloop; out[1] = s.tmove; out[2] = s.null; out[3] = hmm_tbm(M); out[4] = s.nloop; out[5] = s.nmove;
    return GS_OK;
}

int gs_hmm_logsum_table(uint16_t *out, uint64_t cap)
{
    GS_REQUIRE(out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(cap >= GS_HMM_LSE_N, GS_ERR_INVALID, "hmm: the table has %u entries, cap = %llu", GS_HMM_LSE_N, (unsigned long long)cap);
    for (uint32_t j = 0; j < GS_HMM_LSE_N; j++) out[j] = gs::hmm_lse_entry(j);
    return GS_OK;
}

int gs_hmm_viterbi_floor(double mu, double lambda, double p, int32_t *floor_out)
{
    GS_REQUIRE(floor_out, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(lambda > 0 && p > 0 && p < 1 && mu == mu, GS_ERR_INVALID, "hmm: the floor needs lambda > 0 and 0 < P < 1 (lambda = %g, P = %g)", lambda, p);
    const double units = ::floor((mu - ::log(-::log1p(-p)) / lambda) * 1024.0 + 0.5);
    *floor_out = units <= (double)(INT32_MIN + 1) ? INT32_MIN + 1 : (units >= (double)INT32_MAX ? INT32_MAX : (int32_t)units);
    return GS_OK;
}

double gs_hmm_bits(int32_t raw) { return (double)raw / 1024.0; }
double gs_hmm_evalue(double bits, double mu, double lambda, double Z) { return Z * -::expm1(-::exp(-lambda * (bits - mu))); }
double gs_hmm_forward_evalue(double bits, double tau, double lambda, double Z) { return Z * (bits < tau ? 1.0 : ::exp(-lambda * (bits - tau))); }

}  // extern "C"
