// gs_hmm_parse.hpp — the host half of hmmsearch (SPEC 13): the units of a profile file, the length model, and the reader of HMMER3 text. Plain C++, no
// HIP: gs_hmm_db_load{,_mem} (gs_hmm.hip) parse with it, then build the device tables; gs_hmm_parse_mem and the other calls that touch no device
// (gs_hmm_parse.cpp) are the same code without a context. gs_spec.hpp includes this file for the arithmetic, so device code reads the same lines.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/gsearch_amd.h"
#include "gs_host.hpp"

#if defined(__HIPCC__)
#define GS_HMM_HD __host__ __device__ __forceinline__
#else
#define GS_HMM_HD inline
#endif

// ---- SPEC 13: hmmsearch - Viterbi score of a protein against a HMMER3 profile, all in int32 units of 2^-10 bit. [CHOICE] throughout (hmmsearch_rs is
// not in the reference; the profiles under data/HMM_* are, and pin the model through their own cutoffs and STATS lines).
#define GS_HMM_UNIT_C 1015206383ULL      // 2^36 * 1024 / (10^5 ln 2): a file value of d * 10^-5 nats is -((d * C + 2^35) >> 36) units
#define GS_HMM_UNIT_S 36
#define GS_HMM_MAX_FILE_VALUE 9999999u   // d: a file value is below 100 nats, so a score from a file is above -2^18
#define GS_HMM_STAR (-(1 << 18))         // `*` of a file (probability 0): below every score a file value can give
#define GS_HMM_NEG (-(1 << 29))          // floor of every cell
#define GS_HMM_TEJ (-1024)               // E -> J and E -> C, one bit each (multihit)
#define GS_HMM_AA_MASK 0x016FBDFDu       // the letters A..Z that are residues; a residue's index is its rank among them (ACDEFGHIKLMNPQRSTVWY)
#define GS_HMM_BG_LIST {-3754, -6189, -4325, -3997, -4766, -3939, -5578, -4181, -4170, -3456, -5524, -4703, -4477, -4772, -4309, -3964, -4310, -3986, -6608, -5160}

namespace gs {

// log2(n) in units of 2^-20 for 1 <= n < 2^32: the exponent, then 20 fraction bits by squaring a 32-bit mantissa on 64-bit words (each squaring
// doubles the logarithm, the bit that carries out is the next fraction bit; the dropped low bits cost less than 2^-20 in all)
GS_HMM_HD int32_t hmm_lgq(uint32_t n)
{
    int e = 31;
    while (!((n >> e) & 1u)) e--;
    uint64_t x = (uint64_t)n << (31 - e);
    int32_t r = e << 20;
    for (int j = 19; j >= 0; j--) {
        x = (x * x) >> 31;
        if (x >> 32) { x >>= 1; r |= 1 << j; }
    }
    return r;
}
// units(ln(num / den)), to the nearest unit
GS_HMM_HD int32_t hmm_units_log(uint32_t num, uint32_t den) { return (hmm_lgq(num) - hmm_lgq(den) + 512) >> 10; }
struct HmmSpecials { int32_t tloop, tmove, null, nloop, nmove; };
// the length model of a target of L residues, 1 <= L <= GS_HMM_MAX_L
GS_HMM_HD HmmSpecials hmm_specials(uint32_t L)
{
    HmmSpecials s;
    s.tloop = hmm_units_log(L, L + 3); s.tmove = hmm_units_log(3, L + 3);
    s.nloop = hmm_units_log(L, L + 1); s.nmove = hmm_units_log(1, L + 1);
    s.null = (int32_t)L * s.nloop + s.nmove;
    return s;
}
GS_HMM_HD int32_t hmm_tbm(uint32_t M) { return hmm_units_log(2, M * (M + 1)); }

// ---- profile files ----------------------------------------------------------------------------------------------------------------------------
struct HmmModel {
    gs_hmm_info info; std::vector<int32_t> tab;                         // tab: [27][M + 1] as gs_hmm_parse_mem documents it
    double stats[6] = {}; uint32_t has_stats = 0;                       // as gs_hmm_parse_stats_mem documents them
};
// the models of a text, appended to `out`
int hmm_parse_all(const char *text, size_t n, std::vector<HmmModel> &out);
// T of SPEC 13.1 on the host: no entry lies closer than 3.5e-6 to a rounding boundary, so the f64 log2 of any libm gives the same integers
uint16_t hmm_lse_entry(uint32_t j);
// EXP2 of SPEC 13.6 on the host: no entry's unrounded value lies within 1e-6 of a half-integer (the CPU test shows it), so any libm gives the same integers
uint32_t hmm_exp2_entry(uint32_t f);

}  // namespace gs
