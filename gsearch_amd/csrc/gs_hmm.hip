// gs_hmm.hip — hmmsearch (SPEC 13): HMMER3 profiles as integer tables, the local multihit Viterbi score of every (record, profile) pair on the
// device, the Forward score (SPEC 13.1) of the pairs that pass a per-profile Viterbi floor, the best record per genome and profile, the domains of
// the Viterbi path of a list of pairs, traced back on the device (SPEC 13.2), the Backward pass and posterior envelopes of a list of pairs
// (SPEC 13.4), the null2 bias correction of those envelopes (SPEC 13.5), their optimal-accuracy alignments (SPEC 13.6) and the packed int16 Viterbi
// filter in front of the int32 program (SPEC 13.7). Integers only from the file's digits to the raw score. The reader of profile files and the calls that touch no device are
// gs_hmm_parse.cpp, a host-only unit; the doubles of hmmsearch (bits, E-values, the table of lse, the Viterbi floor, the reported cutoffs) are all there.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <numeric>
#include <utility>
#include "gs_internal.hpp"
#include "gs_spec.hpp"           // (brings gs_hmm_parse.hpp)

namespace gs {

// ---- device side --------------------------------------------------------------------------------------------------------------------------------
// A profile in device memory: 28 rows of MP = 64 Q words, word j of a row belongs to node j + 1. Rows 0..26 as in the host table, row 27 = PDD,
// the sum of tDD over the nodes in front of j inside its lane's group of Q. Nodes past M hold GS_HMM_STAR everywhere: they take no part in E and
// nothing flows from a node to a lower one.
enum { HMM_ROWS_DEV = 28, HMM_ROW_MM = 20, HMM_ROW_MI = 21, HMM_ROW_MD = 22, HMM_ROW_IM = 23, HMM_ROW_II = 24, HMM_ROW_DM = 25, HMM_ROW_DD = 26, HMM_ROW_PDD = 27 };
enum { HMM_BLOCK = 512, HMM_WAVES = HMM_BLOCK / 64, HMM_MAX_WG_PER_PROFILE = 64 };
struct HmmDesc { uint64_t off; uint32_t M; int32_t tbm; };             // off: first word of the profile's table
static constexpr int HMM_CLASS_Q[] = {1, 2, 3, 4, 6, 8, 12, 16, 20};       // nodes per lane a kernel is compiled for; a profile runs in the smallest that holds it
enum { HMM_CLASSES = sizeof HMM_CLASS_Q / sizeof HMM_CLASS_Q[0] };
// The class a profile of M nodes runs in, and its HMM_CLASS_Q for device code too (k_hmm_walk): a loop of its own, so that device code compares with
// constants where HMM_CLASS_Q[hmm_class_of(M)] would look the array up in memory.
constexpr int hmm_class_of(uint32_t M)
{
    for (int c = 0; c < HMM_CLASSES - 1; c++) if ((M + 63) / 64 <= (uint32_t)HMM_CLASS_Q[c]) return c;
    return HMM_CLASSES - 1;
}
__host__ __device__ constexpr int hmm_q_of(uint32_t M)
{
    for (int c = 0; c < HMM_CLASSES - 1; c++) if ((M + 63) / 64 <= (uint32_t)HMM_CLASS_Q[c]) return HMM_CLASS_Q[c];
    return HMM_CLASS_Q[HMM_CLASSES - 1];
}
constexpr bool hmm_classes_hold()
{
    for (int c = 0; c < HMM_CLASSES; c++) {
        const uint32_t top = 64u * (uint32_t)HMM_CLASS_Q[c];
        if (hmm_q_of(top) != HMM_CLASS_Q[c] || hmm_class_of(top) != c) return false;
        if (c + 1 < HMM_CLASSES && (hmm_q_of(top + 1) != HMM_CLASS_Q[c + 1] || hmm_class_of(top + 1) != c + 1)) return false;
    }
    return true;
}
static_assert(hmm_classes_hold(), "a profile of 64 Q nodes runs in class Q, one of 64 Q + 1 in the next class");
static_assert(HMM_CLASS_Q[HMM_CLASSES - 1] * 64 == GS_HMM_MAX_M, "the largest class holds GS_HMM_MAX_M nodes");
static_assert((size_t)HMM_ROWS_DEV * GS_HMM_MAX_M * 4 <= 160 * 1024, "the largest table fits the LDS of a CU");

// in LDS T[0 .. 5902] is followed by the 0 that every larger difference reads, so the look-up needs no branch
enum { HMM_LSE_LDS_N = GS_HMM_LSE_N + 1, HMM_LSE_LDS_BYTES = 2 * HMM_LSE_LDS_N };
static_assert((size_t)HMM_ROWS_DEV * GS_HMM_MAX_M * 4 + HMM_LSE_LDS_BYTES <= 160 * 1024, "the largest table and T behind it fit the LDS of a CU");
static_assert(((size_t)HMM_ROWS_DEV * 64 * 4) % 4 == 0, "T starts on a word");

// lse(a, b) of SPEC 13.1. The difference is taken on unsigned words: hi - lo can pass 2^31 (a cell near the top of the range beside one near NEG)
__device__ __forceinline__ int32_t hmm_lse(int32_t a, int32_t b, const uint16_t *__restrict__ T)
{
    const int32_t hi = max(a, b), lo = min(a, b);
    const uint32_t j = min(((uint32_t)hi - (uint32_t)lo + 1u) >> 1, (uint32_t)GS_HMM_LSE_N);
    return hi + (int32_t)T[j];
}

// The dynamic programs over the cells of a (record, profile) pair (Backward has a row loop of its own, further down). They share one prologue (hmm_stage) and one row loop (hmm_rows) and differ at
// compile time only, at the points the row loop names.
enum HmmProg { HMM_VIT, HMM_FWD, HMM_TRACE, HMM_FWD_ROWS, HMM_FWD_SEG, HMM_PROGS };     // HMM_FWD_ROWS: Forward that keeps the special-state rows (SPEC 13.4);
                                                                                       // HMM_FWD_SEG: and M and I of every row as well (SPEC 13.5)
// what joins alternatives: max (SPEC 13, 13.2) or lse (SPEC 13.1). T is read by lse alone.
template <HmmProg P> __device__ __forceinline__ int32_t hmm_join(int32_t a, int32_t b, const uint16_t *T)
{
    if constexpr (P == HMM_FWD || P == HMM_FWD_ROWS || P == HMM_FWD_SEG) return hmm_lse(a, b, T); else return max(a, b);
}
// The join over the wavefront, in every lane: neighbours, pairs of pairs, ... - for lse the balanced tree of SPEC 13.1. After the two quad steps the four
// lanes of a quad hold one value, so the mirrors hand a lane the value of the other quad / the other half row; that is the tree because the join is
// symmetric - a lane and its partner compute join(x, y) and join(y, x).
template <HmmProg P> __device__ __forceinline__ int hmm_wave_join(int x, const uint16_t *T)
{
    x = hmm_join<P>(x, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false), T);        // quad_perm [1,0,3,2]
    x = hmm_join<P>(x, __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false), T);        // quad_perm [2,3,0,1]
    x = hmm_join<P>(x, __builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false), T);       // row_half_mirror
    x = hmm_join<P>(x, __builtin_amdgcn_update_dpp(x, x, 0x140, 0xF, 0xF, false), T);       // row_mirror
    const int a = __builtin_amdgcn_readlane(x, 0), b = __builtin_amdgcn_readlane(x, 16), c = __builtin_amdgcn_readlane(x, 32),
              d = __builtin_amdgcn_readlane(x, 48);
    return hmm_join<P>(hmm_join<P>(a, b, T), hmm_join<P>(c, d, T), T);
}

// ---- trace-back (SPEC 13.2): what the row loop records -----------------------------------------------------------------------------------------
// A pair of a block: where its back-pointers and its row specials start in the block's scratch, its place in the caller's pair list, its record.
struct HmmTracePair { uint64_t ptr_off, row_off; uint32_t pair, rec; };           // ptr_off in words, row_off in rows (int4)
struct HmmTraceProf { uint32_t prof, start, cnt; };                               // the pairs [start, start + cnt) of the call's list belong to prof
// A cell's pointers are a nibble: bits 0-1 where M[i][k] came from (0 M, 1 I, 2 D of node k - 1 in row i - 1, 3 B[i-1]), bit 2 set: I[i][k] came from
// I[i-1][k] (clear: M[i-1][k]), bit 3 set: D[i][k] came from D[i][k-1] (clear: M[i][k-1]). A lane's Q nibbles fill NW = ceil(Q / 8) words; word w of
// lane l in row i lies at ((i - 1) NW + w) 64 + l, so a row is NW bursts of 256 bytes.
enum { HMM_PTR_B = 3, HMM_ROW_C_FROM_E = 1, HMM_ROW_J_FROM_E = 2, HMM_ROW_B_FROM_N = 4, HMM_WALK_BLOCK = 64 };
__host__ __device__ constexpr int hmm_ptr_words(int Q) { return (Q + 7) / 8; }

// ---- the shared prologue and row loop -----------------------------------------------------------------------------------------------------------
// One workgroup per (profile, slice of a list of records): the profile's table goes to LDS once, then each of its wavefronts takes the entries
// j = its number, its number + the waves of the grid's row, ... of the list (longest record first, so the waves of a row end together). Every kernel
// bounds that loop by a count that is at most n_rec, and a workgroup whose slice of a selected list is empty returns before it loads anything.
// Lane l keeps nodes l Q + 1 .. l Q + Q of M, I and D of the current row in registers; 64 residues are loaded at a time, the next 64 while these run.
//   M and I of a row need the row before only: the value a node hands to the next, join(M + tMM, I + tIM, D + tDM), moves up one lane at the group's edge.
//   D of a row is the recurrence D[k+1] = join(D[k] + tDD[k], M[k] + tMD[k]) along k. Each lane runs it over its own nodes from NEG (Dloc) and
//   gets its group as the map x -> join(x + a, b): a = the group's sum of tDD (a constant of the profile, scanned once per workgroup), b = what leaves
//   the group when nothing enters. Six steps of b = join(b, b(lane - d) + a_d) give every lane what really leaves it, the lane above takes that as
//   c_in and D[q] = join(Dloc[q], c_in + PDD[q]).
// Viterbi (SPEC 13): integer max and add, the same words as the serial recurrence in any order. In the scan a lane below 2^s gets its own b back
//   (b + a <= b), so the step needs no select. E = max_k M[k] needs M alone: D[k] is some M[j] of the same row plus non-positive transitions, or NEG,
//   so max(M, D) over the row is max M. Up to Q = 16 the eight transition rows of a lane stay in registers across rows (8 Q of them); at 20 they do
//   not fit beside the 3 Q states, and a compiler barrier keeps the compiler from holding some and spilling others: every row reads them from LDS again.
// Forward (SPEC 13.1): every join is hmm_lse, a gather from T, which sits in LDS behind the profile's table. lse is not associative, so the order of
//   the row loop IS the score: D inside a lane from NEG, six scan steps in which a lane below 2^s keeps its b by a select (lse(b, b + a) is more than
//   b), then c_in from the lane below; D is clamped at NEG, and E folds M and D of a lane's nodes in node order and joins the lanes through
//   hmm_wave_join. The barrier starts at Q = 12: beside 3 Q states, Q give values and the lse temporaries the transition rows do not fit.
// Trace (SPEC 13.2): Viterbi, and beyond the score every row leaves the nibbles of its cells and, through lane 0, {E[i], B[i], the lowest k with
//   M[i][k] == E[i], the decisions of C[i], J[i] and B[i]}; row 0 is {NEG, tmove, 0, B from N}. The barrier starts at Q = 12, as Forward's does.
//   The M pointer of node k + 1 is decided in the lane of node k: give = max(a, b, c) there, and the first of a, b, c, entry that equals
//   max(give, entry) is the first of a, b, c that equals give when give >= entry, else the entry. The code of a lane's last node moves up one lane
//   together with the D decision of the next lane's first node (M + tMD of the last node == what leaves the lane after the scan), in one word.
//   The D pointers inside a lane are taken after D is final. No traced cell is at the clamp (SPEC 13.2), so an equality that a clamped cell decides
//   differently is never followed.
// Forward with rows (SPEC 13.4): Forward's arithmetic and barrier, and lane 0 leaves {E[i], J[i], C[i]} of every row; row 0 is NEG.
// Forward over a segment (SPEC 13.5): Forward with rows, and every lane leaves M and I of its nodes: word q (M) and Q + q (I) of lane l in row i lie at
//   ((i - 1) 2 Q + q) 64 + l of pp, so a row is 2 Q bursts of 256 bytes, written here and read back by Backward in the same shape.
// The specials come from a length of their own (Lsp): the record's for every program but the envelope scores, which run Forward over a stretch of a
//   record under the whole record's length model.
template <int Q> struct HmmLane {
    const int32_t *ms, *tMM, *tMI, *tMD, *tIM, *tII, *tDM, *tDD, *PDD;  // the lane's Q words of match row 0, of the transition rows and of PDD, in LDS
    const uint16_t *T;                                      // the table of lse in LDS (Forward)
    int32_t a_step[6], tbm;                                 // a of the lanes a scan step joins: sums of tDD, at least 1280 * GS_HMM_STAR; A_l(s) of SPEC 13.1
    int lane, wave, nvalid;                                 // nvalid: how many of the lane's nodes are nodes of the profile
};
template <int Q, bool LSE>
__device__ __forceinline__ HmmLane<Q> hmm_stage(const int32_t *tables, const HmmDesc d, const uint16_t *lse_tab)
{
    extern __shared__ int32_t hmm_lds[];
    constexpr int MP = 64 * Q;
    uint16_t *Tw = (uint16_t *)(hmm_lds + HMM_ROWS_DEV * MP);
    for (int i = (int)threadIdx.x; i < HMM_ROWS_DEV * MP; i += HMM_BLOCK) hmm_lds[i] = tables[d.off + i];
    if constexpr (LSE) for (int i = (int)threadIdx.x; i < HMM_LSE_LDS_N; i += HMM_BLOCK) Tw[i] = lse_tab[i];
    __syncthreads();
    HmmLane<Q> ln;
    ln.lane = (int)threadIdx.x & 63; ln.wave = (int)threadIdx.x >> 6;
    const int base = ln.lane * Q;
    ln.nvalid = min(max((int)d.M - base, 0), Q);
    ln.tbm = d.tbm; ln.T = Tw;
    ln.ms = hmm_lds + base;
    ln.tMM = hmm_lds + HMM_ROW_MM * MP + base; ln.tMI = hmm_lds + HMM_ROW_MI * MP + base; ln.tMD = hmm_lds + HMM_ROW_MD * MP + base;
    ln.tIM = hmm_lds + HMM_ROW_IM * MP + base; ln.tII = hmm_lds + HMM_ROW_II * MP + base; ln.tDM = hmm_lds + HMM_ROW_DM * MP + base;
    ln.tDD = hmm_lds + HMM_ROW_DD * MP + base; ln.PDD = hmm_lds + HMM_ROW_PDD * MP + base;
    int32_t a = ln.PDD[Q - 1] + ln.tDD[Q - 1];
    for (int s = 0; s < 6; s++) {
        ln.a_step[s] = a;
        const int32_t up = __shfl_up(a, 1 << s);
        if (ln.lane >= (1 << s)) a += up;
    }
    return ln;
}

// The rows of one record against the staged profile: the raw score in every lane, GS_HMM_NO_SCORE for an empty record or a byte that is no residue.
// Trace also writes the record's pointer words to pp (the lane's column) and its row specials to rr. x, pp and rr carry no __restrict__ and ln comes by
// value: either costs some trace instances registers and a wave per SIMD, at the same instruction counts (NOTES.md).
template <int Q, HmmProg P>
__device__ __forceinline__ int32_t hmm_rows(const HmmLane<Q> ln, const uint8_t *x, uint32_t L, uint32_t Lsp, uint32_t *pp, int4 *rr)
{
    constexpr int MP = 64 * Q, NW = hmm_ptr_words(Q);
    constexpr bool SEG = P == HMM_FWD_SEG, ROWS = P == HMM_FWD_ROWS || SEG, FWD = P == HMM_FWD || ROWS, TRACE = P == HMM_TRACE;
    constexpr int RELOAD_FROM_Q = P == HMM_VIT ? 20 : 12;     // from here the transition rows are read from LDS in every row (above)
    const uint16_t *T = ln.T;
    const int lane = ln.lane, nvalid = ln.nvalid;
    if (!TRACE && L == 0) return GS_HMM_NO_SCORE;             // (the host puts no empty record on a trace list)
    const HmmSpecials sp = hmm_specials(Lsp);
    int32_t Mv[Q], Iv[Q], Dv[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) Mv[q] = Iv[q] = Dv[q] = GS_HMM_NEG;
    int32_t J = GS_HMM_NEG, C = GS_HMM_NEG, B = sp.tmove, N = 0;
    if constexpr (TRACE) if (lane == 0) rr[0] = make_int4(GS_HMM_NEG, B, 0, HMM_ROW_B_FROM_N);
    if constexpr (ROWS) if (lane == 0) rr[0] = make_int4(GS_HMM_NEG, GS_HMM_NEG, GS_HMM_NEG, 0);
    bool bad = false;
    int cur = (uint32_t)lane < L ? hmm_residue(x[lane]) : 0;
    for (uint32_t i0 = 0; i0 < L; i0 += 64) {
        const int nxt = i0 + 64 + (uint32_t)lane < L ? hmm_residue(x[i0 + 64 + lane]) : 0;     // the next 64 residues are on their way while these run
        bad |= cur < 0;
        const int res = max(cur, 0);
        const int cnt = (int)min(64u, L - i0);
        for (int t = 0; t < cnt; t++) {
            if (Q >= RELOAD_FROM_Q) asm volatile("" ::: "memory");
            const int32_t *ms = ln.ms + __builtin_amdgcn_readlane(res, t) * MP;
            const int32_t entry = B + ln.tbm;
            uint32_t pk[NW], code_out = HMM_PTR_B;            // trace: the row's nibbles, and the M pointer of the next lane's first node
#pragma unroll
            for (int w = 0; w < NW; w++) pk[w] = 0;
            int32_t give[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int32_t a = Mv[q] + ln.tMM[q], b = Iv[q] + ln.tIM[q], c = Dv[q] + ln.tDM[q];
                const int32_t g = hmm_join<P>(hmm_join<P>(a, b, T), c, T);
                give[q] = g;
                if constexpr (TRACE) {
                    const uint32_t code = g >= entry ? (a == g ? 0u : (b == g ? 1u : 2u)) : (uint32_t)HMM_PTR_B;
                    if (q + 1 < Q) pk[(q + 1) >> 3] |= code << (4 * ((q + 1) & 7)); else code_out = code;
                }
            }
            int32_t up = __shfl_up(give[Q - 1], 1);
            if (lane == 0) up = GS_HMM_NEG;                   // node 0 has no states: B + tBM is far above NEG
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int32_t fromM = Mv[q] + ln.tMI[q];
                Iv[q] = max(hmm_join<P>(fromM, Iv[q] + ln.tII[q], T), GS_HMM_NEG);
                if constexpr (TRACE) pk[q >> 3] |= (fromM == Iv[q] ? 0u : 4u) << (4 * (q & 7));
            }
#pragma unroll
            for (int q = 0; q < Q; q++) Mv[q] = max(ms[q] + hmm_join<P>(q ? give[q - 1] : up, entry, T), GS_HMM_NEG);
            int32_t dl = GS_HMM_NEG;
            Dv[0] = dl;
#pragma unroll
            for (int q = 1; q < Q; q++) { dl = max(hmm_join<P>(dl + ln.tDD[q - 1], Mv[q - 1] + ln.tMD[q - 1], T), GS_HMM_NEG); Dv[q] = dl; }
            const int32_t m_out = Mv[Q - 1] + ln.tMD[Q - 1];
            int32_t b = max(hmm_join<P>(dl + ln.tDD[Q - 1], m_out, T), GS_HMM_NEG);
#pragma unroll
            for (int s = 0; s < 6; s++) {                     // the scan step: Forward's select and clamp
                const int32_t nb = hmm_join<P>(b, __shfl_up(b, 1 << s) + ln.a_step[s], T);
                if constexpr (FWD) b = lane >= (1 << s) ? max(nb, GS_HMM_NEG) : b; else b = nb;
            }
            int32_t c_in = __shfl_up(b, 1);
            if (lane == 0) c_in = GS_HMM_NEG;
            if constexpr (TRACE) {
                uint32_t edge = (uint32_t)__shfl_up((int)(code_out | (m_out == b ? 0u : 8u)), 1);
                if (lane == 0) edge = HMM_PTR_B | 8u;
                pk[0] |= edge;
            }
            int32_t e = GS_HMM_NEG;
#pragma unroll
            for (int q = 0; q < Q; q++) {                     // D final and the E fold: Forward clamps D and folds it into E
                Dv[q] = hmm_join<P>(Dv[q], c_in + ln.PDD[q], T);
                if constexpr (FWD) Dv[q] = max(Dv[q], GS_HMM_NEG);
                if constexpr (TRACE) if (q >= 1) pk[q >> 3] |= (Mv[q - 1] + ln.tMD[q - 1] == Dv[q] ? 0u : 8u) << (4 * (q & 7));
                int32_t e2 = hmm_join<P>(e, Mv[q], T);
                if constexpr (FWD) e2 = hmm_join<P>(e2, Dv[q], T);
                e = q < nvalid ? e2 : e;
            }
            const int32_t E = hmm_wave_join<P>(e, T);
            const uint32_t row = i0 + (uint32_t)t;            // row i = row + 1
            int kE = 0;
            if constexpr (SEG) {
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    pp[((uint64_t)row * (2 * Q) + q) * 64] = (uint32_t)Mv[q];
                    pp[((uint64_t)row * (2 * Q) + Q + q) * 64] = (uint32_t)Iv[q];
                }
            }
            if constexpr (TRACE) {
#pragma unroll
                for (int w = 0; w < NW; w++) pp[((uint64_t)row * NW + w) * 64] = pk[w];
                // the lowest node of the row's maximum: the first lane that holds it, and that lane's first node
                int first = 0;
#pragma unroll
                for (int q = Q - 1; q >= 0; q--) if (q < nvalid && Mv[q] == E) first = q;
                const int fl = __ffsll((unsigned long long)__ballot(e == E)) - 1;     // some lane holds it: E is the maximum of the e
                kE = fl * Q + __builtin_amdgcn_readlane(first, fl) + 1;
            }
            N += sp.tloop;
            const int32_t Jn = max(hmm_join<P>(J + sp.tloop, E + GS_HMM_TEJ, T), GS_HMM_NEG), Cn = max(hmm_join<P>(C + sp.tloop, E + GS_HMM_TEJ, T), GS_HMM_NEG);
            const int flags = (E + GS_HMM_TEJ == Cn ? HMM_ROW_C_FROM_E : 0) | (E + GS_HMM_TEJ == Jn ? HMM_ROW_J_FROM_E : 0) | (N >= Jn ? HMM_ROW_B_FROM_N : 0);
            J = Jn; C = Cn;
            B = hmm_join<P>(N, J, T) + sp.tmove;
            if constexpr (TRACE) if (lane == 0) rr[row + 1] = make_int4(E, B, kE, flags);
            if constexpr (ROWS) if (lane == 0) rr[row + 1] = make_int4(E, J, C, 0);
        }
        cur = nxt;
    }
    return __any(bad) ? GS_HMM_NO_SCORE : C + sp.tmove - sp.null;
}

// Viterbi score of every record against the profiles plist[] of one class: a wavefront takes the records order[j] (all n_rec of them, longest first)
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_viterbi(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const uint32_t *__restrict__ plist,
                                                           const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                           const uint32_t *__restrict__ order, uint32_t n_rec, uint32_t n_prof, int32_t *__restrict__ score)
{
    const uint32_t p = plist[blockIdx.y];
    const HmmLane<Q> ln = hmm_stage<Q, false>(tables, desc[p], nullptr);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < n_rec; j += gridDim.x * HMM_WAVES) {
        const uint32_t r = order[j];
        const int32_t raw = hmm_rows<Q, HMM_VIT>(ln, aa + rec_start[r], (uint32_t)rec_len[r], (uint32_t)rec_len[r], nullptr, nullptr);
        if (ln.lane == 0) score[(uint64_t)r * n_prof + p] = raw;
    }
}

// Forward score of the records sel[p][0 .. sel_cnt[p]) of each profile of plist[]
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_forward(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const uint32_t *__restrict__ plist,
                                                           const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start,
                                                           const uint64_t *__restrict__ rec_len, const uint32_t *__restrict__ sel, const uint32_t *__restrict__ sel_cnt,
                                                           uint32_t n_rec, uint32_t n_prof, int32_t *__restrict__ score)
{
    const uint32_t p = plist[blockIdx.y];
    const uint32_t cnt = min(sel_cnt[p], n_rec);
    if ((uint64_t)blockIdx.x * HMM_WAVES >= cnt) return;
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, desc[p], lse_tab);
    const uint32_t *list = sel + (uint64_t)p * n_rec;
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < cnt; j += gridDim.x * HMM_WAVES) {
        const uint32_t r = list[j];
        const int32_t raw = hmm_rows<Q, HMM_FWD>(ln, aa + rec_start[r], (uint32_t)rec_len[r], (uint32_t)rec_len[r], nullptr, nullptr);
        if (ln.lane == 0) score[(uint64_t)r * n_prof + p] = raw;
    }
}

// Viterbi score, back-pointers and row specials of the pairs of each profile of profs[]; 1 <= L <= GS_HMM_TRACE_MAX_L: the host put no other pair on a list
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_trace(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                         const HmmTracePair *__restrict__ pairs, const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start,
                                                         const uint64_t *__restrict__ rec_len, uint32_t *__restrict__ ptrs, int4 *__restrict__ rows,
                                                         int32_t *__restrict__ raw_out)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmLane<Q> ln = hmm_stage<Q, false>(tables, desc[tp.prof], nullptr);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const int32_t raw = hmm_rows<Q, HMM_TRACE>(ln, aa + rec_start[pr.rec], (uint32_t)rec_len[pr.rec], (uint32_t)rec_len[pr.rec], ptrs + pr.ptr_off + ln.lane, rows + pr.row_off);
        if (ln.lane == 0) raw_out[pr.pair] = raw;
    }
}

// Viterbi score of the records sel[p][0 .. sel_cnt[p]) of each profile of plist[] (SPEC 13.3: the pairs that passed the MSV floor); the other words of
// `score` keep what k_hmm_fill wrote
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_viterbi_sel(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const uint32_t *__restrict__ plist,
                                                               const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                               const uint32_t *__restrict__ sel, const uint32_t *__restrict__ sel_cnt, uint32_t n_rec, uint32_t n_prof,
                                                               int32_t *__restrict__ score)
{
    const uint32_t p = plist[blockIdx.y];
    const uint32_t cnt = min(sel_cnt[p], n_rec);
    if ((uint64_t)blockIdx.x * HMM_WAVES >= cnt) return;
    const HmmLane<Q> ln = hmm_stage<Q, false>(tables, desc[p], nullptr);
    const uint32_t *list = sel + (uint64_t)p * n_rec;
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < cnt; j += gridDim.x * HMM_WAVES) {
        const uint32_t r = list[j];
        const int32_t raw = hmm_rows<Q, HMM_VIT>(ln, aa + rec_start[r], (uint32_t)rec_len[r], (uint32_t)rec_len[r], nullptr, nullptr);
        if (ln.lane == 0) score[(uint64_t)r * n_prof + p] = raw;
    }
}

// ---- MSV (SPEC 13.3): ungapped diagonals, any number of them ----------------------------------------------------------------------------------
// The model of SPEC 13 without I and D and with tMM = 0, so a row is M[k] = max(NEG, msc[k] + max(M'[k-1], B + tBM)) and E = max_k M[k]. The launch
// geometry, the lane layout and the residue loads are k_hmm_viterbi's; the row loop is its own, because nothing of hmm_rows but the specials is left:
// no give, no I, no D scan, no transition rows. Only the 20 match rows of the profile's table go to LDS (5 120 Q bytes against 7 168 Q), so two
// workgroups of class 12 and 16 fit a CU where one Viterbi workgroup does, four of class 6 and 8 where three and two do.
// Per row a node costs a max, an add and half a max3 of the fold into e; M of a lane's last node moves up one lane; E is hmm_wave_join<HMM_VIT>, and
// B of the next row waits for it: that chain, not the node work, is what a lone wavefront feels.
//   No clamp: the max(NEG, .) of SPEC 13.3 never binds. B >= i tloop + tmove with i tloop >= -8 864 (tloop is 4 432 / L rounded to a unit, 0 from
//   L = 8 865 on) and tmove >= -16 810, tBM >= -20 120 for L <= 2^18 and M <= 1 280, so B + tBM > -50 000; every word of a match row is at least
//   STAR = -2^18, so a cell is above -320 000, far above NEG = -2^29: the integers are the clamped ones.
//   No nvalid: the staged copy holds HMM_MSV_PAD, not STAR, in the match rows of the padding nodes (they follow node M, so only padding is fed by
//   padding). A padding cell is PAD + max(cell, entry): at least PAD - 50 000 > INT32_MIN and at most PAD + 6 608 * 2^18 = -415 105 024, below the
//   -320 000 that E = max over the M >= 1 real nodes is above. So padding never reaches E and the fold needs no select.
//   Blocks of four: where Q is a multiple of 4 the staged copy does not keep a lane's Q words together. Word q of lane l lies at
//   (q / 4) 256 + 4 l + q % 4 of its row, so the ds_read_b128 that fetches words 4 b .. 4 b + 3 of every lane reads 1 024 contiguous bytes. With
//   the lane's words together the lanes of a read are Q words apart, a many-way bank conflict at Q = 8 and Q = 16: the first form of this
//   kernel ran class 16 at 13 % of its issue ceiling for that reason.
enum { HMM_MSV_ROWS = 20, HMM_MSV_PAD = INT32_MIN + (1 << 17) };
__host__ __device__ constexpr int hmm_msv_block(int Q) { return Q % 4 == 0 ? 4 : Q; }          // words of a lane that stay together in the staged copy
// where word q of a lane lies from the lane's first word of a row
__host__ __device__ constexpr int hmm_msv_at(int Q, int q) { return (q / hmm_msv_block(Q)) * 64 * hmm_msv_block(Q) + q % hmm_msv_block(Q); }
static_assert((int64_t)HMM_MSV_PAD + 6608ll * GS_HMM_MAX_L < -320000 && (int64_t)HMM_MSV_PAD - 50000 > INT32_MIN, "a padding cell stays below every E and inside int32");
template <int Q> struct HmmMsvLane {
    const int32_t *ms;                                      // the lane's first word of match row 0, in LDS: word q at ms[hmm_msv_at(Q, q)]
    int32_t tbm;
    int lane, wave;
};
template <int Q>
__device__ __forceinline__ HmmMsvLane<Q> hmm_msv_stage(const int32_t *tables, const HmmDesc d)
{
    extern __shared__ int4 hmm_msv_lds[];                     // (int4: the blocks of four are read as ds_read_b128, which wants their alignment known)
    int32_t *hmm_lds = (int32_t *)hmm_msv_lds;
    constexpr int MP = 64 * Q;
    for (int i = (int)threadIdx.x; i < HMM_MSV_ROWS * MP; i += HMM_BLOCK) {
        const int j = i % MP;                                 // the word of node j + 1, lane j / Q
        hmm_lds[i - j + (j / Q) * hmm_msv_block(Q) + hmm_msv_at(Q, j % Q)] = (uint32_t)j < d.M ? tables[d.off + i] : (int32_t)HMM_MSV_PAD;
    }
    __syncthreads();
    HmmMsvLane<Q> ln;
    ln.lane = (int)threadIdx.x & 63; ln.wave = (int)threadIdx.x >> 6;
    ln.tbm = d.tbm;
    ln.ms = hmm_lds + ln.lane * hmm_msv_block(Q);
    return ln;
}

// The MSV rows of one record against the staged match rows: the raw score in every lane, GS_HMM_NO_SCORE for an empty record or a byte that is no residue
template <int Q>
__device__ __forceinline__ int32_t hmm_msv_rows(const HmmMsvLane<Q> ln, const uint8_t *x, uint32_t L)
{
    constexpr int MP = 64 * Q;
    const int lane = ln.lane;
    if (L == 0) return GS_HMM_NO_SCORE;
    const HmmSpecials sp = hmm_specials(L);
    int32_t Mv[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) Mv[q] = GS_HMM_NEG;
    int32_t J = GS_HMM_NEG, C = GS_HMM_NEG, B = sp.tmove, N = 0;
    bool bad = false;
    int cur = (uint32_t)lane < L ? hmm_residue(x[lane]) : 0;
    for (uint32_t i0 = 0; i0 < L; i0 += 64) {
        const int nxt = i0 + 64 + (uint32_t)lane < L ? hmm_residue(x[i0 + 64 + lane]) : 0;     // the next 64 residues are on their way while these run
        bad |= cur < 0;
        const int res = max(cur, 0);                              // a byte that is no residue reads row 0: inside the table, and the pair gets no score
        const int cnt = (int)min(64u, L - i0);
        for (int t = 0; t < cnt; t++) {
            const int32_t *ms = ln.ms + __builtin_amdgcn_readlane(res, t) * MP;
            const int32_t entry = B + ln.tbm;
            int32_t sc[Q];                                        // the row's match scores of the lane's nodes
            if constexpr (Q % 4 == 0) {
#pragma unroll
                for (int b = 0; b < Q / 4; b++) {
                    const int4 v = ((const int4 *)ms)[b * 64];
                    sc[4 * b] = v.x; sc[4 * b + 1] = v.y; sc[4 * b + 2] = v.z; sc[4 * b + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < Q; q++) sc[q] = ms[q];
            }
            int32_t up = __shfl_up(Mv[Q - 1], 1);
            if (lane == 0) up = GS_HMM_NEG;                       // node 0 has no states
#pragma unroll
            for (int q = Q - 1; q >= 1; q--) Mv[q] = sc[q] + max(Mv[q - 1], entry);        // downwards: Mv[q - 1] is still the row before
            Mv[0] = sc[0] + max(up, entry);
            int32_t e = Mv[0];
#pragma unroll
            for (int q = 1; q < Q; q++) e = max(e, Mv[q]);            // padding cells are below every real one (above)
            const int32_t E = hmm_wave_join<HMM_VIT>(e, nullptr);
            N += sp.tloop;
            J = max(max(J + sp.tloop, E + GS_HMM_TEJ), GS_HMM_NEG);
            C = max(max(C + sp.tloop, E + GS_HMM_TEJ), GS_HMM_NEG);
            B = max(N, J) + sp.tmove;
        }
        cur = nxt;
    }
    return __any(bad) ? GS_HMM_NO_SCORE : C + sp.tmove - sp.null;
}

// MSV score of every record against the profiles plist[] of one class; the arguments of k_hmm_viterbi
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_msv(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const uint32_t *__restrict__ plist,
                                                       const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                       const uint32_t *__restrict__ order, uint32_t n_rec, uint32_t n_prof, int32_t *__restrict__ score)
{
    const uint32_t p = plist[blockIdx.y];
    const HmmMsvLane<Q> ln = hmm_msv_stage<Q>(tables, desc[p]);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < n_rec; j += gridDim.x * HMM_WAVES) {
        const uint32_t r = order[j];
        const int32_t raw = hmm_msv_rows<Q>(ln, aa + rec_start[r], (uint32_t)rec_len[r]);
        if (ln.lane == 0) score[(uint64_t)r * n_prof + p] = raw;
    }
}

// ---- the packed int16 Viterbi filter (SPEC 13.7): vf >= vit, two nodes a register --------------------------------------------------------------------
// The cells of SPEC 13 in half units (2^-9 bit) as int16, every cell operation a packed saturating add (v_pk_add_i16 clamp) or a packed max
// (v_pk_max_i16); the specials stay int32 scalars in the units of SPEC 13 with E = 2 E16. The launch geometry, the class lists and the residue loads are
// k_hmm_viterbi's; a class of Q nodes a lane runs with H = ceil(Q / 2) registers a state (classes 1 and 2 share an instance, 3 and 4 another).
//   Layout: lane l holds the 2 H node slots from l 2 H on as two runs - slots l 2 H + r in the low halves of its registers r = 0 .. H - 1, slots
//   l 2 H + H + r in the high halves. The move up one node is then a rename of registers and one combine at register 0: its low half takes the high
//   half of the last register of the lane below, its high half the low half of the lane's own last register (one shuffle and one v_alignbit).
//   D: both runs go from NEG16 in one packed chain (Dloc) and leave b_lo, b_hi. With tDD <= 0 and every M + tMD at least NEG16, the chain of
//   saturating steps equals max(NEG16, wide sums) (SPEC 13.7), so the runs are joined on int32 scalars with the WIDE sums of tDD16 of a run (a_lo,
//   a_hi): b = max(b_hi, b_lo + a_hi), the six scan steps of hmm_rows over the lanes, then what enters the low run (c_in) and the high run
//   (max(b_lo, c_in + a_lo)) is carried along both runs by saturating steps - no PDD row, whose int16 form would clamp.
//   The staged copy is made on the host in the order the lanes read it: register r of lane l lies at (r / B) 64 B + l B + r % B of its row of 64 H
//   words, B = 4, 2 or 1 the largest of them that divides H, so a ds_read_b128 / b64 / b32 of all lanes reads contiguous bytes (the lesson of k_hmm_msv).
//   Padding slots hold NEG16 in every row. The lower clamp is not sticky (NEG16 plus a positive entry is above NEG16), so a padding cell can rise:
//   it feeds padding only, and the fold into E16 takes min(M, lim) with lim = NEG16 in the padding halves.
//   The first row with E16 == 32767 ends the record's rows, for the whole wavefront (E16 is uniform); the bytes behind it are still looked at, since a
//   byte that is no residue goes before an overflow.
typedef short hmm_s2 __attribute__((ext_vector_type(2)));
enum { HMM16_ROWS = 27, HMM16_NEG = -32768, HMM16_MAX = 32767 };
static_assert(HMM16_ROWS == GS_HMM_TABLE_ROWS && HMM_ROW_DD == HMM16_ROWS - 1, "the int16 table has the rows of the host table");
__host__ __device__ constexpr int hmm16_regs(int Q) { return (Q + 1) / 2; }
__host__ __device__ constexpr int hmm16_block(int H) { return H % 4 == 0 ? 4 : (H % 2 == 0 ? 2 : 1); }
__host__ __device__ constexpr int hmm16_at(int H, int r) { return (r / hmm16_block(H)) * 64 * hmm16_block(H) + r % hmm16_block(H); }
// the word of a row that holds node slot j (node j + 1), and whether it is the word's high half
__host__ __device__ constexpr int hmm16_word(int H, int j) { return (j / (2 * H)) * hmm16_block(H) + hmm16_at(H, j % H); }
__host__ __device__ constexpr bool hmm16_high(int H, int j) { return j % (2 * H) >= H; }
static_assert((size_t)HMM16_ROWS * 64 * hmm16_regs(HMM_CLASS_Q[HMM_CLASSES - 1]) * 4 <= 160 * 1024 / 2, "two workgroups of the largest class fit the LDS of a CU");
// h of SPEC 13.7: the ceiling of x / 2, kept inside int16
__host__ __device__ inline int32_t hmm16_half(int32_t x)
{
    const int32_t h = (x + 1) >> 1;
    return h < HMM16_NEG ? HMM16_NEG : (h > HMM16_MAX ? HMM16_MAX : h);
}
__device__ __forceinline__ hmm_s2 hmm16_add(hmm_s2 a, hmm_s2 b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ hmm_s2 hmm16_max(hmm_s2 a, hmm_s2 b) { return __builtin_elementwise_max(a, b); }

template <int H> struct Hmm16Lane {
    const hmm_s2 *row0;                                     // the lane's first word of table row 0 in LDS: register r of row w at row0[w * 64 H + hmm16_at(H, r)]
    hmm_s2 lim[H];                                          // 32767 in the halves that are nodes of the profile, NEG16 in the padding
    int32_t a_step[6], a_lo, a_hi, tbm;                     // wide sums of tDD16: of the lanes a scan step joins, of the lane's low and high run
    int lane, wave;
};
template <int H>
__device__ __forceinline__ Hmm16Lane<H> hmm16_stage(const int32_t *tables16, const HmmDesc d)
{
    extern __shared__ int4 hmm16_lds[];                     // (int4: the blocks of four are read as ds_read_b128)
    int32_t *lds = (int32_t *)hmm16_lds;
    constexpr int RW = 64 * H;
    for (int i = (int)threadIdx.x; i < HMM16_ROWS * RW; i += HMM_BLOCK) lds[i] = tables16[d.off + i];
    __syncthreads();
    Hmm16Lane<H> ln;
    ln.lane = (int)threadIdx.x & 63; ln.wave = (int)threadIdx.x >> 6;
    ln.tbm = d.tbm;
    ln.row0 = (const hmm_s2 *)lds + ln.lane * hmm16_block(H);
    const hmm_s2 *tDD = ln.row0 + HMM_ROW_DD * RW;
    ln.a_lo = ln.a_hi = 0;
#pragma unroll
    for (int r = 0; r < H; r++) {
        const int slot = ln.lane * 2 * H + r;
        ln.lim[r] = hmm_s2{(short)(slot < (int)d.M ? HMM16_MAX : HMM16_NEG), (short)(slot + H < (int)d.M ? HMM16_MAX : HMM16_NEG)};
        const hmm_s2 t = tDD[hmm16_at(H, r)];
        ln.a_lo += t.x; ln.a_hi += t.y;
    }
    int32_t a = ln.a_lo + ln.a_hi;                          // at least 1280 * NEG16: far inside int32
    for (int s = 0; s < 6; s++) {
        ln.a_step[s] = a;
        const int32_t up = __shfl_up(a, 1 << s);
        if (ln.lane >= (1 << s)) a += up;
    }
    return ln;
}

// The rows of one record against the staged int16 profile: vf in every lane - GS_HMM_NO_SCORE for an empty record or a byte that is no residue, else
// GS_HMM_VF_OVER from the first row whose E16 is 32767
template <int H>
__device__ __forceinline__ int32_t hmm16_rows(const Hmm16Lane<H> &ln, const uint8_t *x, uint32_t L)
{
    constexpr int RW = 64 * H;
    const int lane = ln.lane;
    if (L == 0) return GS_HMM_NO_SCORE;
    const HmmSpecials sp = hmm_specials(L);
    const hmm_s2 NEG2 = {(short)HMM16_NEG, (short)HMM16_NEG};
    const hmm_s2 *tMM = ln.row0 + HMM_ROW_MM * RW, *tMI = ln.row0 + HMM_ROW_MI * RW, *tMD = ln.row0 + HMM_ROW_MD * RW, *tIM = ln.row0 + HMM_ROW_IM * RW,
                 *tII = ln.row0 + HMM_ROW_II * RW, *tDM = ln.row0 + HMM_ROW_DM * RW, *tDD = ln.row0 + HMM_ROW_DD * RW;
    hmm_s2 Mv[H], Iv[H], Dv[H];
#pragma unroll
    for (int r = 0; r < H; r++) Mv[r] = Iv[r] = Dv[r] = NEG2;
    int32_t J = GS_HMM_NEG, C = GS_HMM_NEG, B = sp.tmove, N = 0;
    bool bad = false, over = false;
    int cur = (uint32_t)lane < L ? hmm_residue(x[lane]) : 0;
    for (uint32_t i0 = 0; i0 < L; i0 += 64) {
        const int nxt = i0 + 64 + (uint32_t)lane < L ? hmm_residue(x[i0 + 64 + lane]) : 0;     // the next 64 residues are on their way while these run
        bad |= cur < 0;
        const int res = max(cur, 0);
        const int cnt = over ? 0 : (int)min(64u, L - i0);         // behind an overflow only the bytes are looked at
        for (int t = 0; t < cnt; t++) {
            const hmm_s2 *ms = ln.row0 + __builtin_amdgcn_readlane(res, t) * RW;
            const short ent16 = (short)hmm16_half(B + ln.tbm);
            const hmm_s2 ent = {ent16, ent16};
            hmm_s2 give[H];
#pragma unroll
            for (int r = 0; r < H; r++)
                give[r] = hmm16_max(hmm16_max(hmm16_add(Mv[r], tMM[hmm16_at(H, r)]), hmm16_add(Iv[r], tIM[hmm16_at(H, r)])), hmm16_add(Dv[r], tDM[hmm16_at(H, r)]));
            const uint32_t gl = __builtin_bit_cast(uint32_t, give[H - 1]);
            uint32_t up = (uint32_t)__shfl_up((int)gl, 1);
            if (lane == 0) up = 0x80000000u;                      // node 0 has no states: NEG16 enters node 1
            const hmm_s2 in0 = __builtin_bit_cast(hmm_s2, __builtin_amdgcn_alignbit(gl, up, 16));        // {high half of the lane below, own low half}
#pragma unroll
            for (int r = 0; r < H; r++) Iv[r] = hmm16_max(hmm16_add(Mv[r], tMI[hmm16_at(H, r)]), hmm16_add(Iv[r], tII[hmm16_at(H, r)]));
#pragma unroll
            for (int r = 0; r < H; r++) Mv[r] = hmm16_add(ms[hmm16_at(H, r)], hmm16_max(r ? give[r - 1] : in0, ent));
            hmm_s2 dl = NEG2;
            Dv[0] = dl;
#pragma unroll
            for (int r = 1; r < H; r++) { dl = hmm16_max(hmm16_add(dl, tDD[hmm16_at(H, r - 1)]), hmm16_add(Mv[r - 1], tMD[hmm16_at(H, r - 1)])); Dv[r] = dl; }
            const hmm_s2 bo = hmm16_max(hmm16_add(dl, tDD[hmm16_at(H, H - 1)]), hmm16_add(Mv[H - 1], tMD[hmm16_at(H, H - 1)]));
            const int32_t b_lo = bo.x;
            int32_t b = max((int32_t)bo.y, b_lo + ln.a_hi);
#pragma unroll
            for (int s = 0; s < 6; s++) b = max(b, __shfl_up(b, 1 << s) + ln.a_step[s]);      // a lane below 2^s gets its own b back (b + a <= b)
            int32_t c_in = __shfl_up(b, 1);
            if (lane == 0) c_in = HMM16_NEG;
            hmm_s2 carry = {(short)c_in, (short)max(b_lo, c_in + ln.a_lo)};                   // both inside int16: each is some b, or NEG16
            hmm_s2 e = NEG2;
#pragma unroll
            for (int r = 0; r < H; r++) {
                Dv[r] = hmm16_max(Dv[r], carry);
                if (r + 1 < H) carry = hmm16_add(carry, tDD[hmm16_at(H, r)]);
                e = hmm16_max(e, __builtin_elementwise_min(Mv[r], ln.lim[r]));
            }
            const int32_t E16 = hmm_wave_join<HMM_VIT>(max((int)e.x, (int)e.y), nullptr);
            if (E16 == HMM16_MAX) { over = true; break; }
            const int32_t E = 2 * E16;
            N += sp.tloop;
            J = max(max(J + sp.tloop, E + GS_HMM_TEJ), GS_HMM_NEG);
            C = max(max(C + sp.tloop, E + GS_HMM_TEJ), GS_HMM_NEG);
            B = max(N, J) + sp.tmove;
        }
        cur = nxt;
    }
    return __any(bad) ? GS_HMM_NO_SCORE : (over ? GS_HMM_VF_OVER : C + sp.tmove - sp.null);
}

// vf of every record against the profiles plist[] of one class; the arguments of k_hmm_viterbi, with the int16 tables and their descriptors
template <int H>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_vit16(const int32_t *__restrict__ tables16, const HmmDesc *__restrict__ desc16, const uint32_t *__restrict__ plist,
                                                         const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                         const uint32_t *__restrict__ order, uint32_t n_rec, uint32_t n_prof, int32_t *__restrict__ score)
{
    const uint32_t p = plist[blockIdx.y];
    const Hmm16Lane<H> ln = hmm16_stage<H>(tables16, desc16[p]);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < n_rec; j += gridDim.x * HMM_WAVES) {
        const uint32_t r = order[j];
        const int32_t vf = hmm16_rows<H>(ln, aa + rec_start[r], (uint32_t)rec_len[r]);
        if (ln.lane == 0) score[(uint64_t)r * n_prof + p] = vf;
    }
}

// vf of the records sel[p][0 .. sel_cnt[p]) of each profile of plist[]; the arguments of k_hmm_viterbi_sel, and its rule for the other words of `score`
template <int H>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_vit16_sel(const int32_t *__restrict__ tables16, const HmmDesc *__restrict__ desc16, const uint32_t *__restrict__ plist,
                                                             const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                             const uint32_t *__restrict__ sel, const uint32_t *__restrict__ sel_cnt, uint32_t n_rec, uint32_t n_prof,
                                                             int32_t *__restrict__ score)
{
    const uint32_t p = plist[blockIdx.y];
    const uint32_t cnt = min(sel_cnt[p], n_rec);
    if ((uint64_t)blockIdx.x * HMM_WAVES >= cnt) return;
    const Hmm16Lane<H> ln = hmm16_stage<H>(tables16, desc16[p]);
    const uint32_t *list = sel + (uint64_t)p * n_rec;
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < cnt; j += gridDim.x * HMM_WAVES) {
        const uint32_t r = list[j];
        const int32_t vf = hmm16_rows<H>(ln, aa + rec_start[r], (uint32_t)rec_len[r]);
        if (ln.lane == 0) score[(uint64_t)r * n_prof + p] = vf;
    }
}

// one thread per (genome, profile): the records of the genome in order, so the first of equal scores stays
__global__ __launch_bounds__(256) void k_hmm_best(const int32_t *__restrict__ score, const uint64_t *__restrict__ goff, uint64_t n_genomes, uint32_t n_prof,
                                                  const int32_t *__restrict__ thr, uint32_t *__restrict__ best_rec, int32_t *__restrict__ best_score)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_genomes * n_prof) return;
    const uint64_t g = i / n_prof;
    const uint32_t p = (uint32_t)(i % n_prof);
    const int32_t t = thr[p];
    uint32_t br = GS_HMM_NO_HIT;
    int32_t bs = GS_HMM_NO_SCORE;
    for (uint64_t r = goff[g], r1 = goff[g + 1]; r < r1; r++) {
        const int32_t s = score[r * n_prof + p];
        if (s != GS_HMM_NO_SCORE && s >= t && s > bs) { bs = s; br = (uint32_t)r; }
    }
    best_rec[i] = br;
    best_score[i] = bs;
}

// Per profile the records whose Viterbi score reaches the profile's floor, in the order of `order` (longest first), and their number. One workgroup per
// profile walks `order` 256 at a time: a ballot per wavefront, the wavefronts' counts through LDS, a running base. No atomics: the list is the same
// every time. sel: [n_prof][n_rec], only the first cnt[p] words of a row are written (and read). floor = nullptr: every pair that has a score.
enum { HMM_SEL_BLOCK = 256 };
__global__ __launch_bounds__(HMM_SEL_BLOCK) void k_hmm_select(const int32_t *__restrict__ vit, const uint32_t *__restrict__ order, uint32_t n_rec, uint32_t n_prof,
                                                              const int32_t *__restrict__ floor, uint32_t *__restrict__ sel, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t wsum[HMM_SEL_BLOCK / 64];
    const uint32_t p = blockIdx.x;
    const int32_t fl = floor ? floor[p] : INT32_MIN + 1;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint32_t *out = sel + (uint64_t)p * n_rec;
    uint32_t base = 0;
    for (uint64_t j0 = 0; j0 < n_rec; j0 += HMM_SEL_BLOCK) {
        const uint64_t j = j0 + threadIdx.x;
        uint32_t r = 0;
        bool pass = false;
        if (j < n_rec) {
            r = order[j];
            const int32_t v = vit[(uint64_t)r * n_prof + p];
            pass = v != GS_HMM_NO_SCORE && v >= fl;
        }
        const uint64_t bal = __ballot(pass);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = base, total = 0;
        for (int w = 0; w < HMM_SEL_BLOCK / 64; w++) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        if (pass) out[before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = r;       // below base + total <= n_rec
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[p] = base;
}

__global__ __launch_bounds__(256) void k_hmm_fill(int32_t *__restrict__ out, uint64_t n, int32_t v)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

// The walk of SPEC 13.2, one lane per pair of the block: from C[L] back to N, once to count the domains and once to write the first max_dom of them
// in sequence order. Every step lowers i or k, so a walk ends after at most 2 (L + M) steps whatever the scratch holds; L + M dependent loads a pair.
__global__ __launch_bounds__(HMM_WALK_BLOCK) void k_hmm_walk(const HmmDesc *__restrict__ desc, const HmmTracePair *__restrict__ pairs, uint32_t n, const uint32_t *__restrict__ pair_prof,
                                                             const uint64_t *__restrict__ rec_len, const uint32_t *__restrict__ ptrs, const int4 *__restrict__ rows,
                                                             const int32_t *__restrict__ raw, uint32_t max_dom, uint32_t *__restrict__ n_dom_out, int32_t *__restrict__ dom_out)
{
    const uint32_t t = blockIdx.x * HMM_WALK_BLOCK + threadIdx.x;
    if (t >= n) return;
    const HmmTracePair pr = pairs[t];
    if (raw[pr.pair] == GS_HMM_NO_SCORE) return;                   // a byte that is no residue: the outputs keep what the fill wrote
    const int M = (int)desc[pair_prof[pr.pair]].M;
    const int Q = hmm_q_of((uint32_t)M), NW = hmm_ptr_words(Q);
    const int L = (int)rec_len[pr.rec];
    const uint32_t *pp = ptrs + pr.ptr_off;
    const int4 *rr = rows + pr.row_off;
    auto nibble = [&](int i, int k) {
        const int node = k - 1, ln = node / Q, q = node - ln * Q;
        return (pp[((uint64_t)(i - 1) * NW + (q >> 3)) * 64 + ln] >> (4 * (q & 7))) & 15u;
    };
    int32_t *dom = dom_out + (uint64_t)pr.pair * max_dom * GS_HMM_DOM_WORDS;
    uint32_t total = 0;
    for (int pass = 0; pass < 2; pass++) {
        uint32_t found = 0;
        int i = L;
        bool more = true;
        while (more && i >= 1) {
            while (i > 1 && !(rr[i].w & (found ? HMM_ROW_J_FROM_E : HMM_ROW_C_FROM_E))) i--;       // C[i] (first) or J[i] (later) back to the row it left E in
            const int4 re = rr[i];
            const int i_to = i, k_to = min(max(re.z, 1), M);
            int k = k_to, st = 0, nm = 0, ni = 0, nd = 0, i_from = 0, k_from = 0;
            while (i >= 1 && k >= 1) {
                const uint32_t nb = nibble(i, k);
                if (st == 0) {
                    nm++;
                    const uint32_t from = nb & 3u;
                    if (from == HMM_PTR_B || i == 1 || k == 1) { i_from = i; k_from = k; break; }
                    st = (int)from; i--; k--;
                } else if (st == 1) {
                    ni++;
                    st = nb & 4u ? 1 : 0; i--;
                } else {
                    nd++;
                    st = nb & 8u ? 2 : 0; k--;
                }
            }
            if (!i_from) break;                                     // not a path: only scratch that no trace kernel wrote leads here
            const int4 rb = rr[i_from - 1];
            if (pass == 1 && total - 1 - found < max_dom) {
                int32_t *o = dom + (uint64_t)(total - 1 - found) * GS_HMM_DOM_WORDS;
                o[0] = i_from; o[1] = i_to; o[2] = k_from; o[3] = k_to; o[4] = re.x - rb.y; o[5] = nm; o[6] = ni; o[7] = nd;
            }
            found++;
            i = i_from - 1;
            more = !(rb.w & HMM_ROW_B_FROM_N);
        }
        if (pass == 0) { total = found; n_dom_out[pr.pair] = total; }
    }
}

// raw = GS_HMM_NO_SCORE, n_dom = 0 and zeroed slots for every pair; the pairs that are traced overwrite theirs
__global__ __launch_bounds__(256) void k_hmm_trace_fill(uint64_t n_pairs, uint64_t n_dom_words, int32_t *__restrict__ raw, uint32_t *__restrict__ n_dom, int32_t *__restrict__ dom)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_pairs) { raw[i] = GS_HMM_NO_SCORE; n_dom[i] = 0; }
    if (i < n_dom_words) dom[i] = 0;
}

// ---- Backward and posterior envelopes (SPEC 13.4) -------------------------------------------------------------------------------------------------
// The pairs of a block come as the trace's lists do (HmmTraceProf, HmmTracePair; ptr_off is not used): row_off is where the pair's L + 1 kept rows
// start, in the Forward rows {E[i], J[i], C[i], 0} (int4) and in the Backward rows {bN[i], bJ[i]} (int2) alike.
//   Backward walks the rows L .. 0. A row needs bM and bI of the row below only (bD of a row is a recurrence along descending k inside the row), so
//   lane l keeps those 2 Q words; residues are loaded 64 at a time from the record's end, lane t of a load holding the residue of step t. Row L
//   has no row below: it runs the same step with no node valid (every take = NEG) and bJ = bN = NEG. take of a lane's first node moves DOWN one
//   lane. The D scan is Forward's mirrored: each lane runs bD over its own nodes from its last one with nothing entering (Dloc), its group is the map
//   x -> lse(x + gsum, Dloc[first]), six steps of b = lse(b, b(lane + d) + a_d) with a select for the lanes that take no step, c_in from the lane
//   above, bD[q] = lse(Dloc[q], c_in + the sum of tDD from q to the group's end). Padding nodes hold NEG in bD and in take, so nothing of them
//   reaches node M; the transition rows are read from LDS in every row from Q = 12, as Forward reads them.
enum { HMM_ENV_BLOCK = 64, HMM_ENV_LO = -156, HMM_ENV_HI = -425 };
// 24 bytes a row: 768 MB of kept rows alive at once. A block is two launches per class and each ends with its longest record, so small blocks are
// paid for in tails: at 2^23 the 4 000 x 120 shape of DESIGN 3.24 ran 18 blocks and Forward with rows took 2.5 times the seconds of k_hmm_forward.
static constexpr uint64_t HMM_ENV_DEFAULT_BLOCK_ROWS = 1ull << 25;

// With N2 (SPEC 13.5) the rows are those of a segment: L of them under the length model of Lsp residues, bC from the segment's rows. No row is kept;
// at every row i >= 1 the lane reads M and I of the kept Forward row (keep: the lane's column, in the layout hmm_rows<HMM_FWD_SEG> wrote) and the
// specials of row i - 1 (fr) and advances the folds of fM + bM, fI + bI over its nodes and of the N, J and C emissions, which it hands back in occ.
// With ALI (SPEC 13.6) the rows are a segment's too and nothing is folded: at every row i >= 1 the posteriors pM = fM + bM - total and pI = fI + bI - total
// (64 bits, kept inside NEG .. 0; NEG for I of node M and for padding nodes) take the place of the kept fM and fI, and pX[i] goes to word 3 of the
// Forward row i, which Forward left 0 and which no later step reads (a step reads row i - 1). keep and fr are written through in this form alone.
template <int Q> struct HmmOcc { int32_t m[Q], i[Q], x; };
enum HmmBack { HMM_BACK_ROWS, HMM_BACK_N2, HMM_BACK_ALI };
template <int Q, HmmBack BK>
__device__ __forceinline__ int32_t hmm_back_rows(const HmmLane<Q> ln, const uint8_t *x, uint32_t L, uint32_t Lsp, int2 *rr, const int4 *fr, const int32_t *keep,
                                                 HmmOcc<Q> *occ, int32_t total = 0, uint32_t M = 0)
{
    constexpr int MP = 64 * Q;
    constexpr bool N2 = BK == HMM_BACK_N2, ALI = BK == HMM_BACK_ALI, KEPT = N2 || ALI;
    const uint16_t *T = ln.T;
    const int lane = ln.lane, nvalid = ln.nvalid;
    const HmmSpecials sp = hmm_specials(Lsp);
    int32_t oM[N2 ? Q : 1], oI[N2 ? Q : 1], oX = GS_HMM_NEG;
    if constexpr (N2) {
#pragma unroll
        for (int q = 0; q < Q; q++) oM[q] = oI[q] = GS_HMM_NEG;
    }
    const int32_t gsum = ln.PDD[Q - 1] + ln.tDD[Q - 1];       // the group's sum of tDD
    int32_t a_dn[6];                                          // a of the lanes a scan step joins: the sums of gsum over lanes l .. l + 2^s - 1
    {
        int32_t a = gsum;
        for (int s = 0; s < 6; s++) {
            a_dn[s] = a;
            const int32_t dn = __shfl_down(a, 1 << s);
            if (lane + (1 << s) < 64) a += dn;
        }
    }
    int32_t Mv[Q], Iv[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) Mv[q] = Iv[q] = GS_HMM_NEG;
    int32_t bJ = GS_HMM_NEG, bN = GS_HMM_NEG;
    bool bad = false;
    int res = 0;
    int nxt = (uint32_t)lane < L ? hmm_residue(x[L - 1 - (uint32_t)lane]) : 0;
    for (uint32_t s = 0; s <= L; s++) {                       // row i = L - s; step s >= 1 reads residue x_(i+1) = x[L - s]
        const uint32_t j = s - 1;
        if (s && (j & 63u) == 0) {
            bad |= nxt < 0;
            res = max(nxt, 0);
            const uint32_t at = j + 64 + (uint32_t)lane;      // the next 64 residues are on their way while these run
            nxt = at < L ? hmm_residue(x[L - 1 - at]) : 0;
        }
        if (Q >= 12) asm volatile("" ::: "memory");
        // N2: the kept Forward row of this step is asked for here and read at the step's end, so that the row's own work covers the loads; the step
        // of row 0 reads row 1 again and uses nothing of it
        int32_t kM[KEPT ? Q : 1], kI[KEPT ? Q : 1];
        int4 fp = make_int4(0, 0, 0, 0);
        if constexpr (KEPT) {
            const uint32_t row = s < L ? L - s - 1 : 0;
            const int32_t *kr = keep + (uint64_t)row * (2 * Q * 64);
#pragma unroll
            for (int q = 0; q < Q; q++) { kM[q] = kr[q * 64]; kI[q] = kr[(Q + q) * 64]; }
            fp = fr[row];
        }
        const int32_t *ms = ln.ms + (s ? __builtin_amdgcn_readlane(res, (int)(j & 63u)) : 0) * MP;
        const int nv = s ? nvalid : 0;
        int32_t take[Q], e = GS_HMM_NEG;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            take[q] = q < nv ? ms[q] + Mv[q] : GS_HMM_NEG;
            e = q < nv ? hmm_lse(e, take[q], T) : e;
        }
        const int32_t bB = hmm_wave_join<HMM_FWD>(e, T) + ln.tbm;
        const int32_t bC = (int32_t)s * sp.tloop + sp.tmove;
        if (s) {
            bJ = max(hmm_lse(bJ + sp.tloop, bB + sp.tmove, T), GS_HMM_NEG);
            bN = max(hmm_lse(bN + sp.tloop, bB + sp.tmove, T), GS_HMM_NEG);
        }
        const int32_t bE = hmm_lse(bJ + GS_HMM_TEJ, bC + GS_HMM_TEJ, T);
        if constexpr (BK == HMM_BACK_ROWS) if (lane == 0) rr[L - s] = make_int2(bN, bJ);
        int32_t dn = __shfl_down(take[0], 1);
        if (lane == 63) dn = GS_HMM_NEG;
        int32_t Dv[Q], dl = GS_HMM_NEG;
#pragma unroll
        for (int q = Q - 1; q >= 0; q--) {
            const int32_t c = hmm_lse(bE, (q + 1 < Q ? take[q + 1] : dn) + ln.tDM[q], T);
            dl = q == Q - 1 ? c : max(hmm_lse(c, dl + ln.tDD[q], T), GS_HMM_NEG);
            dl = q < nvalid ? dl : GS_HMM_NEG;
            Dv[q] = dl;
        }
        int32_t b = dl;
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const int32_t nb = hmm_lse(b, __shfl_down(b, 1 << t) + a_dn[t], T);
            b = lane + (1 << t) < 64 ? max(nb, GS_HMM_NEG) : b;
        }
        int32_t c_in = __shfl_down(b, 1);                     // bD of the next lane's first node
        if (lane == 63) c_in = GS_HMM_NEG;
#pragma unroll
        for (int q = 1; q < Q; q++) Dv[q] = max(hmm_lse(Dv[q], c_in + (gsum - ln.PDD[q]), T), GS_HMM_NEG);
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int32_t tk = q + 1 < Q ? take[q + 1] : dn, dnext = q + 1 < Q ? Dv[q + 1] : c_in;
            const int32_t m = hmm_lse(hmm_lse(hmm_lse(bE, tk + ln.tMM[q], T), Iv[q] + ln.tMI[q], T), dnext + ln.tMD[q], T);
            Iv[q] = max(hmm_lse(tk + ln.tIM[q], Iv[q] + ln.tII[q], T), GS_HMM_NEG);
            Mv[q] = max(m, GS_HMM_NEG);
        }
        if constexpr (N2) if (s < L) {                        // rows L .. 1, in this order (SPEC 13.5)
            const uint32_t i = L - s;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                oM[q] = hmm_lse(oM[q], kM[q] + Mv[q], T);
                oI[q] = hmm_lse(oI[q], kI[q] + Iv[q], T);
            }
            oX = hmm_lse(oX, hmm_lse(hmm_lse((int32_t)i * sp.tloop + bN, fp.y + sp.tloop + bJ, T), fp.z + sp.tloop + bC, T), T);
        }
        if constexpr (ALI) if (s < L) {                       // rows L .. 1: the posteriors in the place of the kept Forward cells (SPEC 13.6)
            const uint32_t i = L - s;
            const int nvi = min(max((int)M - 1 - lane * Q, 0), Q);
            int32_t *kw = const_cast<int32_t *>(keep) + (uint64_t)(i - 1) * (2 * Q * 64);
            auto post = [&](int64_t v) { return (int32_t)min(max(v - total, (int64_t)GS_HMM_NEG), (int64_t)0); };
#pragma unroll
            for (int q = 0; q < Q; q++) {
                kw[q * 64] = q < nvalid ? post((int64_t)kM[q] + Mv[q]) : GS_HMM_NEG;
                kw[(Q + q) * 64] = q < nvi ? post((int64_t)kI[q] + Iv[q]) : GS_HMM_NEG;
            }
            const int32_t xn = hmm_lse(hmm_lse((int32_t)i * sp.tloop + bN, fp.y + sp.tloop + bJ, T), fp.z + sp.tloop + bC, T);
            if (lane == 0) ((int32_t *)const_cast<int4 *>(fr + i))[3] = post(xn);
        }
    }
    if constexpr (N2) {
#pragma unroll
        for (int q = 0; q < Q; q++) { occ->m[q] = oM[q]; occ->i[q] = oI[q]; }
        occ->x = oX;
    }
    return __any(bad) ? GS_HMM_NO_SCORE : bN - sp.null;
}

// The end of a segment's Backward (SPEC 13.5): the folds become log2 of expected usage (minus total, floor NEG), 22 joins over the wavefront give ii, the
// mass word and n2[a] of the 20 residues (lane a keeps n2[a]), and corr is the exact 64-bit sum of n2[x_i] over the segment, lanes striding its residues.
// slot: {corr, dom_bias, seg_raw, mass}, of which seg_raw is Forward's; n2_out, occm, occi: optional (occm and occi together).
enum { HMM_N2_OMEGA = -8192, HMM_N2_CORR_MAX = 1 << 30, HMM_N2_DEFAULT_BLOCK_CELLS = 1 << 26 };
template <int Q>
__device__ __forceinline__ void hmm_n2_finish(const HmmLane<Q> ln, const HmmOcc<Q> &o, int32_t total, const uint8_t *x, uint32_t Ld, uint32_t M, int32_t *slot,
                                              int32_t *n2_out, int32_t *occm, int32_t *occi)
{
    constexpr int MP = 64 * Q;
    const uint16_t *T = ln.T;
    const int lane = ln.lane, nvalid = ln.nvalid;
    const int nvi = min(max((int)M - 1 - lane * Q, 0), Q);    // the lane's nodes k < M: I of node M and of padding nodes holds mass that no path carries
    int32_t om[Q], oi[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        om[q] = (int32_t)max((int64_t)o.m[q] - total, (int64_t)GS_HMM_NEG);
        oi[q] = (int32_t)max((int64_t)o.i[q] - total, (int64_t)GS_HMM_NEG);
    }
    const int32_t ox = (int32_t)max((int64_t)o.x - total, (int64_t)GS_HMM_NEG);
    int32_t e = GS_HMM_NEG;
#pragma unroll
    for (int q = 0; q < Q; q++) e = q < nvi ? hmm_lse(e, oi[q], T) : e;
    const int32_t ii = hmm_wave_join<HMM_FWD>(e, T);
    e = GS_HMM_NEG;
#pragma unroll
    for (int q = 0; q < Q; q++) e = q < nvalid ? hmm_lse(e, om[q], T) : e;
    const int32_t lgd = hmm_units_log(Ld, 1);
    const int32_t mass = hmm_lse(hmm_lse(hmm_wave_join<HMM_FWD>(e, T), ii, T), ox, T) - lgd;
    int32_t mine = 0;
#pragma unroll 1
    for (int a = 0; a < 20; a++) {
        const int32_t *ms = ln.ms + a * MP;
        e = GS_HMM_NEG;
#pragma unroll
        for (int q = 0; q < Q; q++) e = q < nvalid ? hmm_lse(e, om[q] + ms[q], T) : e;
        const int32_t v = hmm_lse(hmm_lse(hmm_wave_join<HMM_FWD>(e, T), ii, T), ox, T) - lgd;
        if (lane == a) mine = v;
    }
    int64_t sum = 0;
    for (uint32_t i0 = 0; i0 < Ld; i0 += 64) {                // every lane takes every trip: the shuffle reads lanes 0 .. 19
        const uint32_t i = i0 + (uint32_t)lane;
        const int r = i < Ld ? max(hmm_residue(x[i]), 0) : 0;
        const int32_t v = __shfl(mine, r);
        sum += i < Ld ? v : 0;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
    const int32_t corr = (int32_t)min(max(sum, -(int64_t)HMM_N2_CORR_MAX), (int64_t)HMM_N2_CORR_MAX);
    if (lane == 0) { slot[0] = corr; slot[1] = hmm_lse(0, HMM_N2_OMEGA + corr, T); slot[3] = mass; }
    if (n2_out && lane < 20) n2_out[lane] = mine;
    if (occm) {
#pragma unroll
        for (int q = 0; q < Q; q++)
            if (q < nvalid) { occm[lane * Q + q] = om[q]; occi[lane * Q + q] = q < nvi ? oi[q] : GS_HMM_NEG; }
    }
}

// Forward score and the rows {E[i], J[i], C[i]} of the pairs of each profile of profs[]; 1 <= L <= GS_HMM_FWD_MAX_L: the host put no other pair on a list
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_forward_rows(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                                const HmmTracePair *__restrict__ pairs, const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa,
                                                                const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len, int4 *__restrict__ rows,
                                                                int32_t *__restrict__ fwd_out)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, desc[tp.prof], lse_tab);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const int32_t raw = hmm_rows<Q, HMM_FWD_ROWS>(ln, aa + rec_start[pr.rec], (uint32_t)rec_len[pr.rec], (uint32_t)rec_len[pr.rec], nullptr, rows + pr.row_off);
        if (ln.lane == 0) fwd_out[pr.pair] = raw;
    }
}

// Backward score bN[0] - null and the rows {bN[i], bJ[i]} of the same lists
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_backward(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                            const HmmTracePair *__restrict__ pairs, const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa,
                                                            const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len, int2 *__restrict__ rows,
                                                            int32_t *__restrict__ bck_out)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, desc[tp.prof], lse_tab);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const int32_t raw = hmm_back_rows<Q, HMM_BACK_ROWS>(ln, aa + rec_start[pr.rec], (uint32_t)rec_len[pr.rec], (uint32_t)rec_len[pr.rec], rows + pr.row_off, nullptr, nullptr, nullptr);
        if (ln.lane == 0) bck_out[pr.pair] = raw;
    }
}

// Occupancy, runs and envelopes of SPEC 13.4, one wavefront per pair of the block: the lanes form out / exit / cont of 64 rows at a time from the kept
// rows (T is read from device memory here: five look-ups a row), a ballot gives which rows are in and which continue, and the run rule walks the 64
// bits on the scalar side. Writes n_env (the true count) and i_from, i_to, 0, peak of the first max_env envelopes; k_hmm_env_score fills the third
// word. A pair whose Forward raw is GS_HMM_NO_SCORE keeps what the fill wrote.
__global__ __launch_bounds__(HMM_ENV_BLOCK) void k_hmm_envelopes(const HmmTracePair *__restrict__ pairs, const uint64_t *__restrict__ rec_len, const uint16_t *__restrict__ T,
                                                                 const int4 *__restrict__ frows, const int2 *__restrict__ brows, const int32_t *__restrict__ fwd,
                                                                 uint32_t max_env, uint32_t *__restrict__ n_env_out, int32_t *__restrict__ env_out,
                                                                 const uint64_t *__restrict__ row_off, int32_t *__restrict__ out_rows, int32_t *__restrict__ cont_rows)
{
    const HmmTracePair pr = pairs[blockIdx.x];
    if (fwd[pr.pair] == GS_HMM_NO_SCORE) return;
    const uint32_t L = (uint32_t)rec_len[pr.rec], lane = threadIdx.x;
    const HmmSpecials sp = hmm_specials(L);
    const int4 *f = frows + pr.row_off;
    const int2 *bk = brows + pr.row_off;
    const int32_t total_f = f[L].z + sp.tmove;
    int32_t *env = env_out + (uint64_t)pr.pair * max_env * GS_HMM_ENV_WORDS;
    const uint64_t ro = row_off ? row_off[pr.pair] : 0;
    uint32_t n = 0, a = 0;
    int32_t peak = 0;
    bool open = false, prev_ct = false;
    auto close = [&](uint32_t last) {
        if (peak <= HMM_ENV_HI) {
            if (n < max_env && lane == 0) { int32_t *o = env + (uint64_t)n * GS_HMM_ENV_WORDS; o[0] = (int32_t)a; o[1] = (int32_t)last; o[2] = 0; o[3] = peak; }
            n++;
        }
        open = false;
    };
    for (uint32_t i0 = 1; i0 <= L; i0 += 64) {
        const uint32_t i = i0 + lane;
        int32_t out = 0, cont = 0;
        if (i <= L) {
            const int4 fp = f[i - 1];
            const int2 b = bk[i];
            const int32_t bC = (int32_t)(L - i) * sp.tloop + sp.tmove;
            out = hmm_lse(hmm_lse((int32_t)i * sp.tloop + b.x, fp.y + sp.tloop + b.y, T), fp.z + sp.tloop + bC, T) - total_f;
            const int32_t ex = f[i].x + hmm_lse(b.y + GS_HMM_TEJ, bC + GS_HMM_TEJ, T) - total_f;
            cont = hmm_lse(out, ex, T);
            if (out_rows) { out_rows[ro + i - 1] = out; cont_rows[ro + i - 1] = cont; }
        }
        const uint64_t inm = __ballot(i <= L && out <= HMM_ENV_LO), ctm = __ballot(cont <= HMM_ENV_LO);
        const int cnt = (int)min(64u, L - i0 + 1);
        for (int t = 0; t < cnt; t++) {
            const bool in_t = (inm >> t) & 1;
            if (open && !(in_t && prev_ct)) close(i0 + (uint32_t)t - 1);
            if (in_t) {
                const int32_t o = __builtin_amdgcn_readlane(out, t);
                if (!open) { open = true; a = i0 + (uint32_t)t; peak = o; } else peak = min(peak, o);
            }
            prev_ct = (ctm >> t) & 1;
        }
    }
    if (open) close(L);
    if (lane == 0) n_env_out[pr.pair] = n;
}

// env_raw of the listed envelopes: Forward over the rows i_from .. i_to of the record under the length model of the whole record. The slots of the pairs
// of a profile are consecutive, so a workgroup stages the profile once and its wavefronts take the written slots in turn.
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_env_score(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                             const HmmTracePair *__restrict__ pairs, const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa,
                                                             const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len, uint32_t max_env,
                                                             const uint32_t *__restrict__ n_env, int32_t *env_out)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    const uint64_t slots = (uint64_t)tp.cnt * max_env;
    if ((uint64_t)blockIdx.x * HMM_WAVES >= slots) return;
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, desc[tp.prof], lse_tab);
    for (uint64_t j = (uint64_t)blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < slots; j += (uint64_t)gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + (uint32_t)(j / max_env)];
        const uint32_t e = (uint32_t)(j % max_env);
        if (e >= n_env[pr.pair]) continue;
        int32_t *o = env_out + ((uint64_t)pr.pair * max_env + e) * GS_HMM_ENV_WORDS;
        const uint32_t L = (uint32_t)rec_len[pr.rec], from = (uint32_t)o[0], Ld = (uint32_t)o[1] - from + 1;
        const int32_t raw = hmm_rows<Q, HMM_FWD>(ln, aa + rec_start[pr.rec] + (from - 1), Ld, L, nullptr, nullptr);
        if (ln.lane == 0) o[2] = raw + (int32_t)(L - Ld) * hmm_specials(L).tloop;
    }
}

// fwd = bck = GS_HMM_NO_SCORE, n_env = 0 and zeroed slots for every pair; the pairs that are listed overwrite theirs
__global__ __launch_bounds__(256) void k_hmm_env_fill(uint64_t n_pairs, uint64_t n_env_words, int32_t *__restrict__ fwd, int32_t *__restrict__ bck, uint32_t *__restrict__ n_env,
                                                      int32_t *__restrict__ env)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_pairs) { fwd[i] = GS_HMM_NO_SCORE; bck[i] = GS_HMM_NO_SCORE; n_env[i] = 0; }
    if (i < n_env_words) env[i] = 0;
}

// ---- null2 (SPEC 13.5): the bias correction of envelope and sequence scores --------------------------------------------------------------------------
// The unit of work is a listed envelope (a slot of its pair), one wavefront each. The blocks' lists are the trace's with a slot in the place of a pair:
// HmmTracePair::pair numbers the call's slots (HmmN2Slot), ptr_off is where the slot's kept M and I words start (2 * 64 Q * Ld of them), row_off where its
// Ld + 1 Forward rows {E, J, C, 0} start.
struct HmmN2Slot { uint64_t occ_at; uint32_t pair, e, rec, from, Ld, pad; };          // occ_at: the first word of the slot's occM / occI row
struct HmmN2Pair { uint32_t rec, listed; };                                           // listed = min(n_env, max_env)

// per pair of the call: 1 iff it has a record of at least one residue and every byte of it is a residue
__global__ __launch_bounds__(64) void k_hmm_n2_flag(const HmmN2Pair *__restrict__ np, const uint8_t *__restrict__ aa, const uint64_t *__restrict__ rec_start,
                                                    const uint64_t *__restrict__ rec_len, uint32_t *__restrict__ ok)
{
    const uint32_t rec = np[blockIdx.x].rec;
    bool bad = rec == GS_HMM_NO_HIT;
    if (!bad) {
        const uint64_t L = rec_len[rec];
        const uint8_t *x = aa + rec_start[rec];
        bad = L == 0;
        for (uint64_t i = threadIdx.x; i < L; i += 64) bad |= hmm_residue(x[i]) < 0;
    }
    const bool any_bad = __any(bad);
    if (threadIdx.x == 0) ok[blockIdx.x] = any_bad ? 0u : 1u;
}

// zeros in every output a pair may go without
__global__ __launch_bounds__(256) void k_hmm_n2_fill(uint64_t n_slot_words, uint64_t n_pairs, uint64_t n_n2_words, int32_t *__restrict__ slot, int32_t *__restrict__ seq,
                                                     int32_t *__restrict__ n2)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_slot_words) slot[i] = 0;
    if (i < n_pairs) seq[i] = 0;
    if (n2 && i < n_n2_words) n2[i] = 0;
}

// Forward over the slots of each profile of profs[], M and I of every row kept; writes seg_raw
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_n2_forward(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                              const HmmTracePair *__restrict__ pairs, const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa,
                                                              const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                              const HmmN2Slot *__restrict__ slots, const uint32_t *__restrict__ ok, uint32_t max_env, int4 *rows,
                                                              uint32_t *keep, int32_t *slot_out)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, desc[tp.prof], lse_tab);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const HmmN2Slot sl = slots[pr.pair];
        if (!ok[sl.pair]) continue;
        const uint32_t L = (uint32_t)rec_len[sl.rec];
        const int32_t raw = hmm_rows<Q, HMM_FWD_SEG>(ln, aa + rec_start[sl.rec] + (sl.from - 1), sl.Ld, L, keep + pr.ptr_off + ln.lane, rows + pr.row_off);
        if (ln.lane == 0) slot_out[((uint64_t)sl.pair * max_env + sl.e) * GS_HMM_N2_WORDS + 2] = raw + (int32_t)(L - sl.Ld) * hmm_specials(L).tloop;
    }
}

// Backward over the same slots with the folds of SPEC 13.5 beside the row, then n2, mass and corr
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_n2_backward(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                               const HmmTracePair *__restrict__ pairs, const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa,
                                                               const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                               const HmmN2Slot *__restrict__ slots, const uint32_t *__restrict__ ok, uint32_t max_env,
                                                               const int4 *__restrict__ rows, const uint32_t *__restrict__ keep, int32_t *slot_out, int32_t *n2_out,
                                                               int32_t *occm_out, int32_t *occi_out)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmDesc d = desc[tp.prof];
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, d, lse_tab);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const HmmN2Slot sl = slots[pr.pair];
        if (!ok[sl.pair]) continue;
        const uint32_t L = (uint32_t)rec_len[sl.rec];
        const uint8_t *x = aa + rec_start[sl.rec] + (sl.from - 1);
        const int4 *fr = rows + pr.row_off;
        HmmOcc<Q> occ;
        (void)hmm_back_rows<Q, HMM_BACK_N2>(ln, x, sl.Ld, L, nullptr, fr, (const int32_t *)keep + pr.ptr_off + ln.lane, &occ);
        const uint64_t at = (uint64_t)sl.pair * max_env + sl.e;
        hmm_n2_finish<Q>(ln, occ, fr[sl.Ld].z + hmm_specials(L).tmove, x, sl.Ld, d.M, slot_out + at * GS_HMM_N2_WORDS, n2_out ? n2_out + at * 20 : nullptr,
                         occm_out ? occm_out + sl.occ_at : nullptr, occm_out ? occi_out + sl.occ_at : nullptr);
    }
}

// seq_bias of every pair that has a score: lse(0, OMEGA + the clamped sum of corr over its listed slots)
__global__ __launch_bounds__(256) void k_hmm_n2_seq(const HmmN2Pair *__restrict__ np, const uint32_t *__restrict__ ok, uint64_t n_pairs, uint32_t max_env,
                                                    const uint16_t *__restrict__ T, const int32_t *__restrict__ slot, int32_t *__restrict__ seq)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pairs || !ok[j]) return;
    int64_t sum = 0;
    for (uint32_t e = 0; e < np[j].listed; e++) sum += slot[(j * max_env + e) * GS_HMM_N2_WORDS];
    const int32_t corr = (int32_t)min(max(sum, -(int64_t)HMM_N2_CORR_MAX), (int64_t)HMM_N2_CORR_MAX);
    seq[j] = hmm_lse(0, HMM_N2_OMEGA + corr, T);
}

// ---- optimal-accuracy alignment (SPEC 13.6): one alignment of every listed envelope ------------------------------------------------------------------
// The unit of work and the blocks' lists are null2's (HmmN2Slot, HmmTracePair): k_hmm_n2_forward keeps fM and fI of a slot, k_hmm_ali_backward turns them
// into pM and pI in place and leaves pX[i] in word 3 of the Forward row i, k_hmm_ali_rows runs the max-plus program of SPEC 13.6 over them with the trace's
// nibbles (HMM_PTR_B and the bit meanings of SPEC 13.2) and a row record {lowest k of A_E[i], C[i] came from E[i]}, k_hmm_ali_walk follows them.
//   A cell's weight is w(p) = EXP2[-p & 1023] >> (-p >> 10), Q16, from the 1 024 words of EXP2 in LDS; a transition counts 0 (its table word > STAR) or
//   OFF, eight rows of such masks in LDS: the seven transition rows and, in the place of PDD, the minimum of the tDD masks in front of a node inside its
//   lane's group. A chain of masks counts by its minimum, so the scan's a of SPEC 13 (a sum of tDD) is a minimum here. Every stored value is at least OFF
//   and one step adds at most one OFF to it, so nothing leaves int32; a reachable value is >= 0 and below 2^29 (Ld <= 8 192 weights of at most 2^16),
//   and a value that a disallowed link or an unreachable cell feeds stays below 0: the walk starts at oa >= 0 and reads reachable cells only.
enum { HMM_ALI_OFF = -(1 << 30), HMM_ALI_MASK_ROWS = 8, HMM_ALI_ROW_PDD = 7, HMM_ALI_C_FROM_E = 1 };
static_assert(HMM_ROW_DD - HMM_ROW_MM == 6 && HMM_ROW_PDD == HMM_ROW_MM + HMM_ALI_ROW_PDD, "the seven transition rows lie together, PDD behind them");
static_assert((int64_t)GS_HMM_ALI_MAX_LD * 65536 <= (1ll << 29), "a reachable value stays below 2^29, so OFF plus every weight of a segment stays below 0");
struct HmmAliSlot { uint64_t nib_off, col_at; };        // where the slot's nibble words start in the block's scratch; its first column of col_out
__device__ __forceinline__ int32_t hmm_ali_w(int32_t p, const uint32_t *__restrict__ EX)
{
    const uint32_t n = (uint32_t)(-p);                        // 0 .. 2^29
    return (int32_t)(EX[n & 1023u] >> min(n >> 10, 31u));     // EXP2 <= 2^16, so a shift of 17 or more gives the 0 of SPEC 13.6
}

// zeros in every slot word
__global__ __launch_bounds__(256) void k_hmm_ali_fill(uint64_t n_slot_words, int32_t *__restrict__ slot)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_slot_words) slot[i] = 0;
}

// Backward over the slots of each profile of profs[]: pM, pI in the place of the kept fM, fI, pX in the Forward rows
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_ali_backward(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                                const HmmTracePair *__restrict__ pairs, const uint16_t *__restrict__ lse_tab, const uint8_t *__restrict__ aa,
                                                                const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len,
                                                                const HmmN2Slot *__restrict__ slots, const uint32_t *__restrict__ ok, int4 *rows, uint32_t *keep)
{
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmDesc d = desc[tp.prof];
    const HmmLane<Q> ln = hmm_stage<Q, true>(tables, d, lse_tab);
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)ln.wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const HmmN2Slot sl = slots[pr.pair];
        if (!ok[sl.pair]) continue;
        const uint32_t L = (uint32_t)rec_len[sl.rec];
        const int4 *fr = rows + pr.row_off;
        (void)hmm_back_rows<Q, HMM_BACK_ALI>(ln, aa + rec_start[sl.rec] + (sl.from - 1), sl.Ld, L, nullptr, fr, (const int32_t *)keep + pr.ptr_off + ln.lane, nullptr,
                                             fr[sl.Ld].z + hmm_specials(L).tmove, d.M);
    }
}

// The program of SPEC 13.6 over the posteriors of each slot, one wavefront a slot: nibbles, row records and oa (word 4 of the slot). The lane layout, the
// D scan and the pointer decisions are hmm_rows<HMM_TRACE>'s with masks for transition scores and a weight per cell for the match score; the next row's
// posteriors are asked for before the current row's work, as hmm_back_rows asks for its kept row.
template <int Q>
__global__ __launch_bounds__(HMM_BLOCK) void k_hmm_ali_rows(const int32_t *__restrict__ tables, const HmmDesc *__restrict__ desc, const HmmTraceProf *__restrict__ profs,
                                                            const HmmTracePair *__restrict__ pairs, const uint32_t *__restrict__ exp2_tab,
                                                            const HmmN2Slot *__restrict__ slots, const HmmAliSlot *__restrict__ aslots, const uint32_t *__restrict__ ok,
                                                            uint32_t max_env, const int4 *__restrict__ rows, const int32_t *__restrict__ keep, uint32_t *__restrict__ ptrs,
                                                            int2 *__restrict__ arows, int32_t *__restrict__ slot_out)
{
    extern __shared__ int32_t hmm_ali_lds[];
    constexpr int MP = 64 * Q, NW = hmm_ptr_words(Q), OFF = HMM_ALI_OFF;
    const HmmTraceProf tp = profs[blockIdx.y];
    if ((uint64_t)blockIdx.x * HMM_WAVES >= tp.cnt) return;
    const HmmDesc d = desc[tp.prof];
    uint32_t *EX = (uint32_t *)(hmm_ali_lds + HMM_ALI_MASK_ROWS * MP);
    for (int i = (int)threadIdx.x; i < HMM_ALI_ROW_PDD * MP; i += HMM_BLOCK) hmm_ali_lds[i] = tables[d.off + HMM_ROW_MM * MP + i] > GS_HMM_STAR ? 0 : OFF;
    for (int i = (int)threadIdx.x; i < (int)GS_HMM_EXP2_N; i += HMM_BLOCK) EX[i] = exp2_tab[i];
    __syncthreads();
    for (int j = (int)threadIdx.x; j < MP; j += HMM_BLOCK) {
        int32_t m = 0;
        for (int t = j - j % Q; t < j; t++) m = min(m, hmm_ali_lds[(HMM_ROW_DD - HMM_ROW_MM) * MP + t]);
        hmm_ali_lds[HMM_ALI_ROW_PDD * MP + j] = m;
    }
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, base = lane * Q;
    const int nvalid = min(max((int)d.M - base, 0), Q);
    const int32_t *mMM = hmm_ali_lds + base, *mMI = mMM + MP, *mMD = mMI + MP, *mIM = mMD + MP, *mII = mIM + MP, *mDM = mII + MP, *mDD = mDM + MP, *mPDD = mDD + MP;
    int32_t a_step[6];                                        // the masks of the lanes a scan step joins: the minimum of the groups' chains
    {
        int32_t a = min(mPDD[Q - 1], mDD[Q - 1]);
        for (int s = 0; s < 6; s++) {
            a_step[s] = a;
            const int32_t up = __shfl_up(a, 1 << s);
            if (lane >= (1 << s)) a = min(a, up);
        }
    }
    for (uint32_t j = blockIdx.x * HMM_WAVES + (uint32_t)wave; j < tp.cnt; j += gridDim.x * HMM_WAVES) {
        const HmmTracePair pr = pairs[tp.start + j];
        const HmmN2Slot sl = slots[pr.pair];
        if (!ok[sl.pair]) continue;
        const uint32_t Ld = sl.Ld;
        const int4 *fr = rows + pr.row_off;
        const int32_t *kp = keep + pr.ptr_off + lane;
        uint32_t *pp = ptrs + aslots[pr.pair].nib_off + lane;
        int2 *ar = arows + pr.row_off;
        int32_t Mv[Q], Iv[Q], Dv[Q], nM[Q], nI[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) { Mv[q] = Iv[q] = Dv[q] = OFF; nM[q] = kp[q * 64]; nI[q] = kp[(Q + q) * 64]; }
        int32_t nX = fr[1].w, N = 0, C = OFF;
        for (uint32_t row = 0; row < Ld; row++) {             // row i = row + 1
            if (Q >= 12) asm volatile("" ::: "memory");
            int32_t wM[Q], wI[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) { wM[q] = hmm_ali_w(nM[q], EX); wI[q] = hmm_ali_w(nI[q], EX); }
            const int32_t wX = hmm_ali_w(nX, EX);
            {                                                 // the next row is on its way while this one runs; the last row asks for itself again
                const uint32_t nr = min(row + 1, Ld - 1);
                const int32_t *kr = kp + (uint64_t)nr * (2 * Q * 64);
#pragma unroll
                for (int q = 0; q < Q; q++) { nM[q] = kr[q * 64]; nI[q] = kr[(Q + q) * 64]; }
                nX = fr[nr + 1].w;
            }
            const int32_t entry = N;                          // A_B[i-1] = A_N[i-1] >= 0
            uint32_t pk[NW], code_out = HMM_PTR_B;
#pragma unroll
            for (int w = 0; w < NW; w++) pk[w] = 0;
            int32_t give[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int32_t a = Mv[q] + mMM[q], b = Iv[q] + mIM[q], c = Dv[q] + mDM[q];
                const int32_t g = max(max(a, b), c);
                give[q] = g;
                const uint32_t code = g >= entry ? (a == g ? 0u : (b == g ? 1u : 2u)) : (uint32_t)HMM_PTR_B;
                if (q + 1 < Q) pk[(q + 1) >> 3] |= code << (4 * ((q + 1) & 7)); else code_out = code;
            }
            int32_t up = __shfl_up(give[Q - 1], 1);
            if (lane == 0) up = OFF;                          // node 0 has no states
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int32_t fromM = Mv[q] + mMI[q], v = max(fromM, Iv[q] + mII[q]);
                pk[q >> 3] |= (fromM == v ? 0u : 4u) << (4 * (q & 7));
                Iv[q] = max(wI[q] + v, OFF);
            }
#pragma unroll
            for (int q = 0; q < Q; q++) Mv[q] = wM[q] + max(q ? give[q - 1] : up, entry);      // >= 0: the entry is
            int32_t dl = OFF;
            Dv[0] = dl;
#pragma unroll
            for (int q = 1; q < Q; q++) { dl = max(max(dl + mDD[q - 1], Mv[q - 1] + mMD[q - 1]), OFF); Dv[q] = dl; }
            const int32_t m_out = Mv[Q - 1] + mMD[Q - 1];
            int32_t b = max(max(dl + mDD[Q - 1], m_out), OFF);
#pragma unroll
            for (int s = 0; s < 6; s++) b = max(b, __shfl_up(b, 1 << s) + a_step[s]);          // a lane below 2^s gets its own b back: b + a <= b
            int32_t c_in = __shfl_up(b, 1);
            if (lane == 0) c_in = OFF;
            {
                uint32_t edge = (uint32_t)__shfl_up((int)(code_out | (m_out == b ? 0u : 8u)), 1);
                if (lane == 0) edge = HMM_PTR_B | 8u;
                pk[0] |= edge;
            }
            int32_t e = OFF;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                Dv[q] = max(Dv[q], c_in + mPDD[q]);
                if (q >= 1) pk[q >> 3] |= (Mv[q - 1] + mMD[q - 1] == Dv[q] ? 0u : 8u) << (4 * (q & 7));
                e = q < nvalid ? max(e, Mv[q]) : e;
            }
            const int32_t E = hmm_wave_join<HMM_VIT>(e, nullptr);
#pragma unroll
            for (int w = 0; w < NW; w++) pp[((uint64_t)row * NW + w) * 64] = pk[w];
            int first = 0;
#pragma unroll
            for (int q = Q - 1; q >= 0; q--) if (q < nvalid && Mv[q] == E) first = q;
            const int fl = __ffsll((unsigned long long)__ballot(e == E)) - 1;                 // some lane holds it: E is the maximum of the e
            const int kE = fl * Q + __builtin_amdgcn_readlane(first, fl) + 1;
            N += wX;
            C = max(C + wX, E);
            if (lane == 0) ar[row + 1] = make_int2(kE, C == E ? HMM_ALI_C_FROM_E : 0);
        }
        if (lane == 0) slot_out[((uint64_t)sl.pair * max_env + sl.e) * GS_HMM_ALI_WORDS + 4] = C;
    }
}

// The walk of SPEC 13.6, one lane per slot of the block: from C[Ld] back to the row it left E in, then the cells of the one domain down to its B -> M
// entry. The first pass counts, the second writes the columns from the last one down, so they lie in forward order. Every step lowers i or k: a walk
// ends after at most Ld + M steps whatever the scratch holds, and a slot owns Ld + M columns.
__global__ __launch_bounds__(HMM_WALK_BLOCK) void k_hmm_ali_walk(const HmmDesc *__restrict__ desc, const HmmTracePair *__restrict__ pairs, uint32_t n,
                                                                 const uint32_t *__restrict__ pair_prof, const HmmN2Slot *__restrict__ slots,
                                                                 const HmmAliSlot *__restrict__ aslots, const uint32_t *__restrict__ ok, uint32_t max_env,
                                                                 const uint32_t *__restrict__ ptrs, const int2 *__restrict__ arows, const int32_t *__restrict__ keep,
                                                                 int32_t *__restrict__ slot_out, int32_t *__restrict__ col_out)
{
    const uint32_t t = blockIdx.x * HMM_WALK_BLOCK + threadIdx.x;
    if (t >= n) return;
    const HmmTracePair pr = pairs[t];
    const HmmN2Slot sl = slots[pr.pair];
    if (!ok[sl.pair]) return;
    const HmmAliSlot as = aslots[pr.pair];
    const int M = (int)desc[pair_prof[sl.pair]].M;
    const int Q = hmm_q_of((uint32_t)M), NW = hmm_ptr_words(Q);
    const uint32_t *pp = ptrs + as.nib_off;
    const int2 *ar = arows + pr.row_off;
    const int32_t *kp = keep + pr.ptr_off;
    int i_to = (int)sl.Ld;
    while (i_to > 1 && !(ar[i_to].y & HMM_ALI_C_FROM_E)) i_to--;
    const int k_to = min(max(ar[i_to].x, 1), M);
    int32_t *o = slot_out + ((uint64_t)sl.pair * max_env + sl.e) * GS_HMM_ALI_WORDS;
    uint32_t total = 0;
    for (int pass = 0; pass < (col_out ? 2 : 1); pass++) {
        int i = i_to, k = k_to, st = 0, nm = 0, ni = 0, nd = 0, i_from = 0, k_from = 0;
        uint32_t at = total;
        while (i >= 1 && k >= 1) {
            const int node = k - 1, ln = node / Q, q = node - ln * Q;
            const uint32_t nb = (pp[((uint64_t)(i - 1) * NW + (q >> 3)) * 64 + ln] >> (4 * (q & 7))) & 15u;
            if (pass == 1 && at) {
                at--;
                int32_t *c = col_out + (as.col_at + at) * 2;
                c[0] = (int32_t)((uint32_t)st << 28 | (uint32_t)k << 16 | (sl.from + (uint32_t)i - 2));
                c[1] = st == 2 ? 0 : kp[((uint64_t)(i - 1) * (2 * Q) + (st ? Q : 0) + q) * 64 + ln];
            }
            if (st == 0) {
                nm++;
                const uint32_t from = nb & 3u;
                if (from == HMM_PTR_B || i == 1 || k == 1) { i_from = i; k_from = k; break; }
                st = (int)from; i--; k--;
            } else if (st == 1) {
                ni++;
                st = nb & 4u ? 1 : 0; i--;
            } else {
                nd++;
                st = nb & 8u ? 2 : 0; k--;
            }
        }
        if (!i_from) return;                                    // not a path: only scratch that no row kernel wrote leads here
        if (pass == 0) {
            total = (uint32_t)(nm + ni + nd);
            o[0] = (int32_t)sl.from + i_from - 1; o[1] = (int32_t)sl.from + i_to - 1; o[2] = k_from; o[3] = k_to; o[5] = nm; o[6] = ni; o[7] = nd;
        }
    }
}

// the instances of a class, from the one class list
struct HmmKernels {
    decltype(&k_hmm_viterbi<1>) vit; decltype(&k_hmm_forward<1>) fwd; decltype(&k_hmm_trace<1>) trace; decltype(&k_hmm_msv<1>) msv; decltype(&k_hmm_viterbi_sel<1>) vit_sel;
    decltype(&k_hmm_forward_rows<1>) fwd_rows; decltype(&k_hmm_backward<1>) back; decltype(&k_hmm_env_score<1>) env_score;
    decltype(&k_hmm_n2_forward<1>) n2_fwd; decltype(&k_hmm_n2_backward<1>) n2_back; decltype(&k_hmm_ali_backward<1>) ali_back; decltype(&k_hmm_ali_rows<1>) ali_rows;
    decltype(&k_hmm_vit16<1>) vit16; decltype(&k_hmm_vit16_sel<1>) vit16_sel;      // (instances by registers a state: two classes can share one)
};
template <size_t... I> static const HmmKernels &hmm_kernels(int cls, std::index_sequence<I...>)
{
    static const HmmKernels of_class[] = {{k_hmm_viterbi<HMM_CLASS_Q[I]>, k_hmm_forward<HMM_CLASS_Q[I]>, k_hmm_trace<HMM_CLASS_Q[I]>, k_hmm_msv<HMM_CLASS_Q[I]>,
                                           k_hmm_viterbi_sel<HMM_CLASS_Q[I]>, k_hmm_forward_rows<HMM_CLASS_Q[I]>, k_hmm_backward<HMM_CLASS_Q[I]>,
                                           k_hmm_env_score<HMM_CLASS_Q[I]>, k_hmm_n2_forward<HMM_CLASS_Q[I]>, k_hmm_n2_backward<HMM_CLASS_Q[I]>,
                                           k_hmm_ali_backward<HMM_CLASS_Q[I]>, k_hmm_ali_rows<HMM_CLASS_Q[I]>,
                                           k_hmm_vit16<hmm16_regs(HMM_CLASS_Q[I])>, k_hmm_vit16_sel<hmm16_regs(HMM_CLASS_Q[I])>}...};
    return of_class[cls];
}
static const HmmKernels &hmm_kernels(int cls) { return hmm_kernels(cls, std::make_index_sequence<HMM_CLASSES>()); }
static size_t hmm_lds_bytes(int cls, HmmProg prog) { return (size_t)HMM_ROWS_DEV * 64 * HMM_CLASS_Q[cls] * 4 + (prog == HMM_FWD || prog == HMM_FWD_ROWS ? HMM_LSE_LDS_BYTES : 0); }
static size_t hmm_msv_lds_bytes(int cls) { return (size_t)HMM_MSV_ROWS * 64 * HMM_CLASS_Q[cls] * 4; }
static size_t hmm16_lds_bytes(int cls) { return (size_t)HMM16_ROWS * 64 * hmm16_regs(HMM_CLASS_Q[cls]) * 4; }
static size_t hmm_ali_lds_bytes(int cls) { return ((size_t)HMM_ALI_MASK_ROWS * 64 * HMM_CLASS_Q[cls] + GS_HMM_EXP2_N) * 4; }
// which kernel a (kernel, class) flag of the profile set belongs to: the three programs of hmm_rows, then MSV and Viterbi over a selected list, ...,
// the int16 filter over all records and over a selected list
enum { HMM_K_MSV = HMM_PROGS, HMM_K_VIT_SEL, HMM_K_BACK, HMM_K_ENV_SCORE, HMM_K_N2_BACK, HMM_K_ALI_BACK, HMM_K_ALI_ROWS, HMM_K_VIT16, HMM_K_VIT16_SEL, HMM_KERNEL_KINDS };

}  // namespace gs

struct gs_hmm_db {
    gs_ctx *ctx = nullptr;
    std::vector<gs::HmmModel> models;
    std::vector<gs::HmmDesc> desc;
    std::vector<uint32_t> plist;                    // profile numbers, class by class
    uint32_t class_start[gs::HMM_CLASSES + 1] = {};
    bool all_ga = true;
    bool lds_set[gs::HMM_KERNEL_KINDS][gs::HMM_CLASSES] = {};
    std::vector<gs::HmmDesc> desc16;                // the int16 tables (SPEC 13.7): off in words of d_tables16
    gs::DevBuf d_tables, d_desc, d_plist, d_ga, d_lse, d_exp2, d_tables16, d_desc16;
};

namespace gs {

// The launches of one program for one class: the n_in profiles (or profile groups) from `first`, wg workgroups each, `lds` bytes of dynamic LDS.
// launch(grid, first) queues kernel k for a stretch of them; lds_set is the (program, class) flag of the profile set.
template <class K, class Launch>
static int hmm_launch_class(gs_ctx *c, bool &lds_set, K k, uint32_t first, uint32_t n_in, uint32_t wg, size_t lds, Launch launch)
{
    if (!n_in) return GS_OK;
    if (!lds_set) {
        if (lds > 64 * 1024) GS_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set = true;
    }
    for (uint32_t y0 = 0; y0 < n_in; y0 += 65535) {           // (the y dimension of a grid ends at 65535)
        ProfScope ps(c, FAM_SEARCH);
        launch(dim3(wg, std::min<uint32_t>(n_in - y0, 65535)), first + y0);
        GS_HIP_CHECK(hipGetLastError());
    }
    return GS_OK;
}

static int hmm_db_build(gs_ctx *c, std::vector<HmmModel> &&models, gs_hmm_db **out)
{
    GS_REQUIRE(models.size() < (1ull << 31), GS_ERR_UNSUPPORTED, "hmm: too many profiles");
    std::unique_ptr<gs_hmm_db> db(new gs_hmm_db());
    db->ctx = c;
    db->models = std::move(models);
    const size_t np = db->models.size();
    std::vector<int32_t> words, ga(np, 0);
    std::vector<uint32_t> words16;                  // the int16 tables, two node slots a word in the order the lanes of k_hmm_vit16 read them
    std::vector<std::vector<uint32_t>> by_class(HMM_CLASSES);
    for (size_t p = 0; p < np; p++) {
        const HmmModel &m = db->models[p];
        const uint32_t M = m.info.M, W = M + 1;
        const int cls = hmm_class_of(M), Q = HMM_CLASS_Q[cls], MP = 64 * Q;
        by_class[cls].push_back((uint32_t)p);
        db->desc.push_back(HmmDesc{(uint64_t)words.size(), M, m.info.tbm});
        const size_t at = words.size();
        words.resize(at + (size_t)HMM_ROWS_DEV * MP, GS_HMM_STAR);
        for (int row = 0; row < (int)GS_HMM_TABLE_ROWS; row++)
            for (uint32_t k = 1; k <= M; k++) words[at + (size_t)row * MP + (k - 1)] = m.tab[(size_t)row * W + k];
        for (int j = 0; j < MP; j++)
            words[at + (size_t)HMM_ROW_PDD * MP + j] = j % Q == 0 ? 0 : words[at + (size_t)HMM_ROW_PDD * MP + j - 1] + words[at + (size_t)HMM_ROW_DD * MP + j - 1];
        if (m.info.flags & GS_HMM_HAS_GA) ga[p] = m.info.ga_units; else db->all_ga = false;
        const int H = hmm16_regs(Q), RW = 64 * H;
        const size_t at16 = words16.size();
        db->desc16.push_back(HmmDesc{(uint64_t)at16, M, m.info.tbm});
        words16.resize(at16 + (size_t)HMM16_ROWS * RW, 0x80008000u);           // NEG16 in both halves
        for (int row = 0; row < HMM16_ROWS; row++)
            for (uint32_t k = 1; k <= M; k++) {
                uint32_t &w = words16[at16 + (size_t)row * RW + hmm16_word(H, (int)k - 1)];
                const uint32_t v = (uint32_t)hmm16_half(m.tab[(size_t)row * W + k]) & 0xFFFFu;
                w = hmm16_high(H, (int)k - 1) ? (w & 0x0000FFFFu) | (v << 16) : (w & 0xFFFF0000u) | v;
            }
    }
    for (int cls = 0; cls < HMM_CLASSES; cls++) {
        db->class_start[cls] = (uint32_t)db->plist.size();
        db->plist.insert(db->plist.end(), by_class[cls].begin(), by_class[cls].end());
    }
    db->class_start[HMM_CLASSES] = (uint32_t)db->plist.size();
    GS_CTX_LOCK(c);
    int rc;
    if ((rc = db->d_tables.alloc(4 * words.size())) || (rc = db->d_desc.alloc(sizeof(HmmDesc) * np)) || (rc = db->d_plist.alloc(4 * np)) || (rc = db->d_ga.alloc(4 * np)) ||
        (rc = db->d_lse.alloc(HMM_LSE_LDS_BYTES)) || (rc = db->d_exp2.alloc(4 * GS_HMM_EXP2_N)) || (rc = db->d_tables16.alloc(4 * words16.size())) ||
        (rc = db->d_desc16.alloc(sizeof(HmmDesc) * np))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(db->d_tables16.p, words16.data(), 4 * words16.size(), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(db->d_desc16.p, db->desc16.data(), sizeof(HmmDesc) * np, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(db->d_tables.p, words.data(), 4 * words.size(), hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(db->d_desc.p, db->desc.data(), sizeof(HmmDesc) * np, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(db->d_plist.p, db->plist.data(), 4 * np, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(hipMemcpyAsync(db->d_ga.p, ga.data(), 4 * np, hipMemcpyHostToDevice, c->stream));
    std::vector<uint16_t> lse(HMM_LSE_LDS_N, 0);
    for (uint32_t j = 0; j < GS_HMM_LSE_N; j++) lse[j] = hmm_lse_entry(j);
    GS_HIP_CHECK(hipMemcpyAsync(db->d_lse.p, lse.data(), HMM_LSE_LDS_BYTES, hipMemcpyHostToDevice, c->stream));
    std::vector<uint32_t> exp2w(GS_HMM_EXP2_N);
    for (uint32_t f = 0; f < GS_HMM_EXP2_N; f++) exp2w[f] = hmm_exp2_entry(f);
    GS_HIP_CHECK(hipMemcpyAsync(db->d_exp2.p, exp2w.data(), 4 * GS_HMM_EXP2_N, hipMemcpyHostToDevice, c->stream));
    GS_HIP_CHECK(stream_wait(c));           // the host vectors go out of scope
    *out = db.release();
    return GS_OK;
}

// ---- the arguments of a call ----------------------------------------------------------------------------------------------------------------------
// Every operation is in the ABI twice, over device pointers (_dev) and over host pointers. Both entries hand their pointers to ONE body (hmm_*_form),
// which states the refusals once, builds the views below and runs the implementation; `host` says where the caller's pointers live.
// One array argument: the caller's device memory where there is some, else the slot - the staging of a host form (filled from the caller's array with
// HMM_UP, copied back to it by hmm_fetch with HMM_DOWN), or the place of an output that has to be computed although nobody asked for it.
enum { HMM_UP = 1, HMM_DOWN = 2 };
struct HmmArg {
    PoolBuf buf; void *dev = nullptr, *back = nullptr; size_t bytes = 0;
    HmmArg(gs_ctx *c, ScratchSlot s) : buf(c, s) {}
    int bind(bool host, const void *p, size_t n, int dir)
    {
        if (!host && (p || !n)) { dev = (void *)p; return GS_OK; }
        int rc = buf.alloc(n);
        if (rc) return rc;
        dev = buf.p;
        if (!host || !p) return GS_OK;
        if ((dir & HMM_UP) && n) GS_HIP_CHECK(hipMemcpyAsync(dev, p, n, hipMemcpyHostToDevice, buf.c->stream));
        if (dir & HMM_DOWN) { back = (void *)p; bytes = n; }
        return GS_OK;
    }
    template <class T> T *as() const { return (T *)dev; }
};
struct HmmIn {          // the caller's records
    bool host; const uint8_t *aa; const uint64_t *rs, *rl; uint64_t n_rec;
    bool given() const { return rs && rl && (host || aa); }             // (a host form that reads no residue may pass a null aa: HmmRecs::fill decides)
};
// The records as the implementations read them: aa, rec_start and rec_len on the device, the lengths on the host too.
struct HmmRecs {
    const uint8_t *aa = nullptr; const uint64_t *rs = nullptr, *rl = nullptr, *lens = nullptr; uint64_t n_rec = 0;
    std::vector<uint64_t> fetched; HmmArg d_aa, d_rs, d_rl;
    explicit HmmRecs(gs_ctx *c) : d_aa(c, SL_HMMB_AA), d_rs(c, SL_HMMB_REC_START), d_rl(c, SL_HMMB_REC_LEN) {}
    // Host forms: the three arrays go to their slots, aa as far as the call reads it (n_bytes). _dev forms: the lengths come to the host, behind a wait
    // for whatever the caller, and this call, queued before.
    int fill(const HmmIn &in, uint64_t n_bytes)
    {
        gs_ctx *c = d_aa.buf.c;
        n_rec = in.n_rec;
        GS_REQUIRE(!in.host || in.aa || n_bytes == 0, GS_ERR_INVALID, "null aa");
        int rc;
        if ((rc = d_aa.bind(in.host, in.aa, n_bytes, HMM_UP)) || (rc = d_rs.bind(in.host, in.rs, 8 * n_rec, HMM_UP)) || (rc = d_rl.bind(in.host, in.rl, 8 * n_rec, HMM_UP))) return rc;
        aa = d_aa.as<uint8_t>(); rs = d_rs.as<uint64_t>(); rl = d_rl.as<uint64_t>(); lens = in.rl;
        if (in.host) return GS_OK;
        fetched.resize(n_rec);
        if (n_rec) GS_HIP_CHECK(hipMemcpyAsync(fetched.data(), rl, 8 * n_rec, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(stream_wait(c));
        lens = fetched.data();
        return GS_OK;
    }
};
// The pairs of a call: both lists on the host, pair_prof on the device where a kernel reads it.
struct HmmPairs {
    const uint32_t *rec = nullptr, *prof = nullptr, *prof_dev = nullptr; uint64_t n = 0;
    std::vector<uint32_t> h_rec, h_prof; HmmArg d_prof;
    explicit HmmPairs(gs_ctx *c) : d_prof(c, SL_HMMB_PAIR_PROF) {}
    // Host forms: pair_prof goes to its slot if on_device. _dev forms: both lists are queued for the host and are there after the next wait (HmmRecs::fill).
    int fill(bool host, const uint32_t *pair_rec, const uint32_t *pair_prof, uint64_t n_pairs, bool on_device)
    {
        gs_ctx *c = d_prof.buf.c;
        n = n_pairs; rec = pair_rec; prof = pair_prof;
        int rc;
        if ((!host || on_device) && (rc = d_prof.bind(host, pair_prof, 4 * n, HMM_UP))) return rc;
        prof_dev = d_prof.as<uint32_t>();
        if (host) return GS_OK;
        h_rec.resize(n); h_prof.resize(n);
        GS_HIP_CHECK(hipMemcpyAsync(h_rec.data(), pair_rec, 4 * n, hipMemcpyDeviceToHost, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(h_prof.data(), pair_prof, 4 * n, hipMemcpyDeviceToHost, c->stream));
        rec = h_rec.data(); prof = h_prof.data();
        return GS_OK;
    }
};
// the end of a host form: its outputs to the caller's arrays, in the order given, and the wait for them (a _dev form has nothing to copy and only waits)
static int hmm_fetch(gs_ctx *c, std::initializer_list<const HmmArg *> outs)
{
    for (const HmmArg *o : outs)
        if (o->back && o->bytes) GS_HIP_CHECK(hipMemcpyAsync(o->back, o->dev, o->bytes, hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

static int hmm_check_lens(const uint64_t *lens, uint64_t n_rec, uint32_t max_l)
{
    for (uint64_t r = 0; r < n_rec; r++)
        GS_REQUIRE(lens[r] <= max_l, GS_ERR_UNSUPPORTED, "hmm: record %llu has %llu residues, more than %u", (unsigned long long)r, (unsigned long long)lens[r], max_l);
    return GS_OK;
}
// The context's lock of a body. A body declares it before its views, so that they have given their slots back when it is released, and takes it where
// the form it runs for did: a host form after it has judged the caller's arrays, a _dev form at once, since it judges what it fetches.
using HmmLock = std::unique_lock<std::recursive_mutex>;
static void hmm_lock(gs_ctx *c, HmmLock &lock) { lock = HmmLock(c->mu); (void)hipSetDevice(c->device); }

// R: the records of the call; everything else device memory. Queued on c's stream; the order list lives in its slot until the caller's scope ends.
// msv: the MSV score (SPEC 13.3) of every pair in the place of its Viterbi score - the same launches with k_hmm_msv and its smaller LDS.
// vit16: vf (SPEC 13.7) in that place - the same launches with k_hmm_vit16 over the int16 tables.
static int hmm_search_impl(gs_ctx *c, gs_hmm_db *db, const HmmRecs &R, int32_t *score_dev, PoolBuf &d_order, bool msv = false, bool vit16 = false)
{
    const uint32_t np = (uint32_t)db->models.size();
    const uint64_t n_rec = R.n_rec, *lens = R.lens;
    std::vector<uint32_t> order(n_rec);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
    int rc;
    if ((rc = d_order.alloc(4 * n_rec))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(d_order.p, order.data(), 4 * n_rec, hipMemcpyHostToDevice, c->stream));
    const uint32_t wg = (uint32_t)std::min<uint64_t>((n_rec + HMM_WAVES - 1) / HMM_WAVES, HMM_MAX_WG_PER_PROFILE);
    for (int cls = 0; cls < HMM_CLASSES; cls++) {
        const auto k = vit16 ? hmm_kernels(cls).vit16 : (msv ? hmm_kernels(cls).msv : hmm_kernels(cls).vit);
        const size_t lds = vit16 ? hmm16_lds_bytes(cls) : (msv ? hmm_msv_lds_bytes(cls) : hmm_lds_bytes(cls, HMM_VIT));
        const int32_t *tables = vit16 ? db->d_tables16.as<int32_t>() : db->d_tables.as<int32_t>();
        const HmmDesc *desc = vit16 ? db->d_desc16.as<HmmDesc>() : db->d_desc.as<HmmDesc>();
        rc = hmm_launch_class(c, db->lds_set[vit16 ? HMM_K_VIT16 : (msv ? HMM_K_MSV : HMM_VIT)][cls], k, db->class_start[cls], db->class_start[cls + 1] - db->class_start[cls], wg, lds, [&](dim3 grid, uint32_t first) {
            k<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, db->d_plist.as<uint32_t>() + first, R.aa, R.rs, R.rl,
                                                   d_order.as<uint32_t>(), (uint32_t)n_rec, np, score_dev);
        });
        if (rc) return rc;
    }
    GS_HIP_CHECK(stream_wait(c));           // `order` is read by the copy until here
    return GS_OK;
}

// the order list of a call and, per profile, the selected records and their number; a later selection takes the place of the one before (stream order)
struct HmmLists {
    PoolBuf order, sel, cnt;
    explicit HmmLists(gs_ctx *c) : order(c, SL_HMM_ORDER), sel(c, SL_HMM_SEL), cnt(c, SL_HMM_SEL_COUNT) {}
};
// One program over the pairs another score selects: out_dev filled with GS_HMM_NO_SCORE, per profile the list of the records whose in_dev reaches
// floor_dev (nullptr: every pair that has a score there), then prog - HMM_FWD: k_hmm_forward, HMM_VIT: k_hmm_viterbi_sel, HMM_K_VIT16_SEL: k_hmm_vit16_sel -
// over those lists into out_dev.
// Queued on c's stream.
static int hmm_selected_pass(gs_ctx *c, gs_hmm_db *db, int prog, const HmmRecs &R, const int32_t *in_dev, const int32_t *floor_dev, int32_t *out_dev, HmmLists &l)
{
    const uint32_t np = (uint32_t)db->models.size();
    const uint64_t n_rec = R.n_rec;
    int rc;
    if (!l.sel.p && ((rc = l.sel.alloc(4 * n_rec * np)) || (rc = l.cnt.alloc(4 * (size_t)np)))) return rc;
    const uint64_t n = n_rec * np;
    GS_REQUIRE(n < (1ull << 31) * 256, GS_ERR_UNSUPPORTED, "hmm: too many (record, profile) pairs");
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_fill<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(out_dev, n, GS_HMM_NO_SCORE);
        GS_HIP_CHECK(hipGetLastError());
    }
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_select<<<np, HMM_SEL_BLOCK, 0, c->stream>>>(in_dev, l.order.as<uint32_t>(), (uint32_t)n_rec, np, floor_dev, l.sel.as<uint32_t>(), l.cnt.as<uint32_t>());
        GS_HIP_CHECK(hipGetLastError());
    }
    const uint32_t wg = (uint32_t)std::min<uint64_t>((n_rec + HMM_WAVES - 1) / HMM_WAVES, HMM_MAX_WG_PER_PROFILE);
    for (int cls = 0; cls < HMM_CLASSES; cls++) {
        // the two programs differ in the kernel, its LDS, its flag and the table of lse that Forward takes behind the profile list
        const bool v16 = prog == HMM_K_VIT16_SEL;
        const int32_t *tables = v16 ? db->d_tables16.as<int32_t>() : db->d_tables.as<int32_t>();
        const HmmDesc *desc = v16 ? db->d_desc16.as<HmmDesc>() : db->d_desc.as<HmmDesc>();
        auto run = [&](auto k, int kind, size_t lds, auto... lse) {
            return hmm_launch_class(c, db->lds_set[kind][cls], k, db->class_start[cls], db->class_start[cls + 1] - db->class_start[cls], wg, lds, [&](dim3 grid, uint32_t first) {
                k<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, db->d_plist.as<uint32_t>() + first, lse..., R.aa, R.rs, R.rl,
                                                       l.sel.as<uint32_t>(), l.cnt.as<uint32_t>(), (uint32_t)n_rec, np, out_dev);
            });
        };
        rc = prog == HMM_FWD ? run(hmm_kernels(cls).fwd, HMM_FWD, hmm_lds_bytes(cls, HMM_FWD), db->d_lse.as<uint16_t>())
             : v16           ? run(hmm_kernels(cls).vit16_sel, HMM_K_VIT16_SEL, hmm16_lds_bytes(cls))
                             : run(hmm_kernels(cls).vit_sel, HMM_K_VIT_SEL, hmm_lds_bytes(cls, HMM_VIT));
        if (rc) return rc;
    }
    return GS_OK;
}

// ---- lists of pairs: trace-back (SPEC 13.2) and posterior envelopes (SPEC 13.4), host side -------------------------------------------------------------
// max_block_cells = 0: 2^27 cells (sum of L * 64 Q) of back-pointers alive at once - 64 MB of nibbles at Q = 8 and 16, 0.5 GB at Q = 1 where a lane's
// one nibble still takes a word. The longest record against the largest profile (65 536 x 1 280) is 84 million cells, so it fits one default block.
static constexpr uint64_t HMM_TRACE_DEFAULT_BLOCK_CELLS = 1ull << 27;

// The pairs of a call cut into blocks: blocks in the caller's order, a block's pairs by class
// and profile, longest record first. cost(i) is what pair i adds to its block; a block ends before the pair that would take it past cap, and always
// holds at least one pair. A pair without a record or with an empty one is on no list. ptr_off counts the pair's back-pointer words, row_off its L + 1 rows.
struct HmmPairBlock { uint32_t start, n, prof_start[HMM_CLASSES + 1], max_cnt[HMM_CLASSES]; };
struct HmmPairBlocks {
    std::vector<HmmTracePair> tp; std::vector<HmmTraceProf> tprof; std::vector<HmmPairBlock> blocks;
    uint64_t max_ptr = 0, max_rows = 0;                          // the largest block's pointer words and rows
};
template <class Cost>
static HmmPairBlocks hmm_pair_blocks(const gs_hmm_db *db, const uint64_t *lens, const uint32_t *prec, const uint32_t *pprof, uint64_t n_pairs, uint64_t cap, Cost cost)
{
    HmmPairBlocks out;
    std::vector<uint32_t> cur;
    uint64_t used = 0;
    auto flush = [&]() {
        if (cur.empty()) return;
        std::stable_sort(cur.begin(), cur.end(), [&](uint32_t a, uint32_t b) {
            const int ca = hmm_class_of(db->desc[pprof[a]].M), cb = hmm_class_of(db->desc[pprof[b]].M);
            if (ca != cb) return ca < cb;
            if (pprof[a] != pprof[b]) return pprof[a] < pprof[b];
            return lens[prec[a]] > lens[prec[b]];
        });
        HmmPairBlock b{};
        b.start = (uint32_t)out.tp.size(); b.n = (uint32_t)cur.size();
        uint64_t ptr = 0, row = 0;
        size_t at = 0;
        for (int cls = 0; cls < HMM_CLASSES; cls++) {
            b.prof_start[cls] = (uint32_t)out.tprof.size();
            while (at < cur.size() && hmm_class_of(db->desc[pprof[cur[at]]].M) == cls) {
                const uint32_t prof = pprof[cur[at]];
                HmmTraceProf g{prof, (uint32_t)out.tp.size(), 0};
                for (; at < cur.size() && pprof[cur[at]] == prof; at++, g.cnt++) {
                    const uint64_t L = lens[prec[cur[at]]];
                    out.tp.push_back(HmmTracePair{ptr, row, cur[at], prec[cur[at]]});
                    ptr += L * hmm_ptr_words(HMM_CLASS_Q[cls]) * 64;
                    row += L + 1;
                }
                b.max_cnt[cls] = std::max(b.max_cnt[cls], g.cnt);
                out.tprof.push_back(g);
            }
        }
        b.prof_start[HMM_CLASSES] = (uint32_t)out.tprof.size();
        out.max_ptr = std::max(out.max_ptr, ptr); out.max_rows = std::max(out.max_rows, row);
        out.blocks.push_back(b);
        cur.clear(); used = 0;
    };
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (prec[i] == GS_HMM_NO_HIT || lens[prec[i]] == 0) continue;
        const uint64_t pc = cost(i);
        if (!cur.empty() && used + pc > cap) flush();
        cur.push_back((uint32_t)i);
        used += pc;
    }
    flush();
    return out;
}

// The blocks of a call, run: both lists go to the device, `scratch(pb)` takes what a block needs beside them, then block by block every class that
// occurs gets per_class(d, b, cls, wg) - wg workgroups for each of its profiles b.prof_start[cls] .. b.prof_start[cls + 1], enough for the profile with the
// most pairs - and the block per_block(d, b). All on c's stream, which is waited for once, at the end: the lists are read by the copies until then, and the
// slots go back.
struct HmmBlockLists { const HmmTracePair *tp; const HmmTraceProf *tprof; };
static uint32_t hmm_block_wg(uint64_t per_profile) { return (uint32_t)std::min<uint64_t>((per_profile + HMM_WAVES - 1) / HMM_WAVES, HMM_MAX_WG_PER_PROFILE); }
template <class Scratch, class PerClass, class PerBlock>
static int hmm_run_blocks(gs_ctx *c, const HmmPairBlocks &pb, Scratch scratch, PerClass per_class, PerBlock per_block)
{
    PoolBuf d_tp(c, SL_HMMP_PAIRS), d_tprof(c, SL_HMMP_PROFS);
    if (!pb.blocks.empty()) {
        int rc;
        if ((rc = d_tp.alloc(sizeof(HmmTracePair) * pb.tp.size())) || (rc = d_tprof.alloc(sizeof(HmmTraceProf) * pb.tprof.size())) || (rc = scratch(pb))) return rc;
        GS_HIP_CHECK(hipMemcpyAsync(d_tp.p, pb.tp.data(), sizeof(HmmTracePair) * pb.tp.size(), hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(d_tprof.p, pb.tprof.data(), sizeof(HmmTraceProf) * pb.tprof.size(), hipMemcpyHostToDevice, c->stream));
        const HmmBlockLists d{d_tp.as<HmmTracePair>(), d_tprof.as<HmmTraceProf>()};
        for (const HmmPairBlock &b : pb.blocks) {
            for (int cls = 0; cls < HMM_CLASSES; cls++)
                if ((rc = per_class(d, b, cls, hmm_block_wg(b.max_cnt[cls])))) return rc;
            if ((rc = per_block(d, b))) return rc;
        }
    }
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}
// one kernel of a block for one class: kind is its (kernel, class) flag, launch(grid, tprof) queues it for a stretch of the class's profile lists
template <class K, class Launch>
static int hmm_block_launch(gs_ctx *c, gs_hmm_db *db, int kind, K k, size_t lds, const HmmBlockLists &d, const HmmPairBlock &b, int cls, uint32_t wg, Launch launch)
{
    return hmm_launch_class(c, db->lds_set[kind][cls], k, b.prof_start[cls], b.prof_start[cls + 1] - b.prof_start[cls], wg, lds,
                            [&](dim3 grid, uint32_t first) { launch(grid, d.tprof + first); });
}

// What gs_hmm_trace refuses of its lists, and gs_hmm_envelopes with max_l = GS_HMM_FWD_MAX_L, decided on host copies before anything is queued.
// ro: row_off of the envelopes or nullptr - every listed pair's rows must fit between its offset and the next.
static int hmm_pair_check(const gs_hmm_db *db, const uint64_t *lens, uint64_t n_rec, const uint32_t *prec, const uint32_t *pprof, uint64_t n_pairs, uint32_t max_l,
                          const uint64_t *ro)
{
    const uint64_t np = db->models.size();
    for (uint64_t i = 0; i < n_pairs; i++) {
        GS_REQUIRE(pprof[i] < np, GS_ERR_INVALID, "hmm: pair %llu names profile %u of %llu", (unsigned long long)i, pprof[i], (unsigned long long)np);
        GS_REQUIRE(prec[i] == GS_HMM_NO_HIT || prec[i] < n_rec, GS_ERR_INVALID, "hmm: pair %llu names record %u of %llu", (unsigned long long)i, prec[i], (unsigned long long)n_rec);
    }
    for (uint64_t i = 0; i < n_pairs; i++)
        GS_REQUIRE(prec[i] == GS_HMM_NO_HIT || lens[prec[i]] <= max_l, GS_ERR_UNSUPPORTED, "hmm: pair %llu names record %u of %llu residues, more than %u",
                   (unsigned long long)i, prec[i], (unsigned long long)lens[prec[i]], max_l);
    for (uint64_t i = 0; ro && i < n_pairs; i++)
        GS_REQUIRE(ro[i] <= ro[i + 1] && (prec[i] == GS_HMM_NO_HIT || ro[i + 1] - ro[i] >= lens[prec[i]]), GS_ERR_INVALID,
                   "hmm: row_off leaves pair %llu fewer words than its record has residues", (unsigned long long)i);
    return GS_OK;
}
// What both forms over a list of pairs refuse, and their records and pairs as the implementation reads them. ro: row_off of the envelopes where the
// caller has it (nullptr: none); ro_host: where a _dev form keeps the host's copy. The lists are judged as soon as the host has them. A host form stages
// aa as far as the records that a pair names reach: the others may be any length. outs_given: the outputs the form cannot do without are there;
// rows_together: row_off, out_rows and cont_rows are all there or none is. HMM_NOTHING_TO_DO (no code of the ABI) stands for GS_OK without any work.
enum { HMM_NOTHING_TO_DO = 1 };
static int hmm_pair_args(gs_ctx *c, const gs_hmm_db *db, const HmmIn &in, const uint32_t *pair_rec, const uint32_t *pair_prof, uint64_t n_pairs, bool outs_given,
                         bool rows_together, uint32_t max_l, bool prof_on_device, const uint64_t *ro, std::vector<uint64_t> &ro_host, HmmLock &lock, HmmRecs &R,
                         HmmPairs &P)
{
    GS_REQUIRE(c && db && db->ctx == c, GS_ERR_INVALID, "hmm: null argument, or a profile set of another context");
    if (n_pairs == 0) return HMM_NOTHING_TO_DO;
    GS_REQUIRE(pair_rec && pair_prof && outs_given, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(in.n_rec == 0 || in.given(), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(rows_together, GS_ERR_INVALID, "hmm: an offset array and the outputs it addresses go together (row_off, out_rows, cont_rows; occ_off, occm_out, occi_out; col_off, col_out)");
    GS_REQUIRE(in.n_rec < (1ull << 32) && n_pairs < (1ull << 32), GS_ERR_UNSUPPORTED, "hmm: 2^32 records or pairs, or more, in one call");
    int rc;
    if (in.host) {
        if ((rc = hmm_pair_check(db, in.rl, in.n_rec, pair_rec, pair_prof, n_pairs, max_l, ro))) return rc;
        uint64_t n_bytes = 0;
        for (uint64_t i = 0; i < n_pairs; i++)
            if (pair_rec[i] != GS_HMM_NO_HIT && in.rl[pair_rec[i]]) n_bytes = std::max(n_bytes, in.rs[pair_rec[i]] + in.rl[pair_rec[i]]);
        hmm_lock(c, lock);
        if ((rc = R.fill(in, n_bytes)) || (rc = P.fill(true, pair_rec, pair_prof, n_pairs, prof_on_device))) return rc;
    } else {
        hmm_lock(c, lock);
        if ((rc = P.fill(false, pair_rec, pair_prof, n_pairs, prof_on_device))) return rc;
        if (ro) {
            ro_host.resize(n_pairs + 1);
            GS_HIP_CHECK(hipMemcpyAsync(ro_host.data(), ro, 8 * (n_pairs + 1), hipMemcpyDeviceToHost, c->stream));
        }
        if ((rc = R.fill(in, 0)) || (rc = hmm_pair_check(db, R.lens, in.n_rec, P.rec, P.prof, n_pairs, max_l, ro ? ro_host.data() : nullptr))) return rc;
    }
    return GS_OK;
}

// R, P: the records and pairs of the call, which hmm_pair_check has passed; everything else device memory. A block is a trace launch per class that
// occurs and one walk.
static int hmm_trace_impl(gs_ctx *c, gs_hmm_db *db, const HmmRecs &R, const HmmPairs &P, uint32_t max_dom, uint64_t max_block_cells, int32_t *raw_dev, uint32_t *ndom_dev,
                          int32_t *dom_dev)
{
    const uint64_t n_pairs = P.n, n_dom_words = n_pairs * max_dom * GS_HMM_DOM_WORDS, n_fill = std::max(n_pairs, n_dom_words);
    GS_REQUIRE(n_fill < (1ull << 31) * 256, GS_ERR_UNSUPPORTED, "hmm: too many domain slots");
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_trace_fill<<<(unsigned)((n_fill + 255) / 256), 256, 0, c->stream>>>(n_pairs, n_dom_words, raw_dev, ndom_dev, dom_dev);
        GS_HIP_CHECK(hipGetLastError());
    }
    const HmmPairBlocks pb = hmm_pair_blocks(db, R.lens, P.rec, P.prof, n_pairs, max_block_cells ? max_block_cells : HMM_TRACE_DEFAULT_BLOCK_CELLS, [&](uint64_t i) {
        return R.lens[P.rec[i]] * 64 * HMM_CLASS_Q[hmm_class_of(db->desc[P.prof[i]].M)];
    });
    PoolBuf d_ptr(c, SL_HMMT_PTR), d_rows(c, SL_HMMT_ROWS);
    return hmm_run_blocks(
        c, pb, [&](const HmmPairBlocks &pb) { int rc = d_ptr.alloc(4 * pb.max_ptr); return rc ? rc : d_rows.alloc(sizeof(int4) * pb.max_rows); },
        [&](const HmmBlockLists &d, const HmmPairBlock &b, int cls, uint32_t wg) -> int {
            const auto k = hmm_kernels(cls).trace;
            const size_t lds = hmm_lds_bytes(cls, HMM_TRACE);
            return hmm_block_launch(c, db, HMM_TRACE, k, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                k<<<grid, HMM_BLOCK, lds, c->stream>>>(db->d_tables.as<int32_t>(), db->d_desc.as<HmmDesc>(), tprof, d.tp, R.aa, R.rs, R.rl, d_ptr.as<uint32_t>(), d_rows.as<int4>(), raw_dev);
            });
        },
        [&](const HmmBlockLists &d, const HmmPairBlock &b) -> int {
            ProfScope ps(c, FAM_SEARCH);
            k_hmm_walk<<<(b.n + HMM_WALK_BLOCK - 1) / HMM_WALK_BLOCK, HMM_WALK_BLOCK, 0, c->stream>>>(db->d_desc.as<HmmDesc>(), d.tp + b.start, b.n, P.prof_dev, R.rl, d_ptr.as<uint32_t>(),
                                                                                                        d_rows.as<int4>(), raw_dev, max_dom, ndom_dev, dom_dev);
            GS_HIP_CHECK(hipGetLastError());
            return GS_OK;
        });
}

// R, P: the records and pairs of the call, which hmm_pair_check has passed under Forward's length limit; everything else device memory. Blocks of at most
// max_block_rows kept rows (sum of L + 1). A block is a Forward-with-rows and a Backward launch per class that occurs, k_hmm_envelopes, and a
// k_hmm_env_score launch per class.
static int hmm_env_impl(gs_ctx *c, gs_hmm_db *db, const HmmRecs &R, const HmmPairs &P, uint32_t max_env, uint64_t max_block_rows, int32_t *fwd_dev, int32_t *bck_dev,
                        uint32_t *nenv_dev, int32_t *env_dev, const uint64_t *row_off_dev, int32_t *out_rows_dev, int32_t *cont_rows_dev)
{
    const uint64_t n_pairs = P.n, n_env_words = n_pairs * max_env * GS_HMM_ENV_WORDS, n_fill = std::max(n_pairs, n_env_words);
    GS_REQUIRE(n_fill < (1ull << 31) * 256, GS_ERR_UNSUPPORTED, "hmm: too many envelope slots");
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_env_fill<<<(unsigned)((n_fill + 255) / 256), 256, 0, c->stream>>>(n_pairs, n_env_words, fwd_dev, bck_dev, nenv_dev, env_dev);
        GS_HIP_CHECK(hipGetLastError());
    }
    const HmmPairBlocks pb = hmm_pair_blocks(db, R.lens, P.rec, P.prof, n_pairs, max_block_rows ? max_block_rows : HMM_ENV_DEFAULT_BLOCK_ROWS,
                                             [&](uint64_t i) { return R.lens[P.rec[i]] + 1; });
    PoolBuf d_frows(c, SL_HMME_FROWS), d_brows(c, SL_HMME_BROWS);
    const int32_t *tables = db->d_tables.as<int32_t>();
    const HmmDesc *desc = db->d_desc.as<HmmDesc>();
    const uint16_t *lse = db->d_lse.as<uint16_t>();
    return hmm_run_blocks(
        c, pb, [&](const HmmPairBlocks &pb) { int rc = d_frows.alloc(sizeof(int4) * pb.max_rows); return rc ? rc : d_brows.alloc(sizeof(int2) * pb.max_rows); },
        [&](const HmmBlockLists &d, const HmmPairBlock &b, int cls, uint32_t wg) -> int {
            const auto kf = hmm_kernels(cls).fwd_rows;
            const size_t lds = hmm_lds_bytes(cls, HMM_FWD);
            int rc = hmm_block_launch(c, db, HMM_FWD_ROWS, kf, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kf<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, d_frows.as<int4>(), fwd_dev);
            });
            if (rc) return rc;
            const auto kb = hmm_kernels(cls).back;
            return hmm_block_launch(c, db, HMM_K_BACK, kb, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kb<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, d_brows.as<int2>(), bck_dev);
            });
        },
        [&](const HmmBlockLists &d, const HmmPairBlock &b) -> int {
            {
                ProfScope ps(c, FAM_SEARCH);
                k_hmm_envelopes<<<b.n, HMM_ENV_BLOCK, 0, c->stream>>>(d.tp + b.start, R.rl, lse, d_frows.as<int4>(), d_brows.as<int2>(), fwd_dev, max_env, nenv_dev, env_dev,
                                                                       row_off_dev, out_rows_dev, cont_rows_dev);
                GS_HIP_CHECK(hipGetLastError());
            }
            for (int cls = 0; max_env && cls < HMM_CLASSES; cls++) {         // the envelopes' own scores: a wave per (pair, envelope slot)
                const auto ks = hmm_kernels(cls).env_score;
                const size_t lds = hmm_lds_bytes(cls, HMM_FWD);
                int rc = hmm_block_launch(c, db, HMM_K_ENV_SCORE, ks, lds, d, b, cls, hmm_block_wg((uint64_t)b.max_cnt[cls] * max_env), [&](dim3 grid, const HmmTraceProf *tprof) {
                    ks<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, max_env, nenv_dev, env_dev);
                });
                if (rc) return rc;
            }
            return GS_OK;
        });
}

// What gs_hmm_null2 refuses of the envelopes it is given, decided on host copies before any output is touched. A pair without a record or with an empty
// one lists nothing and its words are not read. oo: occ_off or nullptr - the rows of a pair's listed slots, M words each, must fit between its offset
// and the next.
static int hmm_null2_check(const gs_hmm_db *db, const uint64_t *lens, const uint32_t *prec, const uint32_t *pprof, uint64_t n_pairs, uint32_t max_env, const uint32_t *n_env,
                           const int32_t *env, const uint64_t *oo)
{
    for (uint64_t j = 0; j < n_pairs; j++) {
        GS_REQUIRE(!oo || oo[j] <= oo[j + 1], GS_ERR_INVALID, "hmm: occ_off decreases at pair %llu", (unsigned long long)j);
        if (prec[j] == GS_HMM_NO_HIT || lens[prec[j]] == 0) continue;
        const uint64_t L = lens[prec[j]], listed = std::min<uint64_t>(n_env[j], max_env);
        for (uint64_t e = 0; e < listed; e++) {
            const int64_t a = env[(j * max_env + e) * GS_HMM_ENV_WORDS], b = env[(j * max_env + e) * GS_HMM_ENV_WORDS + 1];
            GS_REQUIRE(a >= 1 && a <= b && (uint64_t)b <= L, GS_ERR_INVALID, "hmm: envelope %llu of pair %llu is %lld .. %lld on a record of %llu residues",
                       (unsigned long long)e, (unsigned long long)j, (long long)a, (long long)b, (unsigned long long)L);
        }
        GS_REQUIRE(!oo || oo[j + 1] - oo[j] >= listed * db->desc[pprof[j]].M, GS_ERR_INVALID, "hmm: occ_off leaves pair %llu fewer words than its listed envelopes times M",
                   (unsigned long long)j);
    }
    return GS_OK;
}

// R, P: the records and pairs of the call, which hmm_pair_check has passed under Forward's length limit; n_env, env, oo: host copies that hmm_null2_check has
// passed; everything else device memory. The listed envelopes are cut into blocks of at most max_block_cells cells (sum of 64 Q * Ld; two kept words a
// cell); a block is a Forward and a Backward launch per class that occurs. The sequence biases follow the last block.
static int hmm_null2_impl(gs_ctx *c, gs_hmm_db *db, const HmmRecs &R, const HmmPairs &P, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env,
                          const uint64_t *oo, int32_t *slot_dev, int32_t *seq_dev, int32_t *n2_dev, int32_t *occm_dev, int32_t *occi_dev)
{
    const uint64_t n_pairs = P.n, n_slot_words = n_pairs * max_env * GS_HMM_N2_WORDS, n_n2_words = n2_dev ? n_pairs * max_env * 20 : 0,
                   n_fill = std::max(std::max(n_pairs, n_slot_words), n_n2_words);
    GS_REQUIRE(n_fill < (1ull << 31) * 256 && n_pairs * max_env < (1ull << 32) && n_pairs < (1ull << 31), GS_ERR_UNSUPPORTED, "hmm: too many envelope slots");
    std::vector<HmmN2Pair> np(n_pairs);
    std::vector<HmmN2Slot> slots;
    std::vector<uint64_t> slot_len;                               // Ld of every slot: the `lens` of the block builder, whose records are the slots
    std::vector<uint32_t> slot_id, slot_prof;
    for (uint64_t j = 0; j < n_pairs; j++) {
        const bool has = P.rec[j] != GS_HMM_NO_HIT && R.lens[P.rec[j]] != 0;
        np[j] = HmmN2Pair{P.rec[j], has ? std::min(n_env[j], max_env) : 0u};
        for (uint32_t e = 0; e < np[j].listed; e++) {
            const int32_t *w = env + (j * max_env + e) * GS_HMM_ENV_WORDS;
            slot_id.push_back((uint32_t)slots.size()); slot_prof.push_back(P.prof[j]); slot_len.push_back((uint64_t)(w[1] - w[0] + 1));
            slots.push_back(HmmN2Slot{oo ? oo[j] + (uint64_t)e * db->desc[P.prof[j]].M : 0, (uint32_t)j, e, P.rec[j], (uint32_t)w[0], (uint32_t)(w[1] - w[0] + 1), 0});
        }
    }
    auto cells = [&](uint64_t i) { return slot_len[i] * 64 * HMM_CLASS_Q[hmm_class_of(db->desc[slot_prof[i]].M)]; };
    HmmPairBlocks pb = hmm_pair_blocks(db, slot_len.data(), slot_id.data(), slot_prof.data(), slots.size(), max_block_cells ? max_block_cells : HMM_N2_DEFAULT_BLOCK_CELLS, cells);
    uint64_t max_keep = 0;                                        // the kept words of the largest block; ptr_off: where a slot's start
    for (const HmmPairBlock &b : pb.blocks) {
        uint64_t at = 0;
        for (uint32_t t = b.start; t < b.start + b.n; t++) { pb.tp[t].ptr_off = at; at += 2 * cells(pb.tp[t].pair); }
        max_keep = std::max(max_keep, at);
    }
    PoolBuf d_np(c, SL_HMMN_PAIRS), d_slots(c, SL_HMMN_SLOTS), d_ok(c, SL_HMMN_OK), d_keep(c, SL_HMMN_KEEP), d_rows(c, SL_HMME_FROWS);
    int rc;
    if ((rc = d_np.alloc(sizeof(HmmN2Pair) * n_pairs)) || (rc = d_slots.alloc(sizeof(HmmN2Slot) * slots.size())) || (rc = d_ok.alloc(4 * n_pairs))) return rc;
    GS_HIP_CHECK(hipMemcpyAsync(d_np.p, np.data(), sizeof(HmmN2Pair) * n_pairs, hipMemcpyHostToDevice, c->stream));
    if (!slots.empty()) GS_HIP_CHECK(hipMemcpyAsync(d_slots.p, slots.data(), sizeof(HmmN2Slot) * slots.size(), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_n2_fill<<<(unsigned)((n_fill + 255) / 256), 256, 0, c->stream>>>(n_slot_words, n_pairs, n_n2_words, slot_dev, seq_dev, n2_dev);
        GS_HIP_CHECK(hipGetLastError());
    }
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_n2_flag<<<(unsigned)n_pairs, 64, 0, c->stream>>>(d_np.as<HmmN2Pair>(), R.aa, R.rs, R.rl, d_ok.as<uint32_t>());
        GS_HIP_CHECK(hipGetLastError());
    }
    const int32_t *tables = db->d_tables.as<int32_t>();
    const HmmDesc *desc = db->d_desc.as<HmmDesc>();
    const uint16_t *lse = db->d_lse.as<uint16_t>();
    rc = hmm_run_blocks(
        c, pb, [&](const HmmPairBlocks &pb) { int rc = d_keep.alloc(4 * max_keep); return rc ? rc : d_rows.alloc(sizeof(int4) * pb.max_rows); },
        [&](const HmmBlockLists &d, const HmmPairBlock &b, int cls, uint32_t wg) -> int {
            const auto kf = hmm_kernels(cls).n2_fwd;
            const size_t lds = hmm_lds_bytes(cls, HMM_FWD);
            int rc = hmm_block_launch(c, db, HMM_FWD_SEG, kf, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kf<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, d_slots.as<HmmN2Slot>(), d_ok.as<uint32_t>(), max_env, d_rows.as<int4>(),
                                                        d_keep.as<uint32_t>(), slot_dev);
            });
            if (rc) return rc;
            const auto kb = hmm_kernels(cls).n2_back;
            return hmm_block_launch(c, db, HMM_K_N2_BACK, kb, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kb<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, d_slots.as<HmmN2Slot>(), d_ok.as<uint32_t>(), max_env, d_rows.as<int4>(),
                                                        d_keep.as<uint32_t>(), slot_dev, n2_dev, occm_dev, occi_dev);
            });
        },
        [&](const HmmBlockLists &, const HmmPairBlock &) -> int { return GS_OK; });
    if (rc) return rc;
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_n2_seq<<<(unsigned)((n_pairs + 255) / 256), 256, 0, c->stream>>>(d_np.as<HmmN2Pair>(), d_ok.as<uint32_t>(), n_pairs, max_env, lse, slot_dev, seq_dev);
        GS_HIP_CHECK(hipGetLastError());
    }
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

// What gs_hmm_align refuses beyond hmm_null2_check, on the same host copies: a listed envelope longer than GS_HMM_ALI_MAX_LD, and - co: col_off or nullptr -
// a pair whose columns, Ld + M for every listed slot, do not fit between its offset and the next.
static int hmm_align_check(const gs_hmm_db *db, const uint64_t *lens, const uint32_t *prec, const uint32_t *pprof, uint64_t n_pairs, uint32_t max_env, const uint32_t *n_env,
                           const int32_t *env, const uint64_t *co)
{
    for (uint64_t j = 0; j < n_pairs; j++) {
        GS_REQUIRE(!co || co[j] <= co[j + 1], GS_ERR_INVALID, "hmm: col_off decreases at pair %llu", (unsigned long long)j);
        if (prec[j] == GS_HMM_NO_HIT || lens[prec[j]] == 0) continue;
        const uint64_t listed = std::min<uint64_t>(n_env[j], max_env);
        uint64_t need = 0;
        for (uint64_t e = 0; e < listed; e++) {
            const uint64_t Ld = (uint64_t)(env[(j * max_env + e) * GS_HMM_ENV_WORDS + 1] - env[(j * max_env + e) * GS_HMM_ENV_WORDS] + 1);
            GS_REQUIRE(Ld <= GS_HMM_ALI_MAX_LD, GS_ERR_UNSUPPORTED, "hmm: envelope %llu of pair %llu has %llu residues, more than %u", (unsigned long long)e,
                       (unsigned long long)j, (unsigned long long)Ld, GS_HMM_ALI_MAX_LD);
            need += Ld + db->desc[pprof[j]].M;
        }
        GS_REQUIRE(!co || co[j + 1] - co[j] >= need, GS_ERR_INVALID, "hmm: col_off leaves pair %llu fewer columns than its listed envelopes' residues and nodes",
                   (unsigned long long)j);
    }
    return GS_OK;
}

// R, P: the records and pairs of the call; n_env, env, co: host copies that hmm_null2_check and hmm_align_check have passed; everything else device memory.
// The blocks are null2's, cut by max_block_cells; a block is a Forward, a Backward and a row launch per class that occurs and one walk.
static int hmm_align_impl(gs_ctx *c, gs_hmm_db *db, const HmmRecs &R, const HmmPairs &P, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env,
                          const uint64_t *co, int32_t *slot_dev, int32_t *col_dev)
{
    const uint64_t n_pairs = P.n, n_slot_words = n_pairs * max_env * GS_HMM_ALI_WORDS;
    GS_REQUIRE(n_slot_words < (1ull << 31) * 256 && n_pairs * max_env < (1ull << 32) && n_pairs < (1ull << 31), GS_ERR_UNSUPPORTED, "hmm: too many envelope slots");
    std::vector<HmmN2Pair> np(n_pairs);
    std::vector<HmmN2Slot> slots;
    std::vector<HmmAliSlot> aslots;
    std::vector<uint64_t> slot_len;
    std::vector<uint32_t> slot_id, slot_prof;
    for (uint64_t j = 0; j < n_pairs; j++) {
        const bool has = P.rec[j] != GS_HMM_NO_HIT && R.lens[P.rec[j]] != 0;
        np[j] = HmmN2Pair{P.rec[j], has ? std::min(n_env[j], max_env) : 0u};
        uint64_t col = co ? co[j] : 0;
        for (uint32_t e = 0; e < np[j].listed; e++) {
            const int32_t *w = env + (j * max_env + e) * GS_HMM_ENV_WORDS;
            const uint32_t Ld = (uint32_t)(w[1] - w[0] + 1);
            slot_id.push_back((uint32_t)slots.size()); slot_prof.push_back(P.prof[j]); slot_len.push_back(Ld);
            slots.push_back(HmmN2Slot{0, (uint32_t)j, e, P.rec[j], (uint32_t)w[0], Ld, 0});
            aslots.push_back(HmmAliSlot{0, col});
            col += (uint64_t)Ld + db->desc[P.prof[j]].M;
        }
    }
    auto cells = [&](uint64_t i) { return slot_len[i] * 64 * HMM_CLASS_Q[hmm_class_of(db->desc[slot_prof[i]].M)]; };
    HmmPairBlocks pb = hmm_pair_blocks(db, slot_len.data(), slot_id.data(), slot_prof.data(), slots.size(), max_block_cells ? max_block_cells : HMM_N2_DEFAULT_BLOCK_CELLS, cells);
    uint64_t max_keep = 0;                                        // the builder's ptr_off counts the nibble words; it becomes the kept words' start, as in null2
    for (const HmmPairBlock &b : pb.blocks) {
        uint64_t at = 0;
        for (uint32_t t = b.start; t < b.start + b.n; t++) { aslots[pb.tp[t].pair].nib_off = pb.tp[t].ptr_off; pb.tp[t].ptr_off = at; at += 2 * cells(pb.tp[t].pair); }
        max_keep = std::max(max_keep, at);
    }
    PoolBuf d_np(c, SL_HMMN_PAIRS), d_slots(c, SL_HMMN_SLOTS), d_aslots(c, SL_HMMA_SLOTS), d_ok(c, SL_HMMN_OK), d_keep(c, SL_HMMN_KEEP), d_rows(c, SL_HMME_FROWS),
        d_arows(c, SL_HMME_BROWS), d_ptr(c, SL_HMMT_PTR), d_seg(c, SL_HMMA_SEG);
    int rc;
    if ((rc = d_np.alloc(sizeof(HmmN2Pair) * n_pairs)) || (rc = d_slots.alloc(sizeof(HmmN2Slot) * slots.size())) || (rc = d_aslots.alloc(sizeof(HmmAliSlot) * slots.size())) ||
        (rc = d_ok.alloc(4 * n_pairs)) || (rc = d_seg.alloc(4 * n_pairs * max_env * GS_HMM_N2_WORDS)))
        return rc;
    GS_HIP_CHECK(hipMemcpyAsync(d_np.p, np.data(), sizeof(HmmN2Pair) * n_pairs, hipMemcpyHostToDevice, c->stream));
    if (!slots.empty()) {
        GS_HIP_CHECK(hipMemcpyAsync(d_slots.p, slots.data(), sizeof(HmmN2Slot) * slots.size(), hipMemcpyHostToDevice, c->stream));
        GS_HIP_CHECK(hipMemcpyAsync(d_aslots.p, aslots.data(), sizeof(HmmAliSlot) * slots.size(), hipMemcpyHostToDevice, c->stream));
    }
    if (n_slot_words) {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_ali_fill<<<(unsigned)((n_slot_words + 255) / 256), 256, 0, c->stream>>>(n_slot_words, slot_dev);
        GS_HIP_CHECK(hipGetLastError());
    }
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_n2_flag<<<(unsigned)n_pairs, 64, 0, c->stream>>>(d_np.as<HmmN2Pair>(), R.aa, R.rs, R.rl, d_ok.as<uint32_t>());
        GS_HIP_CHECK(hipGetLastError());
    }
    const int32_t *tables = db->d_tables.as<int32_t>();
    const HmmDesc *desc = db->d_desc.as<HmmDesc>();
    const uint16_t *lse = db->d_lse.as<uint16_t>();
    return hmm_run_blocks(
        c, pb,
        [&](const HmmPairBlocks &pb) {
            int rc;
            if ((rc = d_keep.alloc(4 * max_keep)) || (rc = d_rows.alloc(sizeof(int4) * pb.max_rows)) || (rc = d_arows.alloc(sizeof(int2) * pb.max_rows))) return rc;
            return d_ptr.alloc(4 * pb.max_ptr);
        },
        [&](const HmmBlockLists &d, const HmmPairBlock &b, int cls, uint32_t wg) -> int {
            const auto kf = hmm_kernels(cls).n2_fwd;           // (its seg_raw goes to a scratch of null2's slot shape: nobody reads it)
            const size_t lds = hmm_lds_bytes(cls, HMM_FWD);
            int rc = hmm_block_launch(c, db, HMM_FWD_SEG, kf, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kf<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, d_slots.as<HmmN2Slot>(), d_ok.as<uint32_t>(), max_env, d_rows.as<int4>(),
                                                        d_keep.as<uint32_t>(), d_seg.as<int32_t>());
            });
            if (rc) return rc;
            const auto kb = hmm_kernels(cls).ali_back;
            rc = hmm_block_launch(c, db, HMM_K_ALI_BACK, kb, lds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kb<<<grid, HMM_BLOCK, lds, c->stream>>>(tables, desc, tprof, d.tp, lse, R.aa, R.rs, R.rl, d_slots.as<HmmN2Slot>(), d_ok.as<uint32_t>(), d_rows.as<int4>(),
                                                        d_keep.as<uint32_t>());
            });
            if (rc) return rc;
            const auto kr = hmm_kernels(cls).ali_rows;
            const size_t alds = hmm_ali_lds_bytes(cls);
            return hmm_block_launch(c, db, HMM_K_ALI_ROWS, kr, alds, d, b, cls, wg, [&](dim3 grid, const HmmTraceProf *tprof) {
                kr<<<grid, HMM_BLOCK, alds, c->stream>>>(tables, desc, tprof, d.tp, db->d_exp2.as<uint32_t>(), d_slots.as<HmmN2Slot>(), d_aslots.as<HmmAliSlot>(), d_ok.as<uint32_t>(),
                                                         max_env, d_rows.as<int4>(), d_keep.as<int32_t>(), d_ptr.as<uint32_t>(), d_arows.as<int2>(), slot_dev);
            });
        },
        [&](const HmmBlockLists &d, const HmmPairBlock &b) -> int {
            ProfScope ps(c, FAM_SEARCH);
            k_hmm_ali_walk<<<(b.n + HMM_WALK_BLOCK - 1) / HMM_WALK_BLOCK, HMM_WALK_BLOCK, 0, c->stream>>>(desc, d.tp + b.start, b.n, P.prof_dev, d_slots.as<HmmN2Slot>(),
                                                                                                            d_aslots.as<HmmAliSlot>(), d_ok.as<uint32_t>(), max_env, d_ptr.as<uint32_t>(),
                                                                                                            d_arows.as<int2>(), d_keep.as<int32_t>(), slot_dev, col_dev);
            GS_HIP_CHECK(hipGetLastError());
            return GS_OK;
        });
}

// ---- the bodies of the ABI pairs: in.host says which entry called -----------------------------------------------------------------------------------
// The four pairs that score every (record, profile) pair: gs_hmm_search (Viterbi), gs_hmm_search_msv (MSV; SPEC 13.3), gs_hmm_search_forward (Viterbi,
// then Forward for the pairs at or above vit_floor; SPEC 13.1) and gs_hmm_search_filtered (MSV, Viterbi at or above msv_floor and, with fwd_out, Forward
// as before). A floor of nullptr takes every pair that has the score in front of it; a pair that is not taken gets GS_HMM_NO_SCORE. `needed` is the output
// the pair cannot do without; a matrix that has to be computed although the caller did not ask for it goes to its slot.
static int hmm_scores_form(gs_ctx *c, gs_hmm_db *db, const HmmIn &in, bool run_msv, bool run_vit, const int32_t *msv_floor, const int32_t *vit_floor,
                           int32_t *msv_out, int32_t *vit_out, int32_t *fwd_out, const void *needed)
{
    GS_REQUIRE(c && db && db->ctx == c, GS_ERR_INVALID, "hmm: null argument, or a profile set of another context");
    if (in.n_rec == 0) return GS_OK;
    GS_REQUIRE(in.given() && needed, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(in.n_rec < (1ull << 32), GS_ERR_UNSUPPORTED, "hmm: 2^32 records or more in one call");
    const uint32_t max_l = fwd_out ? GS_HMM_FWD_MAX_L : GS_HMM_MAX_L;
    const uint64_t np = db->models.size(), n_bytes = 4 * in.n_rec * np;
    HmmLock lock;
    HmmRecs R(c); HmmArg mfloor(c, SL_HMMB_MSV_FLOOR), floor(c, SL_HMMB_FLOOR), msv(c, SL_HMM_MSV), vit(c, SL_HMM_VIT), fwd(c, SL_HMM_FWD); HmmLists l(c);
    int rc;
    if (in.host) {                      // the lengths are judged as soon as the host has them
        if ((rc = hmm_check_lens(in.rl, in.n_rec, max_l))) return rc;
        uint64_t aa_bytes = 0;          // where the residues of all records end
        for (uint64_t r = 0; r < in.n_rec; r++) if (in.rl[r]) aa_bytes = std::max(aa_bytes, in.rs[r] + in.rl[r]);
        hmm_lock(c, lock);
        if ((rc = R.fill(in, aa_bytes))) return rc;
    } else {
        hmm_lock(c, lock);
        if ((rc = R.fill(in, 0)) || (rc = hmm_check_lens(R.lens, in.n_rec, max_l))) return rc;
    }
    const bool select_vit = run_msv && run_vit;
    if ((run_msv && (rc = msv.bind(in.host, msv_out, n_bytes, HMM_DOWN))) || (run_vit && (rc = vit.bind(in.host, vit_out, n_bytes, HMM_DOWN))) ||
        (fwd_out && (rc = fwd.bind(in.host, fwd_out, n_bytes, HMM_DOWN))) || (select_vit && msv_floor && (rc = mfloor.bind(in.host, msv_floor, 4 * np, HMM_UP))) ||
        (fwd_out && vit_floor && (rc = floor.bind(in.host, vit_floor, 4 * np, HMM_UP))))
        return rc;
    if ((run_msv && (rc = hmm_search_impl(c, db, R, msv.as<int32_t>(), l.order, true))) ||
        (run_vit && (rc = select_vit ? hmm_selected_pass(c, db, HMM_VIT, R, msv.as<int32_t>(), mfloor.as<int32_t>(), vit.as<int32_t>(), l)
                                     : hmm_search_impl(c, db, R, vit.as<int32_t>(), l.order))) ||
        (fwd_out && (rc = hmm_selected_pass(c, db, HMM_FWD, R, vit.as<int32_t>(), floor.as<int32_t>(), fwd.as<int32_t>(), l))))
        return rc;
    return in.host || select_vit || fwd_out ? hmm_fetch(c, {&msv, &vit, &fwd}) : GS_OK;       // (hmm_search_impl has waited, a selected pass is still queued)
}

// gs_hmm_search_vit16 (run_vit false: vf of every pair, SPEC 13.7) and gs_hmm_search_staged: MSV of every pair if use_msv, vf of every pair or of the
// pairs at or above msv_floor, Viterbi (k_hmm_viterbi_sel) of the pairs with vf >= vf_floor and, with fwd_out, Forward behind vit_floor as before.
static int hmm_staged_form(gs_ctx *c, gs_hmm_db *db, const HmmIn &in, bool use_msv, bool run_vit, const int32_t *msv_floor, const int32_t *vf_floor,
                           const int32_t *vit_floor, int32_t *msv_out, int32_t *vf_out, int32_t *vit_out, int32_t *fwd_out, const void *needed)
{
    GS_REQUIRE(c && db && db->ctx == c, GS_ERR_INVALID, "hmm: null argument, or a profile set of another context");
    if (in.n_rec == 0) return GS_OK;
    GS_REQUIRE(in.given() && needed, GS_ERR_INVALID, "null argument");
    GS_REQUIRE(in.n_rec < (1ull << 32), GS_ERR_UNSUPPORTED, "hmm: 2^32 records or more in one call");
    const uint32_t max_l = fwd_out ? GS_HMM_FWD_MAX_L : GS_HMM_MAX_L;
    const uint64_t np = db->models.size(), n_bytes = 4 * in.n_rec * np;
    HmmLock lock;
    HmmRecs R(c); HmmArg mfloor(c, SL_HMMB_MSV_FLOOR), vffloor(c, SL_HMMB_VF_FLOOR), floor(c, SL_HMMB_FLOOR), msv(c, SL_HMM_MSV), vf(c, SL_HMM_VF), vit(c, SL_HMM_VIT),
        fwd(c, SL_HMM_FWD);
    HmmLists l(c);
    int rc;
    if (in.host) {
        if ((rc = hmm_check_lens(in.rl, in.n_rec, max_l))) return rc;
        uint64_t aa_bytes = 0;
        for (uint64_t r = 0; r < in.n_rec; r++) if (in.rl[r]) aa_bytes = std::max(aa_bytes, in.rs[r] + in.rl[r]);
        hmm_lock(c, lock);
        if ((rc = R.fill(in, aa_bytes))) return rc;
    } else {
        hmm_lock(c, lock);
        if ((rc = R.fill(in, 0)) || (rc = hmm_check_lens(R.lens, in.n_rec, max_l))) return rc;
    }
    if ((use_msv && (rc = msv.bind(in.host, msv_out, n_bytes, HMM_DOWN))) || (rc = vf.bind(in.host, vf_out, n_bytes, HMM_DOWN)) ||
        (run_vit && (rc = vit.bind(in.host, vit_out, n_bytes, HMM_DOWN))) || (fwd_out && (rc = fwd.bind(in.host, fwd_out, n_bytes, HMM_DOWN))) ||
        (use_msv && msv_floor && (rc = mfloor.bind(in.host, msv_floor, 4 * np, HMM_UP))) || (run_vit && vf_floor && (rc = vffloor.bind(in.host, vf_floor, 4 * np, HMM_UP))) ||
        (fwd_out && vit_floor && (rc = floor.bind(in.host, vit_floor, 4 * np, HMM_UP))))
        return rc;
    if ((use_msv && ((rc = hmm_search_impl(c, db, R, msv.as<int32_t>(), l.order, true)) ||
                     (rc = hmm_selected_pass(c, db, HMM_K_VIT16_SEL, R, msv.as<int32_t>(), mfloor.as<int32_t>(), vf.as<int32_t>(), l)))) ||
        (!use_msv && (rc = hmm_search_impl(c, db, R, vf.as<int32_t>(), l.order, false, true))) ||
        (run_vit && (rc = hmm_selected_pass(c, db, HMM_VIT, R, vf.as<int32_t>(), vffloor.as<int32_t>(), vit.as<int32_t>(), l))) ||
        (fwd_out && (rc = hmm_selected_pass(c, db, HMM_FWD, R, vit.as<int32_t>(), floor.as<int32_t>(), fwd.as<int32_t>(), l))))
        return rc;
    return in.host || use_msv || run_vit ? hmm_fetch(c, {&msv, &vf, &vit, &fwd}) : GS_OK;       // (hmm_search_impl has waited, a selected pass is still queued)
}

// gs_hmm_trace{,_dev}
static int hmm_trace_form(gs_ctx *c, gs_hmm_db *db, const HmmIn &in, const uint32_t *pair_rec, const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_dom,
                          uint64_t max_block_cells, int32_t *raw_out, uint32_t *n_dom_out, int32_t *dom_out)
{
    HmmLock lock;
    HmmRecs R(c); HmmPairs P(c); HmmArg raw(c, SL_HMMB_PAIR_SCORE), nd(c, SL_HMMB_PAIR_COUNT), dom(c, SL_HMMB_PAIR_ITEMS);
    std::vector<uint64_t> no_rows;
    int rc = hmm_pair_args(c, db, in, pair_rec, pair_prof, n_pairs, raw_out && n_dom_out && (dom_out || max_dom == 0), true, GS_HMM_TRACE_MAX_L, true, nullptr, no_rows, lock, R, P);
    if (rc) return rc == HMM_NOTHING_TO_DO ? GS_OK : rc;
    if ((rc = raw.bind(in.host, raw_out, 4 * n_pairs, HMM_DOWN)) || (rc = nd.bind(in.host, n_dom_out, 4 * n_pairs, HMM_DOWN)) ||
        (rc = dom.bind(in.host, dom_out, 4 * n_pairs * max_dom * GS_HMM_DOM_WORDS, HMM_DOWN)) ||
        (rc = hmm_trace_impl(c, db, R, P, max_dom, max_block_cells, raw.as<int32_t>(), nd.as<uint32_t>(), dom.as<int32_t>())))
        return rc;
    return in.host ? hmm_fetch(c, {&raw, &nd, &dom}) : GS_OK;     // (hmm_trace_impl has waited)
}

// gs_hmm_envelopes{,_dev}. A host form uploads out_rows and cont_rows too: the rows of a pair that gets none keep what the caller's arrays hold.
static int hmm_env_form(gs_ctx *c, gs_hmm_db *db, const HmmIn &in, const uint32_t *pair_rec, const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env,
                        uint64_t max_block_rows, int32_t *fwd_out, int32_t *bck_out, uint32_t *n_env_out, int32_t *env_out, const uint64_t *row_off, int32_t *out_rows,
                        int32_t *cont_rows)
{
    HmmLock lock;
    HmmRecs R(c); HmmPairs P(c);
    HmmArg fwd(c, SL_HMMB_PAIR_SCORE), bck(c, SL_HMMB_PAIR_BCK), ne(c, SL_HMMB_PAIR_COUNT), env(c, SL_HMMB_PAIR_ITEMS), ro(c, SL_HMMB_ROW_OFF), out(c, SL_HMMB_OUT_ROWS),
        cont(c, SL_HMMB_CONT_ROWS);
    std::vector<uint64_t> ro_host;
    int rc = hmm_pair_args(c, db, in, pair_rec, pair_prof, n_pairs, fwd_out && bck_out && n_env_out && (env_out || max_env == 0),
                           !row_off == !out_rows && !row_off == !cont_rows, GS_HMM_FWD_MAX_L, false, row_off, ro_host, lock, R, P);
    if (rc) return rc == HMM_NOTHING_TO_DO ? GS_OK : rc;
    const uint64_t n_row_bytes = in.host && row_off ? 4 * row_off[n_pairs] : 0;
    if ((rc = fwd.bind(in.host, fwd_out, 4 * n_pairs, HMM_DOWN)) || (rc = bck.bind(in.host, bck_out, 4 * n_pairs, HMM_DOWN)) ||
        (rc = ne.bind(in.host, n_env_out, 4 * n_pairs, HMM_DOWN)) || (rc = env.bind(in.host, env_out, 4 * n_pairs * max_env * GS_HMM_ENV_WORDS, HMM_DOWN)))
        return rc;
    if (row_off && ((rc = ro.bind(in.host, row_off, 8 * (n_pairs + 1), HMM_UP)) || (rc = out.bind(in.host, out_rows, n_row_bytes, HMM_UP | HMM_DOWN)) ||
                    (rc = cont.bind(in.host, cont_rows, n_row_bytes, HMM_UP | HMM_DOWN))))
        return rc;
    if ((rc = hmm_env_impl(c, db, R, P, max_env, max_block_rows, fwd.as<int32_t>(), bck.as<int32_t>(), ne.as<uint32_t>(), env.as<int32_t>(), ro.as<uint64_t>(), out.as<int32_t>(),
                           cont.as<int32_t>())))
        return rc;
    return in.host ? hmm_fetch(c, {&fwd, &bck, &ne, &env, &out, &cont}) : GS_OK;        // (hmm_env_impl has waited)
}

// gs_hmm_null2{,_dev}. n_env and env come as gs_hmm_envelopes wrote them; a _dev form fetches them, and occ_off, once. A host form uploads occm and occi too:
// the rows of a pair that gets none keep what the caller's arrays hold.
static int hmm_null2_form(gs_ctx *c, gs_hmm_db *db, const HmmIn &in, const uint32_t *pair_rec, const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env,
                          uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env, int32_t *slot_out, int32_t *seq_out, int32_t *n2_out, const uint64_t *occ_off,
                          int32_t *occm_out, int32_t *occi_out)
{
    HmmLock lock;
    HmmRecs R(c); HmmPairs P(c);
    HmmArg slot(c, SL_HMMB_PAIR_ITEMS), seq(c, SL_HMMB_PAIR_SCORE), n2(c, SL_HMMB_PAIR_N2), om(c, SL_HMMB_OUT_ROWS), oi(c, SL_HMMB_CONT_ROWS);
    std::vector<uint64_t> no_rows, h_oo;
    std::vector<uint32_t> h_nenv;
    std::vector<int32_t> h_env;
    int rc = hmm_pair_args(c, db, in, pair_rec, pair_prof, n_pairs, seq_out && n_env && (max_env == 0 || (env && slot_out)), !occ_off == !occm_out && !occ_off == !occi_out,
                           GS_HMM_FWD_MAX_L, false, nullptr, no_rows, lock, R, P);
    if (rc) return rc == HMM_NOTHING_TO_DO ? GS_OK : rc;
    const uint64_t n_env_words = n_pairs * max_env * GS_HMM_ENV_WORDS;
    if (!in.host) {
        h_nenv.resize(n_pairs); h_env.resize(n_env_words);
        GS_HIP_CHECK(hipMemcpyAsync(h_nenv.data(), n_env, 4 * n_pairs, hipMemcpyDeviceToHost, c->stream));
        if (n_env_words) GS_HIP_CHECK(hipMemcpyAsync(h_env.data(), env, 4 * n_env_words, hipMemcpyDeviceToHost, c->stream));
        if (occ_off) {
            h_oo.resize(n_pairs + 1);
            GS_HIP_CHECK(hipMemcpyAsync(h_oo.data(), occ_off, 8 * (n_pairs + 1), hipMemcpyDeviceToHost, c->stream));
        }
        GS_HIP_CHECK(stream_wait(c));
        n_env = h_nenv.data(); env = h_env.data();
    }
    const uint64_t *oo = !occ_off ? nullptr : in.host ? occ_off : h_oo.data();
    if ((rc = hmm_null2_check(db, R.lens, P.rec, P.prof, n_pairs, max_env, n_env, env, oo))) return rc;
    const uint64_t n_row_bytes = in.host && oo ? 4 * oo[n_pairs] : 0;
    if ((rc = slot.bind(in.host, slot_out, 4 * n_pairs * max_env * GS_HMM_N2_WORDS, HMM_DOWN)) || (rc = seq.bind(in.host, seq_out, 4 * n_pairs, HMM_DOWN)) ||
        (n2_out && (rc = n2.bind(in.host, n2_out, 4 * n_pairs * max_env * 20, HMM_DOWN))))
        return rc;
    if (oo && ((rc = om.bind(in.host, occm_out, n_row_bytes, HMM_UP | HMM_DOWN)) || (rc = oi.bind(in.host, occi_out, n_row_bytes, HMM_UP | HMM_DOWN)))) return rc;
    if ((rc = hmm_null2_impl(c, db, R, P, max_env, max_block_cells, n_env, env, oo, slot.as<int32_t>(), seq.as<int32_t>(), n2.as<int32_t>(), om.as<int32_t>(), oi.as<int32_t>())))
        return rc;
    return in.host ? hmm_fetch(c, {&slot, &seq, &n2, &om, &oi}) : GS_OK;          // (hmm_null2_impl has waited)
}

// gs_hmm_align{,_dev}. n_env and env as for null2; a _dev form fetches them, and col_off, once. A host form uploads col_out too: the columns no slot
// writes keep what the caller's array holds.
static int hmm_align_form(gs_ctx *c, gs_hmm_db *db, const HmmIn &in, const uint32_t *pair_rec, const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env,
                          uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env, int32_t *slot_out, const uint64_t *col_off, int32_t *col_out)
{
    HmmLock lock;
    HmmRecs R(c); HmmPairs P(c);
    HmmArg slot(c, SL_HMMB_PAIR_ITEMS), cols(c, SL_HMMB_PAIR_COLS);
    std::vector<uint64_t> no_rows, h_co;
    std::vector<uint32_t> h_nenv;
    std::vector<int32_t> h_env;
    int rc = hmm_pair_args(c, db, in, pair_rec, pair_prof, n_pairs, n_env && (max_env == 0 || (env && slot_out)), !col_off == !col_out, GS_HMM_FWD_MAX_L, true, nullptr, no_rows,
                           lock, R, P);
    if (rc) return rc == HMM_NOTHING_TO_DO ? GS_OK : rc;
    const uint64_t n_env_words = n_pairs * max_env * GS_HMM_ENV_WORDS;
    if (!in.host) {
        h_nenv.resize(n_pairs); h_env.resize(n_env_words);
        GS_HIP_CHECK(hipMemcpyAsync(h_nenv.data(), n_env, 4 * n_pairs, hipMemcpyDeviceToHost, c->stream));
        if (n_env_words) GS_HIP_CHECK(hipMemcpyAsync(h_env.data(), env, 4 * n_env_words, hipMemcpyDeviceToHost, c->stream));
        if (col_off) {
            h_co.resize(n_pairs + 1);
            GS_HIP_CHECK(hipMemcpyAsync(h_co.data(), col_off, 8 * (n_pairs + 1), hipMemcpyDeviceToHost, c->stream));
        }
        GS_HIP_CHECK(stream_wait(c));
        n_env = h_nenv.data(); env = h_env.data();
    }
    const uint64_t *co = !col_off ? nullptr : in.host ? col_off : h_co.data();
    if ((rc = hmm_null2_check(db, R.lens, P.rec, P.prof, n_pairs, max_env, n_env, env, nullptr)) ||
        (rc = hmm_align_check(db, R.lens, P.rec, P.prof, n_pairs, max_env, n_env, env, co)))
        return rc;
    if ((rc = slot.bind(in.host, slot_out, 4 * n_pairs * max_env * GS_HMM_ALI_WORDS, HMM_DOWN)) ||
        (co && (rc = cols.bind(in.host, col_out, in.host ? 8 * co[n_pairs] : 0, HMM_UP | HMM_DOWN))))
        return rc;
    if ((rc = hmm_align_impl(c, db, R, P, max_env, max_block_cells, n_env, env, co, slot.as<int32_t>(), co ? cols.as<int32_t>() : nullptr))) return rc;
    return in.host ? hmm_fetch(c, {&slot, &cols}) : GS_OK;                        // (hmm_align_impl has waited)
}

}  // namespace gs

extern "C" {

int gs_hmm_align_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec, const uint32_t *pair_rec_dev,
                     const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env_dev, const int32_t *env_dev,
                     int32_t *slot_out_dev, const uint64_t *col_off_dev, int32_t *col_out_dev)
{
    return gs::hmm_align_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, pair_rec_dev, pair_prof_dev, n_pairs, max_env, max_block_cells, n_env_dev, env_dev,
                              slot_out_dev, col_off_dev, col_out_dev);
}
int gs_hmm_align(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                 const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env, int32_t *slot_out,
                 const uint64_t *col_off, int32_t *col_out)
{
    return gs::hmm_align_form(c, db, {true, aa, rec_start, rec_len, n_rec}, pair_rec, pair_prof, n_pairs, max_env, max_block_cells, n_env, env, slot_out, col_off, col_out);
}

int gs_hmm_null2_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec, const uint32_t *pair_rec_dev,
                     const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env_dev, const int32_t *env_dev,
                     int32_t *slot_out_dev, int32_t *seq_bias_out_dev, int32_t *n2_out_dev, const uint64_t *occ_off_dev, int32_t *occm_out_dev, int32_t *occi_out_dev)
{
    return gs::hmm_null2_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, pair_rec_dev, pair_prof_dev, n_pairs, max_env, max_block_cells, n_env_dev, env_dev,
                              slot_out_dev, seq_bias_out_dev, n2_out_dev, occ_off_dev, occm_out_dev, occi_out_dev);
}
int gs_hmm_null2(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                 const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_cells, const uint32_t *n_env, const int32_t *env, int32_t *slot_out,
                 int32_t *seq_bias_out, int32_t *n2_out, const uint64_t *occ_off, int32_t *occm_out, int32_t *occi_out)
{
    return gs::hmm_null2_form(c, db, {true, aa, rec_start, rec_len, n_rec}, pair_rec, pair_prof, n_pairs, max_env, max_block_cells, n_env, env, slot_out, seq_bias_out, n2_out,
                              occ_off, occm_out, occi_out);
}

int gs_hmm_db_load_mem(gs_ctx *c, const void *const *texts, const uint64_t *n_bytes, uint64_t n_texts, gs_hmm_db **out)
{
    using namespace gs;
    GS_REQUIRE(c && out && n_texts >= 1 && texts && n_bytes, GS_ERR_INVALID, "null argument");
    *out = nullptr;
    std::vector<HmmModel> ms;
    for (uint64_t i = 0; i < n_texts; i++) {
        GS_REQUIRE(texts[i] || n_bytes[i] == 0, GS_ERR_INVALID, "null text %llu", (unsigned long long)i);
        int rc = hmm_parse_all((const char *)texts[i], (size_t)n_bytes[i], ms);
        if (rc) return rc;
    }
    return hmm_db_build(c, std::move(ms), out);
}

int gs_hmm_db_load(gs_ctx *c, const char *const *paths, uint64_t n_paths, gs_hmm_db **out)
{
    using namespace gs;
    GS_REQUIRE(c && out && n_paths >= 1 && paths, GS_ERR_INVALID, "null argument");
    *out = nullptr;
    std::vector<HmmModel> ms;
    for (uint64_t i = 0; i < n_paths; i++) {
        GS_REQUIRE(paths[i], GS_ERR_INVALID, "null path %llu", (unsigned long long)i);
        FILE *fp = fopen(paths[i], "rb");
        GS_REQUIRE(fp, GS_ERR_IO, "cannot open %s", paths[i]);
        std::string text;
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
        const bool failed = ferror(fp) != 0;
        fclose(fp);
        GS_REQUIRE(!failed, GS_ERR_IO, "cannot read %s", paths[i]);
        int rc = hmm_parse_all(text.data(), text.size(), ms);
        if (rc) return rc;
    }
    return hmm_db_build(c, std::move(ms), out);
}

void gs_hmm_db_free(gs_hmm_db *db)
{
    if (!db) return;
    { GS_CTX_LOCK(db->ctx); (void)gs::stream_wait(db->ctx); }
    delete db;
}

int gs_hmm_db_info(gs_hmm_db *db, uint64_t *n_prof_out, gs_hmm_info *info_out, uint64_t cap)
{
    GS_REQUIRE(db && n_prof_out, GS_ERR_INVALID, "null argument");
    *n_prof_out = db->models.size();
    if (info_out) for (uint64_t p = 0; p < cap && p < db->models.size(); p++) info_out[p] = db->models[p].info;
    return GS_OK;
}

int gs_hmm_db_tables(gs_hmm_db *db, uint64_t p, int32_t *tables_out, uint64_t cap_words)
{
    using namespace gs;
    GS_REQUIRE(db && tables_out && p < db->models.size(), GS_ERR_INVALID, "bad argument");
    const HmmModel &m = db->models[p];
    const uint32_t M = m.info.M, W = M + 1;
    GS_REQUIRE(cap_words >= (uint64_t)GS_HMM_TABLE_ROWS * W, GS_ERR_INVALID, "hmm: the table needs %llu words", (unsigned long long)GS_HMM_TABLE_ROWS * W);
    gs_ctx *c = db->ctx;
    GS_CTX_LOCK(c);
    const int MP = 64 * HMM_CLASS_Q[hmm_class_of(M)];
    std::vector<int32_t> dev((size_t)HMM_ROWS_DEV * MP);
    GS_HIP_CHECK(hipMemcpyAsync(dev.data(), db->d_tables.as<int32_t>() + db->desc[p].off, 4 * dev.size(), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    for (uint32_t row = 0; row < GS_HMM_TABLE_ROWS; row++) {
        tables_out[(size_t)row * W] = m.tab[(size_t)row * W];                 // node 0 is not on the device: no state of it exists (SPEC 13)
        for (uint32_t k = 1; k <= M; k++) tables_out[(size_t)row * W + k] = dev[(size_t)row * MP + (k - 1)];
    }
    return GS_OK;
}

int gs_hmm_db_tables16(gs_hmm_db *db, uint64_t p, int16_t *tables_out, uint64_t cap_words)
{
    using namespace gs;
    GS_REQUIRE(db && tables_out && p < db->models.size(), GS_ERR_INVALID, "bad argument");
    const HmmModel &m = db->models[p];
    const uint32_t M = m.info.M, W = M + 1;
    GS_REQUIRE(cap_words >= (uint64_t)GS_HMM_TABLE_ROWS * W, GS_ERR_INVALID, "hmm: the table needs %llu words", (unsigned long long)GS_HMM_TABLE_ROWS * W);
    gs_ctx *c = db->ctx;
    GS_CTX_LOCK(c);
    const int H = hmm16_regs(HMM_CLASS_Q[hmm_class_of(M)]), RW = 64 * H;
    std::vector<uint32_t> dev((size_t)HMM16_ROWS * RW);
    GS_HIP_CHECK(hipMemcpyAsync(dev.data(), db->d_tables16.as<uint32_t>() + db->desc16[p].off, 4 * dev.size(), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    for (uint32_t row = 0; row < GS_HMM_TABLE_ROWS; row++) {
        tables_out[(size_t)row * W] = (int16_t)hmm16_half(m.tab[(size_t)row * W]);           // node 0 is not on the device (SPEC 13)
        for (uint32_t k = 1; k <= M; k++) {
            const uint32_t w = dev[(size_t)row * RW + hmm16_word(H, (int)k - 1)];
            tables_out[(size_t)row * W + k] = (int16_t)(hmm16_high(H, (int)k - 1) ? w >> 16 : w & 0xFFFFu);
        }
    }
    return GS_OK;
}

int gs_hmm_db_consensus(gs_hmm_db *db, uint64_t p, char *out, uint64_t cap)
{
    using namespace gs;
    GS_REQUIRE(db && out && p < db->models.size(), GS_ERR_INVALID, "bad argument");
    const HmmModel &m = db->models[p];
    const uint32_t M = m.info.M, W = M + 1;
    GS_REQUIRE(cap >= M, GS_ERR_INVALID, "hmm: the consensus has %u letters, cap = %llu", M, (unsigned long long)cap);
    static const int32_t bg[20] = GS_HMM_BG_LIST;
    static const char aa[] = "ACDEFGHIKLMNPQRSTVWY";
    for (uint32_t k = 1; k <= M; k++) {             // the most probable residue: match score plus background, the first in alphabet order on a tie
        int best = 0;
        for (int a = 1; a < 20; a++)
            if ((int64_t)m.tab[(size_t)a * W + k] + bg[a] > (int64_t)m.tab[(size_t)best * W + k] + bg[best]) best = a;
        out[k - 1] = aa[best];
    }
    return GS_OK;
}

int gs_hmm_search_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec, int32_t *score_out_dev)
{
    return gs::hmm_scores_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, false, true, nullptr, nullptr, nullptr, score_out_dev, nullptr, score_out_dev);
}
int gs_hmm_search(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int32_t *score_out)
{
    return gs::hmm_scores_form(c, db, {true, aa, rec_start, rec_len, n_rec}, false, true, nullptr, nullptr, nullptr, score_out, nullptr, score_out);
}
int gs_hmm_search_msv_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec, int32_t *msv_out_dev)
{
    return gs::hmm_scores_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, true, false, nullptr, nullptr, msv_out_dev, nullptr, nullptr, msv_out_dev);
}
int gs_hmm_search_msv(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int32_t *msv_out)
{
    return gs::hmm_scores_form(c, db, {true, aa, rec_start, rec_len, n_rec}, true, false, nullptr, nullptr, msv_out, nullptr, nullptr, msv_out);
}

int gs_hmm_best_hits_dev(gs_ctx *c, gs_hmm_db *db, const int32_t *score_dev, uint64_t n_rec, const uint64_t *genome_rec_off_dev, uint64_t n_genomes,
                         const int32_t *thr_dev, uint32_t *best_rec_out, int32_t *best_score_out)
{
    using namespace gs;
    GS_REQUIRE(c && db && db->ctx == c, GS_ERR_INVALID, "hmm: null argument, or a profile set of another context");
    if (n_genomes == 0) return GS_OK;
    GS_REQUIRE(genome_rec_off_dev && best_rec_out && best_score_out && (score_dev || n_rec == 0), GS_ERR_INVALID, "null argument");
    GS_REQUIRE(n_rec < (1ull << 32), GS_ERR_UNSUPPORTED, "hmm: 2^32 records or more in one call");
    GS_REQUIRE(thr_dev || db->all_ga, GS_ERR_INVALID, "hmm: a profile of the set has no GA cutoff: give thresholds");
    const uint64_t np = db->models.size(), n = n_genomes * np;
    GS_REQUIRE(n < (1ull << 31) * 256, GS_ERR_UNSUPPORTED, "hmm: too many (genome, profile) pairs");
    GS_CTX_LOCK(c);
    std::vector<uint64_t> off(n_genomes + 1);
    GS_HIP_CHECK(hipMemcpyAsync(off.data(), genome_rec_off_dev, 8 * (n_genomes + 1), hipMemcpyDeviceToHost, c->stream));
    GS_HIP_CHECK(stream_wait(c));
    for (uint64_t g = 0; g < n_genomes; g++) GS_REQUIRE(off[g] <= off[g + 1], GS_ERR_INVALID, "hmm: genome offsets decrease at genome %llu", (unsigned long long)g);
    GS_REQUIRE(off[n_genomes] <= n_rec, GS_ERR_INVALID, "hmm: genome offsets end at %llu, past n_rec = %llu", (unsigned long long)off[n_genomes], (unsigned long long)n_rec);
    {
        ProfScope ps(c, FAM_SEARCH);
        k_hmm_best<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(score_dev, genome_rec_off_dev, n_genomes, (uint32_t)np, thr_dev ? thr_dev : db->d_ga.as<int32_t>(),
                                                                      best_rec_out, best_score_out);
        GS_HIP_CHECK(hipGetLastError());
    }
    GS_HIP_CHECK(stream_wait(c));
    return GS_OK;
}

int gs_hmm_search_forward_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                              const int32_t *vit_floor_dev, int32_t *vit_out_dev, int32_t *fwd_out_dev)
{
    return gs::hmm_scores_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, false, true, nullptr, vit_floor_dev, nullptr, vit_out_dev, fwd_out_dev, fwd_out_dev);
}
int gs_hmm_search_forward(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const int32_t *vit_floor,
                          int32_t *vit_out, int32_t *fwd_out)
{
    return gs::hmm_scores_form(c, db, {true, aa, rec_start, rec_len, n_rec}, false, true, nullptr, vit_floor, nullptr, vit_out, fwd_out, fwd_out);
}

int gs_hmm_search_filtered_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                               const int32_t *msv_floor_dev, const int32_t *vit_floor_dev, int32_t *msv_out_dev, int32_t *vit_out_dev, int32_t *fwd_out_dev)
{
    return gs::hmm_scores_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, true, true, msv_floor_dev, vit_floor_dev, msv_out_dev, vit_out_dev, fwd_out_dev, vit_out_dev);
}
int gs_hmm_search_filtered(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const int32_t *msv_floor,
                           const int32_t *vit_floor, int32_t *msv_out, int32_t *vit_out, int32_t *fwd_out)
{
    return gs::hmm_scores_form(c, db, {true, aa, rec_start, rec_len, n_rec}, true, true, msv_floor, vit_floor, msv_out, vit_out, fwd_out, vit_out);
}

int gs_hmm_search_vit16_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec, int32_t *vf_out_dev)
{
    return gs::hmm_staged_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, false, false, nullptr, nullptr, nullptr, nullptr, vf_out_dev, nullptr, nullptr, vf_out_dev);
}
int gs_hmm_search_vit16(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int32_t *vf_out)
{
    return gs::hmm_staged_form(c, db, {true, aa, rec_start, rec_len, n_rec}, false, false, nullptr, nullptr, nullptr, nullptr, vf_out, nullptr, nullptr, vf_out);
}
int gs_hmm_search_staged_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec, int use_msv,
                             const int32_t *msv_floor_dev, const int32_t *vf_floor_dev, const int32_t *vit_floor_dev, int32_t *msv_out_dev, int32_t *vf_out_dev,
                             int32_t *vit_out_dev, int32_t *fwd_out_dev)
{
    return gs::hmm_staged_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, use_msv != 0, true, msv_floor_dev, vf_floor_dev, vit_floor_dev, msv_out_dev, vf_out_dev,
                               vit_out_dev, fwd_out_dev, vit_out_dev);
}
int gs_hmm_search_staged(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, int use_msv,
                         const int32_t *msv_floor, const int32_t *vf_floor, const int32_t *vit_floor, int32_t *msv_out, int32_t *vf_out, int32_t *vit_out, int32_t *fwd_out)
{
    return gs::hmm_staged_form(c, db, {true, aa, rec_start, rec_len, n_rec}, use_msv != 0, true, msv_floor, vf_floor, vit_floor, msv_out, vf_out, vit_out, fwd_out, vit_out);
}

int gs_hmm_trace_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                     const uint32_t *pair_rec_dev, const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_dom, uint64_t max_block_cells, int32_t *raw_out_dev,
                     uint32_t *n_dom_out_dev, int32_t *dom_out_dev)
{
    return gs::hmm_trace_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, pair_rec_dev, pair_prof_dev, n_pairs, max_dom, max_block_cells, raw_out_dev,
                              n_dom_out_dev, dom_out_dev);
}
int gs_hmm_trace(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                 const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_dom, uint64_t max_block_cells, int32_t *raw_out, uint32_t *n_dom_out, int32_t *dom_out)
{
    return gs::hmm_trace_form(c, db, {true, aa, rec_start, rec_len, n_rec}, pair_rec, pair_prof, n_pairs, max_dom, max_block_cells, raw_out, n_dom_out, dom_out);
}

int gs_hmm_envelopes_dev(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa_dev, const uint64_t *rec_start_dev, const uint64_t *rec_len_dev, uint64_t n_rec,
                         const uint32_t *pair_rec_dev, const uint32_t *pair_prof_dev, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_rows, int32_t *fwd_out_dev,
                         int32_t *bck_out_dev, uint32_t *n_env_out_dev, int32_t *env_out_dev, const uint64_t *row_off_dev, int32_t *out_rows_dev, int32_t *cont_rows_dev)
{
    return gs::hmm_env_form(c, db, {false, aa_dev, rec_start_dev, rec_len_dev, n_rec}, pair_rec_dev, pair_prof_dev, n_pairs, max_env, max_block_rows, fwd_out_dev,
                            bck_out_dev, n_env_out_dev, env_out_dev, row_off_dev, out_rows_dev, cont_rows_dev);
}
int gs_hmm_envelopes(gs_ctx *c, gs_hmm_db *db, const uint8_t *aa, const uint64_t *rec_start, const uint64_t *rec_len, uint64_t n_rec, const uint32_t *pair_rec,
                     const uint32_t *pair_prof, uint64_t n_pairs, uint32_t max_env, uint64_t max_block_rows, int32_t *fwd_out, int32_t *bck_out, uint32_t *n_env_out,
                     int32_t *env_out, const uint64_t *row_off, int32_t *out_rows, int32_t *cont_rows)
{
    return gs::hmm_env_form(c, db, {true, aa, rec_start, rec_len, n_rec}, pair_rec, pair_prof, n_pairs, max_env, max_block_rows, fwd_out, bck_out, n_env_out, env_out,
                            row_off, out_rows, cont_rows);
}

}  // extern "C"
