// micro-benchmark: issue rate of the integer VALU instructions the sketch kernels lean on (gfx950).
// build: hipcc -O3 --offload-arch=gfx950 tools/ubench_valu.hip -o tools/ubench_valu ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#define REP 64
#define ITERS 4096
template <int OP>
__global__ __launch_bounds__(256) void k(uint32_t *out, uint32_t seed)
{
    uint32_t a0 = threadIdx.x + seed, a1 = a0 * 3 + 1, a2 = a0 ^ 0x1234567, a3 = a0 + 77, b = seed | 1, c = seed + 5;
    uint64_t q0 = ((uint64_t)a0 << 32) | a1, q1 = ((uint64_t)a2 << 32) | a3, q2 = q0 * 3, q3 = q1 + 9;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int r = 0; r < REP / 4; r++) {
            if (OP == 0) { asm volatile("v_xor_b32 %0, %0, %1" : "+v"(a0) : "v"(b)); asm volatile("v_xor_b32 %0, %0, %1" : "+v"(a1) : "v"(b)); asm volatile("v_xor_b32 %0, %0, %1" : "+v"(a2) : "v"(b)); asm volatile("v_xor_b32 %0, %0, %1" : "+v"(a3) : "v"(b)); }
            if (OP == 1) { asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a0) : "v"(b)); asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a1) : "v"(b)); asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a2) : "v"(b)); asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a3) : "v"(b)); }
            if (OP == 2) { asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a0) : "v"(b)); asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a1) : "v"(b)); asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a2) : "v"(b)); asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a3) : "v"(b)); }
            if (OP == 3) { asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(q0) : "v"(b), "v"(c) : "vcc"); asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(q1) : "v"(b), "v"(c) : "vcc"); asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(q2) : "v"(b), "v"(c) : "vcc"); asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(q3) : "v"(b), "v"(c) : "vcc"); }
            if (OP == 4) { asm volatile("v_lshrrev_b64 %0, 7, %0" : "+v"(q0)); asm volatile("v_lshrrev_b64 %0, 7, %0" : "+v"(q1)); asm volatile("v_lshrrev_b64 %0, 7, %0" : "+v"(q2)); asm volatile("v_lshrrev_b64 %0, 7, %0" : "+v"(q3)); }
            if (OP == 5) { asm volatile("v_alignbit_b32 %0, %0, %1, 7" : "+v"(a0) : "v"(b)); asm volatile("v_alignbit_b32 %0, %0, %1, 7" : "+v"(a1) : "v"(b)); asm volatile("v_alignbit_b32 %0, %0, %1, 7" : "+v"(a2) : "v"(b)); asm volatile("v_alignbit_b32 %0, %0, %1, 7" : "+v"(a3) : "v"(b)); }
            if (OP == 6) { asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a0) : "v"(b)); asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a1) : "v"(b)); asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a2) : "v"(b)); asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a3) : "v"(b)); }
            if (OP == 7) { asm volatile("v_lshl_add_u64 %0, %0, 3, %1" : "+v"(q0) : "v"(q3)); asm volatile("v_lshl_add_u64 %0, %0, 3, %1" : "+v"(q1) : "v"(q3)); asm volatile("v_lshl_add_u64 %0, %0, 3, %1" : "+v"(q2) : "v"(q3)); asm volatile("v_lshl_add_u64 %0, %0, 3, %1" : "+v"(q0) : "v"(q3)); }
            if (OP == 8) { asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(a0) : "v"(b), "v"(c)); asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(a1) : "v"(b), "v"(c)); asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(a2) : "v"(b), "v"(c)); asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(a3) : "v"(b), "v"(c)); }
            if (OP == 9) { asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a0) : "v"(b), "v"(c)); asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a1) : "v"(b), "v"(c)); asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a2) : "v"(b), "v"(c)); asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a3) : "v"(b), "v"(c)); }
            if (OP == 10) { asm volatile("v_lshlrev_b64 %0, 7, %0" : "+v"(q0)); asm volatile("v_lshlrev_b64 %0, 7, %0" : "+v"(q1)); asm volatile("v_lshlrev_b64 %0, 7, %0" : "+v"(q2)); asm volatile("v_lshlrev_b64 %0, 7, %0" : "+v"(q3)); }
            if (OP == 12) { asm volatile("v_add_u32 %0, %0, %1" : "+v"(a0) : "v"(b)); asm volatile("v_add_u32 %0, %0, %1" : "+v"(a1) : "v"(b)); asm volatile("v_add_u32 %0, %0, %1" : "+v"(a2) : "v"(b)); asm volatile("v_add_u32 %0, %0, %1" : "+v"(a3) : "v"(b)); }
            if (OP == 13) { asm volatile("v_mov_b32 %0, %1" : "=v"(a0) : "v"(a1)); asm volatile("v_mov_b32 %0, %1" : "=v"(a1) : "v"(a2)); asm volatile("v_mov_b32 %0, %1" : "=v"(a2) : "v"(a3)); asm volatile("v_mov_b32 %0, %1" : "=v"(a3) : "v"(a0)); }
            if (OP == 14) { asm volatile("v_dot2_u32_u16 %0, %0, %1, %2" : "+v"(a0) : "v"(b), "v"(c)); asm volatile("v_dot2_u32_u16 %0, %0, %1, %2" : "+v"(a1) : "v"(b), "v"(c)); asm volatile("v_dot2_u32_u16 %0, %0, %1, %2" : "+v"(a2) : "v"(b), "v"(c)); asm volatile("v_dot2_u32_u16 %0, %0, %1, %2" : "+v"(a3) : "v"(b), "v"(c)); }
            if (OP == 15) { asm volatile("v_lshrrev_b32 %0, 7, %0" : "+v"(a0)); asm volatile("v_lshrrev_b32 %0, 7, %0" : "+v"(a1)); asm volatile("v_lshrrev_b32 %0, 7, %0" : "+v"(a2)); asm volatile("v_lshrrev_b32 %0, 7, %0" : "+v"(a3)); }
            if (OP == 11) { asm volatile("v_cmp_lt_u64 vcc, %0, %1" :: "v"(q0), "v"(q1) : "vcc"); asm volatile("v_cmp_lt_u64 vcc, %0, %1" :: "v"(q2), "v"(q3) : "vcc"); asm volatile("v_cmp_lt_u64 vcc, %0, %1" :: "v"(q0), "v"(q3) : "vcc"); asm volatile("v_cmp_lt_u64 vcc, %0, %1" :: "v"(q1), "v"(q2) : "vcc"); }
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ (uint32_t)q0 ^ (uint32_t)q1 ^ (uint32_t)q2 ^ (uint32_t)q3;
}

// Whole 64 x 64 -> 64 multiplies by a constant C = ch:cl (in SGPRs), each chain x <- x * C, four independent chains per wave. Registers are fixed
// (chain c: X = v[b:b+1], Y = v[b+2:b+3], T = v[b+4:b+5], Z = v[b+6:b+7], b = 40 + 8c; Z.lo = 0): a pair operand must be even-aligned on gfx950,
// and the forms differ in which half of a pair the cross term lands. One loop step is X -> Y -> X, so every form renames as the compiler would.
//   SEQ 0  hipcc:  Y = mad_u64(xl, cl, 0); t1 = mul_lo(xh, cl); t2 = mul_lo(xl, ch); Y.hi = add3(Y.hi, t1, t2)
//   SEQ 1  A:      T.lo = mul_lo(xl, ch); T = mad_u64(xh, cl, T); Y = mad_u64(xl, cl, 0); Y.hi = add(Y.hi, T.lo)
//   SEQ 2  B:      T.lo = mul_lo(xl, ch); T = mad_u64(xh, cl, T); Z.hi = mov(T.lo); Y = mad_u64(xl, cl, Z)
//   SEQ 4  B0:     B with the zero of Z.lo moved in again per multiply (what hipcc makes of the C++ form whose sum is left to it)
//   SEQ 5  Bg:     B whose Z.hi is the cross sum + a constant (an addend a = ah:0 folded in by a v_add_u32 instead of the move)
//   SEQ 3  B':     Z.hi = mul_lo(xl, ch) ... two mul_lo into T, Z.hi = add(T.lo, T.hi); Y = mad_u64(xl, cl, Z)
#define GS_STR2(x) #x
#define GS_STR(x) GS_STR2(x)
#define MUL_HIPCC(X0, X1, Y0, Y1, T0, T1, Z0, Z1) \
    "v_mad_u64_u32 v[" #Y0 ":" #Y1 "], vcc, v" #X0 ", %[cl], 0\n v_mul_lo_u32 v" #T0 ", v" #X1 ", %[cl]\n v_mul_lo_u32 v" #T1 ", v" #X0 ", %[ch]\n v_add3_u32 v" #Y1 ", v" #Y1 ", v" #T0 ", v" #T1 "\n"
#define MUL_A(X0, X1, Y0, Y1, T0, T1, Z0, Z1) \
    "v_mul_lo_u32 v" #T0 ", v" #X0 ", %[ch]\n v_mad_u64_u32 v[" #T0 ":" #T1 "], vcc, v" #X1 ", %[cl], v[" #T0 ":" #T1 "]\n v_mad_u64_u32 v[" #Y0 ":" #Y1 "], vcc, v" #X0 ", %[cl], 0\n v_add_u32 v" #Y1 ", v" #Y1 ", v" #T0 "\n"
#define MUL_B(X0, X1, Y0, Y1, T0, T1, Z0, Z1) \
    "v_mul_lo_u32 v" #T0 ", v" #X0 ", %[ch]\n v_mad_u64_u32 v[" #T0 ":" #T1 "], vcc, v" #X1 ", %[cl], v[" #T0 ":" #T1 "]\n v_mov_b32 v" #Z1 ", v" #T0 "\n v_mad_u64_u32 v[" #Y0 ":" #Y1 "], vcc, v" #X0 ", %[cl], v[" #Z0 ":" #Z1 "]\n"
#define MUL_B2(X0, X1, Y0, Y1, T0, T1, Z0, Z1) \
    "v_mul_lo_u32 v" #T0 ", v" #X0 ", %[ch]\n v_mul_lo_u32 v" #T1 ", v" #X1 ", %[cl]\n v_add_u32 v" #Z1 ", v" #T0 ", v" #T1 "\n v_mad_u64_u32 v[" #Y0 ":" #Y1 "], vcc, v" #X0 ", %[cl], v[" #Z0 ":" #Z1 "]\n"
#define MUL_B0(X0, X1, Y0, Y1, T0, T1, Z0, Z1) \
    "v_mul_lo_u32 v" #T0 ", v" #X0 ", %[ch]\n v_mad_u64_u32 v[" #T0 ":" #T1 "], vcc, v" #X1 ", %[cl], v[" #T0 ":" #T1 "]\n v_mov_b32 v" #Z0 ", 0\n v_mov_b32 v" #Z1 ", v" #T0 "\n v_mad_u64_u32 v[" #Y0 ":" #Y1 "], vcc, v" #X0 ", %[cl], v[" #Z0 ":" #Z1 "]\n"
#define MUL_BG(X0, X1, Y0, Y1, T0, T1, Z0, Z1) \
    "v_mul_lo_u32 v" #T0 ", v" #X0 ", %[ch]\n v_mad_u64_u32 v[" #T0 ":" #T1 "], vcc, v" #X1 ", %[cl], v[" #T0 ":" #T1 "]\n v_add_u32 v" #Z1 ", %[ch], v" #T0 "\n v_mad_u64_u32 v[" #Y0 ":" #Y1 "], vcc, v" #X0 ", %[cl], v[" #Z0 ":" #Z1 "]\n"
#define CHAINS(M)                                                                                                                \
    M(40, 41, 42, 43, 44, 45, 46, 47) M(48, 49, 50, 51, 52, 53, 54, 55) M(56, 57, 58, 59, 60, 61, 62, 63) M(64, 65, 66, 67, 68, 69, 70, 71) \
    M(42, 43, 40, 41, 44, 45, 46, 47) M(50, 51, 48, 49, 52, 53, 54, 55) M(58, 59, 56, 57, 60, 61, 62, 63) M(66, 67, 64, 65, 68, 69, 70, 71)
#define CLOB "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", \
             "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "vcc"
template <int SEQ>
__global__ __launch_bounds__(256) void kseq(uint32_t *out, uint32_t seed)
{
    const uint64_t C = 0xbf58476d1ce4e5b9ull;
    const uint32_t cl = (uint32_t)C, ch = (uint32_t)(C >> 32), x = threadIdx.x + seed;
    asm volatile("v_mov_b32 v40, %0\n v_mov_b32 v41, %1\n v_mov_b32 v48, %1\n v_mov_b32 v49, %0\n v_add_u32 v56, 3, %0\n v_mov_b32 v57, %1\n v_add_u32 v64, 5, %0\n v_mov_b32 v65, %0\n"
                 "v_mov_b32 v46, 0\n v_mov_b32 v54, 0\n v_mov_b32 v62, 0\n v_mov_b32 v70, 0\n" :: "v"(x), "v"(seed) : CLOB);
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int r = 0; r < REP / 8; r++) {        // 8 multiplies per asm block
            if (SEQ == 0) asm volatile(CHAINS(MUL_HIPCC) :: [cl] "s"(cl), [ch] "s"(ch) : CLOB);
            if (SEQ == 1) asm volatile(CHAINS(MUL_A) :: [cl] "s"(cl), [ch] "s"(ch) : CLOB);
            if (SEQ == 2) asm volatile(CHAINS(MUL_B) :: [cl] "s"(cl), [ch] "s"(ch) : CLOB);
            if (SEQ == 3) asm volatile(CHAINS(MUL_B2) :: [cl] "s"(cl), [ch] "s"(ch) : CLOB);
            if (SEQ == 4) asm volatile(CHAINS(MUL_B0) :: [cl] "s"(cl), [ch] "s"(ch) : CLOB);
            if (SEQ == 5) asm volatile(CHAINS(MUL_BG) :: [cl] "s"(cl), [ch] "s"(ch) : CLOB);
        }
    }
    uint32_t r;
    asm volatile("v_xor_b32 %0, v40, v41\n v_xor_b32 %0, %0, v48\n v_xor_b32 %0, %0, v49\n v_xor_b32 %0, %0, v56\n v_xor_b32 %0, %0, v57\n v_xor_b32 %0, %0, v64\n v_xor_b32 %0, %0, v65" : "=v"(r) :: CLOB);
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}
template <int OP> void run(const char *name, uint32_t *d)
{
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    int blocks = 256 * 8;                     // 8 blocks x 4 waves per CU = 8 waves per SIMD
    hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(256), 0, 0, d, 1u);
    hipEventRecord(a); hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(256), 0, 0, d, 2u); hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    double winstr = (double)blocks * 4 * ITERS * REP;       // wave-instructions
    double per_simd = winstr / (256.0 * 4);                 // per SIMD
    printf("%-16s %8.3f ms  -> %.2f ns per wave-instr per SIMD  (= %.2f cycles @2.4GHz)\n", name, ms, ms * 1e6 / per_simd, ms * 1e6 / per_simd * 2.4);
}
template <int SEQ> void run_seq(const char *name, uint32_t *d)
{
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    int blocks = 256 * 8;
    hipLaunchKernelGGL(kseq<SEQ>, dim3(blocks), dim3(256), 0, 0, d, 1u);
    hipEventRecord(a); hipLaunchKernelGGL(kseq<SEQ>, dim3(blocks), dim3(256), 0, 0, d, 2u); hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    double mults = (double)blocks * 4 * ITERS * REP;        // 64-bit multiplies of all waves
    double per_simd = mults / (256.0 * 4);
    printf("mul64 %-10s %8.3f ms  -> %.2f ns per wave-multiply per SIMD  (= %.2f cycles @2.4GHz)\n", name, ms, ms * 1e6 / per_simd, ms * 1e6 / per_simd * 2.4);
}

// The hash chain of one k-mer that the filter drops (MinEmitF::full: h + gamma = fx64(v) + gamma, s0 and s3 from two SplitMix64 mixes,
// o1 = rotl(s0 + s3, 23) + s0), fed back into v so that it is one dependency chain; four chains per lane, 8 waves per SIMD. FORM picks how
// the five 64 x 64 multiplies are written in C++ (the instructions are whatever hipcc selects for it):
//   0  plain x * c
//   1  form A: both multiply-adds fenced, the high halves joined by a fenced 32-bit add
//   2  form B: only the cross multiply-add fenced; hipcc adds it through the high half of the final v_mad_u64_u32's addend
//   3  form B, and an offset a = ah:al joins the addend as al : (ah + cross) - one v_add_u32 instead of a 64-bit add after the multiply
template <int FORM> __device__ __forceinline__ uint64_t mulc(uint64_t x, uint64_t c, uint64_t a = 0)
{
    if (FORM == 0) return x * c + a;
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32), cl = (uint32_t)c, ch = (uint32_t)(c >> 32);
    uint64_t cr = (uint64_t)xh * cl + (uint32_t)(xl * ch);
    if (FORM == 2) { asm("" : "+v"(cr)); return (uint64_t)xl * cl + a + ((uint64_t)(uint32_t)cr << 32); }
    if (FORM == 3) {
        asm("" : "+v"(cr));
        if (a == 0) return (uint64_t)xl * cl + ((uint64_t)(uint32_t)cr << 32);
        uint32_t zh = (uint32_t)(a >> 32) + (uint32_t)cr;
        asm("" : "+v"(zh));
        uint64_t z = ((uint64_t)zh << 32) | (uint32_t)a;
        asm("" : "+v"(z));
        return (uint64_t)xl * cl + z;
    }
    uint64_t p = (uint64_t)xl * cl + a;
    asm("" : "+v"(cr), "+v"(p));
    uint32_t hi = (uint32_t)(p >> 32) + (uint32_t)cr;
    asm("" : "+v"(hi));
    return ((uint64_t)hi << 32) | (uint32_t)p;
}
template <int FORM> __device__ __forceinline__ uint64_t mix(uint64_t z)
{
    z = mulc<FORM>(z ^ (z >> 30), 0xbf58476d1ce4e5b9ull);
    z = mulc<FORM>(z ^ (z >> 27), 0x94d049bb133111ebull);
    return z ^ (z >> 31);
}
template <int FORM> __device__ __forceinline__ uint64_t drop_chain(uint64_t v)
{
    uint64_t hg = mulc<FORM>(v, 0x517cc1b727220a95ull, 0x9e3779b97f4a7c15ull);
    asm("" : "+v"(hg));
    const uint64_t s0 = mix<FORM>(hg), s3 = mix<FORM>(hg + 3 * 0x9e3779b97f4a7c15ull);
    const uint64_t t = s0 + s3;
    return ((t << 23) | (t >> 41)) + s0;
}
// The same chain as the filter now asks it (gs_hiword.hpp): only the high words of s0 and s3, B = ((s0_hi + s3_hi + 2) << 23) + s0_hi, fed back as
// B : (s0_hi ^ s3_hi). HI picks how the high word of each mix's second multiply is written:
//   4  mulc64's form B shifted down by 32 (hipcc drops the dead low word by itself: v_mul_hi_u32 in place of the last v_mad_u64_u32)
//   5  written out: __umulhi(x_lo, c_lo) + the fenced cross multiply-add
template <int HI> __device__ __forceinline__ uint32_t mix_hi(uint64_t z)
{
    z = mulc<3>(z ^ (z >> 30), 0xbf58476d1ce4e5b9ull);
    z ^= z >> 27;
    uint32_t b;
    if (HI == 4) b = (uint32_t)(mulc<3>(z, 0x94d049bb133111ebull) >> 32);
    else {
        const uint32_t xl = (uint32_t)z, xh = (uint32_t)(z >> 32), cl = 0x133111ebu, ch = 0x94d049bbu;
        uint64_t cr = (uint64_t)xh * cl + (uint32_t)(xl * ch);
        asm("" : "+v"(cr));
        b = __umulhi(xl, cl) + (uint32_t)cr;
    }
    return b ^ (b >> 31);
}
template <> __device__ __forceinline__ uint64_t drop_chain<4>(uint64_t v)
{
    uint64_t hg = mulc<3>(v, 0x517cc1b727220a95ull, 0x9e3779b97f4a7c15ull);
    asm("" : "+v"(hg));
    const uint32_t s0 = mix_hi<4>(hg), s3 = mix_hi<4>(hg + 3 * 0x9e3779b97f4a7c15ull);
    return ((uint64_t)(((s0 + s3 + 2u) << 23) + s0) << 32) | (s0 ^ s3);
}
template <> __device__ __forceinline__ uint64_t drop_chain<5>(uint64_t v)
{
    uint64_t hg = mulc<3>(v, 0x517cc1b727220a95ull, 0x9e3779b97f4a7c15ull);
    asm("" : "+v"(hg));
    const uint32_t s0 = mix_hi<5>(hg), s3 = mix_hi<5>(hg + 3 * 0x9e3779b97f4a7c15ull);
    return ((uint64_t)(((s0 + s3 + 2u) << 23) + s0) << 32) | (s0 ^ s3);
}
#define CH_ITERS 256
template <int FORM>
__global__ __launch_bounds__(256) void kchain(uint32_t *out, uint32_t seed)
{
    uint64_t v0 = threadIdx.x + seed, v1 = v0 * 3, v2 = v0 ^ 0x5555, v3 = v0 + 99;
    for (int it = 0; it < CH_ITERS; it++) { v0 = drop_chain<FORM>(v0); v1 = drop_chain<FORM>(v1); v2 = drop_chain<FORM>(v2); v3 = drop_chain<FORM>(v3); }
    out[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)(v0 ^ v1 ^ v2 ^ v3) ^ (uint32_t)((v0 + v1 + v2 + v3) >> 32);
}
template <int FORM> void run_chain(const char *name, uint32_t *d)
{
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    int blocks = 256 * 8;
    hipLaunchKernelGGL(kchain<FORM>, dim3(blocks), dim3(256), 0, 0, d, 1u);
    hipEventRecord(a); hipLaunchKernelGGL(kchain<FORM>, dim3(blocks), dim3(256), 0, 0, d, 2u); hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    double steps = (double)blocks * 4 * CH_ITERS * 4;      // wave-level chain steps (4 waves per block, 4 chains per lane)
    double per_simd = steps / (256.0 * 4);
    printf("chain %-10s %8.3f ms  -> %.2f ns per wave-k-mer per SIMD  (= %.2f cycles @2.4GHz)\n", name, ms, ms * 1e6 / per_simd, ms * 1e6 / per_simd * 2.4);
}
int main()
{
    uint32_t *d; hipMalloc(&d, 256 * 8 * 256 * 4);
    run<0>("v_xor_b32", d); run<1>("v_mul_lo_u32", d); run<2>("v_mul_hi_u32", d); run<3>("v_mad_u64_u32", d); run<4>("v_lshrrev_b64", d);
    run<10>("v_lshlrev_b64", d); run<5>("v_alignbit_b32", d); run<6>("v_mul_u32_u24", d); run<9>("v_mad_u32_u24", d); run<7>("v_lshl_add_u64", d); run<8>("v_add3_u32", d); run<11>("v_cmp_lt_u64", d);
    run<12>("v_add_u32", d); run<13>("v_mov_b32", d); run<14>("v_dot2_u32_u16", d); run<15>("v_lshrrev_b32", d);
    run_seq<0>("hipcc", d); run_seq<1>("A", d); run_seq<2>("B", d); run_seq<3>("B2", d); run_seq<4>("B0", d); run_seq<5>("Bg", d);
    run_chain<0>("x*c", d); run_chain<1>("A", d); run_chain<2>("B", d); run_chain<3>("Bg", d); run_chain<4>("Bg hi", d); run_chain<5>("Bg hi mulhi", d);
    return 0;
}
