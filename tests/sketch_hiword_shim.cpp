// host shim of tests/test_sketch_hiword_cpu.py: gsearch_amd/csrc/gs_hiword.hpp as the host compiler sees it, one call per array of (s0, s3) pairs
#include "../gsearch_amd/csrc/gs_hiword.hpp"

extern "C" {
unsigned hiw_slack(void) { return gs::HIW_SLACK; }
// form 0: 23-bit keys (o1 >> 41), 1: u32 keys (o1 >> 32), 2: u64 keys (o1)
unsigned hiw_limit(int form, unsigned long long thr)
{
    if (form == 0) return gs::hiword_limit_r23((uint32_t)thr);
    if (form == 1) return gs::hiword_limit_u32((uint32_t)thr);
    return gs::hiword_limit_u64((uint64_t)thr);
}
// pass[i] = the drop test lets pair i through
void hiw_pass(const unsigned long long *s0, const unsigned long long *s3, unsigned long long n, unsigned limit, unsigned char *pass)
{
    for (unsigned long long i = 0; i < n; i++)
        pass[i] = gs::hiword_may_be_below((uint32_t)(s0[i] >> 32), (uint32_t)(s3[i] >> 32), limit);
}
// the form the emitter runs (hiword_may_be_below_x): s3's word without its last xor-shift, and only its low 9 bits - the bits above them are
// filled from the pair's low words, which must not matter
unsigned hiw_slack_x(void) { return gs::HIW_SLACK_X; }
unsigned hiw_limit_x(int form, unsigned long long thr)
{
    if (form == 0) return gs::hiword_limit_x_r23((uint32_t)thr);
    if (form == 1) return gs::hiword_limit_x_u32((uint32_t)thr);
    return gs::hiword_limit_x_u64((uint64_t)thr);
}
void hiw_pass_x(const unsigned long long *s0, const unsigned long long *s3, unsigned long long n, unsigned limit_x, unsigned char *pass)
{
    for (unsigned long long i = 0; i < n; i++) {
        const uint32_t h = (uint32_t)(s3[i] >> 32), b = h ^ (h >> 31);               // s3_hi = b ^ (b >> 31): bit 31 is its own
        const uint32_t s3_x = (b & 0x1FFu) | (((uint32_t)s3[i] ^ (uint32_t)s0[i]) << 9);
        pass[i] = gs::hiword_may_be_below_x((uint32_t)(s0[i] >> 32), s3_x, limit_x);
    }
}
}
