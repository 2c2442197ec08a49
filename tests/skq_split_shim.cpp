// host shim of tests/test_skq_split_cpu.py: gsearch_amd/csrc/gs_skq.hpp as the host compiler sees it, one call per (qn, cnt)
#include "../gsearch_amd/csrc/gs_skq.hpp"

extern "C" {
unsigned skq_capacity(void) { return gs::SKQ; }
unsigned skq_flush_at(void) { return gs::SKQ_FLUSH; }
// out[0..1] = pending after the push, flush
void skq_probe(unsigned qn, unsigned cnt, unsigned *out)
{
    const gs::SkqPush p = gs::skq_push(qn, cnt);
    out[0] = p.pending; out[1] = p.flush;
}
}
