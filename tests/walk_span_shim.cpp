// C surface over gsearch_amd/csrc/gs_walk_span.hpp for tests/test_walk_span_cpu.py: the cursor of walk_genome's two-stage loop (gs_walk.hpp), compiled with
// the host compiler alone (no HIP, no device). ws_run takes every lane of every workgroup of one genome through the loop's schedule, statement for
// statement, with the walk itself left out, and writes down what the lane knew about each unit and which words it loaded for it.
#include "../gsearch_amd/csrc/gs_walk_span.hpp"

enum { WS_PROLOGUE = 0, WS_LOOKED_UP = 1, WS_INSIDE = 2 };
enum { WS_COLS = 9 };

static void put(long long *out, unsigned long long f, const gs::WalkCursor &c, unsigned k, int how, unsigned long long w, unsigned long long pw)
{
    long long *o = out + WS_COLS * f;
    o[0] = (long long)c.s.lo; o[1] = (long long)c.s.rb; o[2] = (long long)c.s.re; o[3] = (long long)c.u; o[4] = (long long)(c.u << 5);
    o[5] = (long long)gs::span_first_valid(c.s, k); o[6] += 1 + 16 * how;     // visits in the low 4 bits, how the unit was reached above them
    o[7] = (long long)w; o[8] = (long long)pw;
}

extern "C" {
// out[WS_COLS * f ..] for every flat unit f < units (zeroed by the caller): lo, rb, re, u, a0, first_valid, visits + 16 * how, the word loaded as w, the word
// loaded as pw. Returns the number of loads issued ahead of a walk (the WS_INSIDE units), -1 if one was issued for a unit >= units.
long long ws_run(const unsigned long long *rec_start, const unsigned long long *rec_len, const unsigned long long *rec_upre, unsigned long long r0,
                 unsigned long long r1, unsigned long long units, unsigned k, unsigned block, unsigned parts, long long *out)
{
    const uint64_t *rs = (const uint64_t *)rec_start, *rl = (const uint64_t *)rec_len, *ru = (const uint64_t *)rec_upre;
    long long ahead = 0;
    for (unsigned part = 0; part < parts; part++)
        for (unsigned lane = 0; lane < block; lane++) {
            const uint64_t stride = (uint64_t)parts * block;
            uint64_t f = (uint64_t)part * block + lane;
            const uint32_t stride32 = gs::cursor_stride(stride);
            gs::WalkCursor c{{0, 0, 0, 0, 0}, 0, 0};
            if (f < units) {
                gs::cursor_locate(c, rs, rl, ru, r0, r1, units, f);
                put(out, f, c, k, WS_PROLOGUE, c.u, gs::halo_word(c.s, c.u, k));
            }
            while (f < units) {
                f += stride;
                const bool inside = gs::cursor_inside(c, stride32);
                uint64_t un = 0, pn = 0;
                if (inside) { un = gs::inside_word(c, stride32); pn = gs::inside_halo_word(un, k); ahead++; }
                // (the walk of the unit before)
                if (inside && f >= units) return -1;                      // the span cache let a lane load for a unit the genome does not have
                if (inside) { gs::cursor_advance(c, stride32); put(out, f, c, k, WS_INSIDE, un, pn); }
                else if (f < units) {
                    gs::cursor_locate(c, rs, rl, ru, r0, r1, units, f);
                    put(out, f, c, k, WS_LOOKED_UP, c.u, gs::halo_word(c.s, c.u, k));
                }
            }
        }
    return ahead;
}
// one lane looks unit f up and is asked for the unit `stride` further on: out = inside (0 / 1), the word it would load ahead, the count it holds
void ws_probe(const unsigned long long *rec_start, const unsigned long long *rec_len, const unsigned long long *rec_upre, unsigned long long r0,
              unsigned long long r1, unsigned long long units, unsigned long long f, unsigned long long stride, long long *out)
{
    gs::WalkCursor c{{0, 0, 0, 0, 0}, 0, 0};
    gs::cursor_locate(c, (const uint64_t *)rec_start, (const uint64_t *)rec_len, (const uint64_t *)rec_upre, r0, r1, units, f);
    const uint32_t stride32 = gs::cursor_stride(stride);
    out[0] = gs::cursor_inside(c, stride32) ? 1 : 0;
    out[1] = (long long)gs::inside_word(c, stride32);
    out[2] = (long long)c.left;
}
}
