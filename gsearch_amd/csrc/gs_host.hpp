// gs_host.hpp — what the host-only units share: the error text behind gs_last_error(), the check that sets it, and the digest of the verify calls.
// Plain C++: the host-only units (gs_hnswio_parse.cpp, gs_bigsi_file.cpp) are built by g++ alone and include no HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gs {
void set_error(const char *fmt, ...);       // gs_ctx.hip (a stand-alone host program that links only the host-only units brings its own)

// FNV-1a, 64 bit (SPEC 16.3: the digest the verify calls hand back)
inline uint64_t fnv1a(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ULL; }
    return h;
}
constexpr uint64_t FNV_BASIS = 0xcbf29ce484222325ULL;
}  // namespace gs

#define GS_REQUIRE(cond, code, ...)                \
    do {                                           \
        if (!(cond)) {                             \
            gs::set_error(__VA_ARGS__);            \
            return (code);                         \
        }                                          \
    } while (0)
