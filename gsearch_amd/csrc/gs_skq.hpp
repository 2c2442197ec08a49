// gs_skq.hpp — fill count of the per-wave survivor queue of the filtered slot-min emitter (MinEmitF, gs_sketch.hip). Plain integer C++ (no HIP
// builtins): the emitter executes it on the device, tests/test_skq_split_cpu.py compiles it with the host compiler alone.
//
// A push appends cnt <= 64 new hashes behind qn < 64 pending ones. As soon as 64 are pending the wave flushes the first 64, one per lane, and the
// rest (fewer than 64) move to the front: SKQ = 128 entries are never exceeded, and fewer than 64 are pending between two pushes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_SKQ_HD __host__ __device__ __forceinline__
#else
#define GS_SKQ_HD inline
#endif

namespace gs {

constexpr uint32_t SKQ = 128;          // queue entries per wave: < 64 pending + <= 64 new
constexpr uint32_t SKQ_FLUSH = 64;     // one flush feeds every lane

// after a push of cnt entries onto qn pending ones: does the wave flush, and how many entries are pending afterwards (behind a flush: the entries
// SKQ_FLUSH .. SKQ_FLUSH + pending - 1, which move to the front)
struct SkqPush { uint32_t pending; bool flush; };
GS_SKQ_HD SkqPush skq_push(uint32_t qn, uint32_t cnt)
{
    const uint32_t n = qn + cnt;
    if (n >= SKQ_FLUSH) return SkqPush{n - SKQ_FLUSH, true};
    return SkqPush{n, false};
}

}  // namespace gs
