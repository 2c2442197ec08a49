// gs_hamming_split.hpp — the tile geometry of the DistHamming kernels (gs_hamming.hip) and the rule by which their two host drivers split the row
// words of a small problem over blockIdx.z. Plain integer C++ (no HIP): gs_hamming.hip and gs_join.hip include it, tests/test_hamming_split_cpu.py
// compiles it with the host compiler alone.
//
// The rule, for a problem of `units` workgroups (tiles of the dense form, items of the work-list form) and `roww` 32-bit words per row
// (m for 4-byte elements, 2 m for u64) on a device of n_cu compute units:
//   split only if  units * A <= n_cu * B  and  roww >= 8 * HKW (256 words);
//   nz     = min(n_cu * F / units, roww / (4 * HKW))                 (integer divisions; a part is at least 128 words)
//   split only if  nz > 1;
//   ksplit = ceil(ceil(roww / nz) / HKW) * HKW                       (words per part, whole K-chunks)
//   parts  = ceil(roww / ksplit)                                     (grid.z; the last part may be shorter, none is empty)
// with (A, B, F) = (2, 1, 2) for the dense form (hamming_qxc_strided; the 32-bit count output only) and (2, 2, 4) for the work-list form
// (hamming_blocks; units = the items left after the thin kernel took its share). No split: ksplit = 0, parts = 1.
// Part z owns the words [z * ksplit, min((z + 1) * ksplit, roww)). In the work-list form a part takes its MATCHES (its words' elements minus its
// mismatches) off a counter that was set to m, so an empty part would subtract from nothing it owns: parts * ksplit >= roww > (parts - 1) * ksplit.
#pragma once
#include <stdint.h>

namespace gs {

constexpr int HT = 128;     // tile edge (queries and candidates); the match-join cuts its heavy blocks into tiles of this edge
constexpr int HKW = 32;     // words per K-chunk
constexpr int HTQ = 16;     // query rows of a thin item at most
constexpr int HTR = 4;      // candidate rows per wavefront of the thin kernel

struct HammingSplit { uint32_t ksplit_words; uint32_t parts; };

inline HammingSplit hamming_split(uint64_t n_cu, uint64_t units, uint64_t roww_all, uint64_t a, uint64_t b, uint64_t f)
{
    HammingSplit s{0, 1};
    if (units * a <= n_cu * b && roww_all >= 8 * HKW) {
        uint64_t nz = n_cu * f / units;
        if (roww_all / (4 * HKW) < nz) nz = roww_all / (4 * HKW);
        const uint32_t nz32 = (uint32_t)nz;
        if (nz32 > 1) {
            s.ksplit_words = (uint32_t)(((roww_all + nz32 - 1) / nz32 + HKW - 1) / HKW * HKW);
            s.parts = (uint32_t)((roww_all + s.ksplit_words - 1) / s.ksplit_words);
        }
    }
    return s;
}
// dense form: tiles = grid.x * grid.y >= 1
inline HammingSplit hamming_split_tiles(uint64_t n_cu, uint64_t tiles, uint64_t roww_all) { return hamming_split(n_cu, tiles, roww_all, 2, 1, 2); }
// work-list form: items >= 1
inline HammingSplit hamming_split_items(uint64_t n_cu, uint64_t items, uint64_t roww_all) { return hamming_split(n_cu, items, roww_all, 2, 2, 4); }

}  // namespace gs
