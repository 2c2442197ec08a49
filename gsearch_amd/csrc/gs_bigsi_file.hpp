// gs_bigsi_file.hpp — the host half of reading a .gsbx file (layout: above gs_bigsi_save, gs_bigsi.hip; refusal rules: SPEC.md 16.2). Plain C++, no HIP:
// gs_bigsi_load parses with it, then allocates and uploads; gs_bigsi_describe / gs_bigsi_verify (gs_bigsi_file.cpp) are the same code without a context.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/gsearch_amd.h"
#include "gs_host.hpp"

// the parameter limits of SPEC 11 (gs_spec.hpp includes this file for them)
#define GS_BIGSI_KMAX 32u                // 1 <= k <= 32 (15 accepted)
#define GS_BIGSI_HMAX 16u                // 1 <= num_hash <= 16
#define GS_BIGSI_BMAX (1ULL << 40)       // 1 <= bloom_size < 2^40

namespace gs {

constexpr char BX_MAGIC[8] = {'G', 'S', 'B', 'I', 'G', 'S', 'I', '1'};
constexpr uint32_t BX_VERSION = 1, BX_VERSION_MINI = 2;         // a plain index; a minimizer index (one more u32, m, after data_t)

// everything of a .gsbx file but its matrix rows, which start at `rows_at` and are exactly bloom_size x row_words x 8 bytes up to the end of the file
struct BigsiFile {
    gs_bigsi_file_description desc;
    gs_bigsi_params prm;
    std::vector<std::string> names;
    std::vector<uint64_t> t, q;
    uint64_t rows_at = 0;
};

// everything gs_bigsi_load checks before it asks the device for memory; never throws. On GS_OK *keep (optional) is the open file, positioned at the rows.
int bigsi_file_parse(const char *path, BigsiFile *out, FILE **keep);

}  // namespace gs
