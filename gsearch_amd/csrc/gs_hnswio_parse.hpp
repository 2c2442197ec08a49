// gs_hnswio_parse.hpp — the host half of reading an hnsw_rs dump (layout: the header of gs_hnswio.hip; refusal rules: SPEC.md 16) and the host
// validation of a graph handed to gs_index_import. Plain C++, no HIP: gs_index_load_hnswrs parses with it and then creates / imports / uploads;
// gs_hnswrs_describe / gs_hnswrs_verify (gs_hnswio_parse.cpp) are the same code without a context.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/gsearch_amd.h"
#include "gs_host.hpp"

namespace gs {

namespace fmt {                                     // the layout's constants (gs_hnswio.hip header): [RECALL] = restated from the crate as recalled
constexpr uint32_t MAGICDESCR_3 = 0x002a6771u;      // [RECALL] description, format 3 (raw data vectors, mmap-able)
constexpr uint32_t MAGICDESCR_2 = 0x002a677fu;      // [RECALL] format 2 (bincode-encoded vectors): recognised and refused
constexpr uint32_t MAGICPOINT = 0x000a678fu;        // [RECALL]
constexpr uint32_t MAGICLAYER = 0x000a676fu;        // [RECALL]
constexpr uint32_t MAGICDATAP = 0xa67f0000u;        // [RECALL]
constexpr uint8_t NB_LAYER_MAX = 16;                // [REF] Hnsw::new(.., 16, ..) dnasketch.rs:139
constexpr const char *DISTNAME = "anndists::dist::distances::DistHamming";   // [RECALL] std::any::type_name of the distance
}  // namespace fmt

// a verified dump in the form gs_index_import takes: node numbers (DataIds 0..n-1 ARE the node numbers, any other distinct ids number the nodes in
// data-file order and are kept in `oid`), lists in (count, id) order
struct HnswrsDump {
    gs_hnswrs_description desc;
    int kind = -1;
    uint32_t M = 0, m = 0;
    uint64_t n = 0, U = 0, entry = 0;
    bool dense = true;
    std::vector<uint8_t> sigs, lv;
    std::vector<uint64_t> oid;
    std::vector<uint32_t> d0, n0, c0, dU, nU, cU;
    std::vector<int32_t> up;
};

// everything gs_index_load_hnswrs checks before it touches the device; never throws
int hnswrs_parse(const char *basename, HnswrsDump *out);

// levels, degrees, neighbour ids, upidx (in range, consistent with the level, shared by no two nodes), upper links reach their layer, entry on the top layer
int graph_validate(uint64_t n, uint32_t M, uint32_t ML, const uint8_t *levels, int64_t entry, const uint32_t *deg0, const uint32_t *nbr0,
                   const int32_t *upidx, uint64_t n_upper, const uint32_t *degU, const uint32_t *nbrU);

}  // namespace gs
