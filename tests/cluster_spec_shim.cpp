// Host build of the SPEC 10 sampling rules of gsearch_amd/csrc/gs_spec.hpp for tests/test_cluster_spec_cpu.py (no device code is generated or run).
#include "../gsearch_amd/csrc/gs_spec.hpp"

extern "C" {
uint64_t cs_hash(uint64_t seed, uint32_t r, uint64_t i) { return gs::cluster_hash(seed, r, i); }
int cs_keep0(uint64_t h, uint64_t n, uint64_t t0) { return gs::cluster_keep0(h, n, t0); }
int cs_keep1(uint64_t h, uint64_t D, uint64_t t1, uint32_t d0) { return gs::cluster_keep1(h, D, t1, d0); }
}
