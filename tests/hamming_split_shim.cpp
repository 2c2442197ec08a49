// host shim of tests/test_hamming_split_cpu.py: gsearch_amd/csrc/gs_hamming_split.hpp as the host compiler sees it
#include "../gsearch_amd/csrc/gs_hamming_split.hpp"

extern "C" {
// out[0..3] = HT, HKW, HTQ, HTR
void hs_geometry(int *out) { out[0] = gs::HT; out[1] = gs::HKW; out[2] = gs::HTQ; out[3] = gs::HTR; }
// form 0: the dense form (units = tiles), 1: the work-list form (units = items). For every row-word count 1..roww_max: ksplit[roww - 1], parts[roww - 1]
void hs_fill(unsigned n_cu, int form, unsigned units, unsigned roww_max, unsigned *ksplit, unsigned *parts)
{
    for (unsigned roww = 1; roww <= roww_max; roww++) {
        const gs::HammingSplit s = form == 0 ? gs::hamming_split_tiles(n_cu, units, roww) : gs::hamming_split_items(n_cu, units, roww);
        ksplit[roww - 1] = s.ksplit_words; parts[roww - 1] = s.parts;
    }
}
}
