// C surface over gsearch_amd/csrc/gs_insert_rows.hpp for tests/test_insert_rows_cpu.py: the row planner of parallel_insert, compiled with the host
// compiler alone (no HIP, no device). ir_run feeds it one insert call the way InsertCall::batch_counts (gs_index.hip) does.
#include "../gsearch_amd/csrc/gs_insert_rows.hpp"

enum { IR_DENSE = 1, IR_HAVE_SLAB = 2, IR_CAN_GROUP = 4, IR_SLAB_TAKEN = 8, IR_RESET_AFTER = 16 };

extern "C" {
// flags[i]: what batch i of the call meets (IR_*). out[6 * i ..]: row_off, grow_rows, join, nq, node0, nn of a dense batch (untouched otherwise).
// Returns the number of batches.
long long ir_run(unsigned long long first, unsigned long long n, unsigned batch, unsigned group, const unsigned char *flags, long long *out)
{
    gs::InsertRows rows;
    rows.start(first, n, batch, group);
    long long i = 0;
    for (unsigned long long b0 = first; b0 < first + n; b0 += batch, i++) {
        const unsigned nb = (unsigned)std::min<unsigned long long>(batch, first + n - b0);
        if (!(flags[i] & IR_DENSE)) continue;
        if (flags[i] & IR_SLAB_TAKEN) rows.slab_taken(b0);
        const gs::RowPlace r = rows.next(b0, nb, (flags[i] & IR_HAVE_SLAB) != 0, (flags[i] & IR_CAN_GROUP) != 0);
        long long *o = out + 6 * i;
        o[0] = (long long)r.row_off; o[1] = (long long)r.grow_rows; o[2] = r.join; o[3] = (long long)r.nq; o[4] = (long long)r.node0; o[5] = (long long)r.nn;
        if (flags[i] & IR_RESET_AFTER) rows.reset();
    }
    return i;
}
}
