// gs_insert_rows.hpp — where the count rows of a dense insert batch go, and which join fills them. Plain C++ (no HIP): tests/test_insert_rows_cpu.py
// compiles it with the host compiler alone. InsertCall::batch_counts (gs_index.hip) executes what it answers.
//
// The rows of a batch (its points against every node present at batch start) live in the call's slab of the dense pair cache, or, without a slab, in a
// rolling buffer that holds one GROUP of batches. A group is joined once, all its points against the nodes present at its start - the column store is
// streamed once per group instead of once per batch -; a later batch of the group then only lacks the nodes the earlier batches of the group added, and
// takes a small join over their columns. Feed it every dense batch of one insert call, in order.
#pragma once
#include <stdint.h>
#include <algorithm>

namespace gs {

enum RowJoin : int {
    JOIN_GROUP = 0,     // a group starts: `nq` rows, from this batch's first row on, against the nodes [0, b0)
    JOIN_RANGE = 1,     // inside a group: this batch against the nodes [node0, node0 + nn) only (nn = 0: nothing to add)
    JOIN_ALONE = 2      // no grouping: this batch against the nodes [0, b0)
};
struct RowPlace {
    uint64_t row_off;   // the batch's first row, counted from the first row of the slab or of the rolling buffer
    uint64_t grow_rows; // rolling buffer only: 0 = it stays as it is, else it may grow now and has to hold this many rows
    int join;           // RowJoin
    uint64_t nq;        // JOIN_GROUP: the rows of the group; otherwise the batch's
    uint64_t node0, nn; // JOIN_RANGE
};

struct InsertRows {
    uint64_t end = 0, B = 1, grp_n = 1;             // the call inserts nodes [first, end) in batches of B, grp_n batches to a group
    uint64_t grp_b0 = 0, grp_end = 0;               // the group under way: its rows hold their counts against the nodes [0, grp_b0)
    uint64_t slab_first = 0;                        // the batch whose rows open the slab
    void start(uint64_t first, uint64_t n, uint32_t batch, uint32_t group) { end = first + n; B = batch; grp_n = group; grp_b0 = grp_end = slab_first = 0; }
    void slab_taken(uint64_t b0) { slab_first = b0; }
    // the pair cache was given back while the batch's join ran: its rows are produced again, alone, and the next batch starts afresh
    void reset() { grp_b0 = grp_end = 0; }
    bool in_group(uint64_t b0) const { return b0 >= grp_b0 && b0 < grp_end; }
    RowPlace next(uint64_t b0, uint32_t nb, bool have_slab, bool can_group)
    {
        const bool inside = in_group(b0);
        RowPlace r{};
        if (have_slab) r.row_off = b0 - slab_first;
        else {
            r.row_off = inside ? b0 - grp_b0 : 0;
            if (!inside) r.grow_rows = can_group ? grp_n * B : B;        // the buffer only ever grows where a group (or a single batch) starts
        }
        r.nq = nb;
        if (can_group && inside) { r.join = JOIN_RANGE; r.node0 = grp_b0; r.nn = b0 - grp_b0; }
        else if (can_group) {
            grp_b0 = b0; grp_end = std::min<uint64_t>(end, b0 + grp_n * B);
            r.join = JOIN_GROUP; r.nq = grp_end - grp_b0;
        } else { grp_b0 = grp_end = 0; r.join = JOIN_ALONE; }
        return r;
    }
};

}  // namespace gs
