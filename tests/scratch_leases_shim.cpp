// C surface over gsearch_amd/csrc/gs_scratch.hpp for tests/test_scratch_leases.py: the lease bookkeeping of the scratch pool, compiled with the host
// compiler alone (no HIP, no device). A "pool" here is what ScratchPool keeps of it: the shared lease table.
#include <stdarg.h>
#include <stdio.h>
#include "../gsearch_amd/csrc/gs_scratch.hpp"

static char g_err[512];
void gs::set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

using Pool = std::shared_ptr<gs::SlotLeases>;
extern "C" {
int sl_count(void) { return gs::SCRATCH_SLOTS; }
const char *sl_name(int s) { return gs::scratch_slot_name((gs::ScratchSlot)s); }
const char *sl_last_error(void) { return g_err; }
void *sl_pool_new(void) { return new Pool(std::make_shared<gs::SlotLeases>()); }
void sl_pool_delete(void *p) { delete (Pool *)p; }                    // what drop_scratch_pool does to the table: the pool's reference goes
int sl_pool_held(void *p, int s) { return (*(Pool *)p)->held[s]; }
void *sl_lease_new(int s) { return new gs::SlotLease((gs::ScratchSlot)s); }
int sl_lease_take(void *l, void *p) { return ((gs::SlotLease *)l)->take(*(Pool *)p); }
// GS_OK and 1: this call took the lease (its content is unknown); GS_OK and 0: the object held it already; an error leaves 0
int sl_lease_take_fresh(void *l, void *p, int *fresh)
{
    bool f = true;
    const int rc = ((gs::SlotLease *)l)->take(*(Pool *)p, &f);
    *fresh = f ? 1 : 0;
    return rc;
}
void sl_lease_give(void *l) { ((gs::SlotLease *)l)->give(); }
void sl_lease_delete(void *l) { delete (gs::SlotLease *)l; }
}
