// host shim of tests/test_gzdeal_cpu.py: gsearch_amd/csrc/gs_gzdeal.hpp as the host compiler sees it, one GzDeal per handle
#include "../gsearch_amd/csrc/gs_gzdeal.hpp"

extern "C" {
// out[0..4] = LAT, the host prior, the device prior (files/s), done files before a measured rate counts, the smallest claim of the back side
void gzdeal_constants(double *out)
{
    out[0] = GzDeal::LAT; out[1] = GzDeal::RATE_HOST; out[2] = GzDeal::RATE_DEV; out[3] = (double)GzDeal::RATE_AFTER; out[4] = (double)GzDeal::MIN_CLAIM;
}
// fixed_share < 0: the share comes from the rates (GS_GZIP_DEAL_SHARE unset)
void *gzdeal_new(unsigned long long n_gz, long long fixed_share)
{
    GzDeal *d = new GzDeal;
    d->n_gz = n_gz; d->fixed_share = fixed_share;
    return d;
}
void gzdeal_free(void *h) { delete (GzDeal *)h; }
unsigned long long gzdeal_claim(void *h, int from_back, unsigned long long cnt) { return ((GzDeal *)h)->claim(from_back != 0, cnt); }
void gzdeal_finished(void *h, int from_back, unsigned long long n) { ((GzDeal *)h)->finished(from_back != 0, n); }
// out[0..3] = front, back, done_front, done_back
void gzdeal_state(void *h, unsigned long long *out)
{
    const GzDeal *d = (const GzDeal *)h;
    out[0] = d->front; out[1] = d->back; out[2] = d->done_front; out[3] = d->done_back;
}
}
