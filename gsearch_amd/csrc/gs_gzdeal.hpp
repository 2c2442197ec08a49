// The deal of a call's .gz files between the two pipelines of gs_sketch_files (gs_files.hip, sketch_files_all). Host code only: no HIP, so
// that the claim rule can be compiled and checked with the host compiler alone (tests/gzdeal_shim.cpp, tests/test_gzdeal_cpu.py).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <mutex>

// The .gz files of a call are dealt between two pipelines as they go (see gs_sketch_files): the host pipeline claims them from the front of
// the list, the device pipeline from the back, group by group, until the two meet.
// The device pipeline takes a group only as large as lets both finish together. Host pipeline: rate ra (files/s, measured once 256 files are
// done, a prior before). Device pipeline: a start-up latency (reading, copying and inflating its first group: nothing is done before) and a
// rate rb behind it. With pa, pb files claimed but unfinished and R unclaimed: lat + (pb + k) / rb = (R - k + pa) / ra.
struct GzDeal {
    std::mutex m; uint64_t n_gz = 0, front = 0, back = 0, done_front = 0, done_back = 0;
    int64_t fixed_share = -1;            // GS_GZIP_DEAL_SHARE (measurement aid): >= 0 = what device_share answers, whatever the rates
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    static constexpr double LAT = 0.45, RATE_HOST = 2300.0, RATE_DEV = 3500.0;      // the priors
    static constexpr uint64_t RATE_AFTER = 256;          // files a side must have done before its measured rate replaces the prior
    static constexpr uint64_t MIN_CLAIM = 128;           // a launch costs the same ~0.4 s for 100 members as for 1000: below this the device side takes none
    double rate(bool back_side) const
    {
        const uint64_t d = back_side ? done_back : done_front;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - (back_side ? LAT : 0.0);
        return d >= RATE_AFTER && el > 0.05 ? (double)d / el : (back_side ? RATE_DEV : RATE_HOST);
    }
    // members the device pipeline should take now out of `avail`
    double device_share(uint64_t avail) const
    {
        if (fixed_share >= 0) return (double)fixed_share;
        const double ra = rate(false), rb = rate(true);
        const double pa = (double)(front - done_front), pb = (double)(back - done_back);
        return (((double)avail + pa) / ra - pb / rb - (done_back ? 0.0 : LAT)) / (1.0 / rb + 1.0 / ra);
    }
    // One side asks for the next `cnt` members of its end of the list and is told how many it gets. The front (host) side gets what is left of
    // them; the back (device) side at most its share, and none when that share is below MIN_CLAIM. Fewer than cnt: the caller's group is its last.
    uint64_t claim(bool from_back, uint64_t cnt)
    {
        std::lock_guard<std::mutex> lk(m);
        const uint64_t avail = n_gz - front - back;
        uint64_t take = std::min(cnt, avail);
        if (from_back) {
            const double k = device_share(avail);
            take = k < (double)MIN_CLAIM ? 0 : std::min<uint64_t>(take, (uint64_t)k);
        }
        (from_back ? back : front) += take;
        return take;
    }
    // a side has finished (sketched) n of the members it claimed
    void finished(bool from_back, uint64_t n)
    {
        std::lock_guard<std::mutex> lk(m);
        (from_back ? done_back : done_front) += n;
    }
};
