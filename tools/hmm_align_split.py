#!/usr/bin/env python3
"""The second line of profiles/hmm_align_rate.log: how the kernel time of a gs_hmm_align_dev call splits between its launches, from a
kernel trace of one more run of tools/hmm_rate.py --align, taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/hmm_rate.py --align --repeat 1 --check 0 --log OUT/traced.log
    python tools/hmm_align_split.py OUT/kt_kernel_stats.csv [--repeat 1] >> profiles/hmm_align_rate.log

With --repeat R the traced run makes R + 1 rounds (the first is the warm-up) of null2, align and align_cols over each of its two pair lists, so per
list k_hmm_n2_forward runs in 3 (R + 1) calls, k_hmm_n2_backward in R + 1 and the k_hmm_ali_* kernels in 2 (R + 1). The figures are sums over both
lists: milliseconds of one call of each kind."""
import argparse
import collections
import csv
import json
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stats_csv")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    total = collections.Counter()
    for row in csv.DictReader(open(a.stats_csv)):
        m = re.search(r"(k_hmm_\w+)", row["Name"])
        if m:
            total[m.group(1)] += int(row["TotalDurationNs"]) / 1e6
    rounds = a.repeat + 1
    calls = {"k_hmm_n2_forward": 3 * rounds, "k_hmm_n2_backward": rounds, "k_hmm_ali_backward": 2 * rounds, "k_hmm_ali_rows": 2 * rounds, "k_hmm_ali_walk": 2 * rounds}
    per_call = {k: total[k] / n for k, n in calls.items()}
    align = {k: v for k, v in per_call.items() if k != "k_hmm_n2_backward"}
    print(json.dumps({"kernel_trace_of_one_more_run_ms_total": {k: round(total[k], 3) for k in list(calls) + ["k_hmm_n2_flag", "k_hmm_ali_fill"]},
                      "rounds_in_that_run": rounds, "per_call_both_lists_ms": {k: round(v, 1) for k, v in per_call.items()},
                      "share_of_an_align_call": {k: round(v / sum(align.values()), 2) for k, v in align.items()}}))


if __name__ == "__main__":
    main()
