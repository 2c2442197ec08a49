#!/usr/bin/env python3
"""Generates tests/golden/hmm_limits.json: the raw Viterbi and Forward scores of records at the length limits of SPEC 13 and 13.1 (GS_HMM_MAX_L = 2^18,
GS_HMM_FWD_MAX_L = 65536) against the two profiles of tests/hmm_classes_case.py whose cells grow as fast as the tables allow, from the numpy
restatements alone (pyref_hmm.viterbi, pyref_hmm_forward.blocked_batch joining with lse). Same status as the other golden files: it pins THIS
repository's SPEC arithmetic. Per case: the profile kind, M, L, the sha256 of the profile's text (tests/test_gpu_hmm_classes.py builds the text again
and compares, so that a drift of synth_model or write_hmm shows instead of being compared silently), the raw score, and for Forward the largest M or
C cell and the largest hi - lo that lse saw.

The restatement walks every row in numpy, which no test can afford: TIME_TAKEN below. tests/test_hmm_classes_cpu.py recomputes the 2^16 Viterbi case.
Run from the repo root:  python tests/golden/make_golden_hmm_limits.py

TIME_TAKEN: 210 s on one core of a server CPU (Viterbi 9 s per 2^18 rows; Forward, with the recording lse, 33 s for M = 64 and 113 s for M = 1280)."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hmm_classes_case as K  # noqa: E402
import pyref_hmm as R  # noqa: E402
import pyref_hmm_forward as F  # noqa: E402


def recording_lse(seen):
    """F.lse that also keeps the largest hi - lo it is given"""
    def join(a, b):
        seen["max_hi_lo"] = max(seen.get("max_hi_lo", 0), int(np.max(np.abs(a - b))))
        return F.lse(a, b)
    return join


def main():
    cases = []
    for score, kind, M, L in K.LIMIT_CASES:
        t0 = time.time()
        text = K.limit_text(kind, M)
        (m,) = R.parse_hmm(text)
        rec = b"W" * L
        row = {"score": score, "kind": kind, "M": M, "L": L, "sha256": K.sha256(text)}
        if score == "viterbi":
            row["raw"] = R.viterbi(m["tables"], rec)
        else:
            seen = {}
            row["raw"] = int(F.blocked_batch(m["tables"], [rec], join=recording_lse(seen), cells=seen)[0])
            row["max_cell"], row["max_hi_lo"] = seen["max_cell"], seen["max_hi_lo"]
        cases.append(row)
        print(row, "%.1f s" % (time.time() - t0), flush=True)
    with open(os.path.join(HERE, "hmm_limits.json"), "w") as f:
        json.dump({"record": "b'W' * L", "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote hmm_limits.json", len(cases), "cases")


if __name__ == "__main__":
    main()
