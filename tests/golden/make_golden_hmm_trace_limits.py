#!/usr/bin/env python3
"""Generates tests/golden/hmm_trace_limits.json: the trace-back of SPEC 13.2 at its length limit (GS_HMM_TRACE_MAX_L = 65536) against the largest profile
whose cells grow as fast as the tables allow, hmm_classes_case.all_zero_model(1280), record b"W" * 65536, from the numpy restatement alone
(pyref_hmm_trace.trace, which asserts both identities of the spec and raw == pyref_hmm.viterbi on the way). Same status as hmm_limits.json: it pins THIS
repository's SPEC arithmetic. The file holds the profile kind, M, L, the sha256 of the profile's text (tests/test_gpu_hmm_trace.py builds the text again
and compares), the raw score and every domain.

The restatement keeps three int32 matrices and a byte of pointers per cell, 84 million cells: 1.1 GB and TIME_TAKEN below, which no test can afford.
Run from the repo root:  python tests/golden/make_golden_hmm_trace_limits.py

TIME_TAKEN: 15 s on one core of a server CPU."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hmm_classes_case as K  # noqa: E402
import pyref_hmm as R  # noqa: E402
import pyref_hmm_trace as T  # noqa: E402

CASES = (("zero", 1280, T.TRACE_MAX_L),)


def main():
    cases = []
    for kind, M, L in CASES:
        t0 = time.time()
        text = K.limit_text(kind, M)
        (m,) = R.parse_hmm(text)
        raw, doms = T.trace(m["tables"], b"W" * L)
        cases.append({"kind": kind, "M": M, "L": L, "sha256": K.sha256(text), "raw": raw, "domains": [list(d) for d in doms]})
        print(kind, M, L, raw, len(doms), "domains", "%.1f s" % (time.time() - t0), flush=True)
    with open(os.path.join(HERE, "hmm_trace_limits.json"), "w") as f:
        json.dump({"record": "b'W' * L", "cases": cases}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote hmm_trace_limits.json", len(cases), "cases")


if __name__ == "__main__":
    main()
