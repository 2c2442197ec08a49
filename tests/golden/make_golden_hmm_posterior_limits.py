#!/usr/bin/env python
"""Generates tests/golden/hmm_posterior_limits.json: Forward, Backward and the posterior envelopes of SPEC 13.4 at the length limit (GS_HMM_FWD_MAX_L =
65536) against the largest profile (M = 1280), computed by the numpy restatement (pyref_hmm_posterior.posterior). Same status as hmm_limits.json: it pins
THIS repository's SPEC arithmetic. The file holds M, L, the seed and the place of the planted consensus, the sha256 of the profile's text
(tests/test_gpu_hmm_posterior.py builds the text and the record again and checks it), fwd, bck, the envelopes and the sha256 of the int32 out[1..L]
and cont[1..L] rows. It takes about a minute.

Run from the repo root:  python tests/golden/make_golden_hmm_posterior_limits.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hmm_classes_case as K  # noqa: E402
import pyref_hmm as R  # noqa: E402
import pyref_hmm_posterior as P  # noqa: E402

M, L, SEED, AT = 1280, 65536, 1341, 30001


def main():
    text = K.model_text(M)
    tab = R.parse_hmm(text)[0]["tables"]
    rng = np.random.default_rng(SEED)
    c = R.consensus(tab)
    rec = R.background(rng, AT - 1) + c + R.background(rng, L - (AT - 1) - M)
    assert len(rec) == L
    p = P.posterior(tab, rec, rows=True)
    sha = lambda a: hashlib.sha256(a[1:].astype(np.int32).tobytes()).hexdigest()                # noqa: E731
    case = {"M": M, "L": L, "seed": SEED, "planted_at": AT, "sha256": K.sha256(text), "fwd": p["fwd"], "bck": p["bck"], "env": [[int(v) for v in e] for e in p["env"]],
            "out_sha256": sha(p["out"]), "cont_sha256": sha(p["cont"])}
    with open(os.path.join(HERE, "hmm_posterior_limits.json"), "w") as f:
        json.dump({"cases": [case]}, f, indent=1)
    print("wrote hmm_posterior_limits.json", case)


if __name__ == "__main__":
    main()
