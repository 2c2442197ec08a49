"""Inputs of tests/test_hmm_align_cpu.py and tests/test_gpu_hmm_align.py for the rule of allowed transitions (SPEC 13.6): deletion-friendly profiles
(tests/hmm_classes_case.py) with `*` written into transitions BETWEEN valid nodes, each against a record whose best alignment would otherwise delete
across the starred place, so that the masks decide output words. Nothing here calls the library.

Where the star sits matters to the device (k_hmm_ali_rows of gs_hmm.hip): lane l holds nodes l Q + 1 .. l Q + Q. D[k] is handed to D[k + 1] through
d->d of node k. With k % Q != 0 the link lies inside a lane's group - the lane's own D chain and the row of prefix minima decide; with k % Q == 0 it is
the link that leaves the lane - the group's minimum, the scan over lanes and the edge nibble decide. m->d starred at every node closes the way into D."""
import numpy as np

import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_forward as F

# (kind, M, the nodes whose d->d is starred): classes Q = 2, 6, 3, 3, 8, 8, 20, 20
CASES = (("md", 121, ()), ("md", 257, ()), ("dd", 192, (100,)), ("dd", 192, (99,)), ("dd", 512, (203,)), ("dd", 512, (200,)), ("dd", 1280, (630,)), ("dd", 1280, (620,)))


def model(kind, M, nodes):
    """hmm_classes_case.deletion_model(M) with every m->d starred (its probability goes to m->m), or with d->d of `nodes` starred (to d->m)"""
    s = K.deletion_model(M)
    s["name"] = "%s%d_%s" % (kind.upper(), M, "_".join(str(k) for k in nodes))
    if kind == "md":
        for k in range(M + 1):
            s["tr"][k][0] += s["tr"][k][2]
            s["tr"][k][2] = 0.0
    else:
        for k in nodes:
            s["tr"][k][5], s["tr"][k][6] = 1.0, 0.0
    return s


def record(c, M):
    """two ends of the consensus c with the middle left out: 30 + 51 nodes of 121, else 35 nodes from either end"""
    return c[:30] + c[70:] if M == 121 else c[:35] + c[M - 35:]


def where(M, k):
    """'inside' a lane's group or on its 'edge': where the d->d link of node k lies for the kernel class of M"""
    return "edge" if k % F.group_size(M) == 0 else "inside"


def build():
    """-> (texts, models, records): one profile and one record per case, the record inside a few background residues"""
    rng = np.random.default_rng(1371)
    texts = [R.write_hmm(model(*case)) for case in CASES]
    models = [m for t in texts for m in R.parse_hmm(t)]
    records = [R.background(rng, 3) + record(R.consensus(m["tables"]), m["M"]) + R.background(rng, 2) for m in models]
    return texts, models, records
