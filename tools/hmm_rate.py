#!/usr/bin/env python3
"""Rate of hmmsearch on the device: a synthetic proteome of `n` proteins (lengths drawn around 300 residues, background
composition) against 120 synthetic profiles with the node counts of the bacterial universal-gene set
(tests/golden/hmm/bacteria_node_counts.txt).

  search   cells/s of gs_hmm_search_dev (cells = residues of the proteome x nodes of the set), device arrays in place, the best of `repeat` runs
  best     seconds of gs_hmm_best_hits_dev over the score matrix, the proteome as one genome
  check    `check` sampled (protein, profile) pairs compared with the numpy restatement (tests/pyref_hmm.py): the expected difference is 0

--forward (SPEC 13.1), on the same proteome and profile set:
  forward_all   cells/s of the Forward launches alone with every pair selected: gs_hmm_search_forward_dev without a floor, less the Viterbi time above
  filtered      the pipeline at the default floors (P = 1e-3): the share of the pairs that reach their profile's floor, and the seconds of selection
                plus Forward (the call less the Viterbi time) beside the Viterbi seconds
  check         `check` sampled pairs compared with the restatement (tests/pyref_hmm_forward.py): the expected difference is 0

--trace (SPEC 13.2), on the same proteome and profile set:
  trace_best    seconds of gs_hmm_trace_dev over the best hit of every profile (the proteome as one genome): what universal_genes(region="aligned") pays
  trace_all     seconds and cells/s of gs_hmm_trace_dev over ALL pairs with max_dom = 2 (the trace kernels, the walks and the host's grouping of the
                pairs into blocks; the default block size), beside the Viterbi seconds of the same run
  check         the raw of every traced pair against the score matrix, and `check` sampled pairs against the restatement (tests/pyref_hmm_trace.py)

--msv (SPEC 13.3), on the same proteome and profile set:
  msv           cells/s of the MSV launches alone (gs_hmm_search_msv_dev)
  passing       the share of the pairs at or above their profile's MSV floor of P = 0.02 (the STATS LOCAL MSV lines of the synthetic profiles are
                not calibrated: the share is that of this set, not the 2 % of a calibrated one)
  filtered      seconds of gs_hmm_search_filtered_dev (MSV + selection + Viterbi over the selected lists) beside gs_hmm_search_dev of the same build,
                the two alternating in one loop: `repeat` timed pairs after a warm-up pair, every time listed, the minimum and the median reported.
                --parent-s S records beside them the seconds of the parent commit's gs_hmm_search_dev on this input, as the parent's build of this
                tool reports them (search_s): that kernel is the yardstick
  check         the Viterbi words of the filtered search against the unfiltered matrix wherever they ran, the selection against the MSV matrix and the
                floors, and `check` sampled pairs of the MSV matrix against the restatement (tests/pyref_hmm_msv.py): the expected differences are 0

With --posterior also (SPEC 13.4):
  posterior     seconds of gs_hmm_envelopes_dev over ALL pairs with max_env = 2 (per block: Forward with rows, Backward, k_hmm_envelopes, the envelope
                scores) and, alternating with it in the same rounds, of gs_hmm_search_forward_dev with every pair selected: that call is the parent
                commit's code and the yardstick. Times of every round are kept, so the spread is in the log. The split between the four kernel
                families comes from a kernel trace of one more run of this mode (rocprofv3 --kernel-trace --stats, in a run of its own), kept beside the
                line in the log
  check         fwd of every pair against the Forward matrix, |fwd - bck| against the bound of SPEC 13.4, and `check` sampled pairs (fwd, bck, n_env,
                envelopes) against the restatement (tests/pyref_hmm_posterior.py): the expected differences are 0

With --null2 also (SPEC 13.5):
  envelopes     seconds of gs_hmm_envelopes_dev with max_env = 2 over the pairs whose Forward raw reaches the profile's GA (`ga`) and over ALL pairs
                (`all`): the parent commit's code, the yardstick, alternating with null2 in the same rounds
  null2         seconds of gs_hmm_null2_dev over the envelopes those calls listed - what the correction adds to gs_hmm_envelopes -, the listed slots and
                their cells (sum of Ld x M of the slot's profile; the kernels run 64 Q columns a row, of which M are nodes). The split between
                k_hmm_n2_forward and k_hmm_n2_backward comes from a kernel trace of one more run of this mode, kept beside the line in the log
  check         seg_raw of every listed slot against env_raw, both biases >= 0, the largest |mass|, and `check` sampled pairs against the restatement
                (tests/pyref_hmm_null2.py): the expected differences are 0

With --align also (SPEC 13.6), over the same two pair lists (`ga`, `all`) with max_env = 2:
  null2         seconds of gs_hmm_null2_dev on the listed slots: the parent commit's kernels (profiles/hmm_align_resources.txt shows them unchanged; the
                parent's own run is profiles/hmm_null2_rate.log), the yardstick, alternating with align in the same rounds
  align         seconds of gs_hmm_align_dev on the same slots without columns, and with them (`align_cols`); the slots, their rows and cells. The split
                between k_hmm_n2_forward, k_hmm_ali_backward, k_hmm_ali_rows and k_hmm_ali_walk comes from a kernel trace of one more run of this
                mode; tools/hmm_align_split.py turns the trace's statistics into the line kept beside this one in the log
  check         the identities of SPEC 13.6 on every listed slot, and `check` sampled pairs against the restatement (tests/pyref_hmm_align.py): the
                expected differences are 0

--vit16 (SPEC 13.7), on the same proteome and profile set:
  vf            cells/s of the int16 filter launches alone (gs_hmm_search_vit16_dev), beside gs_hmm_search_dev of the same build - the parent commit's
                kernel, unchanged (profiles/hmm_vit16_resources.txt) -, the calls alternating inside a round: `repeat` timed rounds after a warm-up
                round, every time listed, the minimum and the median reported
  staged        seconds of gs_hmm_search_staged_dev with vf_floor = 0 (the score table's raw >= 0; `staged0`), with vf_floor = GA (universal_genes;
                `staged_ga`) and with MSV in front at P = 0.02 and vf_floor = 0 (`msv_staged0`), beside gs_hmm_search_filtered_dev (`msv_filtered`) in
                the same rounds; the share of the pairs that go on to int32 Viterbi in each
  check         no pair with vit >= floor is missing behind the filter and its words are those of the unfiltered matrix, vf >= vit wherever neither
                overflows, the overflowing pairs counted, and `check` sampled pairs of vf against the restatement (tests/pyref_hmm_vit16.py): the
                expected differences are 0

--dump PATH saves the downloaded matrices of the modes that ran as one .npz (the Viterbi scores; both Forward matrices; raw, n_dom and the domain
words of trace_best and trace_all), so that two builds of the library (GS_LIB_PATH) can be compared word for word.

usage: hmm_rate.py [--forward | --trace | --posterior | --null2 | --align | --vit16 | --msv [--parent-s S]] [--n 4000] [--repeat 3] [--check 8] [--dump PATH]
                   [--log profiles/hmm_rate.log | hmm_forward_rate.log | hmm_trace_rate.log | hmm_msv_rate.log | hmm_posterior_rate.log |
                   hmm_null2_rate.log | hmm_align_rate.log | hmm_vit16_rate.log]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--msv", action="store_true")
    ap.add_argument("--posterior", action="store_true")
    ap.add_argument("--null2", action="store_true")
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--vit16", action="store_true")
    ap.add_argument("--parent-s", type=float, default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    if a.log is None and a.align:
        a.log = os.path.join(ROOT, "profiles", "hmm_align_rate.log")
    if a.log is None and a.vit16:
        a.log = os.path.join(ROOT, "profiles", "hmm_vit16_rate.log")
    if a.log is None and a.null2:
        a.log = os.path.join(ROOT, "profiles", "hmm_null2_rate.log")
    if a.log is None:
        a.log = os.path.join(ROOT, "profiles", "hmm_forward_rate.log" if a.forward else ("hmm_trace_rate.log" if a.trace else ("hmm_msv_rate.log" if a.msv else ("hmm_posterior_rate.log" if a.posterior else "hmm_rate.log"))))
    import gsearch_amd as G
    import pyref_hmm as R
    rng = np.random.default_rng(a.seed)
    nodes = [int(x) for x in open(os.path.join(ROOT, "tests", "golden", "hmm", "bacteria_node_counts.txt")).read().split()]
    texts = [R.write_hmm(R.synth_model(rng, M, name="SYN%03d_%d" % (i, M))) for i, M in enumerate(nodes)]
    ctx = G.default_context()
    db = G.HmmDb(texts, ctx, texts=True)
    lens = np.clip(rng.gamma(3.0, 100.0, size=a.n).astype(np.int64), 30, 3000)
    recs = [R.background(rng, int(L)) for L in lens]
    for j in range(0, a.n, 40):                                  # one protein in 40 carries the consensus of a profile, as a proteome would
        recs[j] = R.consensus(R.parse_hmm(texts[(j // 40) % len(texts)])[0]["tables"])
    aa, rs, rl = G.filter_aa_records(recs)
    cells = int(rl.sum()) * sum(nodes)
    res = {"proteins": a.n, "residues": int(rl.sum()), "profiles": len(nodes), "nodes": sum(nodes), "cells": cells}
    goff = np.array([0, a.n], np.uint64)
    thr = db.thresholds("ga")
    arrays = (aa, rs, rl, goff, thr)
    ptrs = [ctx.alloc(max(x.nbytes, 16)) for x in arrays]
    for p, x in zip(ptrs, arrays):
        ctx.upload(p, x)
    d_score = ctx.alloc(4 * a.n * len(db))
    d_rec, d_best = ctx.alloc(4 * len(db)), ctx.alloc(4 * len(db))
    best = float("inf")
    for run in range(a.repeat + 1):                              # the first run pays for the module load and the scratch: not counted
        ctx.sync()
        t = time.perf_counter()
        db.search_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_score)
        ctx.sync()
        if run:
            best = min(best, time.perf_counter() - t)
    res["search_s"] = best
    res["cells_per_s"] = cells / best
    t = time.perf_counter()
    db.best_hits_dev(d_score, a.n, ptrs[3], 1, ptrs[4], d_rec, d_best)
    ctx.sync()
    res["best_hits_s"] = time.perf_counter() - t
    scores = ctx.download(d_score, (a.n, len(db)), np.int32)
    hit = ctx.download(d_rec, (len(db),), np.uint32)
    res["profiles_with_a_hit"] = int((hit != R.NO_HIT).sum())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(len(db)))
        diff += int(scores[r, p]) != R.viterbi(R.parse_hmm(texts[p])[0]["tables"], recs[r])
    res["check_pairs"], res["check_differences"] = a.check, diff
    dump = {"viterbi": scores}
    if a.forward:
        forward_part(a, ctx, db, texts, recs, ptrs, d_score, scores, cells, res, rng, dump)
    if a.trace:
        trace_part(a, ctx, db, texts, recs, ptrs, d_rec, scores, cells, res, rng, dump)
    if a.msv:
        msv_part(a, ctx, db, texts, recs, ptrs, d_score, scores, cells, res, rng, dump)
    if a.posterior:
        posterior_part(a, ctx, db, texts, recs, ptrs, d_score, cells, res, rng, dump)
    if a.null2:
        null2_part(a, ctx, db, texts, recs, ptrs, d_score, res, rng, dump)
    if a.align:
        align_part(a, ctx, db, texts, recs, ptrs, d_score, res, rng, dump)
    if a.vit16:
        vit16_part(a, ctx, db, texts, recs, ptrs, d_score, scores, cells, res, rng, dump)
    if a.dump:
        with open(a.dump, "wb") as f:
            np.savez(f, **dump)
    for p in ptrs + [d_score, d_rec, d_best]:
        ctx.free(p)
    db.close()
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")


def forward_part(a, ctx, db, texts, recs, ptrs, d_vit, vit, cells, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_forward as F
    d_fwd = ctx.alloc(4 * a.n * len(db))
    floor = db.viterbi_floor(1e-3)
    d_floor = ctx.alloc(floor.nbytes)
    ctx.upload(d_floor, floor)
    times = {}
    for name, fl in (("all", None), ("filtered", d_floor)):
        best = float("inf")
        for run in range(a.repeat + 1):
            ctx.sync()
            t = time.perf_counter()
            db.search_forward_dev(ptrs[0], ptrs[1], ptrs[2], a.n, fl, d_vit, d_fwd)
            ctx.sync()
            if run:
                best = min(best, time.perf_counter() - t)
        times[name] = best
        if name == "all":
            fwd_all = ctx.download(d_fwd, (a.n, len(db)), np.int32)
    fwd = ctx.download(d_fwd, (a.n, len(db)), np.int32)
    dump.update(forward_all=fwd_all, forward_filtered=fwd)
    res["forward_all_call_s"] = times["all"]
    res["forward_all_s"] = times["all"] - res["search_s"]
    res["forward_cells_per_s"] = cells / res["forward_all_s"]
    res["forward_over_viterbi"] = res["forward_all_s"] / res["search_s"]
    res["filter_p"] = 1e-3
    res["selected_share"] = float((fwd != R.NO_SCORE).mean())
    res["filtered_call_s"] = times["filtered"]
    res["select_plus_forward_s"] = times["filtered"] - res["search_s"]
    sel = (vit != R.NO_SCORE) & (vit.astype(np.int64) >= floor[None, :])
    res["selection_differences"] = int(((fwd != R.NO_SCORE) != sel).sum())
    res["filtered_differs_from_all"] = int((fwd[sel] != fwd_all[sel]).sum())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(len(db)))
        diff += int(fwd_all[r, p]) != F.forward(R.parse_hmm(texts[p])[0]["tables"], recs[r])
    res["forward_check_pairs"], res["forward_check_differences"] = a.check, diff
    ctx.free(d_fwd)
    ctx.free(d_floor)


def posterior_part(a, ctx, db, texts, recs, ptrs, d_vit, cells, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_posterior as P
    n_prof, max_env = len(db), 2
    n = a.n * n_prof
    pr, pp = np.repeat(np.arange(a.n, dtype=np.uint32), n_prof), np.tile(np.arange(n_prof, dtype=np.uint32), a.n)
    d_pr, d_pp = ctx.alloc(pr.nbytes), ctx.alloc(pp.nbytes)
    ctx.upload(d_pr, pr); ctx.upload(d_pp, pp)
    d_fwd_all = ctx.alloc(4 * n)
    bufs = [ctx.alloc(4 * n) for _ in range(3)] + [ctx.alloc(4 * n * max_env * 4)]

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t

    runs = {"forward_all": lambda: db.search_forward_dev(ptrs[0], ptrs[1], ptrs[2], a.n, None, d_vit, d_fwd_all),
            "posterior": lambda: db.envelopes_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, *bufs)}
    times = {k: [] for k in runs}
    for it in range(a.repeat + 1):                               # the first round is the warm-up of both; the two alternate inside a round
        for k, call in runs.items():
            t = timed(call)
            if it:
                times[k].append(t)
    fwd_all = ctx.download(d_fwd_all, (a.n, n_prof), np.int32)
    fwd, bck = ctx.download(bufs[0], (n,), np.int32), ctx.download(bufs[1], (n,), np.int32)
    ne, env = ctx.download(bufs[2], (n,), np.uint32), ctx.download(bufs[3], (n, max_env, 4), np.int32)
    dump.update(posterior_fwd=fwd, posterior_bck=bck, posterior_n_env=ne, posterior_env=env)
    for k, ts in times.items():
        res[k + "_times_s"] = ts
        res[k + "_min_s"], res[k + "_median_s"] = min(ts), float(np.median(ts))
    res["forward_all_minus_viterbi_s"] = res["forward_all_min_s"] - res["search_s"]          # the call runs Viterbi in front of Forward
    res["forward_cells_per_s"] = cells / res["forward_all_minus_viterbi_s"]
    res["posterior_over_forward"] = res["posterior_min_s"] / res["forward_all_minus_viterbi_s"]
    res["posterior_pairs"], res["envelopes"], res["pairs_with_more_than_2"] = n, int(ne.sum()), int((ne > max_env).sum())
    res["fwd_differs_from_forward_matrix"] = int((fwd.reshape(a.n, n_prof) != fwd_all).sum())
    res["largest_fwd_minus_bck"] = int(np.abs(fwd.astype(np.int64) - bck)[fwd != R.NO_SCORE].max())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(n_prof))
        want = P.envelope_pairs([R.parse_hmm(texts[p])[0]], recs, [r], [0], max_env)
        j = r * n_prof + p
        diff += int(not (fwd[j] == want[0][0] and bck[j] == want[1][0] and ne[j] == want[2][0] and np.array_equal(env[j], want[3][0])))
    res["posterior_check_pairs"], res["posterior_check_differences"] = a.check, diff
    for ptr in [d_pr, d_pp, d_fwd_all] + bufs:
        ctx.free(ptr)


def null2_part(a, ctx, db, texts, recs, ptrs, d_vit, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_null2 as N
    n_prof, max_env = len(db), 2
    M = np.array([int(m) for m in db.M], np.int64)
    d_fwd_all = ctx.alloc(4 * a.n * n_prof)
    db.search_forward_dev(ptrs[0], ptrs[1], ptrs[2], a.n, None, d_vit, d_fwd_all)
    ctx.sync()
    fwd_all = ctx.download(d_fwd_all, (a.n, n_prof), np.int32)
    ctx.free(d_fwd_all)
    thr = db.thresholds("ga").astype(np.int64)
    ga = np.argwhere((fwd_all != R.NO_SCORE) & (fwd_all.astype(np.int64) >= thr[None, :]))
    lists = {"ga": (ga[:, 0].astype(np.uint32), ga[:, 1].astype(np.uint32)),
             "all": (np.repeat(np.arange(a.n, dtype=np.uint32), n_prof), np.tile(np.arange(n_prof, dtype=np.uint32), a.n))}

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t

    for name, (pr, pp) in lists.items():
        n = len(pr)
        d_pr, d_pp = ctx.alloc(max(pr.nbytes, 16)), ctx.alloc(max(pp.nbytes, 16))
        ctx.upload(d_pr, pr); ctx.upload(d_pp, pp)
        e_bufs = [ctx.alloc(max(4 * n, 16)) for _ in range(3)] + [ctx.alloc(max(4 * n * max_env * 4, 16))]
        n_bufs = [ctx.alloc(max(4 * n * max_env * 4, 16)), ctx.alloc(max(4 * n, 16))]
        runs = {"envelopes": lambda: db.envelopes_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, *e_bufs),
                "null2": lambda: db.null2_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, e_bufs[2], e_bufs[3], n_bufs[0], n_bufs[1])}
        times = {k: [] for k in runs}
        for it in range(a.repeat + 1):                           # the first round is the warm-up of both; the two alternate inside a round
            for k, call in runs.items():
                t = timed(call)
                if it:
                    times[k].append(t)
        fwd = ctx.download(e_bufs[0], (n,), np.int32)
        ne, env = ctx.download(e_bufs[2], (n,), np.uint32), ctx.download(e_bufs[3], (n, max_env, 4), np.int32)
        slots, sb = ctx.download(n_bufs[0], (n, max_env, 4), np.int32), ctx.download(n_bufs[1], (n,), np.int32)
        dump.update({"null2_%s_slots" % name: slots, "null2_%s_seq_bias" % name: sb})
        listed = np.arange(max_env)[None, :] < np.minimum(ne, max_env)[:, None]
        Ld = (env[:, :, 1] - env[:, :, 0] + 1).astype(np.int64) * listed
        for k, ts in times.items():
            res["%s_%s_times_s" % (k, name)] = ts
            res["%s_%s_min_s" % (k, name)], res["%s_%s_median_s" % (k, name)] = min(ts), float(np.median(ts))
        res["null2_%s_pairs" % name], res["null2_%s_slots" % name] = n, int(listed.sum())
        res["null2_%s_rows" % name] = int(Ld.sum())
        res["null2_%s_cells" % name] = int((Ld * M[pp][:, None]).sum())
        res["null2_%s_over_envelopes" % name] = res["null2_%s_min_s" % name] / res["envelopes_%s_min_s" % name]
        res["null2_%s_seg_raw_differs_from_env_raw" % name] = int((slots[:, :, 2] != env[:, :, 2])[listed].sum())
        res["null2_%s_negative_biases" % name] = int((slots[:, :, 1] < 0).sum() + (sb < 0).sum())
        res["null2_%s_largest_abs_mass" % name] = int(np.abs(slots[:, :, 3]).max()) if n else 0
        res["null2_%s_pairs_below_ga_after_correction" % name] = int(((fwd.astype(np.int64) >= thr[pp]) & (fwd.astype(np.int64) - sb < thr[pp]) & (fwd != R.NO_SCORE)).sum())
        if name == "ga":
            res["null2_ga_largest_seq_bias_bits"] = float(sb.max() / 1024.0) if n else 0.0
            diff = 0
            for _ in range(a.check):
                j = int(rng.integers(n))
                want = N.null2_pairs([R.parse_hmm(texts[int(pp[j])])[0]], recs, [int(pr[j])], [0], ne[j:j + 1], env[j:j + 1], max_env)
                diff += int(not (np.array_equal(slots[j], want[0][0]) and sb[j] == want[1][0]))
            res["null2_check_pairs"], res["null2_check_differences"] = a.check, diff
        for ptr in [d_pr, d_pp] + e_bufs + n_bufs:
            ctx.free(ptr)


def align_part(a, ctx, db, texts, recs, ptrs, d_vit, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_align as A
    n_prof, max_env = len(db), 2
    M = np.array([int(m) for m in db.M], np.int64)
    d_fwd_all = ctx.alloc(4 * a.n * n_prof)
    db.search_forward_dev(ptrs[0], ptrs[1], ptrs[2], a.n, None, d_vit, d_fwd_all)
    ctx.sync()
    fwd_all = ctx.download(d_fwd_all, (a.n, n_prof), np.int32)
    ctx.free(d_fwd_all)
    thr = db.thresholds("ga").astype(np.int64)
    ga = np.argwhere((fwd_all != R.NO_SCORE) & (fwd_all.astype(np.int64) >= thr[None, :]))
    lists = {"ga": (ga[:, 0].astype(np.uint32), ga[:, 1].astype(np.uint32)),
             "all": (np.repeat(np.arange(a.n, dtype=np.uint32), n_prof), np.tile(np.arange(n_prof, dtype=np.uint32), a.n))}

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t

    for name, (pr, pp) in lists.items():
        n = len(pr)
        d_pr, d_pp = ctx.alloc(max(pr.nbytes, 16)), ctx.alloc(max(pp.nbytes, 16))
        ctx.upload(d_pr, pr); ctx.upload(d_pp, pp)
        e_bufs = [ctx.alloc(max(4 * n, 16)) for _ in range(3)] + [ctx.alloc(max(4 * n * max_env * 4, 16))]
        db.envelopes_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, *e_bufs)
        ctx.sync()
        ne, env = ctx.download(e_bufs[2], (n,), np.uint32), ctx.download(e_bufs[3], (n, max_env, 4), np.int32)
        listed = np.arange(max_env)[None, :] < np.minimum(ne, max_env)[:, None]
        Ld = (env[:, :, 1] - env[:, :, 0] + 1).astype(np.int64) * listed
        co = np.zeros(n + 1, np.uint64)
        co[1:] = np.cumsum(Ld.sum(axis=1) + listed.sum(axis=1) * M[pp])
        d_co, d_cols = ctx.alloc(co.nbytes), ctx.alloc(max(8 * int(co[-1]), 16))
        ctx.upload(d_co, co)
        n_bufs = [ctx.alloc(max(4 * n * max_env * 4, 16)), ctx.alloc(max(4 * n, 16))]
        d_slots = ctx.alloc(max(4 * n * max_env * A.ALI_WORDS, 16))
        runs = {"null2": lambda: db.null2_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, e_bufs[2], e_bufs[3], n_bufs[0], n_bufs[1]),
                "align": lambda: db.align_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, e_bufs[2], e_bufs[3], d_slots),
                "align_cols": lambda: db.align_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, d_pp, n, max_env, e_bufs[2], e_bufs[3], d_slots, d_co, d_cols)}
        times = {k: [] for k in runs}
        for it in range(a.repeat + 1):                           # the first round is the warm-up of all; they alternate inside a round
            for k, call in runs.items():
                t = timed(call)
                if it:
                    times[k].append(t)
        slots = ctx.download(d_slots, (n, max_env, A.ALI_WORDS), np.int32).astype(np.int64)
        cols = ctx.download(d_cols, (max(int(co[-1]), 1), 2), np.int32)
        dump.update({"align_%s_slots" % name: slots})
        for k, ts in times.items():
            res["%s_%s_times_s" % (k, name)] = ts
            res["%s_%s_min_s" % (k, name)], res["%s_%s_median_s" % (k, name)] = min(ts), float(np.median(ts))
        res["align_%s_pairs" % name], res["align_%s_slots" % name] = n, int(listed.sum())
        res["align_%s_rows" % name] = int(Ld.sum())
        res["align_%s_cells" % name] = int((Ld * M[pp][:, None]).sum())
        res["align_%s_over_null2" % name] = res["align_%s_min_s" % name] / res["null2_%s_min_s" % name]
        w = slots[listed]
        e = env[listed].astype(np.int64)
        bad = (w[:, 5] + w[:, 6] != w[:, 1] - w[:, 0] + 1) | (w[:, 5] + w[:, 7] != w[:, 3] - w[:, 2] + 1) | (w[:, 0] < e[:, 0]) | (w[:, 1] > e[:, 1]) | (w[:, 4] < 0)
        res["align_%s_identity_failures" % name] = int(bad.sum())
        res["align_%s_mean_accuracy" % name] = float((w[:, 4] / (65536.0 * (e[:, 1] - e[:, 0] + 1))).mean()) if len(w) else 0.0
        res["align_%s_columns" % name] = int(w[:, 5:8].sum())
        if name == "ga":
            diff = 0
            for _ in range(a.check):
                j = int(rng.integers(n))
                want = A.align_pairs([R.parse_hmm(texts[int(pp[j])])[0]], recs, [int(pr[j])], [0], ne[j:j + 1], env[j:j + 1], max_env)
                got = cols[int(co[j]):int(co[j + 1])]
                at = 0
                ok = np.array_equal(slots[j], want[0][0])
                for d, c in enumerate(want[1][0]):
                    ok = ok and np.array_equal(got[at:at + len(c)], A.column_words(c))
                    at += int(Ld[j, d]) + int(M[pp[j]])
                diff += int(not ok)
            res["align_check_pairs"], res["align_check_differences"] = a.check, diff
        for ptr in [d_pr, d_pp, d_co, d_cols, d_slots] + e_bufs + n_bufs:
            ctx.free(ptr)


def msv_part(a, ctx, db, texts, recs, ptrs, d_vit_all, vit_all, cells, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_msv as V
    n = a.n * len(db)
    d_msv, d_vit = ctx.alloc(4 * n), ctx.alloc(4 * n)
    floor = db.msv_floor(0.02)
    d_floor = ctx.alloc(floor.nbytes)
    ctx.upload(d_floor, floor)

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t

    runs = {"msv": lambda: db.search_msv_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_msv),
            "filtered": lambda: db.search_filtered_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_floor, None, d_msv, d_vit, None),
            "unfiltered": lambda: db.search_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_vit_all)}
    times = {k: [] for k in runs}
    for it in range(a.repeat + 1):                               # the first round is the warm-up of every shape; the three alternate inside a round
        for k, call in runs.items():
            t = timed(call)
            if it:
                times[k].append(t)
    msv = ctx.download(d_msv, (a.n, len(db)), np.int32)
    vit = ctx.download(d_vit, (a.n, len(db)), np.int32)
    dump.update(msv=msv, viterbi_filtered=vit)
    for k, ts in times.items():
        res[k + "_times_s"] = ts
        res[k + "_min_s"], res[k + "_median_s"] = min(ts), float(np.median(ts))
    res["msv_cells_per_s"] = cells / res["msv_min_s"]
    res["msv_p"] = 0.02
    sel = (msv != R.NO_SCORE) & (msv.astype(np.int64) >= floor[None, :])
    res["passing_share"] = float(sel.mean())
    res["filtered_over_unfiltered_min"] = res["filtered_min_s"] / res["unfiltered_min_s"]
    res["filtered_over_unfiltered_median"] = res["filtered_median_s"] / res["unfiltered_median_s"]
    if a.parent_s is not None:
        res["parent_search_s"] = a.parent_s
        res["filtered_over_parent"] = res["filtered_min_s"] / a.parent_s
    res["selection_differences"] = int(((vit != R.NO_SCORE) != sel).sum())
    res["filtered_differs_from_unfiltered"] = int((vit[sel] != vit_all[sel]).sum())
    thr = db.thresholds("ga").astype(np.int64)
    hits = (vit_all != R.NO_SCORE) & (vit_all.astype(np.int64) >= thr[None, :])
    res["ga_hits"], res["ga_hits_lost"] = int(hits.sum()), int((hits & ~sel).sum())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(len(db)))
        diff += int(msv[r, p]) != V.msv(R.parse_hmm(texts[p])[0]["tables"], recs[r])
    res["msv_check_pairs"], res["msv_check_differences"] = a.check, diff
    for p in (d_msv, d_vit, d_floor):
        ctx.free(p)


def vit16_part(a, ctx, db, texts, recs, ptrs, d_vit_all, vit_all, cells, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_vit16 as W
    n = a.n * len(db)
    d_vf, d_vit, d_msv = ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    floors = {"zero": np.zeros(len(db), np.int32), "ga": db.thresholds("ga"), "msv": db.msv_floor(0.02)}
    d_fl = {}
    for k, f in floors.items():
        d_fl[k] = ctx.alloc(f.nbytes)
        ctx.upload(d_fl[k], f)

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        return time.perf_counter() - t

    rec = ptrs[0], ptrs[1], ptrs[2], a.n
    runs = {"unfiltered": lambda: db.search_dev(*rec, d_vit_all),
            "vf": lambda: db.search_vit16_dev(*rec, d_vf),
            "staged0": lambda: db.search_staged_dev(*rec, False, None, d_fl["zero"], None, None, d_vf, d_vit, None),
            "staged_ga": lambda: db.search_staged_dev(*rec, False, None, d_fl["ga"], None, None, d_vf, d_vit, None),
            "msv_filtered": lambda: db.search_filtered_dev(*rec, d_fl["msv"], None, d_msv, d_vit, None),
            "msv_staged0": lambda: db.search_staged_dev(*rec, True, d_fl["msv"], d_fl["zero"], None, d_msv, d_vf, d_vit, None)}
    times = {k: [] for k in runs}
    kept = {}
    for it in range(a.repeat + 1):                               # the first round is the warm-up of every shape; the calls alternate inside a round
        for k, call in runs.items():
            t = timed(call)
            if it:
                times[k].append(t)
            elif k != "unfiltered":
                kept[k] = (ctx.download(d_vf, (a.n, len(db)), np.int32), ctx.download(d_vit, (a.n, len(db)), np.int32))
    for k, ts in times.items():
        res[k + "_times_s"] = ts
        res[k + "_min_s"], res[k + "_median_s"] = min(ts), float(np.median(ts))
    res["vf_cells_per_s"] = cells / res["vf_min_s"]
    for k in ("vf", "staged0", "staged_ga"):
        res[k + "_over_unfiltered_min"] = res[k + "_min_s"] / res["unfiltered_min_s"]
        res[k + "_over_unfiltered_median"] = res[k + "_median_s"] / res["unfiltered_median_s"]
    res["msv_staged0_over_msv_filtered_min"] = res["msv_staged0_min_s"] / res["msv_filtered_min_s"]
    res["msv_staged0_over_msv_filtered_median"] = res["msv_staged0_median_s"] / res["msv_filtered_median_s"]
    vf = kept["vf"][0]
    dump.update(vf=vf)
    has = vit_all != R.NO_SCORE
    over = vf == W.VF_OVER
    res["overflowing_pairs"] = int(over.sum())
    res["vf_below_vit"] = int((has & ~over & (vf.astype(np.int64) < vit_all.astype(np.int64))).sum())
    ex = (vf.astype(np.int64) - vit_all.astype(np.int64))[has & ~over]
    res["excess_max_units"], res["excess_mean_units"] = int(ex.max()), float(ex.mean())
    for k, fl in (("staged0", "zero"), ("staged_ga", "ga"), ("msv_staged0", "zero")):
        svf, svit = kept[k]
        ran = svit != R.NO_SCORE
        res[k + "_viterbi_share"] = float(ran.mean())
        res[k + "_vf_share"] = float((svf != R.NO_SCORE).mean())
        res[k + "_words_differ_from_unfiltered"] = int((svit[ran] != vit_all[ran]).sum())
        if k != "msv_staged0":
            hits = has & (vit_all.astype(np.int64) >= floors[fl][None, :].astype(np.int64))
            res[k + "_hits"], res[k + "_hits_lost"] = int(hits.sum()), int((hits & ~ran).sum())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(len(db)))
        diff += int(vf[r, p]) != W.vit16(R.parse_hmm(texts[p])[0]["tables"], recs[r])
    res["vf_check_pairs"], res["vf_check_differences"] = a.check, diff
    for p in [d_vf, d_vit, d_msv] + list(d_fl.values()):
        ctx.free(p)


def trace_part(a, ctx, db, texts, recs, ptrs, d_best_rec, scores, cells, res, rng, dump):
    import pyref_hmm as R
    import pyref_hmm_trace as T
    n_prof = len(db)

    def run(d_pr, pp, max_dom):
        n = len(pp)
        bufs = [ctx.alloc(max(4 * n, 16)) for _ in range(3)] + [ctx.alloc(max(4 * n * max_dom * 8, 16))]
        ctx.upload(bufs[0], pp)
        best = float("inf")
        for it in range(a.repeat + 1):
            ctx.sync()
            t = time.perf_counter()
            db.trace_dev(ptrs[0], ptrs[1], ptrs[2], a.n, d_pr, bufs[0], n, max_dom, bufs[1], bufs[2], bufs[3])
            ctx.sync()
            if it:
                best = min(best, time.perf_counter() - t)
        out = ctx.download(bufs[1], (n,), np.int32), ctx.download(bufs[2], (n,), np.uint32), ctx.download(bufs[3], (n, max_dom, 8), np.int32)
        for b in bufs:
            ctx.free(b)
        return best, out

    hit = ctx.download(d_best_rec, (n_prof,), np.uint32)
    res["trace_best_s"], (raw, nd, dom) = run(d_best_rec, np.arange(n_prof, dtype=np.uint32), 8)
    dump.update(trace_best_raw=raw, trace_best_n_dom=nd, trace_best_dom=dom)
    on = hit != R.NO_HIT
    res["trace_best_pairs"] = int(on.sum())
    res["trace_best_raw_differences"] = int((raw[on] != scores[hit[on], np.flatnonzero(on)]).sum()) + int((raw[~on] != R.NO_SCORE).sum())
    res["trace_best_domains"] = int(nd.sum())
    pr = np.repeat(np.arange(a.n, dtype=np.uint32), n_prof)
    d_pr = ctx.alloc(pr.nbytes)
    ctx.upload(d_pr, pr)
    res["trace_all_s"], (raw, nd, dom) = run(d_pr, np.tile(np.arange(n_prof, dtype=np.uint32), a.n), 2)
    ctx.free(d_pr)
    dump.update(trace_all_raw=raw, trace_all_n_dom=nd, trace_all_dom=dom)
    res["trace_all_pairs"] = len(pr)
    res["trace_all_cells_per_s"] = cells / res["trace_all_s"]
    res["trace_all_over_viterbi"] = res["trace_all_s"] / res["search_s"]
    res["trace_all_raw_differences"] = int((raw.reshape(a.n, n_prof) != scores).sum())
    res["trace_all_domains"] = int(nd.sum())
    diff = 0
    for _ in range(a.check):
        r, p = int(rng.integers(a.n)), int(rng.integers(n_prof))
        want = T.trace_pairs([R.parse_hmm(texts[p])[0]], recs, [r], [0], 2)
        j = r * n_prof + p
        diff += int(not (raw[j] == want[0][0] and nd[j] == want[1][0] and np.array_equal(dom[j], want[2][0])))
    res["trace_check_pairs"], res["trace_check_differences"] = a.check, diff


if __name__ == "__main__":
    main()
