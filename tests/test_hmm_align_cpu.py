"""SPEC 13.6 on the CPU: the restatement tests/pyref_hmm_align.py (posteriors of an envelope from 13.5's Forward and Backward, the Q16 weights, the
max-plus program with allowed transitions only, the walk and its tie rules) against its twin - the same section cell by cell with an explicit arg-max
walk -, against the identities that hold on the integers, against the Viterbi path of the same segment, on the hand cases of SPEC 13.6, and against an f64
yardstick. No kernel runs; the library is asked for its constants, symbols and EXP2 only, so that without gs_hmm_align every test here fails.

The segments are the world of tests/test_hmm_null2_cpu.py (same recipe, same seeds: every envelope of every pair, the whole record where there is
none) plus the hand cases below. Against the yardstick only values are compared, never paths (ties may fall differently). Each bound is four times the
measurement rounded up to a power of two, and must not be more than 16 times the measurement:

    largest |oa / 65536 - f64| / Ld       0.00294 residues a row (79 segments)          asserted 2^-6 = 0.0156
    largest |w / 65536 - f64 posterior|   0.00397 over every column of every path       asserted 2^-5 = 0.0313

The f64 accuracy of the hand cases: consensus 0.994 (PF00380.20) and 0.987 (TIGR00964); `c[:30] + c[70:]` of PF00380.20 0.981."""
import numpy as np
import pytest

import gsearch_amd as G
import hmm_align_case as HC
import hmm_classes_case as K
import pyref_hmm as R
import pyref_hmm_align as A
import pyref_hmm_posterior as P
import pyref_hmm_trace as T
import test_hmm_null2_cpu as W2
import test_hmm_posterior_cpu as W

FIXTURES = W2.FIXTURES
OA_PER_ROW_BOUND, W_BOUND = 2.0 ** -6, 2.0 ** -5


@pytest.fixture(scope="module", autouse=True)
def the_library_has_the_feature():
    assert all(s in G.SYMBOLS for s in ("gs_hmm_align", "gs_hmm_align_dev", "gs_hmm_exp2_table"))
    assert all(hasattr(G.HmmDb, a) for a in ("align", "align_packed", "align_dev", "align_all"))
    assert (G._lib.HMM_ALI_WORDS, G._lib.HMM_ALI_MAX_LD, G._lib.HMM_EXP2_N) == (A.ALI_WORDS, A.ALI_MAX_LD, len(A.EXP2))


def test_exp2_table_and_weights():
    """no entry's unrounded value lies within 1e-6 of a half-integer, so libm and numpy cannot disagree on the table; the library's table is this one"""
    fr = A.exp2_unrounded()
    margin = float(np.abs(fr - np.floor(fr) - 0.5).min())
    print("EXP2: smallest distance of an unrounded entry from a half-integer %.6f" % margin)
    assert margin > 1e-6
    assert np.array_equal(G.hmm_exp2_table().astype(np.int64), A.EXP2) and A.EXP2[0] == 65536 and A.EXP2[1023] == 32790
    assert A.w(0) == 65536 and A.w(-1024) == 32768 and A.w(-16 * 1024) == 1 and A.w(-16 * 1024 - 1) == 0 and A.w(-17 * 1024) == 0 and A.w(R.NEG) == 0
    u = -np.arange(0, 17 * 1024)
    assert (np.diff(A.w(u)) <= 0).all() and np.abs(A.w(u) - 65536.0 * np.exp2(u / 1024.0)).max() <= 1.0


def hand_cases():
    """(profile name, what, table, record) of SPEC 13.6's hand cases, each record one envelope; seeded background"""
    rng = np.random.default_rng(1361)
    out = []
    for name in FIXTURES:
        tab = W2.model(name)["tables"]
        c = R.consensus(tab)
        out += [(name, "c", tab, c), (name, "bg c bg", tab, R.background(rng, 10) + c + R.background(rng, 10)),
                (name, "insert", tab, c[:20] + R.background(rng, 5) + c[20:])]
        if name == "PF00380.20.HMM":
            out.append((name, "delete", tab, c[:30] + c[70:]))
    return out


def test_hand_cases():
    want_acc = {("PF00380.20.HMM", "c"): 0.994, ("TIGR00964.HMM", "c"): 0.987, ("PF00380.20.HMM", "delete"): 0.981}
    for name, what, tab, rec in hand_cases():
        x, M = R.encode(rec), tab.shape[1] - 1
        slot, cols = A.segment(tab, x, len(x))
        acc_f64 = A.program_f64(tab, *A.posterior_f64(tab, x, len(x))) / len(x)
        print("%-15s %-8s %s %s accuracy %.4f (f64 %.4f)" % (name, what, slot[:4], A.cigar(cols), slot[4] / (65536.0 * len(x)), acc_f64))
        if what == "c":
            assert slot[:4] == (1, M, 1, M) and A.cigar(cols) == "%dM" % M
        elif what == "bg c bg":
            assert slot[:4] == (11, 10 + M, 1, M) and A.cigar(cols) == "%dM" % M
        elif what == "insert":
            assert slot[:4] == (1, M + 5, 1, M) and A.cigar(cols) == "20M5I%dM" % (M - 20)
        else:
            assert slot[:4] == (1, 81, 1, 121) and A.cigar(cols) == "30M40D51M"
            assert len(T.trace(tab, rec)[1]) == 2                                              # the Viterbi path of 13.2 is two domains: the two differ in kind
        if (name, what) in want_acc:
            assert abs(acc_f64 - want_acc[name, what]) < 0.0006 and abs(slot[4] / (65536.0 * len(x)) - acc_f64) < OA_PER_ROW_BOUND


def test_two_copies_in_one_segment_and_in_two():
    """c + c as ONE segment aligns one whole copy and leaves the other to pX (which copy: a tie within 0.002 of accuracy, not asserted); with 13.4's two
    envelopes each segment aligns (.., 1, M)"""
    for name in FIXTURES:
        tab = W2.model(name)["tables"]
        c, M = R.consensus(tab), tab.shape[1] - 1
        x = R.encode(c + c)
        slot, cols = A.segment(tab, x, len(x))
        assert slot[2:4] == (1, M) and slot[:2] in ((1, M), (M + 1, 2 * M)) and A.cigar(cols) == "%dM" % M and 0.49 < slot[4] / (65536.0 * 2 * M) < 0.5
        env = P.posterior(tab, c + c)["env"]
        assert [e[:2] for e in env] == [(1, M), (M + 1, 2 * M)]
        for a, b, _, _ in env:
            s, _ = A.segment(tab, x[a - 1:b], len(x), a)
            assert s[:4] == (a, b, 1, M)


def no_delete_model(M):
    """hmm_classes_case.deletion_model(M) with every m->d of the file `*` (its probability goes to m->m): a distinct consensus and no way into a D state"""
    s = K.deletion_model(M)
    for k in range(M + 1):
        s["tr"][k][0] += s["tr"][k][2]
        s["tr"][k][2] = 0.0
    return R.parse_hmm(R.write_hmm(s))[0]["tables"]


def test_the_mask_of_allowed_transitions():
    """m->d all `*`: c[:30] + c[70:] must align without a deletion. hmm_classes_case's own profile of that kind (w_only_model: W at every node) cannot show
    the difference - its consensus is one letter, every diagonal weighs the same and nothing is gained by deleting, so the program aligns 81 match
    cells with the mask or without it; the same record against a deletion-friendly profile with m->d starred does: with the mask dropped the program
    deletes across the gap (30M 40D 51M), with it the one domain is the longer copy"""
    tab = R.parse_hmm(R.write_hmm(K.w_only_model(121)))[0]["tables"]
    assert (tab[R.ROW_MD, :121] <= R.STAR).all()
    c = R.consensus(tab)
    x = R.encode(c[:30] + c[70:])
    slot, cols = A.program_rows(tab, *A.posterior(P._groups(tab), x, len(x)))
    assert slot[7] == 0 and slot[6] == 0 and A.steps_allowed(tab, cols)
    tab = no_delete_model(121)
    assert (tab[R.ROW_MD, :121] <= R.STAR).all()
    c = R.consensus(tab)
    x = R.encode(c[:30] + c[70:])
    post = A.posterior(P._groups(tab), x, len(x))
    slot, cols = A.program_rows(tab, *post)
    loose, loose_cols = A.program_rows(tab, *post, use_masks=False)
    print("m->d starred: with the mask %s %s, without %s %s" % (slot, A.cigar(cols), loose, A.cigar(loose_cols)))
    assert slot[7] == 0 and slot[:4] == (31, 81, 71, 121) and A.steps_allowed(tab, cols) and A.program_cells(tab, *post)[0] == slot
    assert loose[7] == 40 and A.cigar(loose_cols) == "30M40D51M" and not A.steps_allowed(tab, loose_cols) and loose[4] > slot[4]


def test_a_starred_link_under_a_deletion():
    """tests/hmm_align_case.py: `*` in transitions between valid nodes. With every m->d starred one end of the record is aligned; with d->d of node k
    starred the deletion steps out through M of node k + 1 and in again. Without the masks every case deletes straight across. Both integer definitions
    agree on them (the twin on the profiles of up to 512 nodes)"""
    texts, models, records = HC.build()
    for (kind, M, nodes), m, rec in zip(HC.CASES, models, records):
        tab, x = m["tables"], R.encode(rec)
        post = A.posterior(P._groups(tab), x[3:-2], len(x))
        slot, cols = A.program_rows(tab, *post, 4)
        loose, loose_cols = A.program_rows(tab, *post, 4, use_masks=False)
        print("%s %d %s (%s): %s, without the masks %s" % (kind, M, nodes, [HC.where(M, k) for k in nodes], A.cigar(cols), A.cigar(loose_cols)))
        assert A.steps_allowed(tab, cols) and not A.steps_allowed(tab, loose_cols) and loose[4] > slot[4]
        assert A.cigar(loose_cols) == ("30M40D51M" if M == 121 else "35M%dD35M" % (M - 70))
        if kind == "md":
            assert (tab[R.ROW_MD, :M] <= R.STAR).all() and slot[6] == slot[7] == 0
        else:
            k = nodes[0]
            assert tab[R.ROW_DD, k] <= R.STAR and (tab[R.ROW_DD, 1:k] > R.STAR).all() and slot[5:] == (70, 0, M - 70)
            assert "D1M" in A.cigar(cols) and((cols[:, 0] == 0) & (cols[:, 1] == k + 1)).any()
        if M <= 512:
            twin, twin_cols = A.program_cells(tab, *post, 4)
            assert twin == slot and np.array_equal(twin_cols, cols)


@pytest.fixture(scope="module")
def world():
    """the segments of test_hmm_null2_cpu.world (its recipe and seeds) and the hand cases, each with its posteriors, its alignment and the yardstick's"""
    rng = np.random.default_rng(1349)
    models = [W2.model(n) for n in FIXTURES]
    models += [R.parse_hmm(R.write_hmm(R.synth_model(rng, M)))[0] for M in W.SYN_M]
    pairs = []
    for m in models:
        tab, M = m["tables"], m["M"]
        c = R.consensus(tab)
        recs = [R.background(rng, 1), R.background(rng, 64), R.background(rng, 200), c, c + c, R.background(rng, 30) + c[:max(M // 2, 1)] + R.background(rng, 30)]
        if M > 100:
            recs.append(c[:30] + c[100:])
        pairs += [(tab, rec) for rec in recs]
    pairs += [(tab, rec) for tab, rec, _ in W.hand_cases()]
    for name, m in zip(FIXTURES, models[:2]):
        pairs += [(m["tables"], rec) for rec in W2.record_kinds(name, m["tables"]).values()]
    segs = []
    for tab, rec in pairs:
        x = R.encode(rec)
        env = P.posterior(tab, rec)["env"] or [(1, len(x), 0, 0)]
        segs += [(tab, rec, a, b) for a, b, _, _ in env]
    segs += [(tab, rec, 1, len(rec)) for _, _, tab, rec in hand_cases()]
    out = []
    for tab, rec, a, b in segs:
        x = R.encode(rec)
        g = P._groups(tab)
        post = A.posterior(g, x[a - 1:b], len(x))
        slot, cols = A.program_rows(tab, *post, a)
        out.append({"tab": tab, "rec": rec, "a": a, "b": b, "post": post, "slot": slot, "cols": cols})
    return out


def test_the_two_integer_definitions_agree(world):
    n = 0
    for s in world:
        if (s["b"] - s["a"] + 1) * s["tab"].shape[1] > 40000:                                  # the twin walks Python lists: the smaller segments
            continue
        slot, cols = A.program_cells(s["tab"], *s["post"], s["a"])
        assert slot == s["slot"] and np.array_equal(cols, s["cols"]), (s["a"], s["b"], slot, s["slot"])
        n += 1
    assert n >= 60


def test_identities_and_allowed_transitions(world):
    for s in world:
        i_from, i_to, k_from, k_to, oa, nm, ni, nd = s["slot"]
        cols, (pM, pI, pX) = s["cols"], s["post"]
        assert nm + ni == i_to - i_from + 1 and nm + nd == k_to - k_from + 1 and s["a"] <= i_from <= i_to <= s["b"] and len(cols) == nm + ni + nd
        assert tuple(cols[0, :3]) == (0, k_from, i_from) and tuple(cols[-1, :3]) == (0, k_to, i_to)
        assert oa == A.path_value(s["tab"], cols, pX, s["a"]) and 0 <= oa <= 65536 * (s["b"] - s["a"] + 1)
        assert A.steps_allowed(s["tab"], cols)
        assert (pM <= 0).all() and (pI <= 0).all() and (pX <= 0).all() and (pI[:, s["tab"].shape[1] - 2:] == R.NEG).all()      # I of node M and padding: NEG
        assert np.array_equal(A.column_words(cols)[:, 1], cols[:, 3]) and (A.column_words(cols)[:, 0] >> 28 == cols[:, 0]).all()


def test_at_least_the_viterbi_path(world):
    """optimality: where 13.2 gives the segment one domain, that path is a valid path of the program, so oa is at least its value under the same weights"""
    n = 0
    for s in world:
        x = bytes(s["rec"])[s["a"] - 1:s["b"]]
        doms = A.viterbi_columns(s["tab"], x)
        if len(doms) != 1:
            continue
        pM, pI, pX = s["post"]
        d = doms[0]
        p = np.where(d[:, 0] == 0, pM[d[:, 2], d[:, 1] - 1], np.where(d[:, 0] == 1, pI[d[:, 2], d[:, 1] - 1], 0))
        vcols = np.concatenate([d, p[:, None]], axis=1)
        assert A.steps_allowed(s["tab"], vcols) and s["slot"][4] >= A.path_value(s["tab"], vcols, pX, 1)
        n += 1
    assert n >= 30


def test_deviations_from_the_yardstick(world):
    oa_dev = w_dev = 0.0
    for s in world:
        x = R.encode(s["rec"])
        PM, PI, PX = A.posterior_f64(s["tab"], x[s["a"] - 1:s["b"]], len(x))
        Ld = s["b"] - s["a"] + 1
        oa_dev = max(oa_dev, abs(s["slot"][4] / 65536.0 - A.program_f64(s["tab"], PM, PI, PX)) / Ld)
        for st, k, i, p in s["cols"].tolist():
            if st != 2:
                w_dev = max(w_dev, abs(int(A.w(p)) / 65536.0 - (PM if st == 0 else PI)[i - s["a"] + 1, k]))
    print("segments %d; largest |oa / 65536 - f64| / Ld %.5f, largest |w / 65536 - f64 posterior| %.5f" % (len(world), oa_dev, w_dev))
    assert len(world) >= 70
    for got, bound in ((oa_dev, OA_PER_ROW_BOUND), (w_dev, W_BOUND)):
        assert bound / 16 < got <= bound, (got, bound)


def test_writer_and_pair_lists():
    models = [W2.model(n) for n in FIXTURES]
    c0, c1 = (R.consensus(m["tables"]) for m in models)
    seqs = [c0[:30] + c0[70:], c1 + c1, b"", c0[:10] + b"X" + c0[11:]]
    pr, pp = np.array([0, 1, 2, 3, R.NO_HIT], np.uint32), np.array([0, 1, 0, 0, 1], np.uint32)
    _, _, ne, env = P.envelope_pairs(models, seqs, pr, pp, 2)
    slots, cols = A.align_pairs(models, seqs, pr, pp, ne, env, 2)
    assert slots.shape == (5, 2, 8) and slots.dtype == np.int32 and [len(c) for c in cols] == [1, 2, 0, 0, 0] and not slots[2:].any()
    text = A.alignment_bytes(models, ["a", "b", "e", "x", "-"], seqs, list(zip(pr.tolist()[:2], pp.tolist()[:2])), ne, env, slots, cols)
    print(text.decode())
    lines = text.split(b"\n")
    assert lines[0] == A.ALIGN_HEADER[:-1] and lines[1] == b"==\ta\tRibosomal_S9\tPF00380.20\t1\t1\t1\t81\t1\t121\t121\t0.980\t81\t0\t40"
    model, match, target, pp_line = (ln[9:].decode() for ln in lines[2:6])
    assert [ln[:9] for ln in lines[2:6]] == [b"  model  ", b"  match  ", b"  target ", b"  PP     "]
    assert model == c0.decode().lower() and target == (c0[:30] + b"-" * 40 + c0[70:]).decode() and match == model[:30] + " " * 40 + model[70:]
    assert pp_line[30:70] == "." * 40 and set(pp_line[:30] + pp_line[70:]) <= set("0123456789*") and pp_line.count("*") > 60
    assert text.count(b"==\tb\tTIGR00964\tTIGR00964\t") == 2 and len(lines) == 1 + 3 * 5 + 1
