"""Inputs of the gene tests (SPEC 15): the planted genomes of the method test, the constructed ORFs and tables of the scoring cases and the small
genomes of the pipeline cases. Every case's name promises a property; test_gene_cpu.py checks each against the restatement (tests/pyref_gene.py), so the
GPU tests that run the same table cannot pass on inputs that miss their edge. Bases are codes A C G T = 0 1 2 3."""
import numpy as np

import pyref_gene as R
import pyref_orf as RO

STOPS = (48, 50, 56)                       # TAA TAG TGA
STARTS = (R.ATG, R.GTG, R.TTG)
SENSE = [c for c in range(64) if c not in STOPS]
PLAIN = [c for c in SENSE if c not in STARTS]          # sense codons that are no start


def bases(codons):
    out = []
    for c in codons:
        out += [c >> 4, (c >> 2) & 3, c & 3]
    return np.array(out, np.uint8)


def revcomp(b):
    return (3 - np.asarray(b, np.uint8))[::-1].copy()


# ---- the planted genomes of the method test ------------------------------------------------------------------------------------------------------
def planted_genome(seed, size):
    """uniform random bases with genes planted from base 500 on: ATG, 58 to 598 codons drawn from a gamma(0.5) codon usage over the 61 sense codons, a
    random stop; random strand; gaps uniform in 20..399 -> (code array, [(begin, end, strand)] with the stop codon inside)"""
    rng = np.random.default_rng(seed)
    w = rng.gamma(0.5, size=61)
    w /= w.sum()
    g = rng.integers(0, 4, size).astype(np.uint8)
    genes, pos = [], 500
    while True:
        n = int(rng.integers(58, 599))
        cod = [R.ATG] + [SENSE[i] for i in rng.choice(61, n, p=w)] + [STOPS[int(rng.integers(0, 3))]]
        strand = int(rng.integers(0, 2))
        gap = int(rng.integers(20, 400))
        b = bases(cod)
        if pos + len(b) + 400 > size:
            break
        g[pos:pos + len(b)] = revcomp(b) if strand else b
        genes.append((pos, pos + len(b), strand))
        pos += len(b) + gap
    return g, genes


def accuracy(planted, called):
    """planted: (begin, end, strand); called: gene rows -> (fraction of planted with the 3' end right, with both ends right, fraction of calls that match
    no planted 3' end)"""
    def end3(b, e, s):
        return (s, b if s else e)
    want = {end3(*t): t for t in planted}
    got = [(int(c["begin"]), int(c["end"]), int(c["flags"]) & 1) for c in called]
    hit3 = {end3(*t) for t in got} & set(want)
    both = sum(1 for t in got if want.get(end3(*t)) == t)
    false = sum(1 for t in got if end3(*t) not in want)
    return len(hit3) / max(len(planted), 1), both / max(len(planted), 1), false / max(len(got), 1)


# ---- scoring cases: constructed ORFs and tables for gs_gene_score* ------------------------------------------------------------------------------------
def _rand_table(rng, lo=-700, hi=700):
    return rng.integers(lo, hi + 1, 4096).astype(np.int32)


def _orf_record(codons, strand, stop_before=True, stop_after=True, lead=0, tail=0, rng=None):
    """a record that holds the ORF `codons` (reading direction) on `strand`: [lead] [stop] codons [stop] [tail] in reading direction -> (record, orf tuple
    (begin, n, strand) in forward coordinates)"""
    rng = rng or np.random.default_rng(0)
    pre = list(rng.integers(0, 4, lead)) + ([3, 0, 0] if stop_before else [])
    post = ([3, 0, 0] if stop_after else []) + list(rng.integers(0, 4, tail))
    body = bases(codons)
    rec = np.concatenate([np.array(pre, np.uint8), body, np.array(post, np.uint8)]).astype(np.uint8)
    begin = len(pre)
    if strand:
        rec = revcomp(rec)
        begin = len(post)
    return rec, (begin, len(codons), strand)


def _plain(rng, n):
    return [PLAIN[i] for i in rng.integers(0, len(PLAIN), n)]


def scoring_cases():
    """-> list of dicts: name, records, starts (base offset of every record in the packed buffer), goff, tables, orfs [(rec, begin, n, strand)], min_aa,
    min_score, check(best_j, score, flags) -> bool (the property of the name, evaluated on the restatement's result)"""
    rng = np.random.default_rng(2026)
    cases = []

    def add(name, recs_orfs, tables, check, min_aa=30, min_score=5120, starts=None, goff=None):
        records = [r for r, _ in recs_orfs]
        orfs = [(i, o[0], o[1], o[2]) for i, (_, o) in enumerate(recs_orfs)]
        if starts is None:
            starts, at = [], 0
            for r in records:
                starts.append(at)
                at += (len(r) + 3) // 4 * 4
        cases.append(dict(name=name, records=records, starts=starts, goff=goff or [0, len(records)], tables=np.atleast_2d(tables), orfs=orfs, min_aa=min_aa,
                          min_score=min_score, check=check))

    # lengths: one lane run, lane-run edges, trip edges, several trips; random starts inside, both strands
    ro = []
    for n in (30, 63, 64, 65, 128, 129, 255, 256, 257, 5000):
        for strand in (0, 1):
            cod = _plain(rng, n)
            for j in rng.integers(0, n, max(2, n // 40)):
                cod[int(j)] = STARTS[int(rng.integers(0, 3))]
            ro.append(_orf_record(cod, strand, lead=int(rng.integers(0, 7)), tail=int(rng.integers(0, 7)), rng=rng))
    add("lengths_30_to_5000_both_strands", ro, _rand_table(rng), lambda j, s, f: len(set(f & 1)) == 2 and (f & R.F_HAS_START).any())

    zero, plus = np.zeros(4096, np.int32), np.full(4096, 1024, np.int32)
    # two ATGs with the same score: the smaller j
    cod = _plain(rng, 100); cod[10] = cod[40] = R.ATG
    add("tie_two_atg_equal_score", [_orf_record(cod, 0), _orf_record(cod, 1)], zero, lambda j, s, f: list(j) == [10, 10] and list(s) == [0, 0], min_score=0)
    # GTG two codons upstream of an ATG under +1 bit a dicodon: 2048 more in T, 2048 less in bonus
    cod = _plain(rng, 100); cod[20] = R.GTG; cod[22] = R.ATG
    add("tie_after_bonus_gtg_vs_atg", [_orf_record(cod, 0), _orf_record(cod, 1)], plus,
        lambda j, s, f: list(j) == [20, 20] and list(s) == [1024 * 77, 1024 * 77] and all((f >> 1) & 3 == 1))
    # every start type, and the record's edge
    ro = []
    for st in STARTS:
        cod = _plain(rng, 80); cod[5] = st
        ro += [_orf_record(cod, 0), _orf_record(cod, 1)]
    cod = _plain(rng, 80)
    ro += [_orf_record(cod, 0, stop_before=False), _orf_record(cod, 1, stop_before=False)]          # no stop precedes: edge start at j = 0
    cod = [R.ATG] + _plain(rng, 79)
    ro += [_orf_record(cod, 0, stop_before=False)]                                                   # an ATG at the edge is an ATG start
    add("start_types_atg_gtg_ttg_edge", ro, _rand_table(rng),
        lambda j, s, f: [int(x) for x in (f >> 1) & 3] == [0, 0, 1, 1, 2, 2, 3, 3, 0] and list(j[6:]) == [0, 0, 0] and all(f[6:] & R.F_OPEN5), min_score=-10 ** 6)
    # a start whose tail is min_aa - 1 codons is none; one codon more is one
    c1 = _plain(rng, 60); c1[60 - 29] = R.ATG
    c2 = _plain(rng, 60); c2[60 - 30] = R.ATG
    add("tail_min_aa_minus_one", [_orf_record(c1, 0), _orf_record(c2, 0), _orf_record(c1, 1), _orf_record(c2, 1)], plus,
        lambda j, s, f: [int(x) for x in j] == [R.NO_START, 30, R.NO_START, 30] and list(f & R.F_HAS_START) == [0, 16, 0, 16])
    add("no_start", [_orf_record(_plain(rng, 90), s) for s in (0, 1)], _rand_table(rng), lambda j, s, f: all(j == R.NO_START) and not (f & R.F_CANDIDATE).any())
    # open ends; records shorter than 90 bases
    cod = _plain(rng, 25)
    ro = [_orf_record(cod, s, stop_before=sb, stop_after=sa) for s in (0, 1) for sb in (False, True) for sa in (False, True)]
    add("open_ends_short_records", ro, _rand_table(rng),
        lambda j, s, f, ro=ro: all(len(r) < 90 for r, _ in ro) and [int(bool(x & R.F_OPEN5)) for x in f] == [1, 1, 0, 0] * 2 and
        [int(bool(x & R.F_OPEN3)) for x in f] == [1, 0, 1, 0] * 2, min_aa=10, min_score=-10 ** 6)
    # record starts at every residue mod 32 (bases of the packed buffer)
    ro, starts, at = [], [], 0
    for k in range(32):
        cod = _plain(rng, 40 + k); cod[3 + k % 5] = STARTS[k % 3]
        ro.append(_orf_record(cod, k & 1, lead=k % 4, tail=(k * 7) % 5, rng=rng))
        at = (at + 31) // 32 * 32 + k
        starts.append(at)
        at += len(ro[-1][0])
    add("record_starts_mod_32", ro, _rand_table(rng), lambda j, s, f, starts=starts: sorted(x % 32 for x in starts) == list(range(32)) and all(f & R.F_HAS_START), starts=starts)
    # min_score falls exactly on a score, and one above it
    cod = _plain(rng, 50); cod[4] = R.ATG
    add("min_score_exactly_met", [_orf_record(cod, 0)], plus, lambda j, s, f: list(s) == [45 * 1024] and all(f & R.F_CANDIDATE), min_score=45 * 1024)
    add("min_score_one_above", [_orf_record(cod, 0)], plus, lambda j, s, f: list(s) == [45 * 1024] and not (f & R.F_CANDIDATE).any(), min_score=45 * 1024 + 1)
    # two genomes with their own tables: the same ORF scores differently
    cod = _plain(rng, 70); cod[2] = R.ATG
    add("two_genomes_two_tables", [_orf_record(cod, 0), _orf_record(cod, 0)], np.stack([plus, -plus]), lambda j, s, f: int(s[0]) == -int(s[1]) == 67 * 1024,
        goff=[0, 1, 2], min_score=-10 ** 6)
    return cases


def packed(case):
    """-> (seq, rec_start, rec_len) of a case: its records at their base offsets"""
    seq = RO.pack_at(case["records"], case["starts"])
    return seq, np.array(case["starts"], np.uint64), np.array([len(r) for r in case["records"]], np.uint64)


# ---- pipeline cases: small genomes for gs_gene_call* ---------------------------------------------------------------------------------------------------
SMALL = dict(train_min_aa=80, min_train_codons=2000)          # parameters under which a 30 kb planted genome trains


def codon_usage(seed):
    """the codon usage planted_genome(seed, ...) draws its genes from: weights over SENSE"""
    w = np.random.default_rng(seed).gamma(0.5, size=61)
    return w / w.sum()


def _tie_gene(rng, usage, half=20):
    """TAA TTA G TAA TTA with G = X + revcomp(X) starting with ATG: it reads the same on both strands, so the forward ORF (TTA G, then the stop TAA) and the
    reverse ORF hold the same codons and their genes [b, e + 3) and [b - 3, e) the same score"""
    ok = [c for c in PLAIN if c not in (60, 28, 52, 19, 17, 16)]  # TTA CTA TCA, CAT CAC CAA: their reverse complements are stops and starts
    # codons that the genome uses often and whose reverse complements it uses often too, so that the gene scores above zero on both strands
    w = dict(zip(SENSE, usage))
    ok = sorted(ok, key=lambda c: -min(w[c], w[int(RO.rev_codon([c >> 4, (c >> 2) & 3, c & 3], 0))]))[:5]
    x = bases([R.ATG] + [ok[i] for i in rng.integers(0, len(ok), half - 1)])
    return np.concatenate([bases([48, 60]), x, revcomp(x), bases([48, 60])])


def _check_many(res, rec):
    """more than 64 and more than 4096 candidates in records 2 and 1; in record 1 a pair that overlaps by exactly max_overlap = 20 bases and one by 21"""
    c = res["cands"][1]
    ends = {e for _, e, _ in c}
    return len(c) > 4096 and 64 < len(res["cands"][2]) < 4096 and any(b + 20 in ends for b, _, _ in c) and any(b + 21 in ends for b, _, _ in c)


def _check_ties(res, rec):
    """record 1: the largest f is reached twice; record 2: some candidate's P_k is reached by two candidates below k"""
    v1, v2 = {}, {}
    R.select(res["cands"][1], 20, v1)
    R.select(res["cands"][2], 20, v2)
    end_tie = v1["f"].count(max(v1["f"])) == 2
    pred_tie = any(k and max(v2["f"][:k]) > 0 and v2["f"][:k].count(max(v2["f"][:k])) >= 2 for k in v2["k"])
    return end_tie and pred_tie


def _edge_tail(rng, usage, n=20):
    """TTA TAA ATG and n codons to the record's high edge: forward a 3'-open gene from the ATG, reverse a 5'-open ORF from the edge down to the TAA that TTA
    is on that strand, without a start codon inside - both genes end at the record's length"""
    ok = [c for c in PLAIN if c not in (60, 28, 52, 19, 17, 16)]  # as in _tie_gene: no stop and no start on the reverse strand, codons used often on both
    w = dict(zip(SENSE, usage))
    ok = sorted(ok, key=lambda c: -min(w[c], w[int(RO.rev_codon([c >> 4, (c >> 2) & 3, c & 3], 0))]))[:5]
    return bases([60, 48, R.ATG] + [ok[i] for i in rng.integers(0, len(ok), n)])


def _check_edge(res, rec):
    """records 0 and 2 are 192 k bases long and a forward and a reverse candidate end at exactly that length (a sort key part of the NEXT record's lowest
    and one more); record 1, behind the first, has no candidate and record 3, behind the other, has some; the edge genes are not all passed over"""
    at_edge = [[c for c in res["cands"][r] if c[1] == len(rec[r])] for r in (0, 2)]
    chosen = sum(1 for g in res["gene"] if int(g["rec"]) in (0, 2) and int(g["end"]) == len(rec[int(g["rec"])]))
    return (all(len(rec[r]) % 192 == 0 for r in (0, 2)) and all(len(a) == 2 for a in at_edge) and not res["cands"][1] and len(res["cands"][3]) > 64 and
            chosen >= 1)


def pipeline_cases():
    """-> list of dicts: name, records, goff, params, check(result of the restatement, records) -> bool"""
    cases = []
    g7, _ = planted_genome(7, 30000)
    g11, _ = planted_genome(11, 30000)
    rng = np.random.default_rng(99)

    def counts(res, r):
        return int(res["rec_gene_off"][r + 1]) - int(res["rec_gene_off"][r])

    cases.append(dict(name="one_genome_rounds_1", records=[g7], goff=[0, 1], params=dict(SMALL, rounds=1), check=lambda res, rec: len(res["gene"]) > 20))
    cases.append(dict(name="one_genome_rounds_2", records=[g7], goff=[0, 1], params=dict(SMALL, rounds=2), check=lambda res, rec: len(res["gene"]) > 20))
    # a record without a candidate between two that have some; a record shorter than one codon
    cases.append(dict(name="record_with_no_candidate", records=[g7[:15000], rng.integers(0, 4, 50).astype(np.uint8), np.zeros(2, np.uint8), g7[15000:]], goff=[0, 4],
                      params=dict(SMALL), check=lambda res, rec: counts(res, 0) > 0 and counts(res, 1) == 0 and counts(res, 2) == 0 and counts(res, 3) > 0))
    # two genomes whose tables differ, one call
    cases.append(dict(name="two_genomes_tables_differ", records=[g7, g11], goff=[0, 1, 2], params=dict(SMALL),
                      check=lambda res, rec: (res["tables"][0] != res["tables"][1]).any() and counts(res, 0) > 20 and counts(res, 1) > 20))
    # 300 small records over 3 genomes, the middle one too small to train
    recs = [g7[i:i + 250] for i in range(0, 30000, 250)] + [g11[i:i + 100] for i in range(0, 6000, 100)] + [g11[i:i + 250] for i in range(0, 30000, 250)]
    cases.append(dict(name="300_records_3_genomes_one_untrained", records=recs, goff=[0, 120, 180, 300], params=dict(SMALL, train_min_aa=60, min_train_codons=1000),
                      check=lambda res, rec: len(rec) == 300 and [int(x) for x in res["info"][:, 1]] == [1, 0, 1] and
                      int(res["rec_gene_off"][180]) == int(res["rec_gene_off"][120]) and len(res["gene"]) > 10))
    # every ORF with a start is a candidate: more than 64 and more than 4096 candidates in one record; pairs that overlap by exactly max_overlap and by one more
    big = rng.integers(0, 4, 150000).astype(np.uint8)
    cases.append(dict(name="record_with_over_4096_candidates", records=[g7, big, g11[:9000]], goff=[0, 3],
                      params=dict(SMALL, min_aa=10, max_overlap=20, min_score=-10 ** 6), check=_check_many))
    # the same score on both strands: equal f at the chain's end (record 1) and at a predecessor (record 2)
    tg = _tie_gene(rng, codon_usage(7))
    quiet = np.zeros(40, np.uint8)                                # poly-A: no start codon, no candidate
    h = g7[500:3000]
    cases.append(dict(name="equal_f_at_end_and_at_predecessor", records=[g7, np.concatenate([quiet, tg, quiet]), np.concatenate([quiet, tg, quiet, h])], goff=[0, 3],
                      params=dict(SMALL, min_aa=10, max_overlap=20, min_score=-10 ** 6), check=_check_ties))
    # records of 192 k bases (whole tiles) with a forward and a reverse candidate that end at the high edge, in front of a record without a candidate and of
    # one with candidates: the keys of such genes are the next record's lowest key part and one more
    t1, t2 = _edge_tail(rng, codon_usage(7)), _edge_tail(rng, codon_usage(7))
    a1 = np.concatenate([g7[:192 * 78 - len(t1)], t1])
    a2 = np.concatenate([g7[15000:15000 + 192 * 40 - len(t2)], t2])
    cases.append(dict(name="genes_end_at_the_edge_of_whole_tile_records", records=[a1, quiet[:20], a2, g7[15000:]], goff=[0, 4],     # (20 bases: too short for an ORF of min_aa)
                      params=dict(SMALL, min_aa=10, max_overlap=20, min_score=-10 ** 6), check=_check_edge))
    return cases


def training_input():
    """two genomes over four records and the intervals of a training call: their ORFs of 80 codons and more, then intervals of no, one and two codons and
    overlapping whole-record ones -> (records, genome_rec_off, [(rec, begin, n, strand)])"""
    g7, g11 = planted_genome(7, 30000)[0], planted_genome(11, 12000)[0]
    records = [g7[:20000], g7[20000:], np.zeros(4, np.uint8), g11]
    iv = []
    for r, b in enumerate(records):
        iv += [(r, begin, n, s) for begin, n, s in RO.orfs_scan(b, 80)[0]]
    iv += [(3, 0, 0, 0), (3, 5, 1, 1), (3, 7, 2, 1), (3, 0, 4000, 0), (3, 0, 4000, 1), (3, 1, 3999, 0)]          # no codon, one, two; overlapping, whole-record intervals
    return records, [0, 3, 4], iv


_PIPELINE_RESULTS = {}


def pipeline_result(case):
    """the restatement's result of a pipeline case, computed once (the CPU and the GPU tests share it)"""
    if case["name"] not in _PIPELINE_RESULTS:
        _PIPELINE_RESULTS[case["name"]] = R.call(case["records"], case["goff"], **case["params"])
    return _PIPELINE_RESULTS[case["name"]]
