"""Constructed inputs of the hit-record step (SPEC 13.8) for tests/test_hit_records_cpu.py and tests/test_gpu_hit_records.py. A case is a dict: name,
best_rec [n_genomes, n_prof], aa, rec_start, rec_len and - with spans - n_item, item [pairs, max_item, words]. Records lie in `aa` with gaps of the byte
GAP between them, so a copy that reads outside a record shows. Seeded; no library call."""
import numpy as np

NO_HIT = 0xFFFFFFFF
GAP = ord("x")
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
EDGE_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 4097)
WIDTHS = {"dom": 8, "env": 4, "ali": 8}          # GS_HMM_DOM_WORDS, GS_HMM_ENV_WORDS, GS_HMM_ALI_WORDS


def records_at(rng, lengths, offsets_mod8=None):
    """records of the given lengths; record i starts at an offset = offsets_mod8[i] (mod 8), or wherever a random gap of 0..11 bytes leaves it"""
    parts, starts, at = [], [], 0
    for i, n in enumerate(lengths):
        gap = int(rng.integers(0, 12)) if offsets_mod8 is None else (int(offsets_mod8[i]) - at) % 8
        parts.append(np.full(gap, GAP, np.uint8))
        at += gap
        starts.append(at)
        parts.append(AA[rng.integers(0, 20, n)])
        at += n
    parts.append(np.full(8, GAP, np.uint8))
    return np.concatenate(parts), np.array(starts, np.uint64), np.array(lengths, np.uint64)


def _case(name, best_rec, aa, rs, rl, n_item=None, item=None):
    return {"name": name, "best_rec": np.ascontiguousarray(best_rec, dtype=np.uint32), "aa": aa, "rec_start": rs, "rec_len": rl, "n_item": n_item, "item": item}


def random_matrix(rng, ng, npf, n_rec, p_hit=0.6):
    rec = rng.integers(0, n_rec, (ng, npf)).astype(np.uint32)
    rec[rng.random((ng, npf)) >= p_hit] = NO_HIT
    return rec


def random_spans(rng, best_rec, rl, max_item, words):
    """per pair 0 .. max_item items in sequence order inside the record; the words behind i_from and i_to hold noise that must not be read as coordinates"""
    flat = best_rec.reshape(-1)
    n_item = np.zeros(len(flat), np.uint32)
    item = rng.integers(-5, 5, (len(flat), max_item, words)).astype(np.int32)
    for h, r in enumerate(flat):
        if r == NO_HIT:
            n_item[h] = int(rng.integers(0, max_item + 3))          # the items of a pair that is no hit are not read, their number neither
            continue
        L = int(rl[r])
        k = int(rng.integers(0, max_item + 1))
        cuts = np.sort(rng.integers(1, L + 1, 2 * k))
        n_item[h] = k
        for e in range(k):
            item[h, e, 0], item[h, e, 1] = cuts[2 * e], cuts[2 * e + 1]
    return n_item, item


def shape_cases():
    """every (n_genomes, n_prof) of {1, 3, 70} x {1, 2, 120, 130}: random hits over 40 records of 1 .. 300 residues"""
    rng = np.random.default_rng(1381)
    out = []
    for ng in (1, 3, 70):
        for npf in (1, 2, 120, 130):
            aa, rs, rl = records_at(rng, rng.integers(1, 301, 40))
            out.append(_case("shape %dx%d" % (ng, npf), random_matrix(rng, ng, npf, 40), aa, rs, rl))
    return out


def layout_cases():
    rng = np.random.default_rng(1382)
    aa, rs, rl = records_at(rng, rng.integers(1, 200, 12))
    out = [_case("all NO_HIT", np.full((3, 5), NO_HIT), aa, rs, rl)]
    for where, g0 in (("first", 0), ("middle", 2), ("last", 4)):
        rec = random_matrix(rng, 5, 7, 12, 0.8)
        rec[:, 0] = 3                                                                     # every other genome has a hit
        rec[g0] = NO_HIT
        out.append(_case("empty genome %s" % where, rec, aa, rs, rl))
    rec = np.full((2, 4), NO_HIT)
    rec[0, 1] = rec[0, 3] = 5                                                            # one record, two profiles: it appears twice
    rec[1, 0] = rec[1, 1] = rec[1, 2] = 7
    out.append(_case("record chosen twice", rec, aa, rs, rl))
    out.append(_case("no records, no hits", np.full((2, 3), NO_HIT), np.full(8, GAP, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64)))
    return out


def _alignment_matrix(fill_len):
    """one genome whose hits are (filler, target) pairs: the filler's length brings the target to every destination offset mod 8 in turn; the targets are
    records 8 + 8 i + s = length i at source offset s. -> (n_prof, best_rec row builder)"""
    row = []
    at = 0
    for i in range(len(EDGE_LENGTHS)):
        for s in range(8):
            for d in range(8):
                f = (d - at) % 8 or 8                                                   # filler record f - 1 has f residues
                row += [f - 1, 8 + 8 * i + s]
                at += f + fill_len(i)
    return np.array(row, np.uint32)


def alignment_cases():
    """record lengths 1 .. 4097 at source and destination offsets of every residue mod 8 (whole records), and the same lengths as spans"""
    rng = np.random.default_rng(1383)
    lengths = list(range(1, 9)) + [n for n in EDGE_LENGTHS for _ in range(8)]
    offs = [int(v) for v in rng.integers(0, 8, 8)] + [s for _ in EDGE_LENGTHS for s in range(8)]
    aa, rs, rl = records_at(rng, lengths, offs)
    row = _alignment_matrix(lambda i: EDGE_LENGTHS[i])
    out = [_case("record lengths x offsets", row.reshape(8, -1), aa, rs, rl)]
    # spans: the records are 11 residues longer and the span [3, L + 2] has the edge length; the record starts 2 below the wanted source offset
    lengths = list(range(1, 9)) + [n + 11 for n in EDGE_LENGTHS for _ in range(8)]
    offs = [int(v) for v in rng.integers(0, 8, 8)] + [(s - 2) % 8 for _ in EDGE_LENGTHS for s in range(8)]
    aa, rs, rl = records_at(rng, lengths, offs)
    rec = row.reshape(8, -1)
    flat = rec.reshape(-1)
    for name, words in WIDTHS.items():
        n_item = np.zeros(len(flat), np.uint32)
        item = rng.integers(-9, 9, (len(flat), 3, words)).astype(np.int32)
        for h, r in enumerate(flat):
            if r >= 8:                                                                  # the span over two items: [3, ..] and [.., L - 9]
                L = int(rl[r])
                n_item[h] = 2
                item[h, 0, 0], item[h, 0, 1], item[h, 1, 0], item[h, 1, 1] = 3, 3, L - 9, L - 9
        out.append(_case("span lengths x offsets, %s slots" % name, rec, aa, rs, rl, n_item, item))
    return out


def span_cases():
    rng = np.random.default_rng(1384)
    out = []
    for name, words in WIDTHS.items():
        aa, rs, rl = records_at(rng, rng.integers(1, 120, 20))
        for max_item in (1, 3):
            rec = random_matrix(rng, 4, 9, 20, 0.8)
            n_item, item = random_spans(rng, rec, rl, max_item, words)
            flat = rec.reshape(-1)
            hits = np.flatnonzero(flat != NO_HIT)
            a, b, c = hits[:3]
            n_item[a] = 0                                                               # no item: the whole record
            n_item[b], item[b, 0, 0], item[b, 0, 1] = 1, 1, int(rl[flat[b]])            # one item, i_from = 1 and i_to = L
            n_item[c] = max_item                                                        # every slot used: first i_from = 1, last i_to = L
            cuts = np.sort(rng.integers(1, int(rl[flat[c]]) + 1, 2 * max_item))
            cuts[0], cuts[-1] = 1, int(rl[flat[c]])
            item[c, :, 0], item[c, :, 1] = cuts[0::2], cuts[1::2]
            out.append(_case("spans %s max_item %d" % (name, max_item), rec, aa, rs, rl, n_item, item))
    return out


def all_cases():
    return shape_cases() + layout_cases() + alignment_cases() + span_cases()


def error_cases():
    """(what, case, cap_rec, cap_aa): each refused with GS_ERR_INVALID; cap None = room for everything"""
    rng = np.random.default_rng(1385)
    aa, rs, rl = records_at(rng, rng.integers(5, 60, 10))
    good = random_matrix(rng, 3, 6, 10, 0.7)
    good[0, 0] = 2
    n_item, item = random_spans(rng, good, rl, 2, 4)
    out = []
    bad = good.copy()
    bad[1, 2] = 10                                                                      # = n_rec
    out.append(("bad record", _case("bad record", bad, aa, rs, rl), None, None))
    for what, w0, w1 in (("i_to past the record", 1, int(rl[2]) + 1), ("i_from 0", 0, 3), ("i_to below i_from - 1", 5, 3)):
        ni, it = n_item.copy(), item.copy()
        ni[0], it[0, 0, 0], it[0, 0, 1] = 1, w0, w1
        out.append((what, _case(what, good, aa, rs, rl, ni, it), None, None))
    ni = n_item.copy()
    ni[0] = 3                                                                           # max_item = 2
    out.append(("more items than slots", _case("more items than slots", good, aa, rs, rl, ni, item), None, None))
    n_hit = int((good != NO_HIT).sum())
    n_aa = int(rl[good[good != NO_HIT]].sum())
    out.append(("room for records", _case("room for records", good, aa, rs, rl), n_hit - 1, n_aa))
    out.append(("room for residues", _case("room for residues", good, aa, rs, rl), n_hit, n_aa - 1))
    return out
