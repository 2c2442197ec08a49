"""Numpy restatement of the split-database rules (SPEC 17 items 12-18), written from the text of SPEC, not from gsearch_amd/split.py or gs_split.hip:
the merge of a piece's answers into running lists, the random assignment, the medoid argmin, piece cutting, routing and the id offsets."""
import numpy as np

NOID = np.uint64(0xFFFFFFFFFFFFFFFF)
M64 = (1 << 64) - 1


def empty_lists(nq, knbn):
    """what gs_topk_reset_dev leaves"""
    return (np.full((nq, knbn), NOID, np.uint64), np.full((nq, knbn), np.inf, np.float32), np.zeros(nq, np.uint32), np.zeros(nq, np.uint64))


def merge_rows(run, answers, rows, id_offset):
    """run = (ids, dist, count, evals) of nq rows, answers = (ids, dist, count, evals) of the LISTED rows in list order (rows None: of every row),
    -> the new running lists (copies). Per listed row: the first count entries of both lists, the answers' ids plus id_offset, sorted by
    (distance bits, id) with the running entries first among equals; the first knbn of them, the tail UINT64_MAX / +inf."""
    ids, dist, cnt, ev = (np.array(a, copy=True) for a in run)
    a_ids, a_dist, a_cnt, a_ev = answers
    nq, knbn = ids.shape
    listed = range(nq) if rows is None else [int(r) for r in rows]
    for r, q in enumerate(listed):
        nr, na = min(int(cnt[q]), knbn), min(int(a_cnt[r]), knbn)
        entries = [(int(np.float32(dist[q, j]).view(np.uint32)), int(ids[q, j]), 0, j) for j in range(nr)]
        entries += [(int(np.float32(a_dist[r, j]).view(np.uint32)), (int(a_ids[r, j]) + int(id_offset)) & M64, 1, j) for j in range(na)]
        entries.sort(key=lambda e: (e[0], e[1], e[2]))             # full tie: the running entry first
        entries = entries[:knbn]
        ids[q], dist[q] = NOID, np.float32(np.inf)
        for j, e in enumerate(entries):
            ids[q, j] = np.uint64(e[1])
            dist[q, j] = np.uint32(e[0]).view(np.float32)
        cnt[q] = len(entries)
        ev[q] = (int(ev[q]) + int(a_ev[r])) & M64
    return ids, dist, cnt, ev


def key(seed, i):
    """SPEC 17 item 12: splitmix64's finaliser of seed * 0x9E3779B97F4A7C15 + (i + 1) * 0xBF58476D1CE4E5B9"""
    z = (seed * 0x9E3779B97F4A7C15 + (i + 1) * 0xBF58476D1CE4E5B9) % (1 << 64)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    return z ^ (z >> 31)


def order(n, seed):
    keys = [(key(seed, i), i) for i in range(n)]
    return [i for _, i in sorted(keys)]


def cut_sizes(n, parts):
    """sizes of a contiguous cut into `parts`: the first n mod parts hold one more"""
    return [n // parts + (1 if j < n % parts else 0) for j in range(parts)]


def random_assignment(n, pieces, seed):
    perm, out, at = order(n, seed), [], 0
    for size in cut_sizes(n, pieces):
        out.append(sorted(perm[at:at + size]))
        at += size
    return out


def medoid_argmin(count_matrix):
    """count_matrix[i, j] = mismatches of genome i against medoid j -> the position minimising (count, position)"""
    return np.argmin(np.asarray(count_matrix, np.int64), axis=1)       # the first of equal minima


def cut_pieces(assign, n_medoids, max_piece=None):
    out = []
    for j in range(n_medoids):
        members = [i for i in range(len(assign)) if assign[i] == j]
        if not members:
            continue
        parts = 1 if max_piece is None else (len(members) + max_piece - 1) // max_piece
        at = 0
        for size in cut_sizes(len(members), parts):
            out.append((j, members[at:at + size]))
            at += size
    return out


def routing(table, counts, piece_medoid):
    """per piece the ascending queries that have its medoid among their first counts[q] table entries"""
    return [[q for q in range(len(table)) if mp in [int(x) for x in table[q][:int(counts[q])]]] for mp in piece_medoid]


def offsets(lengths):
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += int(n)
    return out
