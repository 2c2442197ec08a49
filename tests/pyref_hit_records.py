"""numpy restatement of SPEC 13.8 (best hits become sketcher records), written from the SPEC text and sharing no code with the library: a loop over the
matrix in (genome, profile) order. `Refused` carries the code and, for the capacity refusal alone, the true counts."""
import numpy as np

NO_HIT = 0xFFFFFFFF
GS_ERR_INVALID, GS_ERR_UNSUPPORTED = -1, -3


class Refused(Exception):
    def __init__(self, code, counts=None):
        super().__init__("refused with %d" % code)
        self.code, self.counts = code, counts


def hit_records(best_rec, aa, rec_start, rec_len, n_item=None, item=None, cap_rec=None, cap_aa=None):
    """best_rec [n_genomes, n_prof]; item [n_genomes * n_prof, max_item, words] with i_from in word 0 and i_to in word 1 of a slot (1-based, inclusive)
    -> (uint8 residues, uint64 start, uint64 len, uint64 genome_off [n_genomes + 1])"""
    best_rec = np.asarray(best_rec, dtype=np.uint32)
    ng, npf = best_rec.shape
    n_rec = len(rec_start)
    if (n_item is None) != (item is None):
        raise Refused(GS_ERR_INVALID)
    if item is not None:
        item = np.asarray(item)
        if item.shape[1] < 1 or item.shape[2] < 2:
            raise Refused(GS_ERR_INVALID)
    pieces, goff = [], [0]
    for g in range(ng):
        for p in range(npf):
            r, h = int(best_rec[g, p]), g * npf + p
            if r == NO_HIT:
                continue
            if r >= n_rec:
                raise Refused(GS_ERR_INVALID)
            L = int(rec_len[r])
            a, b = 0, L
            if item is not None and int(n_item[h]) >= 1:
                k = int(n_item[h])
                if k > item.shape[1]:
                    raise Refused(GS_ERR_INVALID)
                i_from, i_to = int(item[h, 0, 0]), int(item[h, k - 1, 1])
                if i_from < 1 or i_to > L or i_to < i_from - 1:
                    raise Refused(GS_ERR_INVALID)
                a, b = i_from - 1, i_to
            pieces.append((int(rec_start[r]) + a, b - a))
        goff.append(len(pieces))
    lens = np.array([n for _, n in pieces], np.uint64)
    counts = (len(pieces), int(lens.sum()))
    if (cap_rec is not None and counts[0] > cap_rec) or (cap_aa is not None and counts[1] > cap_aa):
        raise Refused(GS_ERR_INVALID, counts)
    start = np.zeros(len(pieces), np.uint64)
    start[1:] = np.cumsum(lens)[:-1]
    aa = np.asarray(aa, dtype=np.uint8)
    out = np.concatenate([aa[s:s + n] for s, n in pieces]) if pieces else np.zeros(0, np.uint8)
    return out.astype(np.uint8), start, lens, np.array(goff, np.uint64)
