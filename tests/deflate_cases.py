"""The named DEFLATE streams that the device inflater (gs_inflate.hip) is held to zlib on: legal shapes that no installed compressor emits, the
scheduling edges of the pipelined form, the window edges of the LDS form, and the streams a decoder has to refuse. Built with deflate_writer;
test_deflate_cases_cpu.py checks on the CPU that every case has the edge its name promises, test_gpu_inflate_streams.py runs them on the device."""
import random
import zlib

from deflate_writer import Deflate, cl_compress, expand, flat_lens, gzip_member, lit, lits, match, raw_bits, raw_match, raw_sym, FTEXT

# gs_inflate.hpp
E_BTYPE, E_STORED, E_OVERSUB, E_CODE, E_DIST, E_OUTPUT, E_INPUT, E_REPEAT = 1, 2, 3, 4, 5, 6, 7, 8
REJECT_ISIZE = 65536            # trailer ISIZE of a reject case: the output cap is never the first error reached
BOUNDARIES = (16384, 32768, 49152, 65536)
PREFIX = bytes(random.Random(600).randrange(256) for _ in range(600))


class Case:
    def __init__(self, name, group, raw, accept, text=None, code=None, phrase=None, blocks=None, raw_valid=False, **meta):
        self.name, self.group, self.raw, self.accept, self.text = name, group, raw, accept, text
        self.code = code                    # INF_E_* of a reject case, None = any status but 0
        self.phrase = phrase                # what zlib's message has to contain
        self.blocks = blocks                # [("huff", tokens) | ("stored", bytes)]: what the stream was made of
        self.raw_valid = raw_valid          # reject case whose DEFLATE data is fine: the member's trailer is what is wrong
        self.meta = meta

    def member(self):
        """the gzip member that goes to the device"""
        if self.accept:
            return gzip_member(self.raw, self.text)
        if self.raw_valid:
            return gzip_member(self.raw, self.text, isize=len(self.text) - 1)
        return gzip_member(self.raw, crc=0, isize=REJECT_ISIZE)

    def out_cap(self):
        return len(self.text) if self.text is not None else REJECT_ISIZE


CASES = []


def add(name, group, raw, accept, **kw):
    assert all(c.name != name for c in CASES), name
    assert accept is True or accept is False
    CASES.append(Case(name, group, raw, accept, **kw))


class Build:
    """a stream and the record of what it was made of"""

    def __init__(self):
        self.d, self.blocks, self.bitpos = Deflate(), [], []

    def fixed(self, toks, last=False, **kw):
        self.d.fixed(toks, last, **kw); self.blocks.append(("huff", list(toks))); self.bitpos.append(self.d.w.bitpos())
        return self

    def dynamic(self, ll_, dl_, toks, last=False, **kw):
        self.d.dynamic(ll_, dl_, toks, last, **kw); self.blocks.append(("huff", list(toks))); self.bitpos.append(self.d.w.bitpos())
        return self

    def stored(self, data, last=False, **kw):
        self.d.stored(data, last, **kw); self.blocks.append(("stored", bytes(data))); self.bitpos.append(self.d.w.bitpos())
        return self

    def raw(self):
        return self.d.finish()


def layout(blocks):
    """(text, starts): starts[bi][ti] = text position in front of token ti of block bi (for a stored block: [its first position])"""
    text, starts = b"", []
    for kind, body in blocks:
        if kind == "stored":
            starts.append([len(text)])
            text += body
        else:
            text, s = expand(body, text)
            starts.append(s)
    return text, starts


def pipe_schedule(blocks, P=8):
    """The batching rule of k_inflate_pipe<P>, restated: which matches go into a batch (path "fast", with their slot) and which drain it first
    ("slow"). Per match: pos, len, dist, src0, `synced` when it was decided and `head`, the first destination of the batch in flight (None: nothing in
    flight). Per huffman block ("eob", bi): how many matches were in flight when the end-of-block code was met."""
    out, pos, synced = {}, 0, 0
    for bi, (kind, body) in enumerate(blocks):
        if kind == "stored":
            pos += len(body)
            continue
        ti, n, eob, nl, head = 0, len(body), False, 0, None
        while not eob:
            nq, first, slow = 0, None, None
            for j in range(P):
                while ti < n and body[ti][0] == "lit":
                    pos += 1; ti += 1
                if ti == n:
                    eob = True
                    out[("eob", bi)] = dict(inflight=nl, batch=nq)
                    break
                _, ln, d = body[ti][:3]
                rec = dict(pos=pos, len=ln, dist=d, src0=pos - d, synced=synced, slot=j, head=head)
                out[(bi, ti)] = rec
                ti += 1
                if ln <= 64 and pos - d + min(ln, d) <= synced:
                    rec["path"] = "fast"
                    first = pos if first is None else first
                    nq += 1; pos += ln
                else:
                    rec["path"] = "slow"; slow = ln
                    break
            nl, head = nq, first
            synced = first if nq else pos
            if slow or eob:
                pos += slow or 0
                synced, nl, head = pos, 0, None
    return out


def ll(used, n=None, lens=None):
    """code lengths of an alphabet in which exactly `used` have codes: a complete code with two neighbouring lengths, or `lens` in symbol order"""
    used = sorted(used)
    out = [0] * (n or max(257, used[-1] + 1))
    for s, L in zip(used, lens or flat_lens(len(used))):
        out[s] = L
    return out


def ladder(n):
    """1, 2, ..., n - 1, n - 1: the complete code with the longest codes n symbols can have"""
    return list(range(1, n)) + [n - 1]


def used_syms(toks):
    L, D = {256}, set()
    for t in toks:
        if t[0] == "lit":
            L.add(t[1])
        elif t[0] == "match":
            L.add(t[3][0]); D.add(t[4][0])
    return L, D


def auto_lens(toks, nlit=None, ndist=None):
    """complete codes over the symbols the tokens use; the distance alphabet always gets two codes at least, so that only the cases that are ABOUT a
    single distance code or none lean on that exception"""
    L, D = used_syms(toks)
    if len(L) == 1:
        L = L | {0}
    for s in (0, 1):
        if len(D) < 2:
            D = D | {s}
    return ll(L, nlit), ll(D, ndist or max(D) + 1)


def reach(toks, pos, target, dist=600):
    """tokens that take the text from pos to target: length-258 matches of the 600-byte prefix's period, then the rest"""
    assert target >= pos
    while target - pos >= 261:
        toks.append(match(258, dist)); pos += 258
    rem = target - pos
    if rem > 258:
        toks += [match(rem - 3, dist), match(3, dist)]
    elif rem >= 3:
        toks.append(match(rem, dist))
    else:
        toks += lits(b"xy"[:rem])
    return target


def one_block(name, group, toks, dynamic=True, **meta):
    b = Build()
    if dynamic:
        a, d = auto_lens(toks)
        b.dynamic(a, d, toks, True)
    else:
        b.fixed(toks, True)
    add(name, group, b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, **meta)


ACGT = b"ACGT"
ONLY_EOB = ([0] * 256 + [1], [0])

# ---- accept: tables ---------------------------------------------------------------------------------------------------------------------


def _tables():
    toks = lits(ACGT) + [match(8, 4), lit(65), match(5, 4), match(258, 4)]
    a, d = auto_lens(toks)[0], [0, 0, 0, 1]
    b = Build().dynamic(a, d, toks, True)
    add("single_dist_code", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, dist_lens=d)

    toks = lits(b"GATTACA" * 3)
    a, d = auto_lens(toks)[0], [0]
    b = Build().dynamic(a, d, toks, True)
    add("no_dist_code_literals_only", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, dist_lens=d)

    b = Build().dynamic(ONLY_EOB[0], ONLY_EOB[1], [], True)
    add("only_eob", "tables", b.raw(), True, text=b"", blocks=b.blocks, litlen_lens=ONLY_EOB[0], dist_lens=ONLY_EOB[1])

    # a 16 whose copies start in the literal/length lengths and end in the distance lengths (and a 16 right behind a 16)
    a = ll([65, 67, 71, 84, 256, 257, 258, 259, 260, 261, 262], 263, [3] * 5 + [4] * 6)
    d = [4] * 16
    cl = cl_compress(a[:258]) + [(16, 3), (16, 3), (16, 3), (16, 0)]
    toks = lits(ACGT * 4) + [lit(65), match(3, 4), match(4, 8), match(6, 16), match(8, 30), match(5, 1)]
    b = Build().dynamic(a, d, toks, True, cl_syms=cl)
    add("repeat16_across_hlit", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, hlit=263, cl_syms=cl, lens=a + d, rep=16)

    a = ll([65, 67, 71, 84, 256, 257], 286)
    d = [0, 0, 0, 0, 1, 1]
    cl = cl_compress(a[:258]) + [(18, 28 + 4 - 11), (1, 0), (1, 0)]
    toks = lits(ACGT * 2) + [match(3, 5), match(3, 8), match(3, 6)]
    b = Build().dynamic(a, d, toks, True, cl_syms=cl)
    add("repeat18_across_hlit", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, hlit=286, cl_syms=cl, lens=a + d, rep=18)

    # Block 2 opens with 18 (138 zeros: indices 0-137, the last ten written in the third trip of the lanes), then 16. The length a 16 copies behind a run of
    # zeros is zero (RFC 1951 3.2.7); block 1 left NONZERO lengths at 137 and behind it, so a decoder that reads the length in front of the 16 before
    # the run's stores have landed copies a stale 8 and builds other tables
    a1 = [8] * 254 + [9] * 4
    a2 = ll([200, 201, 202, 203, 256, 257])
    d2 = [1, 1]
    cl = [(18, 127), (16, 3)] + cl_compress(a2[144:]) + [(1, 0), (1, 0)]
    b = Build().dynamic(a1, [1, 1], lits(bytes(range(130, 150))), False)
    b.dynamic(a2, d2, lits([200, 201, 202, 203]) + [match(3, 2)], True, cl_syms=cl)
    add("repeat16_after_138_zeros", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, cl_syms=cl, lens=a2 + d2, before=a1)

    toks = lits(ACGT) + [match(258, 4), lit(65), match(258, 3)]
    a, d = auto_lens(toks, nlit=286)
    b = Build().dynamic(a, d, toks, True)
    add("hlit_286_uses_285", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, litlen_lens=a)

    toks = lits(PREFIX)
    reach(toks, 600, 24600)
    toks += [match(10, 24577), match(20, 24590), match(3, 24620)]
    a, d = auto_lens(toks, ndist=30)
    b = Build().dynamic(a, d, toks, True)
    add("hdist_30_uses_29", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, dist_lens=d)

    toks = lits(ACGT * 3)
    a, d = auto_lens(toks)
    cl = cl_compress(a + d)
    used = sorted({s for s, _ in cl} | {15})
    cll = [0] * 19
    for s, L in zip(used, flat_lens(len(used))):
        cll[s] = L
    b = Build().dynamic(a, d, toks, True, cl_syms=cl, cl_lens=cll)
    add("hclen_19", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, hclen=19)

    # HCLEN field 4: eight code-length code lengths (16 17 18 0 8 7 9 6). (A COUNT of four - 16 17 18 0 - can only spell zeros, which leaves no
    # end-of-block code: that is the reject case hclen_count_4.)
    a = [8] * 254 + [9] * 4
    cll = [0] * 19
    cll[8], cll[9], cll[0], cll[6] = 1, 2, 3, 3
    toks = lits(b"eight code length codes")
    b = Build().dynamic(a, [0], toks, True, cl_lens=cll)
    add("hclen_4", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, hclen=8)

    # lengths 1 .. 15, 15: every length from 11 to 15 is decoded, and 'x' / 'y' differ in their 15th bit only (one 10-bit root slot)
    syms = [65, 67, 71, 84, 10, 78, 97, 99, 103, 116, 110, 256, 257, 258, 120, 121]
    a = [0] * 259
    for s, L in zip(syms, ladder(16)):
        a[s] = L
    toks = lits(b"ACGT\nNacgtn") + [match(3, 2), match(4, 5), lit(120), lit(121), lit(65)]
    b = Build().dynamic(a, [0, 1, 0, 0, 1], toks, True)
    add("litlen_15_bit_codes", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, litlen_lens=a, share=(120, 121))

    d = ladder(16)
    toks = lits(PREFIX[:300]) + [match(5, x) for x in (17, 30, 40, 60, 80, 120, 190, 256, 1, 2)]
    a, _ = auto_lens(toks)
    b = Build().dynamic(a, d, toks, True)
    add("dist_15_bit_codes", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, dist_lens=d)

    one_block("len258_as_284_31", "tables", lits(b"AC") + [match(258, 2, True), lit(71), match(258, 1, True), lit(84)], dynamic=False)
    one_block("len258_as_285", "tables", lits(b"AC") + [match(258, 2), lit(71), match(258, 1), lit(84)], dynamic=False)

    # alphabets that shrink from block to block: whatever a block leaves behind in the sorted symbols, the counts and the root tables must not show
    a1 = [8] * 255 + [0] * 31
    for s, L in ((255, 9), (256, 10), (257, 11), (258, 12), (259, 13), (285, 14), (284, 15), (283, 15)):
        a1[s] = L
    t1 = lits(PREFIX[:200]) + [match(3, 10), match(4, 20), match(5, 100), match(258, 7), match(258, 9, True), match(232, 50), match(200, 3)]
    t2 = [lit(65), match(3, 1), lit(65)]
    t3 = lits(b"shrink") + [match(6, 6)]
    s4 = [67, 71, 84, 10, 78, 97, 99, 103, 116, 110, 120, 256, 258]
    a4 = [0] * 259
    for s, L in zip(s4, ladder(13)):
        a4[s] = L
    t4 = lits(b"CGT\nNacgtnx") + [match(4, 3), lit(120)]
    b = Build().dynamic(a1, flat_lens(30), t1, False).dynamic(ll([65, 256, 257]), [1, 1], t2, False).fixed(t3, False).dynamic(a4, [2, 2, 2, 2], t4, True)
    add("shrinking_tables", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, litlen_lens=[a1, ll([65, 256, 257]), a4])

    b = Build().fixed([], False).stored(b"", False).dynamic(ONLY_EOB[0], ONLY_EOB[1], [], False).fixed(lits(b"text after empty blocks"), True)
    add("empty_blocks", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks)

    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts = [b"ACGTTGCA" * 40, b"sync flushed, ", b"partial flushed, ", b"full flushed, ", b"and the end " * 30]
    raw = c.compress(parts[0]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(parts[1]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(parts[2]) + \
        c.flush(zlib.Z_PARTIAL_FLUSH) + c.compress(parts[3]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(parts[4]) + c.flush()
    add("zlib_sync_partial_full_flush", "tables", raw, True, text=b"".join(parts))

    data = bytes(random.Random(65535).randrange(256) for _ in range(65535))
    b = Build().stored(data, True)
    add("stored_len_65535", "tables", b.raw(), True, text=data, blocks=b.blocks)

    b, offs = Build(), []
    for m in range(8):
        b.fixed(lits([200] * m + [65]), False)
        offs.append(b.bitpos[-1] % 8)
        b.stored(b"stored block %d;" % m, m == 7)
    add("stored_after_odd_bits", "tables", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, bit_offsets=offs)


# ---- accept: the pipelined form's scheduling edges --------------------------------------------------------------------------------------
PRIMER = match(65, 600)          # longer than one load per lane: always drains, and leaves synced == pos behind it


def _pipe():
    def short(i):                  # short matches out of the literal prefix: always below `synced`
        return match(3 + i % 5, 590 - 31 * (i % 7))

    for n in (8, 9, 16, 17):
        toks = lits(PREFIX) + [PRIMER] + [short(i) for i in range(n)]
        one_block("run_of_%d" % n, "pipe", toks, dynamic=False, run=n, first=601)

    for name, past in (("source_ends_at_batch_head", 0), ("source_one_past_batch_head", 1)):
        toks = lits(PREFIX) + [PRIMER] + [short(i) for i in range(8)]
        text, st = expand(toks)
        p, pos, ln = st[601], len(text), 10         # p: the first destination of the batch of eight
        toks.append(match(ln, pos - (p + past - ln)))
        toks += [lit(33), short(3)]
        one_block(name, "pipe", toks, dynamic=False, edge=(0, 609), past=past)

    # ... and one whose last source byte is the first destination of a match of the SAME batch, which is stored a round after the batch's loads go out
    toks = lits(PREFIX) + [PRIMER, match(3, 300), match(10, 12), lit(43), short(2)]
    one_block("source_one_past_synced_in_batch", "pipe", toks, dynamic=False, edge=(0, 602))

    # a match whose source is exactly the destination of the match before it: as the second slot of a batch, and as the first slot of the next batch
    toks = lits(PREFIX) + [PRIMER, match(9, 300), match(9, 9), lit(34), PRIMER] + [short(i) for i in range(7)] + [match(11, 200), match(11, 11), lit(35)]
    one_block("source_is_previous_match", "pipe", toks, dynamic=False, edges=((0, 602, 1), (0, 613, 0)))

    toks, where = lits(PREFIX), []
    for ln in (3, 63, 64, 65, 258):
        for d in sorted({1, 2, 63, 64, 65, ln - 1, ln, ln + 1}):
            toks.append(PRIMER)
            where.append((len(toks), ln, d))
            toks.append(match(ln, d))
    one_block("len_64_65", "pipe", toks, dynamic=False, where=where)

    for name, pre in (("overlap_first_after_drain", []), ("overlap_after_literal", [lit(36)])):
        b = Build().fixed(lits(PREFIX), False).fixed(pre + [match(40, 7), lit(37), match(64, 63), lit(38)], True)
        add(name, "pipe", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, edge=(1, len(pre)))

    b = Build().fixed(lits(PREFIX) + [PRIMER] + [short(i) for i in range(8)], False).fixed([match(20, 30), lit(39), match(12, 45)], True)
    add("eob_with_full_batch", "pipe", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, edge=(1, 0))

    b = Build().stored(PREFIX, False).fixed([match(50, 50), match(20, 600), lit(40)], False).stored(b"again stored", False).fixed([match(12, 12), lit(41)], True)
    add("match_into_stored", "pipe", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, edges=((1, 0), (3, 0)))

    toks = [lit(65), match(5, 1), match(6, 6)] + lits(PREFIX[:588]) + [match(20, 600), lit(42), match(100, 621)]
    one_block("dist_equals_pos", "pipe", toks, dynamic=False, edges=(1, 2, 591, 593))


# ---- accept: the LDS form's window edges ------------------------------------------------------------------------------------------------
TAIL = [lit(0x5A), match(20, 600), lit(0x21)]


def _window():
    for bnd in BOUNDARIES:
        toks = lits(PREFIX)
        reach(toks, 600, bnd - 1)
        e = len(toks)
        one_block("literal_ends_on_%d" % bnd, "window", toks + [lit(0x7E)] + TAIL, dynamic=False, b=bnd, edge=(0, e), kind="literal_ends")

        toks = lits(PREFIX)
        reach(toks, 600, bnd - 100)
        data = bytes(random.Random(bnd).randrange(256) for _ in range(200))
        b = Build().fixed(toks, False).stored(data, False).fixed(TAIL, True)
        add("stored_crosses_%d" % bnd, "window", b.raw(), True, text=layout(b.blocks)[0], blocks=b.blocks, b=bnd, edge=(1, 0), kind="stored_crosses")

        toks = lits(PREFIX)
        reach(toks, 600, bnd - 40)
        e = len(toks)
        one_block("match_ends_on_%d" % bnd, "window", toks + [match(40, 600)] + TAIL, dynamic=False, b=bnd, edge=(0, e), kind="match_ends")

        ln = 150
        for tag, d in (("dist_ge_len", 600), ("dist_1", 1), ("dist_len_minus_1", ln - 1), ("dist_32768", 32768), ("dist_32768_minus_len_plus_1", 32768 - ln + 1)):
            if d > bnd - 70:
                continue                    # the distance would reach in front of the text
            toks = lits(PREFIX)
            reach(toks, 600, bnd - 70)
            e = len(toks)
            one_block("match_straddles_%d_%s" % (bnd, tag), "window", toks + [match(ln, d)] + TAIL, dynamic=False, b=bnd, edge=(0, e), kind="straddles_" + tag)

    # (no match with distance 32768 can straddle 32768 itself: it starts there at the earliest)
    toks = lits(PREFIX)
    reach(toks, 600, 32768)
    e = len(toks)
    one_block("match_starts_on_32768_dist_32768", "window", toks + [match(150, 32768)] + TAIL, dynamic=False, b=32768, edge=(0, e), kind="starts_dist_32768")

    for n in (16383, 16384, 16385, 32768, 47, 48, 49):
        toks = lits(PREFIX[:min(n, 600)])
        if n > 600:
            reach(toks, 600, n)
        one_block("text_len_%d" % n, "window", toks, dynamic=False, text_len=n)


# ---- reject ------------------------------------------------------------------------------------------------------------------------------
GOOD_LL = ll([65, 67, 256, 257])             # 2, 2, 2, 2
GOOD_TOKS = lits(b"ACCA")


def _reject():
    def rej(name, raw, code, phrase, **kw):
        add(name, "reject", raw, False, code=code, phrase=phrase, **kw)

    d = Deflate(); d.header(3, True); d.w.bits(0, 13)
    rej("btype3", d.finish(), E_BTYPE, "invalid block type")
    rej("stored_nlen_mismatch", Deflate().stored(b"stored", True, nlen=0xFFF8).finish(), E_STORED, "invalid stored block lengths")

    for name, field in (("hlit_287", 30), ("hlit_288", 31)):
        a = GOOD_LL + [0] * (257 + field - len(GOOD_LL))
        rej(name, Deflate().dynamic(a, [1, 1], GOOD_TOKS, True).finish(), E_CODE, "too many length or distance symbols")
    for name, field in (("hdist_31", 30), ("hdist_32", 31)):
        rej(name, Deflate().dynamic(GOOD_LL, [0] * (field + 1), GOOD_TOKS, True).finish(), E_CODE, "too many length or distance symbols")

    cll = [0] * 19
    cll[0], cll[2], cll[18] = 1, 1, 1
    rej("cl_oversubscribed", Deflate().dynamic(GOOD_LL, [2, 2, 2, 2], GOOD_TOKS, True, cl_lens=cll).finish(), E_OVERSUB, "invalid code lengths set")
    cll = [0] * 19
    cll[0] = 1
    rej("cl_single_code", Deflate().dynamic([0] * 257, [0], [], True, cl_lens=cll, body=False).finish() + b"\0" * 40, E_OVERSUB, "invalid code lengths set")
    # (zlib does not refuse an empty code-length code as such: it reads every length as zero and then misses the end-of-block code)
    rej("cl_all_zero", Deflate().dynamic([], [], [], True, cl_lens=[0] * 19, cl_syms=[], hlit=0, hdist=0, hclen=15, body=False).finish() + b"\0" * 40, E_OVERSUB,
        "missing end-of-block")
    # a COUNT of four code-length code lengths (16 17 18 0) spells nothing but zeros
    cll = [0] * 19
    cll[0], cll[18] = 1, 1
    rej("hclen_count_4", Deflate().dynamic([0] * 257, [0], [], True, cl_lens=cll, cl_syms=[(18, 127), (18, 109)], body=False).finish() + b"\0" * 8, E_CODE,
        "missing end-of-block", hclen=4)

    cl = [(16, 0)] + cl_compress(GOOD_LL[3:]) + [(1, 0), (1, 0)]
    rej("repeat16_first", Deflate().dynamic(GOOD_LL, [1, 1], GOOD_TOKS, True, cl_syms=cl).finish(), E_REPEAT, "invalid bit length repeat")
    # the last code-length symbol runs one length past HLIT + HDIST
    a = ll([65, 67, 256, 257, 258, 259], 260, [2, 2, 3, 3, 3, 3])
    rej("repeat_overruns_total_16", Deflate().dynamic(a, [0], GOOD_TOKS, True, cl_syms=cl_compress(a[:257]) + [(16, 2)]).finish(), E_REPEAT, "invalid bit length repeat")
    rej("repeat_overruns_total_17", Deflate().dynamic(GOOD_LL, [0], GOOD_TOKS, True, cl_syms=cl_compress(GOOD_LL) + [(17, 0)]).finish(), E_REPEAT,
        "invalid bit length repeat")
    rej("repeat_overruns_total_18", Deflate().dynamic(GOOD_LL, [0], GOOD_TOKS, True, cl_syms=cl_compress(GOOD_LL[:257]) + [(18, 127)]).finish(), E_REPEAT,
        "invalid bit length repeat")

    a = ll([65, 67], 257)
    rej("no_eob_code", Deflate().dynamic(a, [1, 1], lits(b"AC"), True, eob=False).finish() + b"\0" * 8, E_CODE, "missing end-of-block")
    a = ll([65, 67, 256], 257, [1, 1, 1])
    rej("litlen_oversubscribed", Deflate().dynamic(a, [1, 1], lits(b"AC"), True).finish(), E_OVERSUB, "invalid literal/lengths set", lens=a)
    a = ll([65, 256], 257, [2, 2])
    rej("litlen_incomplete", Deflate().dynamic(a, [1, 1], lits(b"A"), True).finish(), E_OVERSUB, "invalid literal/lengths set", lens=a)
    rej("dist_oversubscribed", Deflate().dynamic(GOOD_LL, [1, 1, 1], GOOD_TOKS, True).finish(), E_OVERSUB, "invalid distances set", lens=[1, 1, 1])
    rej("dist_incomplete_two_codes", Deflate().dynamic(GOOD_LL, [2, 2], GOOD_TOKS, True).finish(), E_OVERSUB, "invalid distances set", lens=[2, 2])

    rej("no_dist_code_then_match", Deflate().dynamic(GOOD_LL, [0], GOOD_TOKS + [raw_sym(257), raw_bits("0000")], True).finish(), E_CODE, "invalid distance code")
    # the one code is 0: the stream sends the 1 that no symbol has
    rej("single_dist_code_other_bit", Deflate().dynamic(GOOD_LL, [1], GOOD_TOKS + [raw_sym(257), raw_bits("1")], True).finish(), E_CODE, "invalid distance code")

    for s in (286, 287):
        rej("fixed_sym_%d" % s, Deflate().fixed(GOOD_TOKS + [raw_sym(s)], True).finish(), E_CODE, "invalid literal/length code")
    for s in (30, 31):
        rej("fixed_dist_%d" % s, Deflate().fixed(GOOD_TOKS + [raw_match(257, 0, 0, s, 0, 0)], True).finish(), E_CODE, "invalid distance code")

    rej("dist_pos_plus_1_at_0", Deflate().fixed([raw_match(257, 0, 0, 0, 0, 0)], True).finish(), E_DIST, "too far back", pos=0)
    ds = (18, 601 - 513, 8)                     # distance 601 behind 600 literals
    rej("dist_pos_plus_1_at_600", Deflate().fixed(lits(PREFIX) + [raw_match(257, 0, 0, *ds)], True).finish(), E_DIST, "too far back", pos=600)

    toks = lits(PREFIX[:100]) + [match(20, 50), lit(65)]
    b = Build().fixed(toks, True)
    rej("output_past_isize", b.raw(), E_OUTPUT, "incorrect length check", text=layout(b.blocks)[0], raw_valid=True)

    # truncated: zlib never reaches the end of the stream; the device reads the member's trailer as data and may report any error, never 0
    toks = lits(PREFIX) + [match(20, 50), lit(65)]
    a, dl = auto_lens(toks)
    full = Deflate().dynamic(a, dl, toks, True).finish()
    rej("truncated_in_header", full[:20], None, "truncated")
    rej("truncated_in_symbols", full[:len(full) - 200], None, "truncated")
    rej("truncated_in_stored", Deflate().stored(PREFIX, True).finish()[:300], None, "truncated")


_tables()
_pipe()
_window()
_reject()

# ---- gzip headers (RFC 1952), through gs_gunzip_batch -----------------------------------------------------------------------------------
# A wrong FHCRC VALUE is out of scope: zlib checks it, the host decoder in use (libdeflate) and the device both skip the field.
HEADER_TEXT = b">h\nACGTACGTTTGACCA\n"
_hraw = Deflate().fixed(lits(HEADER_TEXT), True).finish()
_all = dict(flags=FTEXT, extra=b"AB\x02\x00xy", name=b"name.fa", comment=b"a comment", hcrc=True)
HEADER_CASES = [          # (name, member, status, text)
    ("ftext", gzip_member(_hraw, HEADER_TEXT, flags=FTEXT), 0, HEADER_TEXT),
    ("fname", gzip_member(_hraw, HEADER_TEXT, name=b"genome.fna"), 0, HEADER_TEXT),
    ("fcomment", gzip_member(_hraw, HEADER_TEXT, comment=b"made by hand"), 0, HEADER_TEXT),
    ("fhcrc", gzip_member(_hraw, HEADER_TEXT, hcrc=True), 0, HEADER_TEXT),
    ("fextra_xlen_0", gzip_member(_hraw, HEADER_TEXT, extra=b""), 0, HEADER_TEXT),
    ("fextra_xlen_300", gzip_member(_hraw, HEADER_TEXT, extra=b"ZZ\x28\x01" + bytes(range(256)) + bytes(40)), 0, HEADER_TEXT),
    ("all_five", gzip_member(_hraw, HEADER_TEXT, **_all), 0, HEADER_TEXT),
    ("reserved_0x20", gzip_member(_hraw, HEADER_TEXT, flags=0x20), 100, None),
    ("reserved_0x40", gzip_member(_hraw, HEADER_TEXT, flags=0x40), 100, None),
    ("reserved_0x80", gzip_member(_hraw, HEADER_TEXT, flags=0x80), 100, None),
    ("cm_7", gzip_member(_hraw, HEADER_TEXT, cm=7), 100, None),
    ("member_of_17_bytes", gzip_member(Deflate().fixed([], True).finish(), b"")[:17], 100, None),
    ("xlen_past_end", gzip_member(_hraw, HEADER_TEXT, extra=b"")[:10] + b"\x60\xea" + gzip_member(_hraw, HEADER_TEXT)[10:], 100, None),
    ("fname_no_terminator", b"\x1f\x8b\x08\x08\0\0\0\0\0\xff" + b"n" * 40, 100, None),
]
