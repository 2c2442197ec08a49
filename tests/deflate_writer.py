"""A DEFLATE (RFC 1951) / gzip (RFC 1952) writer for tests: streams are put together bit by bit, so a case can hold the legal shapes that no
installed compressor emits (single-code alphabets, repeats across the HLIT boundary, 15-bit codes, ...) and the illegal ones a decoder has
to refuse. Pure Python: imports nothing of the library, only zlib for the verdict and the CRC."""
import struct
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """bits go out LSB first within a byte (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        """a plain field: least significant bit first"""
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: most significant bit first"""
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def raw(self, s):
        """an arbitrary bit string such as "0110", written in reading order"""
        for ch in s:
            self.bits(int(ch), 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """{symbol: (code, length)} of the canonical code of these lengths (RFC 1951 3.2.2); lengths that over-subscribe give colliding codes, which is what
    a reject case wants to send"""
    count = [0] * 17
    for L in lens:
        count[L] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, L in enumerate(lens):
        if L:
            out[s] = (nxt[L] & ((1 << L) - 1), L)
            nxt[L] += 1
    return out


def kraft(lens):
    """sum of 2^-L over the used symbols, in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - L) for L in lens if L)


def flat_lens(n):
    """n code lengths of a complete code with two neighbouring lengths (n >= 2)"""
    k = max(1, (n - 1).bit_length())
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------
def lit(b):
    return ("lit", b)


def len_sym(length, as_284=False):
    """(symbol, extra value, extra bits) of a match length; 258 has two spellings: symbol 285, or symbol 284 with extra 31"""
    assert 3 <= length <= 258
    if length == 258 and as_284:
        return 284, 31, 5
    i = max(j for j in range(29) if LEN_BASE[j] <= length)
    assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i]) or LEN_EXTRA[i] == 0 and length == LEN_BASE[i]
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def dist_sym(dist):
    assert 1 <= dist <= 32768
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    return i, dist - DIST_BASE[i], DIST_EXTRA[i]


def match(length, dist, as_284=False):
    """("match", len, dist, (len symbol, extra, bits), (dist symbol, extra, bits))"""
    return ("match", length, dist, len_sym(length, as_284), dist_sym(dist))


def raw_match(lsym, lextra, lbits, dsym, dextra, dbits):
    """a match given by its symbols alone (reject cases: symbols and distances that mean nothing); `expand` refuses it"""
    return ("match", None, None, (lsym, lextra, lbits), (dsym, dextra, dbits))


def raw_sym(sym):
    """one literal/length symbol with nothing behind it, e.g. 286"""
    return ("sym", sym)


def raw_bits(s):
    """an arbitrary bit string in place of a code"""
    return ("bits", s)


def expand(tokens, prefix=b""):
    """the LZ77 expansion in plain Python -> (text, starts): starts[i] = length of the text in front of token i (prefix included)"""
    out = bytearray(prefix)
    starts = []
    for t in tokens:
        starts.append(len(out))
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            _, length, dist = t[:3]
            assert length is not None and 1 <= dist <= len(out), "expand: not a plain match"
            src = len(out) - dist
            if dist >= length:
                out += out[src:src + length]
            else:                                   # the source runs into the target: the last `dist` bytes repeat
                out += (bytes(out[src:]) * (length // dist + 1))[:length]
        else:
            raise AssertionError("expand: raw token")
    return bytes(out), starts


def lits(data):
    return [lit(b) for b in data]


# ---- blocks -----------------------------------------------------------------------------------------------------------------------------
class Deflate:
    """a raw DEFLATE stream, block by block"""

    def __init__(self):
        self.w = BitWriter()

    def header(self, btype, last):
        self.w.bits(1 if last else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, last, nlen=None):
        self.header(0, last)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        assert self.w.n == 0
        self.w.out += bytes(data)
        return self

    def tokens(self, toks, lcodes, dcodes, eob=True):
        w = self.w
        for t in toks:
            if t[0] == "lit":
                w.code(*lcodes[t[1]])
            elif t[0] == "sym":
                w.code(*lcodes[t[1]])
            elif t[0] == "bits":
                w.raw(t[1])
            else:
                (ls, lv, lb), (ds, dv, db) = t[3], t[4]
                w.code(*lcodes[ls])
                w.bits(lv, lb)
                w.code(*dcodes[ds])
                w.bits(dv, db)
        if eob:
            w.code(*lcodes[256])

    def fixed(self, toks, last, eob=True):
        self.header(1, last)
        self.tokens(toks, canonical(FIXED_LITLEN), canonical(FIXED_DIST), eob)
        return self

    def dynamic(self, litlen_lens, dist_lens, toks, last, cl_syms=None, cl_lens=None, hlit=None, hdist=None, hclen=None, eob=True, body=True):
        """litlen_lens / dist_lens: the code lengths the block declares (HLIT = len(litlen_lens) - 257, HDIST = len(dist_lens) - 1).
        cl_syms: the code-length symbols to send, as (symbol, extra value) pairs - (16, r) repeats the previous length 3 + r times, (17, r) is 3 + r
        zeros, (18, r) is 11 + r zeros; default one plain symbol per length. It is sent as given: a case that wants a repeat to run from the
        literal/length lengths into the distance lengths, or past the end, writes exactly that.
        cl_lens: the 19 lengths of the code-length code by symbol; default a complete code over the symbols in use.
        hlit / hdist / hclen: raw values of the three header fields (5, 5, 4 bits) in place of the computed ones.
        body=False stops behind the header fields and code-length code lengths + symbols (nothing of the block's data is written)."""
        w = self.w
        if cl_syms is None:
            cl_syms = [(L, 0) for L in list(litlen_lens) + list(dist_lens)]
        if cl_lens is None:
            used = sorted({s for s, _ in cl_syms})
            if len(used) == 1:
                used = sorted(set(used) | {0 if used[0] else 1})
            cl_lens = [0] * 19
            for s, L in zip(used, flat_lens(len(used))):
                cl_lens[s] = L
        ncl = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
        self.header(2, last)
        w.bits(len(litlen_lens) - 257 if hlit is None else hlit, 5)
        w.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
        w.bits(ncl - 4 if hclen is None else hclen, 4)
        for i in range((ncl if hclen is None else hclen + 4)):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canonical(cl_lens)
        for s, v in cl_syms:
            if isinstance(s, str):
                w.raw(s)
                continue
            w.code(*cc[s])
            w.bits(v, {16: 2, 17: 3, 18: 7}.get(s, 0))
        if body:
            self.tokens(toks, canonical(litlen_lens), canonical(dist_lens), eob)
        return self

    def finish(self):
        return self.w.getvalue()


def cl_expand(cl_syms):
    """the lengths a sequence of code-length symbols stands for, and for every symbol the index range [first, last] it fills"""
    lens, spans = [], []
    for s, v in cl_syms:
        a = len(lens)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + v)
        elif s == 17:
            lens += [0] * (3 + v)
        else:
            lens += [0] * (11 + v)
        spans.append((a, len(lens) - 1))
    return lens, spans


def cl_compress(lens):
    """code-length symbols for a list of lengths with the zeros run-length coded (17 / 18), never across more than the list given"""
    out, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0 and j - i < 138:
                j += 1
            if j - i >= 11:
                out.append((18, j - i - 11))
            elif j - i >= 3:
                out.append((17, j - i - 3))
            else:
                out += [(0, 0)] * (j - i)
            i = j
        else:
            out.append((lens[i], 0))
            i += 1
    return out


# ---- gzip -------------------------------------------------------------------------------------------------------------------------------
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def gzip_member(raw, text=None, flags=0, extra=None, name=None, comment=None, hcrc=False, cm=8, crc=None, isize=None):
    """RFC 1952 member around a raw DEFLATE stream. The optional fields set their flag bits themselves; `flags` adds further bits (FTEXT, reserved
    ones). The header CRC, when asked for, is the correct one. crc / isize override the trailer computed from `text`."""
    flg = flags
    if extra is not None:
        flg |= FEXTRA
    if name is not None:
        flg |= FNAME
    if comment is not None:
        flg |= FCOMMENT
    if hcrc:
        flg |= FHCRC
    h = bytearray(b"\x1f\x8b" + bytes([cm, flg]) + b"\0\0\0\0" + b"\0\xff")
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xFFFF)
    text = b"" if text is None else text
    tr = struct.pack("<II", (zlib.crc32(text) & 0xFFFFFFFF) if crc is None else crc, (len(text) & 0xFFFFFFFF) if isize is None else isize)
    return bytes(h) + raw + tr


def verdict(raw):
    """zlib's answer to a raw DEFLATE stream: (True, text), or (False, message). True needs the stream's end reached and nothing left over."""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(raw) + d.flush()
    except zlib.error as e:
        return False, str(e)
    if not d.eof:
        return False, "incomplete or truncated stream"
    if d.unused_data:
        return False, "unused data after the stream"
    return True, text
