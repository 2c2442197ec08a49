"""The device inflater (gs_inflate.hip) against zlib on hand-built DEFLATE streams: the legal shapes that no installed compressor emits and the
illegal ones a decoder has to refuse (deflate_cases.py; test_deflate_cases_cpu.py holds every case to its name), through both forms of the decoder.
The rule is the one gs_inflate.hip states: the device takes exactly what zlib takes and reports the rest. Beside them, the two paths of the same
file that nothing else runs: the CRC kernel at text lengths on and around its 256-byte piece and 64 KB chunk, and the second pass of the record scan.
Every comparison is equality of bytes or of integer status codes.

One-line changes to gs_inflate.hip and the cases that see them (argued from the code):
  inf_build without its `maxlen > 1` exception    single_dist_code, no_dist_code_literals_only, only_eob, and the cases that cannot do without such
                                                  an alphabet: hclen_4, empty_blocks, no_dist_code_then_match, single_dist_code_other_bit (3, not 4)
  `i + rep > total` checked against hlit          repeat16_across_hlit, repeat18_across_hlit (status 8)
  `lane % dist` -> `lane`                         overlap_first_after_drain, len_64_65 (lanes >= dist read text that is not written yet: the poison)
  `<= synced` -> `< synced + 2`                   source_one_past_synced_in_batch (the byte is stored a round after the load), source_one_past_batch_head,
                                                  overlap_after_literal
  `len <= 64` -> `len <= 65`                      len_64_65 (the 65th byte has no lane)
  half flushed only when a match ENDS on it       every match_straddles_* (a 16 KB half never reaches the text)
  base of symbol 284                              len258_as_284_31, shrinking_tables"""
import zlib

import numpy as np
import pytest

from deflate_cases import CASES, HEADER_CASES
from deflate_writer import Deflate, gzip_member

pytestmark = pytest.mark.gpu

DEVICE_ERRORS = set(range(1, 9)) | {101, 102, 103, 104}


@pytest.mark.parametrize("window", ["lds", "pipe"])
def test_hand_built_streams(gpu_ctx, monkeypatch, window):
    """every case of the table and every gzip header case in ONE call. A wrong FHCRC value is out of scope: zlib checks it, the host decoder in use
    (libdeflate) and the device both skip the field."""
    import gsearch_amd as G
    monkeypatch.setenv("GS_INFLATE_WINDOW", window)
    members = [c.member() for c in CASES] + [h[1] for h in HEADER_CASES]
    caps = [c.out_cap() for c in CASES] + [64] * len(HEADER_CASES)
    G.debug_mem_fill(0xA5)                      # the text buffer starts as poison, not as what the other form left there: a copy that reads a byte
    try:                                        # before it was written gets 0xA5, whatever ran before
        gpu_ctx.release_scratch()
        res = G.gunzip_batch(gpu_ctx, members, out_caps=caps)
    finally:
        G.debug_mem_fill(None)
    wrong = []
    for c, m, (st, text) in zip(CASES, members, res):
        if c.accept:
            want = zlib.decompress(m, 31)
            if st != 0:
                wrong.append("%s [%s]: zlib accepts, status %d" % (c.name, window, st))
            elif text != want:
                wrong.append("%s [%s]: status 0, %d bytes that are not zlib's %d" % (c.name, window, len(text), len(want)))
        elif st == 0:
            wrong.append("%s [%s]: zlib refuses (%s), the device accepted" % (c.name, window, c.phrase))
        elif c.code is not None and st != c.code:
            wrong.append("%s [%s]: status %d, expected %d" % (c.name, window, st, c.code))
        elif c.code is None and st not in DEVICE_ERRORS:
            wrong.append("%s [%s]: status %d is no error of the decoder" % (c.name, window, st))
    for (name, m, status, want), (st, text) in zip(HEADER_CASES, res[len(CASES):]):
        if st != status:
            wrong.append("header %s [%s]: status %d, expected %d" % (name, window, st, status))
        elif status == 0 and text != zlib.decompress(m, 31):
            wrong.append("header %s [%s]: status 0, other bytes than zlib's" % (name, window))
    assert not wrong, "\n".join(wrong)


def _stored_member(text):
    d = Deflate()
    for o in range(0, max(len(text), 1), 65535):
        d.stored(text[o:o + 65535], o + 65535 >= len(text))
    return gzip_member(d.finish(), text)


def test_crc_on_and_around_piece_and_chunk(gpu_ctx):
    """k_crc32_chunks: status 0 means that the device's CRC-32 of the text equalled the trailer zlib wrote; the same text with one bit flipped (in a
    member of stored blocks, so that the flip changes the text and nothing else) must come back as 103. The two texts of leading zeros: a CRC register that
    starts at 0 does not see them, the fold's x^(8 n) term has to."""
    import gsearch_amd as G
    rng = np.random.default_rng(256)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = [bytes(rng.choice(acgt, n)) for n in (0, 1, 255, 256, 257, 65535, 65536, 65537, 131071, 131072, 131073, 3 * 65536 + 256)]
    texts += [b"\0" * 65537, b"\0" * 65536 + b"A"]
    good = []
    for t in texts:
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        good.append(c.compress(t) + c.flush())
    flipped = []
    for t in texts:
        if not t:
            continue                                   # (no bit to flip in an empty text)
        m = bytearray(_stored_member(t))
        k = len(t) // 2
        m[10 + 5 * (k // 65535 + 1) + k] ^= 0x04
        assert zlib.decompressobj(-15).decompress(bytes(m[10:-8])) == t[:k] + bytes([t[k] ^ 0x04]) + t[k + 1:]
        flipped.append(bytes(m))
    members = good + flipped
    res = G.gunzip_batch(gpu_ctx, members, out_caps=[int.from_bytes(m[-4:], "little") for m in members])
    wrong = []
    for t, m, (st, text) in zip(texts, good, res):
        if st != 0 or text != zlib.decompress(m, 31):
            wrong.append("text of %d bytes: status %d" % (len(t), st))
    for t, (st, text) in zip([t for t in texts if t], res[len(good):]):
        if st != 103:
            wrong.append("text of %d bytes with a flipped bit: status %d, expected 103" % (len(t), st))
    assert not wrong, "\n".join(wrong)


def _gz(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("layout", ["as_it_comes", "last_record_on_a_scan_chunk"])
def test_record_scan_second_pass(gpu_ctx, tmp_path, monkeypatch, layout):
    """fasta_scan_dev sizes its first pass for max(65536, bytes / 256) records: a group with 70 000 short protein records takes the second pass. Records,
    symbols and signatures must equal the host decoders' and the plain files'. Second layout: the 70 000th '>' is the first byte of a 16 KB scan chunk, so
    the newline in front of it belongs to the chunk before."""
    import gsearch_amd as G
    rng = np.random.default_rng(70000)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    lens = rng.integers(8, 13, 70000)
    res = bytes(rng.choice(aa, int(lens.sum()) + 16384))
    recs, o = [], 0
    for i, n in enumerate(lens):
        recs.append(b">r%d\n%s\n" % (i, res[o:o + n]))
        o += int(n)
    if layout == "last_record_on_a_scan_chunk":
        at = sum(len(r) for r in recs[:-1])
        recs[0] = recs[0][:-1] + res[o:o + (-at) % 16384] + b"\n"         # (one long first record moves everything behind it)
        assert sum(len(r) for r in recs[:-1]) % 16384 == 0
    big = b"".join(recs)
    assert big.count(b">") == 70000 and len(big) < 2_000_000
    small = [b">a one\nMKVLAAGIVGLLLAQPSA\n>a two\nMSTNPKPQRKTKRNTNRRPQDVKFPGG\n", b">b\n" + bytes(rng.choice(aa, 500)) + b"\n"]
    gz, plain = [], []
    for i, t in enumerate([big] + small):
        (tmp_path / ("f%d.faa.gz" % i)).write_bytes(_gz(t)); gz.append(tmp_path / ("f%d.faa.gz" % i))
        (tmp_path / ("p%d.faa" % i)).write_bytes(t); plain.append(tmp_path / ("p%d.faa" % i))
    sk = G.sketcher_for(G.SeqSketcherParams(7, 800, "optdens", data_t="aa"))
    monkeypatch.setenv("GS_GZIP_DEVICE", "1")
    sig, nrec, nsym, st = sk.sketch_files(gz, pio=0)
    monkeypatch.setenv("GS_GZIP_DEVICE", "0")
    sig_h, nrec_h, nsym_h, _ = sk.sketch_files(gz, pio=0)
    sig_p, nrec_p, nsym_p, _ = sk.sketch_files(plain, pio=0)
    assert st["gz_members_inflated_on_device"] == 3 and st["gz_members_handed_back_to_host"] == 0
    assert list(nrec) == list(nrec_h) == list(nrec_p) == [70000, 2, 1]
    assert list(nsym) == list(nsym_h) == list(nsym_p)
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    assert np.array_equal(bits(sig), bits(sig_h)) and np.array_equal(bits(sig), bits(sig_p))
