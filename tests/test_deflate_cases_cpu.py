"""The hand-built DEFLATE streams of deflate_cases.py, checked without a device: zlib gives every case the verdict the table states (and refuses the
reject cases for the stated reason), and every case has the edge its name promises - asserted from how the stream was put together (code lengths,
tokens and the text positions `expand` gives them), not from a decoder. A case whose name promises an edge that its bytes do not have is the
failure this file exists to catch."""
import zlib

import pytest

from deflate_cases import BOUNDARIES, CASES, HEADER_CASES, layout, pipe_schedule
from deflate_writer import canonical, cl_expand, kraft, verdict

BY_NAME = {c.name: c for c in CASES}
POISON = 0xA5           # what test_gpu_inflate_streams.py fills the text buffer with before the decoder runs


def case(name):
    return BY_NAME[name]


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_zlib_verdict(name):
    c = case(name)
    ok, got = verdict(c.raw)
    if c.accept:
        assert ok, (name, got)
        assert got == c.text, name
        if c.blocks is not None:
            assert layout(c.blocks)[0] == c.text, name
        assert zlib.decompress(c.member(), 31) == c.text, name
        assert c.code is None and len(c.text) <= 102400
    elif c.raw_valid:                       # the data is fine, the member's trailer is not
        assert ok and got == c.text, name
        with pytest.raises(zlib.error, match=c.phrase):
            zlib.decompress(c.member(), 31)
    else:
        assert not ok, name
        assert c.phrase and c.phrase in got, (name, got)
        with pytest.raises(zlib.error):
            zlib.decompress(c.member(), 31)
    assert len(c.member()) >= 18 and c.out_cap() <= 102400


def test_the_table_has_every_group():
    n = {g: sum(c.group == g for c in CASES) for g in ("tables", "pipe", "window", "reject")}
    print("cases:", n, "accept", sum(c.accept for c in CASES), "reject", sum(not c.accept for c in CASES), "header", len(HEADER_CASES))
    assert n["tables"] >= 19 and n["pipe"] >= 13 and n["window"] >= 30 and n["reject"] >= 30
    assert all(c.accept == (c.group != "reject") for c in CASES)
    assert all(c.code in (None, 1, 2, 3, 4, 5, 6, 8) for c in CASES if not c.accept)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def used_lengths(c, bi, lens, alphabet):
    """code lengths of the symbols that block bi's tokens really send"""
    out = set()
    for t in c.blocks[bi][1]:
        if alphabet == "litlen":
            out.add(lens[t[1]] if t[0] == "lit" else lens[t[3][0]])
        elif t[0] == "match":
            out.add(lens[t[4][0]])
    if alphabet == "litlen":
        out.add(lens[256])
    return out


def test_single_code_and_empty_alphabets():
    d = case("single_dist_code").meta["dist_lens"]
    assert sorted(d)[-2:] == [0, 1] and any(t[0] == "match" for t in case("single_dist_code").blocks[0][1])
    d = case("no_dist_code_literals_only").meta["dist_lens"]
    assert not any(d) and all(t[0] == "lit" for t in case("no_dist_code_literals_only").blocks[0][1])
    m = case("only_eob").meta
    assert [i for i, L in enumerate(m["litlen_lens"]) if L] == [256] and m["litlen_lens"][256] == 1 and not any(m["dist_lens"])
    assert case("only_eob").blocks[0][1] == [] and case("only_eob").text == b""


@pytest.mark.parametrize("name", ["repeat16_across_hlit", "repeat18_across_hlit"])
def test_repeat_runs_across_hlit(name):
    m = case(name).meta
    lens, spans = cl_expand(m["cl_syms"])
    assert lens == m["lens"] and len(lens) > m["hlit"]
    crossing = [(s, a, b) for (s, _), (a, b) in zip(m["cl_syms"], spans) if a < m["hlit"] <= b]
    assert len(crossing) == 1 and crossing[0][0] == m["rep"], crossing
    # both alphabets are in use on either side of it
    assert {t[0] for t in case(name).blocks[0][1]} == {"lit", "match"}


def test_repeat16_behind_a_long_zero_run():
    m = case("repeat16_after_138_zeros").meta
    lens, spans = cl_expand(m["cl_syms"])
    assert lens == m["lens"]
    assert m["cl_syms"][0] == (18, 127) and spans[0] == (0, 137)            # 138 zeros: more than one trip of 64 lanes
    assert m["cl_syms"][1][0] == 16 and spans[1][0] == 138
    assert all(m["before"][i] for i in range(128, spans[1][1] + 1))          # what the block before left there is not zero


def test_last_symbols_of_both_alphabets():
    c = case("hlit_286_uses_285")
    assert len(c.meta["litlen_lens"]) == 286 and c.meta["litlen_lens"][285] and any(t[0] == "match" and t[3][0] == 285 for t in c.blocks[0][1])
    c = case("hdist_30_uses_29")
    assert len(c.meta["dist_lens"]) == 30 and c.meta["dist_lens"][29] and sum(t[0] == "match" and t[4][0] == 29 for t in c.blocks[0][1]) >= 2
    c = case("shrinking_tables")
    assert len(c.meta["litlen_lens"][0]) == 286


@pytest.mark.parametrize("name", ["hclen_19", "hclen_4", "hclen_count_4", "hlit_287", "hlit_288", "hdist_31", "hdist_32"])
def test_header_fields_as_named(name):
    c = case(name)
    v = int.from_bytes(c.raw[:3], "little")
    assert (v >> 1) & 3 == 2
    hlit, hdist, hclen = ((v >> 3) & 31) + 257, ((v >> 8) & 31) + 1, ((v >> 13) & 15) + 4
    if "hclen" in c.meta:
        assert hclen == c.meta["hclen"]
    else:
        assert (hlit if name.startswith("hlit") else hdist) == int(name.split("_")[1])


def test_codes_longer_than_the_root_tables():
    c = case("litlen_15_bit_codes")
    lens = c.meta["litlen_lens"]
    assert max(lens) == 15 and kraft(lens) == 32768
    assert used_lengths(c, 0, lens, "litlen") >= {11, 12, 13, 14, 15}
    codes = canonical(lens)
    (ca, la), (cb, lb) = (codes[s] for s in c.meta["share"])
    assert la > 10 and lb > 10 and ca >> (la - 10) == cb >> (lb - 10)           # the first ten bits read are the same
    assert all(any(t == ("lit", s) for t in c.blocks[0][1]) for s in c.meta["share"])
    c = case("dist_15_bit_codes")
    d = c.meta["dist_lens"]
    assert d == list(range(1, 16)) + [15] and kraft(d) == 32768
    assert used_lengths(c, 0, d, "dist") >= {9, 10, 11, 12, 13, 14, 15}
    c = case("shrinking_tables")
    assert max(c.meta["litlen_lens"][0]) == 15 and used_lengths(c, 0, c.meta["litlen_lens"][0], "litlen") >= {11, 12, 13, 14, 15}


def test_both_spellings_of_length_258():
    a = [t for t in case("len258_as_284_31").blocks[0][1] if t[0] == "match"]
    b = [t for t in case("len258_as_285").blocks[0][1] if t[0] == "match"]
    assert a and all(t[1] == 258 and t[3] == (284, 31, 5) for t in a)
    assert b and all(t[1] == 258 and t[3] == (285, 0, 0) for t in b)
    assert case("len258_as_284_31").text == case("len258_as_285").text and case("len258_as_284_31").raw != case("len258_as_285").raw


def test_block_sequences():
    c = case("shrinking_tables")
    assert [k for k, _ in c.blocks] == ["huff"] * 4 and all(any(t[0] == "match" for t in body) and any(t[0] == "lit" for t in body) for _, body in c.blocks)
    nsym = [sum(1 for L in lens if L) for lens in c.meta["litlen_lens"]]
    assert nsym[0] > 256 and nsym[1] == 3 and 3 < nsym[2] < nsym[0]
    c = case("empty_blocks")
    assert [(k, len(body)) for k, body in c.blocks[:3]] == [("huff", 0), ("stored", 0), ("huff", 0)] and c.text
    c = case("stored_after_odd_bits")
    assert sorted(c.meta["bit_offsets"]) == list(range(8))
    assert [k for k, _ in c.blocks] == ["huff", "stored"] * 8
    assert len(case("stored_len_65535").blocks[0][1]) == 65535


# ---- the pipelined form -----------------------------------------------------------------------------------------------------------------
def test_runs_of_matches_fill_batches():
    for n in (8, 9, 16, 17):
        c = case("run_of_%d" % n)
        s = pipe_schedule(c.blocks)
        toks = c.blocks[0][1]
        assert all(t[0] == "match" for t in toks[600:]) and len(toks) == 601 + n
        assert s[(0, 600)]["path"] == "slow"
        assert [s[(0, 601 + i)]["path"] for i in range(n)] == ["fast"] * n
        assert [s[(0, 601 + i)]["slot"] for i in range(n)] == [i % 8 for i in range(n)]
        assert s[("eob", 0)] == dict(inflight=8, batch=n % 8)


def test_sources_at_the_head_of_the_batch_in_flight():
    for name, past, path in (("source_ends_at_batch_head", 0, "fast"), ("source_one_past_batch_head", 1, "slow")):
        c = case(name)
        s = pipe_schedule(c.blocks)
        r = s[c.meta["edge"]]
        assert r["head"] is not None and r["head"] == s[(0, 601)]["pos"] and s[(0, 608)]["slot"] == 7 and s[(0, 608)]["path"] == "fast"
        assert r["dist"] >= r["len"] and r["src0"] + r["len"] == r["head"] + past and r["path"] == path and r["slot"] == 0
    c = case("source_one_past_synced_in_batch")
    s = pipe_schedule(c.blocks)
    r, mate = s[c.meta["edge"]], s[(0, 601)]
    assert mate["path"] == "fast" and mate["slot"] == 0 and mate["pos"] == mate["synced"] == r["synced"] and r["head"] is None
    assert r["dist"] >= r["len"] and r["src0"] + r["len"] == r["synced"] + 1 and r["slot"] == 1 and r["path"] == "slow"
    assert c.text[r["synced"]] != POISON                                           # the byte a too-early load would miss is not the poison's
    c = case("source_is_previous_match")
    s = pipe_schedule(c.blocks)
    for bi, ti, slot in c.meta["edges"]:
        r, prev = s[(bi, ti)], s[(bi, ti - 1)]
        assert prev["path"] == "fast" and r["dist"] == r["len"] == prev["len"] and r["src0"] == prev["pos"]
        assert r["slot"] == slot and r["path"] == "slow" and prev["slot"] == (slot - 1) % 8


def test_lengths_around_64():
    c = case("len_64_65")
    s = pipe_schedule(c.blocks)
    seen = set()
    for ti, ln, d in c.meta["where"]:
        r = s[(0, ti)]
        assert (r["len"], r["dist"]) == (ln, d) and r["synced"] == r["pos"]          # right behind a drain: only the length decides
        assert r["path"] == ("fast" if ln <= 64 else "slow")
        seen.add((ln, d))
    assert seen == {(ln, d) for ln in (3, 63, 64, 65, 258) for d in (1, 2, 63, 64, 65, ln - 1, ln, ln + 1)}


def test_overlaps_block_ends_and_stored_sources():
    c = case("overlap_first_after_drain")
    r = pipe_schedule(c.blocks)[c.meta["edge"]]
    assert c.meta["edge"] == (1, 0) and r["dist"] < r["len"] <= 64 and r["pos"] == r["synced"] and r["path"] == "fast" and r["slot"] == 0
    c = case("overlap_after_literal")
    r = pipe_schedule(c.blocks)[c.meta["edge"]]
    assert c.blocks[1][1][0][0] == "lit" and r["dist"] < r["len"] <= 64 and r["pos"] == r["synced"] + 1 and r["path"] == "slow"
    c = case("eob_with_full_batch")
    s = pipe_schedule(c.blocks)
    assert s[("eob", 0)] == dict(inflight=8, batch=0)
    r = s[c.meta["edge"]]
    assert s[(0, 601)]["pos"] <= r["src0"] and r["src0"] + r["len"] <= r["pos"] == s[(0, 608)]["pos"] + s[(0, 608)]["len"] and r["slot"] == 0
    c = case("match_into_stored")
    text, starts = layout(c.blocks)
    s = pipe_schedule(c.blocks)
    for bi, ti in c.meta["edges"]:
        r = s[(bi, ti)]
        assert c.blocks[bi - 1][0] == "stored" and starts[bi - 1][0] <= r["src0"] and r["src0"] + min(r["len"], r["dist"]) <= starts[bi][0] == r["pos"]
    c = case("dist_equals_pos")
    _, starts = layout(c.blocks)
    assert [starts[0][ti] for ti in c.meta["edges"]] == [c.blocks[0][1][ti][2] for ti in c.meta["edges"]] == [1, 6, 600, 621]


def test_the_schedule_model_agrees_with_expand():
    for c in CASES:
        if c.group == "pipe":
            _, starts = layout(c.blocks)
            for key, r in pipe_schedule(c.blocks).items():
                if key[0] != "eob":
                    assert r["pos"] == starts[key[0]][key[1]], (c.name, key)


# ---- the LDS form's window --------------------------------------------------------------------------------------------------------------
WINDOW = [c for c in CASES if c.group == "window" and "kind" in c.meta]


@pytest.mark.parametrize("name", [c.name for c in WINDOW])
def test_window_case_sits_on_its_boundary(name):
    c = case(name)
    b, (bi, ti), kind = c.meta["b"], c.meta["edge"], c.meta["kind"]
    text, starts = layout(c.blocks)
    pos = starts[bi][ti]
    assert str(b) in name and len(text) > b
    if kind == "stored_crosses":
        assert c.blocks[bi][0] == "stored" and pos < b < pos + len(c.blocks[bi][1])
        return
    t = c.blocks[bi][1][ti]
    if kind == "literal_ends":
        assert t[0] == "lit" and pos + 1 == b
        return
    assert t[0] == "match"
    ln, d = t[1], t[2]
    if kind == "match_ends":
        assert pos + ln == b
    elif kind == "starts_dist_32768":
        assert pos == b == d == 32768
    else:
        assert pos < b < pos + ln and ln > 64
        assert {"straddles_dist_ge_len": d >= ln, "straddles_dist_1": d == 1, "straddles_dist_len_minus_1": d == ln - 1, "straddles_dist_32768": d == 32768,
                "straddles_dist_32768_minus_len_plus_1": d == 32768 - ln + 1}[kind]


def test_every_boundary_has_its_cases():
    for b in BOUNDARIES:
        kinds = {c.meta["kind"] for c in WINDOW if c.meta["b"] == b}
        want = {"literal_ends", "stored_crosses", "match_ends", "straddles_dist_ge_len", "straddles_dist_1", "straddles_dist_len_minus_1"}
        if b >= 32768:
            want.add("straddles_dist_32768_minus_len_plus_1")
        if b > 32768:
            want.add("straddles_dist_32768")            # (at 32768 itself the distance reaches in front of the text: starts_dist_32768 stands in)
        assert kinds >= want, (b, want - kinds)
    assert "starts_dist_32768" in {c.meta["kind"] for c in WINDOW}
    lens = {c.meta["text_len"]: len(c.text) for c in CASES if "text_len" in c.meta}
    assert all(k == v for k, v in lens.items()) and set(lens) >= {16383, 16384, 16385, 32768}
    assert {n % 16 for n in lens} >= {0, 1, 15} and {n % 16 for n in lens if n < 64} >= {0, 1, 15}


# ---- reject -----------------------------------------------------------------------------------------------------------------------------
def test_reject_cases_are_wrong_where_they_say():
    for name in ("litlen_oversubscribed", "dist_oversubscribed"):
        assert kraft(case(name).meta["lens"]) > 32768
    for name in ("litlen_incomplete", "dist_incomplete_two_codes"):
        lens = case(name).meta["lens"]
        assert kraft(lens) < 32768 and max(lens) > 1
    assert case("dist_pos_plus_1_at_0").meta["pos"] == 0 and case("dist_pos_plus_1_at_600").meta["pos"] == 600
    c = case("output_past_isize")
    assert int.from_bytes(c.member()[-4:], "little") == len(c.text) - 1 == c.out_cap() - 1
    for c in CASES:
        if not c.accept and not c.raw_valid:
            assert c.member()[-8:] == b"\0\0\0\0" + (65536).to_bytes(4, "little") and c.out_cap() == 65536


@pytest.mark.parametrize("name,member,status,text", HEADER_CASES, ids=[h[0] for h in HEADER_CASES])
def test_gzip_header_cases(name, member, status, text):
    if status == 0:
        assert zlib.decompress(member, 31) == text
    else:
        with pytest.raises(zlib.error):
            zlib.decompress(member, 31)
    if name == "member_of_17_bytes":
        assert len(member) == 17
    if name == "fextra_xlen_300":
        assert member[3] == 4 and int.from_bytes(member[10:12], "little") == 300
    if name == "all_five":
        assert member[3] == 0x1F
