"""gs_sketch_files with both of its pipelines at work (sketch_files_all in gs_files.hip): the .gz files of a call are dealt between the host decoders,
which claim them from the front of the list, and the device inflater, which claims them from the back (GzDeal, gs_gzdeal.hpp; its claim rule alone:
test_gzdeal_cpu.py). Under the rule's priors the device side declines every list of fewer than some 1250 members, so GS_GZIP_DEAL_SHARE fixes its share
here and the tests can say who did what: both sides running groups until they meet, a device group cut short, the device side declining, awkward
members where the device claims, a group over its byte budget (GS_GZIP_GROUP_MB) and the compressed H2D copy in pieces (GS_COPY_CHUNK_MB).

Every case: signatures (bitwise), records and bases per file against the oracle fed with the records the test wrote (ingest_deal_cases.py), so a file
sketched by nobody or put in another file's row fails; then the same three against one run with every .gz through the host decoders."""
import gzip

import numpy as np
import pytest

import helpers as H
import ingest_deal_cases as D

pytestmark = pytest.mark.gpu

P, N = D.P, D.N_DEALT
N_SHORT = 1400             # (b): the host pipeline's up-front claim is 12 * 64 there; 300 members must be left when the device side claims
KNOBS = ("GS_GZIP_DEVICE", "GS_GZIP_DEVICE_ONLY", "GS_GZIP_DEAL_SHARE", "GS_GZIP_GROUP", "GS_GZIP_GROUP_MB", "GS_COPY_CHUNK_MB", "GS_INGEST_LOOKAHEAD")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return D.Corpus(tmp_path_factory.mktemp("ingest_deal"), N_SHORT)


@pytest.fixture(scope="module")
def reference(corpus):
    return D.Reference(corpus.entries)


@pytest.fixture(scope="module")
def host_runs():
    """the second reference: one GS_GZIP_DEVICE=0 run per (list, block, pio), shared by the tests that use the same list"""
    return {}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _sketch(monkeypatch, paths, env, block=False, pio=0, threads=0):
    import gsearch_amd as G
    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        return G.sketcher_for(G.SeqSketcherParams(D.K, D.M, D.ALGO)).sketch_files(paths, block=block, pio=pio, threads=threads)


def _host_run(host_runs, monkeypatch, paths, block, pio):
    key = (tuple(paths), bool(block), pio)
    if key not in host_runs:
        host_runs[key] = _sketch(monkeypatch, paths, {"GS_GZIP_DEVICE": "0"}, block=block, pio=pio)
    return host_runs[key]


def _same_rows(tag, got, want):
    for what, g, w in zip(("signatures", "records", "bases"), got[:3], want[:3]):
        g, w = _bits(np.asarray(g)), _bits(np.asarray(w))
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, what, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (tag, what, "%d rows differ, the first at" % len(bad), bad[:12].tolist())


def _check(tag, got, paths, rows, host):
    st = got[3]
    print("%s: %d files (%d .gz): inflated on the device %d, handed back %d, wall %.3f s" % (
        tag, len(paths), sum(p.endswith(".gz") for p in paths), st["gz_members_inflated_on_device"], st["gz_members_handed_back_to_host"], st["wall_s"]))
    _same_rows((tag, "against the oracle"), got, rows)
    _same_rows((tag, "host decoders against the oracle"), host, rows)
    _same_rows((tag, "against the host decoders"), got, host)
    return st["gz_members_inflated_on_device"], st["gz_members_handed_back_to_host"]


def _n_gz(paths):
    return sum(p.endswith(".gz") for p in paths)


@pytest.mark.parametrize("block", [False, True])
def test_both_pipelines_run_groups_until_they_meet(gpu_ctx, monkeypatch, corpus, reference, host_runs, block):
    """(a) N .gz files in groups of P, the device side offered P or more at every claim; plain, .bz2 and .xz files among them, their number no multiple
    of P: one host group holds both files that need no claim and dealt ones"""
    order = corpus.dealt(N)
    paths = corpus.paths(order)
    assert _n_gz(paths) == N >= 20 * P and (len(paths) - N) % P != 0
    got = _sketch(monkeypatch, paths, {"GS_GZIP_DEAL_SHARE": str(max(P, 128))}, block=block, pio=P, threads=4)
    dev, back = _check("both pipelines, block=%s" % block, got, paths, reference.rows(order, block), _host_run(host_runs, monkeypatch, paths, block, P))
    assert 0 < dev < N and back == 0, (dev, back)


def test_one_short_device_group(gpu_ctx, monkeypatch, corpus, reference, host_runs):
    """(b) the default group sizes: the device side asks for one group of all the members, is offered 300 and takes them; the host side does the rest"""
    order = corpus.gz[:N_SHORT]
    paths = corpus.paths(order)
    assert _n_gz(paths) == len(paths) == N_SHORT >= 12 * 64 + 300
    got = _sketch(monkeypatch, paths, {"GS_GZIP_DEAL_SHARE": "300"})
    dev, back = _check("short device group", got, paths, reference.rows(order, False), _host_run(host_runs, monkeypatch, paths, False, 0))
    assert dev == 300 - back and back == 0, (dev, back)


def test_device_side_declines(gpu_ctx, monkeypatch, corpus, reference, host_runs):
    """(c) a share below the smallest claim, and the priors at 83 files (no rate is measured before 256 files are done): the host side does every file"""
    order = corpus.dealt(N)
    paths = corpus.paths(order)
    got = _sketch(monkeypatch, paths, {"GS_GZIP_DEAL_SHARE": "127"}, pio=P, threads=4)
    dev, back = _check("share 127", got, paths, reference.rows(order, False), _host_run(host_runs, monkeypatch, paths, False, P))
    assert (dev, back) == (0, 0)
    order = corpus.gz[:83]
    paths = corpus.paths(order)
    got = _sketch(monkeypatch, paths, {}, pio=P, threads=4)
    dev, back = _check("priors, 83 files", got, paths, reference.rows(order, False), _host_run(host_runs, monkeypatch, paths, False, P))
    assert (dev, back) == (0, 0)


def _outcome(monkeypatch, paths, env):
    import gsearch_amd as G
    try:
        return ("rows",) + tuple(_sketch(monkeypatch, paths, env, pio=P, threads=4)[:3])
    except G.GsError as e:
        return ("error", e.code)


def test_awkward_members_where_the_device_claims(gpu_ctx, monkeypatch, corpus, reference, host_runs):
    """(d) among the last P .gz files, the device side's first group: a two-member file (handed back), a member with FNAME, a member of empty text, a
    bgzip file, CRLF, no final newline, a `capsid` record. Then the last member with a wrong stored CRC-32: the call ends as it does with the host
    decoders alone - the device path returns no sketch that they refuse"""
    order = corpus.dealt_awkward_back(N)
    paths = corpus.paths(order)
    assert _n_gz(paths) == N and all(corpus.entries[corpus.awkward[k]].path in paths[-2 * P:] for k in D.AWKWARD)
    got = _sketch(monkeypatch, paths, {"GS_GZIP_DEAL_SHARE": "128"}, pio=P, threads=4)
    dev, back = _check("awkward members", got, paths, reference.rows(order, False), _host_run(host_runs, monkeypatch, paths, False, P))
    assert back == 1 and 0 < dev < N, (dev, back)
    order = corpus.dealt_awkward_back(N, bad_crc=True)
    paths = corpus.paths(order)
    assert paths[-1] == corpus.entries[corpus.bad_crc].path
    want = _outcome(monkeypatch, paths, {"GS_GZIP_DEVICE": "0"})
    have = _outcome(monkeypatch, paths, {"GS_GZIP_DEAL_SHARE": "128"})
    print("wrong CRC-32: host decoders %s, dealt %s" % (want[:2] if want[0] == "error" else want[0], have[:2] if have[0] == "error" else have[0]))
    assert have[0] == want[0], (have[:2], want[:2])
    if want[0] == "error":
        assert have[1] == want[1]
    else:
        _same_rows("wrong CRC-32, against the host decoders", have[1:], want[1:])


@pytest.fixture(scope="module")
def large_files(tmp_path_factory):
    """the two shapes whose point is bytes, not files: (e) 24 members of 150 to 200 KB of text and a bgzip file of a low-entropy text above 2 MiB;
    (f) 16 members of 400 KB of random DNA and a two-member file"""
    wd = tmp_path_factory.mktemp("ingest_deal_large")
    rng = np.random.default_rng(24)
    entries, texts, blobs = [], [], []

    def add(name, blob, text, records):
        (wd / name).write_bytes(blob)
        entries.append(D.Entry(wd / name, [s for _, s in records]))
        texts.append(text); blobs.append(blob)
        return len(entries) - 1
    spill = []
    for i in range(24):
        recs = D._records(rng, i, 150_000, 200_000)
        t = D.fasta(recs, 60 + i % 11)
        spill.append(add("s%02d.fna.gz" % i, D.gz(t, 1 + i % 9), t, recs))
    recs = [(b"low entropy", b"ACGTTGCAAGGCTTAACCGGATATCGCGTTAAGGCCTTGGAACCTTGAGCTAGCTAGGAT" * 37000)]
    t = D.fasta(recs, 60)
    spill.append(add("s_low.fna.gz", H.bgzf_bytes(t), t, recs))
    pieces = []
    recs = D._records(rng, 1, 2000, 3000)
    t = D.fasta(recs, 60)
    pieces.append(add("c_two.fna.gz", D.gz(t[:len(t) // 2]) + D.gz(t[len(t) // 2:]), t, recs))
    for i in range(16):
        recs = D._records(rng, 3 * i, 400_000, 400_000)
        t = D.fasta(recs, 60)
        pieces.append(add("c%02d.fna.gz" % i, gzip.compress(t, 6), t, recs))
    return dict(entries=entries, texts=texts, blobs=blobs, spill=spill, pieces=pieces, ref=D.Reference(entries))


def test_group_over_its_byte_budget(gpu_ctx, monkeypatch, large_files, host_runs):
    """(e) fewer than 64 .gz files: all of them to the device pipeline, in groups of 8 under a budget of 1 MiB of text. A member that does not fit
    stays with that pipeline's host decoders (a mixed group: their texts, then the device's); the bgzip file is admitted on the guess of four times
    its size and handed back when its members add up to more than twice the budget"""
    L = large_files
    order, texts, blobs = L["spill"], L["texts"], L["blobs"]
    paths = [L["entries"][i].path for i in order]
    budget, pio = 1 << 20, 8
    low = order[-1]
    assert len(texts[low]) > 2 * budget and len(blobs[low]) < (256 << 10) and len(order) < 64
    # what the budget admits: the device pipeline's list is the .gz files from the back, in groups of pio; a member is the device's while the texts
    # admitted before it in its group (each rounded up to 64 bytes) and its own stay within the budget
    dev_order = order[::-1]
    admitted = mixed_groups = 0
    for g in range(0, len(dev_order), pio):
        used, mixed = 0, [0, 0]
        for i in dev_order[g:g + pio]:
            if i == low:
                continue
            fits = used + len(texts[i]) <= budget
            mixed[fits] += 1
            if fits:
                used += (len(texts[i]) + 63) // 64 * 64
        admitted += mixed[1]
        mixed_groups += mixed[0] > 0 and mixed[1] > 0
    assert mixed_groups >= 2
    got = _sketch(monkeypatch, paths, {"GS_GZIP_GROUP_MB": "1"}, pio=pio)
    dev, back = _check("budget spill", got, paths, L["ref"].rows(order, False), _host_run(host_runs, monkeypatch, paths, False, pio))
    assert 0 < dev < len(order), (dev, back)
    assert back >= 1, back
    assert dev == admitted, (dev, admitted)


def test_compressed_copy_in_pieces(gpu_ctx, monkeypatch, large_files, host_runs):
    """(f) one group whose device members hold more than a piece of compressed bytes: the H2D copy loop goes round more than once"""
    L = large_files
    order = L["pieces"]
    paths = [L["entries"][i].path for i in order]
    assert sum(len(L["blobs"][i]) for i in order[1:]) > (1 << 20) and sum(len(L["texts"][i]) for i in order) < (8 << 20)
    got = _sketch(monkeypatch, paths, {"GS_COPY_CHUNK_MB": "1", "GS_GZIP_GROUP_MB": "8"}, pio=32)
    dev, back = _check("copy in pieces", got, paths, L["ref"].rows(order, False), _host_run(host_runs, monkeypatch, paths, False, 32))
    assert (dev, back) == (16, 1)
