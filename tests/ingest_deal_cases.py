"""Inputs of the tests that run gs_sketch_files with BOTH of its pipelines at work (test_gpu_ingest_deal.py, and one case of test_gpu_stale_scratch.py):
many tiny FASTA files - the workload is their number, not their size - written once, with the records each holds kept beside them, so that the oracle
is fed with what the test wrote and not with what the library read back. A file is an Entry; a call's input is a list of entry numbers."""
import bz2
import gzip
import io
import lzma
import zlib

import numpy as np

import helpers as H
import oracle_lib as O

K, M, ALGO = 21, 128, "optdens"
P = 16                     # files per group (--pio) of the dealt shapes: the host pipeline claims 12 * P members up front (its look-ahead)
N_DEALT = 640              # .gz files of the smallest dealt shape: 20 * P, so the device side finds full groups whichever thread claims first
N_OTHER = 37               # plain / .bz2 / .xz files beside them: no multiple of P, so one host group holds both unclaimed and dealt files
AWKWARD = ("two_members", "fname", "empty_text", "bgzf", "crlf", "no_final_newline", "capsid")


class Entry:
    def __init__(self, path, recs):
        self.path, self.recs = str(path), recs        # recs: the sequences of the records a reader keeps, in file order, without line ends


def gz(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def fasta(records, width, nl=b"\n", final=True):
    out = []
    for name, s in records:
        out.append(b">" + name + nl)
        out += [s[o:o + width] + nl for o in range(0, len(s), width)]
    t = b"".join(out)
    return t if final or not t else t[:-len(nl)]


def _records(rng, i, lo=300, hi=3000):
    """one to three records of lo..hi bases in all"""
    n = int(rng.integers(lo, hi + 1))
    s = H.dna_ascii(H.rand_dna(rng, n))
    cuts = sorted(int(x) for x in rng.choice(np.arange(40, n - 40, 25), i % 3, replace=False))
    return [(b"g%d_%d some text" % (i, j), s[a:b]) for j, (a, b) in enumerate(zip([0] + cuts, cuts + [n]))]


class Corpus:
    """n_gz single-member .gz files, n_other plain / .bz2 / .xz files, the awkward members of AWKWARD and one member with a wrong stored CRC-32"""
    def __init__(self, wd, n_gz, n_other=N_OTHER, seed=640):
        rng = np.random.default_rng(seed)
        self.entries, self.gz, self.other, self.awkward = [], [], [], {}

        def add(name, blob, records):
            p = wd / name
            p.write_bytes(blob)
            self.entries.append(Entry(p, [s for h, s in records if b"capsid" not in h]))
            return len(self.entries) - 1
        for i in range(n_gz):
            recs = _records(rng, i)
            self.gz.append(add("z%04d.fna.gz" % i, gz(fasta(recs, 60 + i % 20), 1 + i % 9), recs))
        for i in range(n_other):
            recs = _records(rng, 5000 + i)
            t = fasta(recs, 70)
            name, blob = ("o%02d.fa.bz2" % i, bz2.compress(t)) if i % 9 == 4 else ("o%02d.fasta.xz" % i, lzma.compress(t)) if i % 12 == 7 else ("o%02d.fna" % i, t)
            self.other.append(add(name, blob, recs))
        r = {k: _records(rng, 7001 + 3 * j) for j, k in enumerate(AWKWARD)}            # (three records each)
        t = fasta(r["two_members"], 60)
        self.awkward["two_members"] = add("a_two.fna.gz", gz(t[:len(t) // 2]) + gz(t[len(t) // 2:]), r["two_members"])
        bio = io.BytesIO()
        with gzip.GzipFile(filename="a_member_with_a_name.fna", mode="wb", fileobj=bio, mtime=1) as f:
            f.write(fasta(r["fname"], 60))
        self.awkward["fname"] = add("a_fname.fna.gz", bio.getvalue(), r["fname"])
        self.awkward["empty_text"] = add("a_empty.fna.gz", gz(b""), [])
        self.awkward["bgzf"] = add("a_bgzf.fna.gz", H.bgzf_bytes(fasta(r["bgzf"], 60), block=700), r["bgzf"])
        self.awkward["crlf"] = add("a_crlf.fna.gz", gz(fasta(r["crlf"], 61, b"\r\n")), r["crlf"])
        self.awkward["no_final_newline"] = add("a_nofinal.fna.gz", gz(fasta(r["no_final_newline"], 59, final=False)), r["no_final_newline"])
        cap = r["capsid"]
        assert len(cap) == 3
        cap[1] = (b"x phage capsid protein", cap[1][1])
        self.awkward["capsid"] = add("a_capsid.fna.gz", gz(fasta(cap, 60)), cap)
        # the last ordinary member of the smallest dealt shape once more, a byte of its stored CRC-32 flipped (the trailer is CRC-32, ISIZE)
        twin = self.bad_crc_twin = self.gz[min(n_gz, N_DEALT) - 1]
        blob = bytearray(open(self.entries[twin].path, "rb").read())
        blob[-6] ^= 0xFF
        self.bad_crc = add("a_badcrc.fna.gz", bytes(blob), [(b"", s) for s in self.entries[twin].recs])

    def dealt(self, n_gz=None):
        """n_gz ordinary .gz files with the other files spread among them"""
        g = self.gz[:n_gz or len(self.gz)]
        step = len(g) // len(self.other)
        order = []
        for j, o in enumerate(self.other):
            order += g[j * step:(j + 1) * step] + [o]
        return order + g[len(self.other) * step:]

    def dealt_awkward_back(self, n_gz, bad_crc=False):
        """the same list, the awkward members among its last P .gz files (what the device side claims first)"""
        order = self.dealt(n_gz)
        back = [at for at, i in enumerate(order) if self.entries[i].path.endswith(".gz")][-P:]
        for j, k in enumerate(AWKWARD):
            order[back[-2 - 2 * j]] = self.awkward[k]
        if bad_crc:
            assert order[-1] == self.bad_crc_twin
            order[-1] = self.bad_crc
        return order

    def paths(self, order):
        return [self.entries[i].path for i in order]


class Reference:
    """the oracle's signatures of every entry, by sequence and with --block, and the records and bases a reader keeps: computed once"""
    def __init__(self, entries, nthreads=8):
        import os
        nt = min(nthreads, os.cpu_count() or 1)
        recs = [r for e in entries for r in e.recs]
        goff = np.cumsum([0] + [len(e.recs) for e in entries]).astype(np.uint64)
        seq, rs, rl = O.pack_dna(recs)
        self.nrec = np.array([len(e.recs) for e in entries], np.uint64)
        self.nsym = np.array([int(rl[int(goff[i]):int(goff[i + 1])].sum()) for i in range(len(entries))], np.uint64)
        self.sig = {False: O.sketch_batch(O.params(K, M, ALGO, "dna"), seq, rs, rl, goff, nthreads=nt)}
        joined = [b"".join(e.recs) for e in entries]
        seq, rs, rl = O.pack_dna(joined)
        self.sig[True] = O.sketch_batch(O.params(K, M, ALGO, "dna"), seq, rs, rl, np.arange(len(joined) + 1, dtype=np.uint64), nthreads=nt)

    def rows(self, order, block):
        ix = np.asarray(order, np.int64)
        return self.sig[bool(block)][ix], self.nrec[ix], self.nsym[ix]
