"""The host side of the commands (gsearch_amd/commands.py) against LITERAL expectations: the table of `reformat`, the text of gsearch.matches and Rust's
two number formats. Every expected text below was written out by hand from the format strings of src/bin/reformat.rs:61-86 and src/matcher.rs:262-275;
the ANI digits are (1 + ln(2(1-d)/(2-d))/k) * 100 and (2(1-d)/(2-d))^(1/k) * 100 evaluated with 60 decimal digits and rounded to the nearest f64, then
printed with the shortest digits that round-trip."""
import io

import numpy as np
import pytest

from gsearch_amd.commands import matches_text, reformat, reformat_text, rust_display_f64, rust_upper_exp

from test_answer_format import _parse

K = 16


def _input_text():
    """gsearch.neighbors.txt as ReqAnswer.dump writes it: the requests of tests/golden/reqanswer_case.txt (query_A then query_D: names in order, query_D's
    rows out of distance order with a tie at 9.89995E-1, distance 0.00000E0, paths with directories, query_B with its header line alone) and then a
    request whose name sorts in front of both, with empty fasta_ids, distances 1.00000E-5 and twice 5.40000E-1; hand-made lines that are no answers"""
    import gsearch_amd as G
    seqdict, reqs, _, thr = _parse()
    seqdict = seqdict + [("/db/deep/er/T5.fasta", "", 20000), ("T6.fa", "", 123)]
    reqs = reqs + [(19, ("/data/q/sub/a first.fna", "", 777), [(5, np.float32(1e-5)), (6, np.float32(0.54)), (5, np.float32(0.54))])]
    buf = io.StringIO()
    for rank, item, nbs in reqs:
        G.ReqAnswer(rank, item, [G.Neighbour(i, float(d)) for i, d in nbs]).dump(seqdict, thr, buf)
    text = buf.getvalue() + "\nsome line of a log\n query_id:\tindented, so no answer line\nquery_id_is_not_all:\tx\n"
    for s in ("distance:\t0.00000E0\t", "distance:\t1.00000E-5\t", "distance:\t5.40000E-1\t", "answer_fasta_path\tT6.fa\t \t answer_seq_len:\t 123",
              "\n1\t/data/q/query_B.fna\tfasta_id:\tqB\tlength:\t1000\n"):
        assert s in text, s
    assert text.index("query_A.fna") < text.index("query_D.fna") < text.index("a first.fna")
    return text


ROWS = [    # (Query_Name, Distance, Neighbor_Fasta_name, Neighbor_Seq_Len, ANI model 1, ANI model 2), k = 16
    ("a first.fna", "0.00001", "T5.fasta", "20000", "99.99996874976563", "99.9999687497705"),
    ("a first.fna", "0.54", "T6.fa", "123", "97.1136372208794", "97.15489477088339"),
    ("a first.fna", "0.54", "T5.fasta", "20000", "97.1136372208794", "97.15489477088339"),
    ("query_A.fna", "0", "GCF_000003.fa", "5498578", "100", "100"),
    ("query_A.fna", "0.0000555556", "GCF_000001.fna.gz", "4641652", "99.99982638151587", "99.9998263816666"),
    ("query_A.fna", "0.6075", "GCF_000002.fna", "4631469", "96.41767341238105", "96.48107934063177"),
    ("query_A.fna", "0.98999", "GCF_000004.fna", "5594605", "75.49385164444176", "78.26564162632569"),
    ("query_D.fna", "0.000015", "GCF_000004.fna", "5594605", "99.99995312447265", "99.99995312448362"),
    ("query_D.fna", "0.123457", "GCF_000005.fna", "12", "99.5746650572528", "99.5755683252285"),
    ("query_D.fna", "0.25", "GCF_000003.fa", "5498578", "99.03655825107963", "99.041184482163"),
    ("query_D.fna", "0.989995", "GCF_000002.fna", "4631469", "75.49075992673467", "78.26322191103053"),
    ("query_D.fna", "0.989995", "GCF_000001.fna.gz", "4641652", "75.49075992673467", "78.26322191103053"),
]
HEADER = "Query_Name\tDistance\tNeighbor_Fasta_name\tNeighbor_Seq_Len\tANI\n"


def _table(model):
    return HEADER + "".join("\t".join(r[:4] + ((r[4], r[5])[model - 1] if model in (1, 2) else "Invalid Model",)) + "\n" for r in ROWS)


@pytest.mark.parametrize("model", [1, 2, 3])
def test_reformat_equals_literal_table(model, tmp_path):
    text = _input_text()
    assert reformat_text(K, model, text) == _table(model)
    (tmp_path / "in.txt").write_text(text, encoding="utf-8")
    assert reformat(K, model, tmp_path / "in.txt", tmp_path / "out.txt") == len(ROWS)
    assert (tmp_path / "out.txt").read_bytes() == _table(model).encode()


def test_reformat_columns():
    lines = reformat_text(K, 1, _input_text()).split("\n")
    cols = [ln.split("\t") for ln in lines[1:-1]]
    zero = [c for c in cols if c[0] == "query_A.fna" and c[2] == "GCF_000003.fa"]
    assert zero == [["query_A.fna", "0", "GCF_000003.fa", "5498578", "100"]]                  # distance 0: Distance `0`, ANI `100`
    assert ["a first.fna", "0.00001", "T5.fasta", "20000", "99.99996874976563"] in cols      # no exponent
    assert all(c[3].isdigit() for c in cols)                                                  # the length, not the label of reformat.rs:75
    assert all("E" not in c[1] and "e" not in c[1] for c in cols)


def test_reformat_refuses_a_distance_that_does_not_parse():
    bad = "query_id:\t/q/a.fna\tdistance:\tzero\tanswer_fasta_path\t/db/t.fna\t \t answer_seq_len:\t 5"
    with pytest.raises(ValueError) as e:
        reformat_text(K, 1, "\n0\t/q/a.fna\tfasta_id:\t\tlength:\t9\n" + bad)
    assert "zero" in str(e.value) and "line 3" in str(e.value)


RUST_DISPLAY = [(1e-7, "0.0000001"), (1e-5, "0.00001"), (1e16, "10000000000000000"), (1e15, "1000000000000000"), (0.1, "0.1"), (0.3, "0.3"), (0.54, "0.54"),
                (123456789.125, "123456789.125"), (97.11363636363637, "97.11363636363637"), (99.99965277170676, "99.99965277170676"),
                (1.0 / 3.0, "0.3333333333333333"), (2.0 / 3.0, "0.6666666666666666"), (100.0, "100"), (0.0, "0"), (-0.0, "-0"), (-2.5e-10, "-0.00000000025"),
                (1e21, "1000000000000000000000"), (5e-324, "0." + "0" * 323 + "5"), (float("inf"), "inf"), (float("-inf"), "-inf"), (float("nan"), "NaN")]


@pytest.mark.parametrize("x,want", RUST_DISPLAY)
def test_rust_display_of_f64(x, want):
    assert rust_display_f64(x) == want
    if x == x and abs(x) != float("inf"):
        assert float(want) == x                                                               # the digits round-trip


RUST_EXP3 = [(0.54, "5.400E-1"), (1.0, "1.000E0"), (0.0, "0.000E0"), (-0.0, "-0.000E0"), (0.98999, "9.900E-1"), (3.75e-6, "3.750E-6"), (0.00099995, "9.999E-4"),
             (0.99996, "1.000E0"), (1e-10, "1.000E-10"), (12345.678, "1.235E4"), (float("inf"), "inf"), (float("nan"), "NaN")]


@pytest.mark.parametrize("x,want", RUST_EXP3)
def test_rust_upper_exp_of_f32(x, want):
    assert rust_upper_exp(np.float32(x), 3) == want


def test_rust_upper_exp_five_digits_is_the_answer_format():
    from gsearch_amd.api import _rust_5e
    for x, want in ((0.0, "0.00000E0"), (np.float32(1e-5), "1.00000E-5"), (np.float32(0.6075), "6.07500E-1"), (1.0, "1.00000E0")):
        assert rust_upper_exp(x, 5) == want == _rust_5e(x)


def test_matches_text_equals_literal():
    """a target hit twice (/db/A.fna through ids 0 and 7: 0.5 * 0.5), a tie at 2.500E-1 (A before B: first appearance), six targets of which five are
    listed (C, only at the threshold or above, is the sixth of r1 and is listed for r2 with merit 1.000E0), a second hit AT the threshold that leaves the
    product alone, a request with no neighbour"""
    import gsearch_amd as G
    seqdict = [("/db/A.fna", "", 10), ("/db/B.fna", "", 11), ("/db/C.fna", "", 12), ("/db/D.fna", "", 13), ("/db/E.fna", "", 14), ("/db/F.fna", "", 15),
               ("/db/G.fna", "", 16), ("/db/A.fna", "", 17)]
    f = np.float32

    def nb(*pairs):
        return [G.Neighbour(i, float(f(d))) for i, d in pairs]
    requests = [("/q/r1.fna", nb((0, 0.5), (1, 0.25), (7, 0.5), (2, 0.995), (3, 0.1), (4, 0.75), (5, 0.9))),
                ("/q/r2.fna", nb((2, 0.995), (0, 0.3), (7, 0.99))),
                ("/q/r3.fna", [])]
    want = ("\n\n request genome : /q/r1.fna"
            "\n\t matched genome /db/D.fna  merit : 1.000E-1"
            "\n\t matched genome /db/A.fna  merit : 2.500E-1"
            "\n\t matched genome /db/B.fna  merit : 2.500E-1"
            "\n\t matched genome /db/E.fna  merit : 7.500E-1"
            "\n\t matched genome /db/F.fna  merit : 9.000E-1"
            "\n\n request genome : /q/r2.fna"
            "\n\t matched genome /db/A.fna  merit : 3.000E-1"
            "\n\t matched genome /db/C.fna  merit : 1.000E0"
            "\n\n request genome : /q/r3.fna")
    assert matches_text(requests, seqdict, 0.99) == want
