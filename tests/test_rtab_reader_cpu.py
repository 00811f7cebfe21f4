"""--pres input through the native Rtab reader with the host tokeniser (pyseer_amd/input.py NativeRtabReader(engine=None) /
iter_packed_blocks_rtab_native; csrc/rtab_reader.cpp) against the line-by-line reader (read_variant / iter_packed_blocks, the reference's
pyseer/input.py:301-454) over the same file: names, af, missing, k, status, patterns, sample lists, last_k, the stderr lines in order, and for a
malformed table the same ValueError after the same blocks.  Runs without a GPU."""
import os

import numpy as np
import pandas as pd
import pytest

from pyseer_amd.input import (RTAB_ERRORS, NativeRtabReader, RtabDuplicateSample, iter_call_blocks_rtab_native, iter_packed_blocks,
                              iter_packed_blocks_rtab_native, open_variant_file, read_variant)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WINDOWS = [(0.0, 1.0, 1.0), (0.1, 0.9, 0.05)]             # (min_af, max_af, max_missing): everything kept; every status of a block met


def _series(names):
    return pd.Series(np.zeros(len(names)), index=[str(x) for x in names])


def _same(a, b):
    """equal arrays, NaN equal to NaN, same dtype; None equal to None"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def _drain(gen, capsys):
    capsys.readouterr()
    blocks, error = [], None
    try:
        for blk in gen:
            blocks.append(blk)
    except ValueError as e:
        error = str(e)
    return blocks, error, capsys.readouterr().err


def _python_blocks(path, p, window, bs):
    infile, order = open_variant_file("Rtab", path)
    return iter_packed_blocks(p, "Rtab", infile, set(p.index), order, window[0], window[1], window[2], False, bs)


def _native_blocks(path, p, window, bs):
    return iter_packed_blocks_rtab_native(p, path, None, window[0], window[1], window[2], bs)


def _assert_same_stream(path, p, capsys, bs=7, windows=WINDOWS):
    """both block streams over the file: the same blocks, the same error (or none), the same stderr; returns (blocks, error) of the last window"""
    for window in windows:
        want, want_err, want_said = _drain(_python_blocks(path, p, window, bs), capsys)
        got, got_err, got_said = _drain(_native_blocks(path, p, window, bs), capsys)
        assert got_err == want_err
        assert got_said == want_said
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert list(g.names) == list(w.names)
            assert _same(np.array(g.afs, dtype=float), np.array(w.afs, dtype=float))
            assert list(g.status) == list(w.status) and list(g.row_of) == list(w.row_of)
            assert list(g.patterns) == list(w.patterns)
            assert [list(x) for x in g.kstrains] == [list(x) for x in w.kstrains]
            assert [list(x) for x in g.nkstrains] == [list(x) for x in w.nkstrains]
            assert all(_same(x, y) for x, y in zip(g.ks, w.ks))
            assert _same(g.last_k, w.last_k)
            assert g.bits.shape == w.bits.shape and (g.bits == w.bits).all()
    return got, got_err


def _assert_same_rows(path, p, capsys):
    """NativeRtabReader's raw rows against read_variant's tuples, line by line: name, af, missing, k; the status where read_variant raises"""
    infile, order = open_variant_file("Rtab", path)
    n = len(p)
    reader = NativeRtabReader(path, list(p.index), None, 5)
    assert reader.columns == order
    rows = 0
    try:
        for rb in reader.raw_blocks():
            assert not rb["skip"].any()
            names = [rb["blob"][rb["off"][i]:rb["off"][i + 1]].decode() for i in range(len(rb["status"]))]
            dp = np.unpackbits(rb["present"], axis=1, bitorder="little")
            dm = np.unpackbits(rb["missing"], axis=1, bitorder="little")
            assert not dp[:, n:].any() and not dm[:, n:].any() and not (dp & dm).any()
            for i, name in enumerate(names):
                try:
                    eof, k, var_name, ks, nks, af, missing = read_variant(infile, p, "Rtab", False, None, False, set(p.index), order)
                except ValueError as e:
                    assert RTAB_ERRORS[int(rb["status"][i])] == str(e)
                    assert not rb["present"][i].any() and not rb["missing"][i].any() and rb["n_present"][i] == 0 and rb["n_missing"][i] == 0
                    rows += 1
                    continue
                assert not eof and rb["status"][i] == 0 and name == var_name
                assert (rb["n_present"][i], rb["n_missing"][i]) == (dp[i].sum(), dm[i].sum())
                assert float(rb["n_present"][i] + rb["n_missing"][i]) / n == af and float(rb["n_missing"][i]) / n == missing
                want = np.asarray(k, dtype=float)
                assert ((dp[i, :n] == 1) == (want == 1)).all() and ((dm[i, :n] == 1) == np.isnan(want)).all()
                rows += 1
        assert read_variant(infile, p, "Rtab", False, None, False, set(p.index), order)[0] is True
        assert reader.stats()["rows"] == rows and reader.stats()["launches"] == 0
    finally:
        reader.close()
    capsys.readouterr()
    return rows


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_kmers120_of_the_command_line_fixtures(capsys):
    p = pd.read_csv(os.path.join(GOLD, "cli", "subset.pheno"), index_col=0, sep="\t")["binary"]
    p.index = p.index.astype(str)
    path = os.path.join(GOLD, "cli", "kmers120.Rtab")
    assert _assert_same_rows(path, p, capsys) == 120
    for bs in (7, 3000):
        blocks, error = _assert_same_stream(path, p, capsys, bs=bs)
        assert error is None and sum(len(b) for b in blocks) == 120


@pytest.mark.parametrize("name", ["ref_missing_binary", "ref_missing_continuous"])
def test_missing_rtab_of_the_elastic_net_fixtures(name, capsys):
    g = np.load(os.path.join(GOLD, "enet", name + ".npz"))
    p = pd.Series(g["y"], index=[str(s) for s in g["samples"]])
    path = os.path.join(GOLD, "enet", "missing.Rtab")
    assert _assert_same_rows(path, p, capsys) == int(g["loaded"])
    blocks, error = _assert_same_stream(path, p, capsys, bs=64)
    assert error is None and any(2 in b.status for b in blocks)           # rows with missing calls take their dense k along
    n = sum(len(cb) for cb in iter_call_blocks_rtab_native(p, path, None, 64))
    assert n == int(g["loaded"])


# ---- generated tables --------------------------------------------------------------------------------------------------------------------
CALLS = ["0", "1", ".", ""]


def _table(n_pheno, rng, eol=b"\n", final_eol=True, tail=b"", rows=24):
    """(text, phenotype names): n_pheno phenotype samples in another order than the columns, one of them without a column, three columns
    without a phenotype; every call in first, middle and last position (the last never empty: the strip would take it), adjacent empty calls,
    a name with spaces and an empty name; `tail` (trailing spaces, 0x1c) is appended to every other line."""
    pheno = ["s%d" % i for i in range(n_pheno)]
    cols = pheno[:-1] + ["x1", "x2", "x3"]
    cols = [cols[i] for i in rng.permutation(len(cols))]
    nc = len(cols)
    lines = [b"Gene\t" + "\t".join(cols).encode()]
    forced = [(0, c) for c in CALLS] + [(nc // 2, c) for c in CALLS] + [(nc - 1, c) for c in CALLS[:3]]
    for r in range(rows):
        calls = [CALLS[i] for i in rng.choice(4, size=nc, p=[0.45, 0.35, 0.1, 0.1])]
        if r < len(forced):
            calls[forced[r][0]] = forced[r][1]
        if r == len(forced) and nc >= 4:
            calls[1] = calls[2] = ""                                      # adjacent empty calls
        if r == len(forced) + 1:
            calls = ["0"] * nc                                            # nobody carries it: "No observations of ..."
        if calls[-1] == "":
            calls[-1] = "1"
        name = {3: "a gene with spaces", 5: ""}.get(r, "g%d" % r)
        lines.append(("\t".join([name] + calls)).encode() + (tail if r % 2 else b""))
    text = eol.join(lines) + (eol if final_eol else b"")
    return text, [pheno[i] for i in rng.permutation(n_pheno)]


@pytest.mark.parametrize("n_pheno", [2, 50, 64, 65, 130])
@pytest.mark.parametrize("eol,final_eol,tail", [(b"\n", True, b""), (b"\r\n", True, b"  "), (b"\r", True, b"\x1c"), (b"\n", False, b" \x1c "),
                                                (b"\r\n", False, b"")])
def test_generated_tables(n_pheno, eol, final_eol, tail, tmp_path, capsys):
    rng = np.random.default_rng(1000 * n_pheno + len(eol) + 2 * final_eol + len(tail))
    text, pheno = _table(n_pheno, rng, eol, final_eol, tail)
    path = str(tmp_path / "t.Rtab")
    open(path, "wb").write(text)
    p = _series(pheno)
    assert _assert_same_rows(path, p, capsys) == 24
    blocks, error = _assert_same_stream(path, p, capsys)
    assert error is None and sum(len(b) for b in blocks) == 24
    names = [x for b in blocks for x in b.names]
    assert "a gene with spaces" in names and "" in names


def test_header_with_an_empty_first_cell_loses_its_first_sample(tmp_path, capsys):
    """header.rstrip().split()[1:] drops the first token whatever it is: with an empty first cell that is a sample, and every row mismatches"""
    path = str(tmp_path / "t.Rtab")
    open(path, "wb").write(b"\ta\tb\tc\ng1\t1\t0\t1\n")
    p = _series(["a", "b", "c"])
    assert NativeRtabReader(path, list(p.index), None).columns == ["b", "c"]
    blocks, error = _assert_same_stream(path, p, capsys)
    assert blocks == [] and error == RTAB_ERRORS[2]


# ---- malformed tables --------------------------------------------------------------------------------------------------------------------
HEAD = b"Gene\tc\tx\ta\tb\n"                                # x has no phenotype
GOOD = [b"g%d\t1\t0\t.\t1" % i for i in range(9)] + [b"none\t0\t1\t0\t0"]            # (none: "No observations", said before the error)
MALFORMED = [
    ("no tab", b"justaname", 1),
    ("empty line", b"", 1),
    ("only white space", b" \t \t", 1),
    ("short row", b"bad\t1\t0\t1", 2),
    ("long row", b"bad\t1\t0\t1\t0\t0", 2),
    ("trailing empty call is stripped", b"bad\t1\t0\t1\t", 2),
    ("a digit that is no call", b"bad\t1\t0\t2\t1", 3),
    ("two bytes", b"bad\t1\t0\t10\t1", 3),
    ("a space inside", b"bad\t1\t0\t1 \t1", 3),
    ("first call", b"bad\tx\t0\t1\t1", 3),
    ("last call", b"bad\t1\t0\t1\t11", 3),
    ("a column without phenotype", b"bad\t1\tNA\t1\t1", 3),
    ("short and not binary", b"bad\t1\t7\t1", 2),
]


@pytest.mark.parametrize("what,line,status", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_a_malformed_line_raises_what_the_reference_raises(what, line, status, tmp_path, capsys):
    path = str(tmp_path / "t.Rtab")
    open(path, "wb").write(HEAD + b"\n".join(GOOD + [line] + GOOD[:2]) + b"\n")
    p = _series(["a", "b", "c", "d"])
    _assert_same_rows(path, p, capsys)
    blocks, error = _assert_same_stream(path, p, capsys, bs=4)
    assert error == RTAB_ERRORS[status] and [len(b) for b in blocks] == [4, 4]
    # the call-block stream: the lines before the malformed one, then the same error
    seen = 0
    with pytest.raises(ValueError, match=RTAB_ERRORS[status].replace("?", r"\?")):
        for cb in iter_call_blocks_rtab_native(p, path, None, 4):
            seen += len(cb)
    assert seen == 10


# ---- a header that names a phenotype sample twice --------------------------------------------------------------------------------------
def test_duplicated_sample_column_falls_back_to_the_line_reader(tmp_path, capsys):
    path = str(tmp_path / "t.Rtab")
    rows = [b"g%d\t%s" % (i, b"\t".join(c)) for i, c in enumerate([(b"1", b"0", b"0", b"1"), (b"0", b"1", b"1", b"0"), (b".", b"0", b"1", b"0"),
                                                                    (b"1", b"", b".", b"1"), (b"0", b"0", b"0", b"0")])]
    open(path, "wb").write(b"Gene\ta\tb\ta\tc\n" + b"\n".join(rows) + b"\n")
    p = _series(["c", "a", "b"])
    with pytest.raises(RtabDuplicateSample):
        NativeRtabReader(path, list(p.index), None)
    blocks, error = _assert_same_stream(path, p, capsys, bs=2)
    assert error is None and sum(len(b) for b in blocks) == 5
    # a duplicated column that has no phenotype is no obstacle
    open(path, "wb").write(b"Gene\ta\tx\tx\tc\n" + b"\n".join(rows) + b"\n")
    NativeRtabReader(path, list(p.index), None).close()
    _assert_same_stream(path, p, capsys, bs=2)
