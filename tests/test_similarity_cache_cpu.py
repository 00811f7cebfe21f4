"""similarity --load-packed without a device: what refuses a run is decided before a context exists (one line on stderr, exit status 1,
nothing on stdout), argparse keeps --load-packed and --kmers apart, the 'Matrix size' rule, and the lean walk of the cache
(input.open_packed_cache_rows) against the iterator that has always read it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
CLI = os.path.join(os.path.dirname(__file__), "golden", "cli")
SAMPLES = [s.rstrip() for s in open(os.path.join(CLI, "samples50.txt"))]


def _list(path, names):
    with open(path, "w") as f:
        f.write("".join(n + "\n" for n in names))
    return str(path)


def _pack(tmp_path, names, tag, block=3000):
    from pyseer_amd import pack
    cache = str(tmp_path / (tag + ".seerpack"))
    pack.main([_list(tmp_path / (tag + ".txt"), names), "--kmers", os.path.join(CLI, "kmers.gz"), "-o", cache, "--block", str(block)])
    return cache


@pytest.fixture
def no_engine(monkeypatch):
    """any attempt to create a context fails the test"""
    from pyseer_amd import engine

    class Refused(object):
        def __init__(self, *a, **k):
            raise AssertionError("a context was created")
    monkeypatch.setattr(engine, "Engine", Refused)
    monkeypatch.setattr(engine, "RowSelector", Refused)


def _refused(argv, capsys):
    from pyseer_amd import similarity
    with pytest.raises(SystemExit) as ex:
        similarity.main(argv)
    got = capsys.readouterr()
    assert ex.value.code == 1
    assert got.out == ""
    assert got.err.endswith("\n") and got.err.count("\n") == 1, got.err
    return got.err


def test_refuses_a_file_that_is_no_cache(tmp_path, capsys, no_engine):
    capsys.readouterr()
    err = _refused([os.path.join(CLI, "samples50.txt"), "--load-packed", os.path.join(CLI, "kmers.gz")], capsys)
    assert "is not a packed k-mer cache" in err


def test_refuses_a_truncated_cache(tmp_path, capsys, no_engine):
    cache = _pack(tmp_path, SAMPLES, "all")
    data = open(cache, "rb").read()
    for cut, tag in ((len(data) - 16, "no_end"), (len(data) // 2, "half"), (30, "header")):
        part = str(tmp_path / (tag + ".seerpack"))
        with open(part, "wb") as f:
            f.write(data[:cut])
        capsys.readouterr()
        assert "truncated packed cache" in _refused([os.path.join(CLI, "samples50.txt"), "--load-packed", part], capsys)


def test_refuses_a_cache_that_lacks_a_sample(tmp_path, capsys, no_engine):
    cache = _pack(tmp_path, SAMPLES[:40], "forty")
    capsys.readouterr()
    err = _refused([os.path.join(CLI, "samples50.txt"), "--load-packed", cache], capsys)
    assert "lacks sample " + SAMPLES[40] in err


def test_refuses_a_sample_listed_twice(tmp_path, capsys, no_engine):
    cache = _pack(tmp_path, SAMPLES, "all")
    twice = _list(tmp_path / "twice.txt", SAMPLES[:10] + [SAMPLES[3]])
    capsys.readouterr()
    err = _refused([twice, "--load-packed", cache], capsys)
    assert "sample %s is listed twice" % SAMPLES[3] in err


def test_refuses_the_python_reader(tmp_path, capsys, no_engine):
    cache = _pack(tmp_path, SAMPLES, "all")
    capsys.readouterr()
    err = _refused([os.path.join(CLI, "samples50.txt"), "--load-packed", cache, "--python-reader"], capsys)
    assert "--python-reader" in err and "--load-packed" in err


def test_argparse_keeps_load_packed_and_kmers_apart(tmp_path, capsys):
    from pyseer_amd import similarity
    with pytest.raises(SystemExit) as ex:
        similarity.main([os.path.join(CLI, "samples50.txt"), "--load-packed", "x.seerpack", "--kmers", os.path.join(CLI, "kmers.gz")])
    assert ex.value.code == 2
    assert "not allowed with argument" in capsys.readouterr().err


def test_progress_sizes():
    from pyseer_amd.similarity import progress_sizes
    assert progress_sizes(0) == [1000]
    assert progress_sizes(1) == [1000]
    assert progress_sizes(1000) == [1000]
    assert progress_sizes(1001) == [1000, 2000]
    assert progress_sizes(3000) == [1000, 2000, 3000]


def test_lean_walk_yields_the_iterators_rows(tmp_path, capsys):
    """open_packed_cache_rows against iter_packed_blocks_cached(raw=True) over the cache's own list: the same rows, the same total, and the
    lines nobody carries are the rows whose stored count is zero"""
    import pandas as pd
    from pyseer_amd.input import iter_packed_blocks_cached, open_packed_cache_rows
    cache = _pack(tmp_path, SAMPLES, "all", block=100)
    stored, rb, total, rows = open_packed_cache_rows(cache)
    assert stored == SAMPLES and rb == 8
    got = list(rows())
    assert len(got) > 1 and sum(b.shape[0] for b, _ in got) == total
    p = pd.Series(np.zeros(len(SAMPLES)), index=SAMPLES)
    want = list(iter_packed_blocks_cached(p, cache, 0.0, 1.0, 1, raw=True, say_empty=False))
    assert np.array_equal(np.concatenate([b for b, _ in got]), np.concatenate([w.bits for w in want]))
    names, base = [], 0
    for (b, empty), w in zip(got, want):
        assert b.shape[0] == len(w)
        names += [(base + i, n) for i, n in empty]
        base += b.shape[0]
    counts = np.concatenate([w.counts for w in want])
    assert [i for i, _ in names] == np.nonzero(counts == 0)[0].tolist() and len(names) == 6
    assert all(n.startswith("AAAAAAAAAAA") for _, n in names)
