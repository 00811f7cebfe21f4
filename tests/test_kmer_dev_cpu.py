"""The device route of the k-mer reader without a device: sh_reader_open_dev(NULL, ...) tokenises with host_kmer_pack, the kernel's rule in
plain C++ (csrc/kmer_kernels.h), and must hand out what sh_reader_open's SSE parser hands out -- bits, counts, names and offsets of every
block -- over the corpus of tests/_kmer_dev_corpus.py in its four containers.  The slabs, the plain-text copy into them, the line table
and the place where a line's buffer is looked up are the device route's own and run here too."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _kmer_dev_corpus import assert_same_blocks, containers, corpus, read_blocks, sample_names  # noqa: E402

from pyseer_amd.input import NativeKmerReader  # noqa: E402

HOST_RULE = NativeKmerReader.DEVICE_HOST_RULE


@pytest.mark.parametrize("n", [1, 9, 65, 300])
def test_host_restatement_equals_the_parser(n, tmp_path):
    names = sample_names(n)
    text, n_lines = corpus(names, n_lines=150, seed=n)
    for kind, data in containers(text).items():
        path = str(tmp_path / ("k." + kind))
        open(path, "wb").write(data)
        for bs in (1, 37, 3000):
            want, _ = read_blocks(path, names, bs)
            got, stats = read_blocks(path, names, bs, engine=HOST_RULE)
            assert sum(len(b[1]) for b in want) == n_lines
            assert_same_blocks(got, want, (kind, bs))
            assert stats["lines_dev"] == 0 and stats["lines_host"] == n_lines and stats["launches"] == 0
    assert any(b[1].max() == len(set(names)) for b in want) and any(b[1].min() == 0 for b in want)


def test_straddling_lines_long_names_and_a_damaged_member(tmp_path, monkeypatch):
    names = sample_names(300)
    text, n_lines = corpus(names, n_lines=300, seed=5, long_tokens=2)
    files = containers(text)
    monkeypatch.setenv("SEERHIP_ROUTE", "reader_slab=70000,reader_pad=32768")
    for kind, data in files.items():
        path = str(tmp_path / ("s." + kind))
        open(path, "wb").write(data)
        want, _ = read_blocks(path, names, 37)
        got, stats = read_blocks(path, names, 37, engine=HOST_RULE)
        assert_same_blocks(got, want, kind)
        assert stats["lines_host"] == n_lines
    monkeypatch.delenv("SEERHIP_ROUTE")
    # one 50 000-byte unitig name: the first call is refused (-2) and consumes nothing, the retry returns the host route's block
    path = str(tmp_path / "unitig.gz")
    import gzip
    open(path, "wb").write(gzip.compress(b"ACGT | a:1\n" + b"C" * 50000 + b" | sample_8:1 a:2\nGG | a:1\n"))
    want, _ = read_blocks(path, names, 3000, max_name=4)
    got, _ = read_blocks(path, names, 3000, max_name=4, engine=HOST_RULE)
    assert_same_blocks(got, want, "unitig")
    assert len(got) == 1 and len(got[0][2]) == 50006
    # a flipped bit in the gzip body: the same error text
    bad = bytearray(files["gzip"])
    bad[len(bad) // 2] ^= 0x10
    path = str(tmp_path / "bad.gz")
    open(path, "wb").write(bytes(bad))
    errs = []
    for engine in (None, HOST_RULE):
        with pytest.raises(IOError) as ex:
            read_blocks(path, names, 3000, engine=engine)
        errs.append(str(ex.value))
    assert errs[0] == errs[1] and errs[0].startswith("gzip")
