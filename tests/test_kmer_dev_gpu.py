"""The device route of the k-mer reader (sh_reader_open_dev, k_kmer_pack; csrc/kmer_api.inc, csrc/kmer_kernels.hip) against the host route
(sh_reader_open), bit for bit: bits, counts, names blob and offsets of every block.

The corpus (tests/_kmer_dev_corpus.py; a fixed seed, at most 2000 lines) holds: carriers from none to all; names of 1, 8, 9, 16, 17 and 40 bytes;
two names equal in their first 16 bytes; two that differ only in length; a sample named twice in the phenotype; tokens of samples without a
phenotype; a sample repeated within a line; a token without ':', one with several, one that is only ':3'; tabs and runs of blanks; CRLF line
ends; a line without '|'; lines with an empty segment; a second '|' followed by tokens that must not count; a blank line; a last line
without a newline.  (A sample count below nine takes the first names of the list: what does not fit is not there.)

`lines_host == 0` with `lines_dev` = the number of lines keeps a silent fall-back to the host from passing."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _kmer_dev_corpus import assert_same_blocks, containers, corpus, read_blocks, sample_names  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
CASES = json.load(open(os.path.join(CLI, "cases.json")))
STRADDLE = "reader_slab=70000,reader_pad=32768"           # the smallest the reader accepts: many lines cross slabs


@pytest.fixture(scope="module")
def engine_for():
    """one engine per sample count"""
    from pyseer_amd.engine import Engine
    made = {}

    def get(n):
        if n not in made:
            made[n] = Engine(n)
        return made[n]
    yield get
    for e in made.values():
        e.close()


def _write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 300, 1000])
def test_device_route_equals_host_route(n, tmp_path, engine_for):
    names = sample_names(n)
    text, n_lines = corpus(names, n_lines=300, seed=n)
    e = engine_for(n)
    for kind, data in containers(text).items():
        path = _write(tmp_path, "k." + kind, data)
        for bs in (1, 37, 3000):
            want, _ = read_blocks(path, names, bs)
            got, stats = read_blocks(path, names, bs, engine=e)
            assert sum(len(b[1]) for b in want) == n_lines
            assert_same_blocks(got, want, (kind, bs))
            assert stats["lines_host"] == 0 and stats["lines_dev"] == n_lines, (kind, bs, stats)
            assert stats["launches"] == len(want) and stats["bytes_up"] >= len(text)
    counts = np.concatenate([b[1] for b in want])
    assert counts.max() == len(set(names)) and counts.min() == 0


def test_lines_that_straddle_slabs(tmp_path, monkeypatch, engine_for):
    """Slabs of 70 000 bytes with a pad of 32 768: lines cross slabs all the time and are read in the next slab's pad; two lines of 40 000
    bytes of sample tokens exceed the pad, and the one placed across the first boundary is copied out by the reader and tokenised by the
    host restatement (at most those two may be)."""
    n = 300
    names = sample_names(n)
    text, n_lines = corpus(names, n_lines=300, seed=77, long_tokens=2)
    assert len(text) > 6 * 70000
    e = engine_for(n)
    monkeypatch.setenv("SEERHIP_ROUTE", STRADDLE)
    for kind, data in containers(text).items():
        path = _write(tmp_path, "s." + kind, data)
        for bs in (37, 3000):
            want, _ = read_blocks(path, names, bs)
            got, stats = read_blocks(path, names, bs, engine=e)
            assert_same_blocks(got, want, (kind, bs))
            assert stats["lines_host"] <= 2 and stats["lines_dev"] + stats["lines_host"] == n_lines, (kind, bs, stats)
            if kind == "plain":                           # (its slabs are cut at multiples of 70 000 bytes of the file)
                assert stats["lines_host"] >= 1


def _next(reader, names_cap):
    """one sh_reader_next with a names buffer of names_cap bytes -> (return value, bits, counts, blob, off)"""
    from pyseer_amd import _abi
    bs = reader.block_size
    bits = np.zeros((bs, reader.row_bytes), dtype=np.uint8)
    counts = np.zeros(bs, dtype=np.int32)
    off = np.zeros(bs + 1, dtype=np.int64)
    buf = C.create_string_buffer(names_cap)
    nv = reader._lib.sh_reader_next(reader._h, bs, bits.ctypes.data_as(_abi.c_u8p), reader.row_bytes, counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                    buf, names_cap, off.ctypes.data_as(C.POINTER(C.c_int64)))
    m = max(nv, 0)
    return nv, bits[:m], counts[:m], buf.raw[:off[m]], off[:m + 1]


def test_a_long_unitig_name_is_refused_once_and_read_on_the_retry(tmp_path, engine_for):
    from pyseer_amd.input import NativeKmerReader
    names = sample_names(9)
    path = _write(tmp_path, "unitig.gz", gzip.compress(b"ACGT | a:1\n" + b"C" * 50000 + b" | sample_8:1 a:2 nophenotype:1\nGG | sample__9:1\n"))
    blocks = []
    for engine in (None, engine_for(9)):
        r = NativeKmerReader(path, names, 3000, engine=engine)
        try:
            first = _next(r, 1000)
            assert first[0] == -2 and int(r._lib.sh_reader_names_needed(r._h)) == 50006
            again = _next(r, 1000)
            assert again[0] == -2                         # nothing was consumed
            blocks.append(_next(r, 60000))
            assert _next(r, 60000)[0] == 0
            if engine is not None:
                assert r.dev_stats()["lines_dev"] == 3 and r.dev_stats()["lines_host"] == 0
        finally:
            r.close()
    assert blocks[0][0] == 3 and blocks[0][2].tolist() == [1, 2, 1]
    assert_same_blocks([blocks[1][1:]], [blocks[0][1:]], "unitig")


def test_a_damaged_member_gives_the_same_error(tmp_path, engine_for):
    names = sample_names(65)
    text, _ = corpus(names, n_lines=300, seed=3)
    bad = bytearray(gzip.compress(text, 6))
    bad[len(bad) // 2] ^= 0x10
    path = _write(tmp_path, "bad.gz", bytes(bad))
    errs = []
    for engine in (None, engine_for(65)):
        with pytest.raises(IOError) as ex:
            read_blocks(path, names, 3000, engine=engine)
        errs.append(str(ex.value))
    assert errs[0] == errs[1] and errs[0].startswith("gzip")


def test_a_row_that_does_not_fit_the_lds_is_refused(tmp_path):
    """the library refuses by the limit's name before it touches the device or the file"""
    from pyseer_amd import _abi
    lib = _abi.load()
    n = 523264 + 1
    from pyseer_amd.engine import Engine
    e = Engine(n)
    try:
        arr = (C.c_char_p * n)(*[b"s%d" % i for i in range(n)])
        h = lib.sh_reader_open_dev(e._h, str(tmp_path / "nothing").encode(), arr, n)
        assert not h and "at most 523 264" in lib.sh_reader_error().decode()
    finally:
        e.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _cli(args, module="pyseer_amd", route=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    env.pop("SEERHIP_ROUTE", None)
    if route:
        env["SEERHIP_ROUTE"] = route
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def plain_runs():
    """the four cases without the flag, run once"""
    return {name: _cli(list(CASES[name])) for name in ("fixed", "fixed_cov", "lmm", "cont")}


@pytest.mark.parametrize("name", ["fixed", "fixed_cov", "lmm", "cont"])
def test_cli_prints_the_same_bytes(name, plain_runs):
    """With the flag and without it: the same bytes on stdout and stderr.  Against the committed expected/ files: of stderr, the lines a reader
    decides (every "No observations of ..." line, in order, and the four counters; 'lmm' also prints a numpy warning with a path of the
    machine in it, with either reader); stdout is held to them by the rule of test_cli_gpu.py::test_cli_matches_reference (same rows, names and notes; a '%.2E' number may sit
    one unit of its last printed digit away, an MDS axis has no sign): the engine's numbers are not the reference's to the byte with either
    reader -- measured for 'lmm', one digit of one row (7 against 8); 'fixed' and 'fixed_cov' are the same bytes."""
    from test_cli_gpu import _num_close
    out, err = _cli(list(CASES[name]) + ["--device-reader"])
    assert out == plain_runs[name][0] and err == plain_runs[name][1]
    reader_lines = lambda t: [l for l in t.splitlines() if l.startswith("No observations of ") or l.endswith(" variants")]
    assert reader_lines(err.decode()) == reader_lines(open(os.path.join(CLI, "expected", name + ".err")).read())
    got, want = out.decode().splitlines(), open(os.path.join(CLI, "expected", name + ".log")).read().splitlines()
    assert got[0] == want[0] and len(got) == len(want)
    header = want[0].split("\t")
    for g, w in zip(got[1:], want[1:]):
        gf, wf = g.split("\t"), w.split("\t")
        assert gf[0] == wf[0] and len(gf) == len(wf) and set(gf[-1].split(",")) == set(wf[-1].split(",")), (g, w)
        for c in range(1, len(wf) - 1):
            assert _num_close(gf[c], wf[c], sign_free=(len(wf) == len(header) and header[c].startswith("PC"))), (header[c], g, w)


def test_cli_route_key_and_python_reader(plain_runs):
    out, err = _cli(list(CASES["fixed"]), route="kmer_dev=1")
    assert (out, err) == plain_runs["fixed"]
    base = _cli(list(CASES["fixed"]) + ["--python-reader"])
    assert _cli(list(CASES["fixed"]) + ["--python-reader", "--device-reader"]) == base


def test_cli_save_packed_writes_the_same_cache(tmp_path):
    a, b = str(tmp_path / "a.seerpack"), str(tmp_path / "b.seerpack")
    ra = _cli(list(CASES["fixed"]) + ["--save-packed", a])
    rb = _cli(list(CASES["fixed"]) + ["--save-packed", b, "--device-reader"])
    assert ra == rb
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 0


def test_similarity_prints_the_expected_matrix():
    args = ["samples50.txt", "--kmers", "kmers.gz"]
    out, err = _cli(args + ["--device-reader"], module="pyseer_amd.similarity")
    assert (out, err) == _cli(args, module="pyseer_amd.similarity")
    assert out == open(os.path.join(CLI, "expected", "similarity_kmers.tsv"), "rb").read()
    # (python -m on a module of an imported package makes runpy warn, two lines that begin with a path and with blanks; the rest is the reference's)
    said = [l for l in err.decode().splitlines() if not l.startswith(("/", " "))]
    assert said == open(os.path.join(CLI, "expected", "similarity_kmers.err")).read().splitlines()
