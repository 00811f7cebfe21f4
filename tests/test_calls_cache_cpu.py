"""The call cache without a device: the file format of input.CallCacheWriter / open_call_cache round trip and its rules
(planes on 8-byte boundaries, no file after abort() or a failed write, truncation and the wrong kind of cache refused by name), the host
restatement of k_calls_select (sh_select_calls_host) against the numpy yardstick of tests/_cache_select.py, and every refusal of
--save-calls / --load-calls that needs no input file.  The route key this cache adds is calls_cache (SEERHIP_ROUTE=calls_cache=rows)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _cache_select import MAP_KINDS, N_SRC, make_map, n_dsts, numpy_select, source_rows  # noqa: E402
from pyseer_amd import input as I  # noqa: E402
from pyseer_amd.packing import row_bytes_for  # noqa: E402


def _block(rng, n, nv, tag, messages=None, skip=None, names=None):
    rb = row_bytes_for(n)
    present = rng.integers(0, 256, (nv, rb), dtype=np.uint8)
    missing = rng.integers(0, 256, (nv, rb), dtype=np.uint8) & ~present
    names = names if names is not None else ["%s_%d" % (tag, i) for i in range(nv)]
    enc = [x.encode() for x in names]
    off = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum([len(x) for x in enc], out=off[1:])
    skip = np.zeros(nv, dtype=np.int32) if skip is None else np.asarray(skip, dtype=np.int32)
    return I.CallBlock(b"".join(enc), off, skip, present, missing, rng.integers(0, n + 1, nv).astype(np.int32), rng.integers(0, n + 1, nv).astype(np.int32),
                       list(messages) if messages is not None else [""] * nv)


def _flat(blocks):
    """what a list of CallBlocks holds, variant by variant"""
    out = []
    for cb in blocks:
        for i in range(len(cb)):
            out.append((bytes(cb.blob[cb.off[i]:cb.off[i + 1]]), int(cb.skip[i]), int(cb.n_present[i]), int(cb.n_missing[i]), cb.messages[i],
                        bytes(np.asarray(cb.present[i])), bytes(np.asarray(cb.missing[i]))))
    return out


def _hand_made(rng, n):
    """7 + 5 variants: non-empty messages, a skipped row, a row with every call missing, names of length zero"""
    a = _block(rng, n, 7, "a", messages=["", "Multiple alleles at chr_12. Skipping\n", "", "", "Could not parse region None\nMultiple alleles at c_3. Skipping\n", "", ""],
               skip=[0, 2, 0, 0, 0, 0, 0], names=["v0", "", "v2", "", "v4", "v5", "é_6"])
    a.missing[3] = 0xFF; a.present[3] = 0; a.n_present[3] = 0; a.n_missing[3] = n
    b = _block(rng, n, 5, "b", messages=["", "", "", "", "last\n"])
    return [a, b]


def test_round_trip_and_the_fixed_stored_blocks(tmp_path):
    rng = np.random.default_rng(1)
    n = 70
    samples = ["s%d" % i for i in range(n)]
    given = _hand_made(rng, n)
    path = str(tmp_path / "c.seercalls")
    w = I.CallCacheWriter(path, samples, 4)
    for cb in given:
        w.write(cb)
    assert not os.path.exists(path) and os.path.exists(path + ".part")
    w.close()
    assert os.path.exists(path) and not os.path.exists(path + ".part")
    stored, rb, rows, blocks = I.open_call_cache(path)
    got = list(blocks())
    assert stored == samples and rb == row_bytes_for(n) and rows == 12
    assert [len(cb) for cb in got] == [4, 4, 4]
    assert _flat(got) == _flat(given)
    for cb in got:
        assert cb.present.dtype == np.uint8 and cb.present.shape == (4, rb) == cb.missing.shape
        assert cb.skip.dtype == cb.n_present.dtype == cb.n_missing.dtype == np.int32 and cb.off.dtype == np.int64
        assert cb.msg_rows.tolist() == [i for i, m in enumerate(cb.messages) if m]
    assert got[0].names == ["v0", "", "v2", ""] and got[1].names[2] == "é_6"
    joined = I.join_call_blocks(got)
    assert len(joined) == 12 and _flat([joined]) == _flat(given) and joined.msg_rows.tolist() == [1, 4, 11]


@pytest.mark.parametrize("n", [1, 8, 63, 64, 65])
def test_planes_start_on_8_byte_boundaries(n, tmp_path):
    rng = np.random.default_rng(n)
    path = str(tmp_path / "c")
    w = I.CallCacheWriter(path, ["sample%d" % i for i in range(n)], 3)
    given = [_block(rng, n, 5, "x" * k, messages=["m" * (k + i) for i in range(5)]) for k in range(1, 4)]
    for cb in given:
        w.write(cb)
    w.close()
    got = list(I.open_call_cache(path)[3]())
    assert [len(cb) for cb in got] == [3, 3, 3, 3, 3] and _flat(got) == _flat(given)
    raw = open(path, "rb").read()
    for cb in got:
        for plane in (cb.present, cb.missing):
            at = raw.find(bytes(plane))                         # (random rows: the first match is the plane)
            assert at > 0 and at % 8 == 0
            assert np.array_equal(np.frombuffer(raw, dtype="<u8", count=plane.size // 8, offset=at), np.ascontiguousarray(plane).view("<u8").reshape(-1))


def test_abort_and_a_failed_write_leave_nothing(tmp_path):
    rng = np.random.default_rng(2)
    path = str(tmp_path / "c")
    w = I.CallCacheWriter(path, ["a", "b"], 2)
    w.write(_block(rng, 2, 3, "x"))
    w.abort()
    assert not os.path.exists(path) and not os.path.exists(path + ".part")
    w.close()                                                   # (nothing to close any more)
    assert not os.path.exists(path)
    # a block of the wrong width is refused; a writer that is dropped without close() leaves nothing either
    w = I.CallCacheWriter(path, ["a", "b"], 2)
    with pytest.raises(ValueError):
        w.write(_block(rng, 100, 3, "x"))
    del w
    assert not os.path.exists(path) and not os.path.exists(path + ".part")
    # the write itself fails (the file is gone from under the writer): close() raises and leaves neither file

    class Broken(object):
        def write(self, b):
            raise IOError("disk full")

        def close(self):
            pass
    w = I.CallCacheWriter(path, ["a", "b"], 2)
    w._f.close()
    w._f = Broken()
    with pytest.raises(IOError):
        w.write(_block(rng, 2, 3, "x"))
    w.abort()
    assert not os.path.exists(path) and not os.path.exists(path + ".part")
    w = I.CallCacheWriter(path, ["a", "b"], 5)
    w.write(_block(rng, 2, 3, "x"))                             # (held: fewer than a stored block)
    w._f.close()
    w._f = Broken()
    with pytest.raises(IOError):
        w.close()
    assert not os.path.exists(path) and not os.path.exists(path + ".part")


def test_a_cache_cut_anywhere_in_its_last_block_is_truncated(tmp_path):
    rng = np.random.default_rng(3)
    path = str(tmp_path / "c")
    w = I.CallCacheWriter(path, ["s%d" % i for i in range(9)], 4)
    w.write(_block(rng, 9, 6, "x", messages=["", "m\n", "", "", "", ""]))
    w.close()
    raw = open(path, "rb").read()
    blocks = list(I.open_call_cache(path)[3]())
    assert [len(cb) for cb in blocks] == [4, 2]
    meta = 16 * 3 + 12 * 2 + len(blocks[1].blob) + sum(len(m_) for m_ in blocks[1].messages)
    last = len(raw) - 32 - (32 + meta + (-meta) % 8 + 2 * 2 * 8)        # where the last stored block's header starts (behind it: the terminator)
    assert raw.find(bytes(blocks[1].present)) == last + 32 + meta + (-meta) % 8
    cut = str(tmp_path / "cut")
    for size in range(last, len(raw)):
        with open(cut, "wb") as f:
            f.write(raw[:size])
        with pytest.raises(IOError) as ex:
            I.open_call_cache(cut)
        assert str(ex.value) == "truncated call cache %s (delete it, or run without --load-calls)" % cut, size
    with open(cut, "wb") as f:
        f.write(raw)
    assert I.open_call_cache(cut)[2] == 6


def test_the_other_kind_of_cache_is_named(tmp_path):
    rng = np.random.default_rng(4)
    calls, kmers, junk = str(tmp_path / "calls"), str(tmp_path / "kmers"), str(tmp_path / "junk")
    w = I.CallCacheWriter(calls, ["a", "b"], 2)
    w.write(_block(rng, 2, 3, "x"))
    w.close()
    k = I.PackedCacheWriter(kmers, ["a", "b"])
    k.write_block(b"xy", np.array([0, 1, 2], dtype=np.int64), np.array([1, 1], dtype=np.int32), np.ones((2, 8), dtype=np.uint8))
    k.close()
    with open(junk, "wb") as f:
        f.write(b"not a cache at all, whatever its length" * 3)
    with pytest.raises(IOError) as ex:
        I.open_call_cache(kmers)
    assert str(ex.value) == "%s is a packed k-mer cache, not a call cache (it is read by --load-packed)" % kmers
    with pytest.raises(IOError) as ex:
        I.open_call_cache(junk)
    assert str(ex.value) == "%s is not a call cache" % junk
    import pandas as pd
    p = pd.Series([0.0, 1.0], index=["a", "b"])
    for fn in (lambda: I.check_packed_cache(p, calls), lambda: I._map_packed_cache(calls), lambda: I.open_packed_cache_rows(calls)):
        with pytest.raises(IOError) as ex:
            fn()
        assert str(ex.value) == "%s is a call cache, not a packed k-mer cache (it is read by --load-calls)" % calls
    with pytest.raises(IOError) as ex:
        I.check_packed_cache(p, junk)
    assert str(ex.value) == "%s is not a packed k-mer cache" % junk


def test_a_loader_joins_whole_stored_blocks_up_to_the_job_block(tmp_path, capsys):
    """never more than job_block variants in a group, never a stored block split; a stored block larger than job_block goes alone"""
    import pandas as pd
    rng = np.random.default_rng(6)
    samples = ["s%d" % i for i in range(9)]
    path = str(tmp_path / "c")
    w = I.CallCacheWriter(path, samples, 4)
    given = _block(rng, 9, 22, "x", messages=["m%d\n" % i if i % 5 == 0 else "" for i in range(22)])
    given.n_present[:] = 1
    w.write(given)
    w.close()
    p = pd.Series(np.zeros(9), index=samples)
    for job_block, want in ((4, [4, 4, 4, 4, 4, 2]), (9, [8, 8, 6]), (10, [8, 8, 6]), (12, [12, 10]), (3, [4, 4, 4, 4, 4, 2]), (100, [22])):
        got = list(I.iter_call_cache_blocks(p, I.open_call_cache(path)[3], job_block, "job"))
        assert [len(cb) for cb in got] == want, job_block
        assert _flat(got) == _flat([given])
        assert capsys.readouterr().err == "".join(given.messages)


def test_the_sample_map_and_its_refusals(monkeypatch):
    monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
    stored = ["a", "b", "c", "d"]
    assert I.call_cache_sample_map(stored, list(stored)) is None
    assert I.call_cache_sample_map(stored, ["d", "b"]).tolist() == [3, 1] and I.call_cache_sample_map(stored, ["d", "b"]).dtype == np.int32
    for samples, text in ((["a", "x"], "the call cache does not hold sample x of the run"),
                          (["a", "b", "a"], "sample a is listed twice in the run: a call cache is selected for distinct samples")):
        with pytest.raises(ValueError) as ex:
            I.call_cache_sample_map(stored, samples)
        assert str(ex.value) == text
    with pytest.raises(ValueError) as ex:
        I.call_cache_sample_map(["a", "b", "a"], ["a", "b"])
    assert str(ex.value) == "the call cache lists sample a twice: it is served to its own sample list only"
    assert I.call_cache_sample_map(["a", "b", "a"], ["a", "b", "a"]) is None          # (as stored: absent columns and all)
    monkeypatch.setenv("SEERHIP_ROUTE", "cache_select=0")
    assert I.call_cache_sample_map(stored, list(stored)) is None
    with pytest.raises(ValueError) as ex:
        I.call_cache_sample_map(stored, ["d", "b"])
    assert str(ex.value) == "call cache was written for a different sample list / order (4 vs 2 samples)"


# ---- the host restatement of k_calls_select ------------------------------------------------------------------------------------------------
def _check_calls(got, present, missing, n_src, m):
    for (bits, counts), src in (((got[0], got[2]), present), ((got[1], got[3]), missing)):
        want_bits, want_counts = numpy_select(src, n_src, m)
        assert bits.dtype == np.uint8 and bits.shape == want_bits.shape and np.array_equal(bits, want_bits)
        assert not np.unpackbits(np.ascontiguousarray(bits), axis=1, bitorder="little")[:, len(m):].any()
        assert counts.dtype == np.int32 and np.array_equal(counts, want_counts)


@pytest.mark.parametrize("n_src", N_SRC)
def test_host_restatement_equals_numpy(n_src):
    from pyseer_amd.engine import select_calls_host
    rng = np.random.default_rng(100 + n_src)
    for V in (0, 1, 5, 257):
        present, _ = source_rows(V, n_src, rng, 0.4)            # (padding bits all ones)
        missing, _ = source_rows(V, n_src, rng, 0.1)
        for n_dst in n_dsts(n_src):
            for kind in MAP_KINDS:
                m = make_map(kind, n_src, n_dst, rng)
                _check_calls(select_calls_host(present, missing, n_src, m), present, missing, n_src, m)
    # the two planes overlapping: one array given as both
    both, _ = source_rows(5, n_src, rng, 0.5)
    m = make_map("permuted", n_src, n_dsts(n_src)[-1], rng)
    _check_calls(select_calls_host(both, both, n_src, m), both, both, n_src, m)


def test_host_restatement_refuses_a_bad_map():
    from pyseer_amd import _abi
    from pyseer_amd.engine import select_calls_host
    rows = np.zeros((2, 8), dtype=np.uint8)
    for m in ([0, 0], [0, 64], [-1]):
        with pytest.raises(_abi.SeerHipError):
            select_calls_host(rows, rows, 64, m)


# ---- the command line's refusals that need no input file (tests/test_cli_options_cpu.py's way) ------------------------------------------------
P = ["--phenotypes", "p.tsv", "--no-distances"]
L = P + ["--load-calls", "c.seercalls"]
S = P + ["--vcf", "v.vcf", "--save-calls", "c.seercalls"]
KMER_CACHE_L = "--load-calls reads a call cache, not a packed k-mer cache: not available with --save-packed / --load-packed / --packed-cache\n"
KMER_CACHE_S = "--save-calls is no packed k-mer cache: not available with --save-packed / --load-packed / --packed-cache / --packed-part\n"
REFUSALS = [
    ("load burden", L + ["--burden", "b.txt"],
     "--load-calls serves the variants its cache holds: --burden regions are not applied to it (write the cache with --save-calls --burden)\n"),
    ("load two devices", L + ["--gpus", "0,0"], "--load-calls selects and tests on one device: not available with more than one device in --gpus\n"),
    ("load a count of two", L + ["--gpus", "2"], "--load-calls selects and tests on one device: not available with more than one device in --gpus\n"),
    ("load packed-part", L + ["--packed-part", "0/2"], "--load-calls reads one whole cache: not available with --packed-part\n"),
    ("load wg", L + ["--wg", "enet"], "--load-calls serves the per-variant models: not available with --wg\n"),
    ("load save-packed", L + ["--save-packed", "k"], KMER_CACHE_L),
    ("load load-packed", L + ["--load-packed", "k"], KMER_CACHE_L),
    ("load packed-cache", L + ["--packed-cache"], KMER_CACHE_L),
    ("save python-reader", S + ["--python-reader"], "--save-calls writes what the native readers deliver: not available with --python-reader\n"),
    ("save gpus", S + ["--gpus", "1"], "--save-calls is written by a run on one device: not available with --gpus\n"),
    ("save wg", S + ["--wg", "enet"], "--save-calls is written by a per-variant run: not available with --wg\n"),
    ("save kmers", P + ["--kmers", "k.gz", "--save-calls", "c"], "--save-calls caches VCF, BCF and Rtab calls: k-mers have --save-packed\n"),
    ("save load", L + ["--save-calls", "d"], "--save-calls writes the calls a VCF, BCF or Rtab is parsed into: not available with --load-calls\n"),
    ("save save-packed", P + ["--pres", "r.Rtab", "--save-calls", "c", "--save-packed", "k"], KMER_CACHE_S),
    ("save packed-part", P + ["--pres", "r.Rtab", "--save-calls", "c", "--packed-part", "0/2"], KMER_CACHE_S),
]


@pytest.mark.parametrize("tag,argv,text", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal_exits_1_with_its_message(tag, argv, text, capsys):
    from pyseer_amd.__main__ import main
    with pytest.raises(SystemExit) as ex:
        main(argv)
    assert ex.value.code == 1
    out = capsys.readouterr()
    assert out.err == text and out.out == ""


def test_load_calls_is_one_of_the_variant_inputs(capsys):
    from pyseer_amd.__main__ import get_options
    with pytest.raises(SystemExit) as ex:
        get_options(["--phenotypes", "p.tsv", "--load-calls", "c", "--vcf", "v.vcf"])
    assert ex.value.code == 2 and "not allowed with argument" in capsys.readouterr().err
    o = get_options(["--phenotypes", "p.tsv", "--load-calls", "c"])
    assert o.load_calls == "c" and o.save_calls is None and o.vcf is None and o.pres is None and o.kmers is None


def test_pack_takes_one_of_three_inputs(capsys):
    from pyseer_amd.pack import get_options, main
    with pytest.raises(SystemExit):
        get_options(["samples.txt", "-o", "out"])
    with pytest.raises(SystemExit):
        get_options(["samples.txt", "-o", "out", "--kmers", "k.gz", "--vcf", "v.vcf"])
    capsys.readouterr()
    o = get_options(["samples.txt", "-o", "out", "--pres", "r.Rtab", "--block", "7"])
    assert o.pres == "r.Rtab" and o.kmers is None and o.vcf is None and o.block == 7
    assert get_options(["samples.txt", "-o", "out", "--kmers", "k.gz"]).kmers == "k.gz"


def test_the_plan_of_load_calls(monkeypatch):
    """--load-calls takes the job stream unless a cross-check sink or job=0 is asked for; calls_cache=rows and cache_select=host choose how a cache over
    other samples is restricted"""
    from pyseer_amd import cli_run
    from pyseer_amd.__main__ import get_options
    monkeypatch.delenv("SEERHIP_ROUTE", raising=False)

    def plan(extra, routes=None):
        return cli_run.make_plan(get_options(L + extra), lambda key, default=None: (routes or {}).get(key, default), True)
    pl = plan([])
    assert pl.calls_job and pl.job_path and pl.var_type == "calls" and not (pl.native or pl.native_vcf or pl.native_rtab) and not pl.packed_c_loop and not pl.proc_mode
    assert pl.job_block == 1 << 14 and plan(["--print-filtered"]).job_block == 3000
    for extra, routes in ((["--python-sink"], None), (["--serial-sink"], None), ([], {"job": "0"})):
        pl = plan(extra, routes)
        assert not pl.calls_job and not pl.job_path and pl.job_block == 3000
    assert cli_run.call_cache_select_mode() == "fused"
    monkeypatch.setenv("SEERHIP_ROUTE", "calls_cache=rows")
    assert cli_run.call_cache_select_mode() == "rows"
    monkeypatch.setenv("SEERHIP_ROUTE", "calls_cache=rows,cache_select=host")
    assert cli_run.call_cache_select_mode() == "host"
