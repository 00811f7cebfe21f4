"""k_bgzf_inflate (csrc/inflate_kernels.hip) and the k-mer reader's device inflate (SEERHIP_ROUTE kmer_inflate=1, --device-inflate) on the
device.  zlib is the yardstick of the kernel, the host route of the reader (sh_reader_open) of everything above it; the member corpus is
tests/_inflate_corpus.py, which tests/test_inflate_cpu.py holds against zlib and runs through the host build of the same decoder.

Every launch decodes into a buffer that also holds 64 bytes of a pattern before, between and behind the members' ranges: the kernel's only
store to the text is its final copy of min(produced, isize) bytes, so no byte of the pattern may change, for malformed members either."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inflate_corpus as ic  # noqa: E402
from _kmer_dev_corpus import assert_same_blocks, corpus, sample_names  # noqa: E402
from _vcf_text import bgzf_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
CASES = json.load(open(os.path.join(CLI, "cases.json")))
STRADDLE = "reader_slab=70000,reader_pad=32768"
GAP, PATTERN = 64, 0x5A


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


def inflate_dev(engine, members, per_launch):
    """members [(cdata, isize)] through sh_inflate_members_dev, per_launch at a time (0: all at once) -> (status, produced, buffer, offsets).
    Member i decodes to buffer[offsets[i] : offsets[i] + isize]; everything else in the buffer was PATTERN before the launches.  The
    offsets follow each other at GAP bytes and are as odd as the sizes make them."""
    from pyseer_amd import _abi
    lib = _abi.load()
    n = len(members)
    clen = np.array([len(c) for c, _ in members], dtype=np.int32)
    isize = np.array([s for _, s in members], dtype=np.int32)
    coff = np.concatenate([[0], np.cumsum(clen[:-1], dtype=np.int64)]).astype(np.int64)
    ooff = (GAP + np.concatenate([[0], np.cumsum(isize[:-1].astype(np.int64) + GAP)])).astype(np.int64)
    comp = np.frombuffer(b"".join(c for c, _ in members) + b"\0", dtype=np.uint8).copy()
    out = np.full(int(ooff[-1] + isize[-1] + GAP), PATTERN, dtype=np.uint8)
    status = np.full(n, -99, dtype=np.int32)
    produced = np.full(n, -99, dtype=np.int32)
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    step = per_launch or n
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        # the launch sees only its members' stretch of both buffers
        c0, c1 = int(coff[lo]), int(coff[hi - 1] + clen[hi - 1])
        o0, o1 = int(ooff[lo]) - GAP, int(ooff[hi - 1] + isize[hi - 1]) + GAP
        sub_c, sub_o = comp[c0:max(c1, c0 + 1)], out[o0:o1]
        lc, lo_ = (coff[lo:hi] - c0).copy(), (ooff[lo:hi] - o0).copy()
        _abi.check(lib.sh_inflate_members_dev(engine._h, sub_c.ctypes.data_as(_abi.c_u8p), sub_c.shape[0], lc.ctypes.data_as(p64),
                                              clen[lo:hi].ctypes.data_as(p32), isize[lo:hi].ctypes.data_as(p32), lo_.ctypes.data_as(p64), hi - lo,
                                              sub_o.ctypes.data_as(_abi.c_u8p), sub_o.shape[0], status[lo:hi].ctypes.data_as(p32),
                                              produced[lo:hi].ctypes.data_as(p32), None))
    return status, produced, out, ooff


def pattern_intact(out, ooff, lengths):
    """every byte outside [ooff[i], ooff[i] + lengths[i]) still holds the pattern"""
    keep = np.ones(out.shape[0], dtype=bool)
    for o, ln in zip(ooff, lengths):
        keep[int(o):int(o) + int(ln)] = False
    return bool((out[keep] == PATTERN).all())


@pytest.fixture(scope="module")
def good():
    return ic.well_formed()


@pytest.mark.parametrize("per_launch", [0, 1, 2, 65])
def test_kernel_decodes_every_well_formed_member(per_launch, good, engine_for):
    status, produced, out, ooff = inflate_dev(engine_for(9), [(c, len(t)) for _, c, t in good], per_launch)
    assert (status == 0).all(), [(good[i][0], int(status[i])) for i in np.nonzero(status)[0][:5]]
    assert (produced == [len(t) for _, _, t in good]).all()
    for (name, _, text), o in zip(good, ooff):
        assert out[int(o):int(o) + len(text)].tobytes() == text, name
    assert pattern_intact(out, ooff, [len(t) for _, _, t in good])


def test_kernel_refuses_every_malformed_member(good, engine_for):
    """the members the host build of the decoder has already refused (test_inflate_cpu.py): the same statuses from the kernel, nothing
    written outside their ranges, and the device answers the next launch"""
    bad = ic.malformed()
    codes = ic.statuses()
    e = engine_for(9)
    status, produced, out, ooff = inflate_dev(e, [(c, s) for _, c, s, _ in bad], 0)
    assert [int(s) for s in status] == [codes[st] for _, _, _, st in bad], [(b[0], int(s)) for b, s in zip(bad, status)]
    assert ((produced >= 0) & (produced <= [s for _, _, s, _ in bad])).all()
    assert pattern_intact(out, ooff, [s for _, _, s, _ in bad])
    # malformed and well-formed members side by side in one launch
    mixed = [(bad[i % len(bad)][1], bad[i % len(bad)][2]) if i % 2 else (good[7 * i % len(good)][1], len(good[7 * i % len(good)][2])) for i in range(40)]
    status, produced, out, ooff = inflate_dev(e, mixed, 0)
    assert all((int(status[i]) != 0) == bool(i % 2) for i in range(40))
    assert pattern_intact(out, ooff, [s for _, s in mixed])
    for i in range(0, 40, 2):
        text = good[7 * i % len(good)][2]
        assert out[int(ooff[i]):int(ooff[i]) + len(text)].tobytes() == text
    import torch
    torch.cuda.synchronize()


def test_members_outside_their_buffers_are_refused(engine_for):
    from pyseer_amd import _abi
    lib = _abi.load()
    comp = np.frombuffer(ic.EOF_MEMBER, dtype=np.uint8).copy()
    out = np.zeros(16, dtype=np.uint8)
    st, pr = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    for coff, clen, isize, ooff in ((0, 3, 0, 0), (1, 2, 0, 0), (-1, 2, 0, 0), (0, 2, 17, 0), (0, 2, 8, 9), (0, 2, 65537, 0), (0, 2, 1, -1)):
        a = [np.array([v], dtype=t) for v, t in ((coff, np.int64), (clen, np.int32), (isize, np.int32), (ooff, np.int64))]
        r = lib.sh_inflate_members_dev(engine_for(9)._h, comp.ctypes.data_as(_abi.c_u8p), 2, a[0].ctypes.data_as(p64), a[1].ctypes.data_as(p32),
                                       a[2].ctypes.data_as(p32), a[3].ctypes.data_as(p64), 1, out.ctypes.data_as(_abi.c_u8p), 16,
                                       st.ctypes.data_as(p32), pr.ctypes.data_as(p32), None)
        assert r != 0 and b"outside the buffer" in lib.sh_last_error(), (coff, clen, isize, ooff)


def read_blocks(path, names, block_size, engine=None):
    from pyseer_amd.input import NativeKmerReader
    r = NativeKmerReader(path, names, block_size, 256, engine=engine)
    try:
        blocks = [(b.copy(), c.copy(), blob, off) for b, c, blob, off in r.raw_blocks()]
        stats = dict(r.dev_stats(), **{"inflate": r.inflate_stats()}) if engine is not None else None
    finally:
        r.close()
    return blocks, stats


@pytest.mark.parametrize("n", [1, 9, 65, 300])
def test_device_inflate_equals_the_host_route(n, tmp_path, monkeypatch, engine_for):
    names = sample_names(n)
    e = engine_for(n)
    for member in (1, 100, 40000, 65280):
        text, n_lines = corpus(names, n_lines=ic.LINES[member], seed=n)
        data = bgzf_bytes(text, block=member)
        n_members = len(ic.members_of(data))
        path = str(tmp_path / ("k%d.bgzf" % member))
        open(path, "wb").write(data)
        for bs in (1, 37, 3000):
            monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
            want, _ = read_blocks(path, names, bs)
            monkeypatch.setenv("SEERHIP_ROUTE", "kmer_inflate=1")
            got, stats = read_blocks(path, names, bs, engine=e)
            assert_same_blocks(got, want, (member, bs))
            assert stats["inflate"]["members_host"] == 0 and stats["inflate"]["members_dev"] == n_members, (member, bs, stats)
            assert stats["lines_host"] == 0 and stats["lines_dev"] == n_lines, (member, bs, stats)
            # the text did not go up: the compressed members did, and the text came down
            assert stats["bytes_up"] < len(text) and stats["inflate"]["bytes_down"] >= len(text), (member, bs, stats)
            assert stats["inflate"]["bytes_up"] >= len(data) - 26 * n_members


@pytest.mark.parametrize("n", [1, 9, 65, 300])
def test_device_inflate_lines_straddling_slabs(n, tmp_path, monkeypatch, engine_for):
    """The same grid with slabs of 70 000 bytes and a pad of 32 768 (ic.straddling_cases).  Every slab but the first carries up to 32 768
    bytes of the text before it in front of its pad, and those tails still go up from the host: slabs of small members hold 4.5 KB of text
    and carry more than they hold, and a text of a few KB is carried whole into the slab of the end marker, so "less than the text" cannot
    hold everywhere.  What holds everywhere: the slabs are cut the same way with and without the device inflate, and without it every
    slab goes up with its tail and its text, so the device inflate must send exactly len(text) bytes less.  "Less than the text" is
    asserted as well wherever the tails cannot reach it: there are at most as many slabs as members, the first carries nothing and the
    others 32 768 bytes at most, so where 32 768 * (members - 1) < len(text); n = 300 with members of 40 000 and 65 280 bytes is such a case."""
    names = sample_names(n)
    e = engine_for(n)
    bounded = []
    for args, member in ic.straddling_cases(n):
        text, n_lines = corpus(names, **args)
        data = bgzf_bytes(text, block=member)
        n_members = len(ic.members_of(data))
        path = str(tmp_path / ("s%d.bgzf" % member))
        open(path, "wb").write(data)
        for bs in (1, 37, 3000):
            monkeypatch.setenv("SEERHIP_ROUTE", STRADDLE)
            want, _ = read_blocks(path, names, bs)
            _, text_up = read_blocks(path, names, bs, engine=e)
            monkeypatch.setenv("SEERHIP_ROUTE", STRADDLE + ",kmer_inflate=1")
            got, stats = read_blocks(path, names, bs, engine=e)
            assert_same_blocks(got, want, (member, bs))
            assert stats["inflate"]["members_host"] == 0 and stats["inflate"]["members_dev"] == n_members, (member, bs, stats)
            assert stats["lines_host"] <= 2 and stats["lines_dev"] + stats["lines_host"] == n_lines, (member, bs, stats)
            assert text_up["inflate"]["members_dev"] == 0 and stats["bytes_up"] == text_up["bytes_up"] - len(text), (member, bs, stats, text_up)
            if 32768 * (n_members - 1) < len(text):
                assert stats["bytes_up"] < len(text), (member, bs, stats)
                bounded.append(member)
    assert n != 300 or {40000, 65280} <= set(bounded)


def test_damaged_and_truncated_files_read_as_on_the_host_route(tmp_path, monkeypatch, engine_for):
    names = sample_names(65)
    text, _ = corpus(names, n_lines=150, seed=2)
    data = bgzf_bytes(text, block=10000)
    for what, bad in (("flipped", ic.flip_member_byte(data, 2)), ("truncated", ic.truncate_last_member(data))):
        path = str(tmp_path / (what + ".bgzf"))
        open(path, "wb").write(bad)
        errs = []
        for route, engine in ((None, None), ("kmer_inflate=1", engine_for(65))):
            if route:
                monkeypatch.setenv("SEERHIP_ROUTE", route)
            else:
                monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
            with pytest.raises(IOError) as ex:
                read_blocks(path, names, 3000, engine=engine)
            errs.append(str(ex.value))
        assert errs[0] == errs[1] and errs[0].startswith("BGZF"), (what, errs)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _cli(args, module="pyseer_amd"):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    env.pop("SEERHIP_ROUTE", None)
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def kmers_bgzf(tmp_path_factory):
    """tests/golden/cli/kmers.gz decoded and written again as BGZF, in members of 20 000 bytes"""
    import gzip
    path = str(tmp_path_factory.mktemp("inflate") / "kmers.bgzf.gz")
    open(path, "wb").write(bgzf_bytes(gzip.open(os.path.join(CLI, "kmers.gz")).read(), block=20000))
    return path


@pytest.mark.parametrize("name", ["fixed", "lmm"])
def test_cli_prints_the_same_bytes(name, kmers_bgzf):
    args = [kmers_bgzf if a == "kmers.gz" else a for a in CASES[name]]
    assert kmers_bgzf in args
    plain = _cli(args)
    assert _cli(args + ["--device-inflate"]) == plain
    assert len(plain[0].splitlines()) > 10


def test_similarity_prints_the_same_bytes(kmers_bgzf):
    args = ["samples50.txt", "--kmers", kmers_bgzf]
    plain = _cli(args, module="pyseer_amd.similarity")
    assert _cli(args + ["--device-inflate"], module="pyseer_amd.similarity") == plain
    assert plain[0] == open(os.path.join(CLI, "expected", "similarity_kmers.tsv"), "rb").read()
