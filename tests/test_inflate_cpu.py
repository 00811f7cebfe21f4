"""The DEFLATE core of the device inflate (csrc/inflate_dev.h) built for the host, and the reader's inflate hook without a device.
zlib is the yardstick of the decoder (decompressobj(wbits=-15)), the host route of the reader (sh_reader_open) of everything above it.
The member corpus is tests/_inflate_corpus.py; it is checked against zlib itself first, so a wrong fixture cannot pass as a decoder finding.
SEERHIP_ROUTE kmer_inflate=1 with a reader opened without a context runs the same hook as on the device (csrc/inflate_api.inc), with the
host build of the kernel's decoder in the kernel's place."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inflate_corpus as ic  # noqa: E402
from _kmer_dev_corpus import assert_same_blocks, corpus, sample_names  # noqa: E402
from _vcf_text import bgzf_bytes  # noqa: E402

from pyseer_amd import _abi  # noqa: E402
from pyseer_amd.input import NativeKmerReader  # noqa: E402

HOST_RULE = NativeKmerReader.DEVICE_HOST_RULE
CANARY = 64


@pytest.fixture(scope="module")
def good():
    return ic.well_formed()


@pytest.fixture(scope="module")
def bad():
    return ic.malformed()


def inflate_host(cdata, isize):
    """(status, produced, bytes written into the window, canaries untouched) of sh_inflate_host on a buffer with 64 canary bytes either side"""
    lib = _abi.load()
    buf = np.full(isize + 2 * CANARY, 0xA5, dtype=np.uint8)
    src = np.frombuffer(cdata, dtype=np.uint8).copy() if cdata else np.zeros(1, dtype=np.uint8)
    produced = C.c_int64(-1)
    st = lib.sh_inflate_host(src.ctypes.data_as(_abi.c_u8p), len(cdata), buf[CANARY:].ctypes.data_as(_abi.c_u8p), isize, C.byref(produced))
    intact = bool((buf[:CANARY] == 0xA5).all() and (buf[CANARY + isize:] == 0xA5).all())
    return st, produced.value, buf[CANARY:CANARY + isize].tobytes(), intact


def test_the_corpus_is_what_it_says(good, bad):
    assert 200 <= len(good) <= 400 and len(bad) >= 20
    assert {len(t) for _, _, t in good} >= set(ic.SIZES)
    for name, cdata, text in good:
        assert ic.yardstick(cdata, len(text)) == text, name
    for name, cdata, isize, _ in bad:
        with pytest.raises((zlib.error, ValueError)):
            ic.yardstick(cdata, isize)
    # every status of the decoder has its member
    want = set(ic.statuses()) - {"SHI_OK"}
    assert {s for _, _, _, s in bad} == want, want
    # stored, fixed and dynamic blocks are all there (the block type of a member's first block)
    assert {(c[0] >> 1) & 3 for _, c, _ in good} == {0, 1, 2}
    # the skewed alphabet does force 15-bit literal codes (a walk over the first block's header), at every level but 0 from 32 768 bytes on
    deep = [name for name, c, _ in good if name.startswith("skewed-") and ic.first_block_code_lengths(c)[1] == 15]
    assert set(deep) == {"skewed-%d-l%d" % (n, lv) for n in (32768, 32769, 65280, 65536) for lv in (1, 6, 9)}, deep
    # the flushes did put their empty stored blocks into the members of several blocks
    for name in ic.FLUSHES:
        body, _, marks = ic.flush_member(name)
        assert marks >= 3 and body.count(ic.EMPTY_STORED) >= marks, (name, marks)
        assert body == dict((n, c) for n, c, _ in good)["blocks-" + name]


def test_host_core_decodes_every_well_formed_member(good):
    for name, cdata, text in good:
        st, produced, out, intact = inflate_host(cdata, len(text))
        assert st == 0 and produced == len(text) and intact, (name, st, produced)
        assert out == text, name


def test_host_core_refuses_every_malformed_member(bad):
    codes = ic.statuses()
    for name, cdata, isize, status in bad:
        st, produced, _, intact = inflate_host(cdata, isize)
        assert st == codes[status], (name, st, status)
        assert 0 <= produced <= isize and intact, name


def read_blocks(path, names, block_size, engine=None):
    r = NativeKmerReader(path, names, block_size, 256, engine=engine)
    try:
        blocks = [(b.copy(), c.copy(), blob, off) for b, c, blob, off in r.raw_blocks()]
        stats = r.inflate_stats() if engine is not None else None
    finally:
        r.close()
    return blocks, stats


@pytest.mark.parametrize("n", [1, 9, 65, 300])
def test_hook_without_a_device_equals_the_host_route(n, tmp_path, monkeypatch):
    names = sample_names(n)
    for member in (1, 100, 40000, 65280):
        text, n_lines = corpus(names, n_lines=ic.LINES[member], seed=n)
        data = bgzf_bytes(text, block=member)
        n_members = len(ic.members_of(data))
        path = str(tmp_path / ("k%d.bgzf" % member))
        open(path, "wb").write(data)
        for bs in (1, 37, 3000):
            monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
            want, _ = read_blocks(path, names, bs)
            assert sum(len(b[1]) for b in want) == n_lines
            monkeypatch.setenv("SEERHIP_ROUTE", "kmer_inflate=1")
            got, stats = read_blocks(path, names, bs, engine=HOST_RULE)
            assert_same_blocks(got, want, (member, bs))
            assert stats["members_host"] == 0 and stats["members_dev"] == n_members, (member, bs, stats, n_members)
    # without the key the hook is not there, and the argument of the reader sets it for that reader alone
    monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
    got, stats = read_blocks(path, names, 3000, engine=HOST_RULE)
    assert_same_blocks(got, want, "key unset")
    assert stats["members_dev"] == 0 and stats["members_host"] == 0
    r = NativeKmerReader(path, names, 3000, engine=HOST_RULE, inflate=True)
    assert sum(len(b[1]) for b in r.raw_blocks()) == n_lines and r.inflate_stats()["members_dev"] == n_members
    r.close()
    assert "SEERHIP_ROUTE" not in os.environ
    # ... and it holds for one open: the next reader of this thread is as the key says again; False overrides a key that is set
    got, stats = read_blocks(path, names, 3000, engine=HOST_RULE)
    assert stats["members_dev"] == 0
    monkeypatch.setenv("SEERHIP_ROUTE", "kmer_inflate=1")
    r = NativeKmerReader(path, names, 3000, engine=HOST_RULE, inflate=False)
    assert sum(len(b[1]) for b in r.raw_blocks()) == n_lines and r.inflate_stats()["members_dev"] == 0
    r.close()


@pytest.mark.parametrize("n", [1, 9, 65, 300])
def test_hook_without_a_device_lines_straddling_slabs(n, tmp_path, monkeypatch):
    """the same grid with slabs of 70 000 bytes and a pad of 32 768 (ic.straddling_cases): lines cross slabs all the time"""
    names = sample_names(n)
    for args, member in ic.straddling_cases(n):
        text, n_lines = corpus(names, **args)
        data = bgzf_bytes(text, block=member)
        path = str(tmp_path / ("s%d.bgzf" % member))
        open(path, "wb").write(data)
        for bs in (1, 37, 3000):
            monkeypatch.setenv("SEERHIP_ROUTE", "reader_slab=70000,reader_pad=32768")
            want, _ = read_blocks(path, names, bs)
            assert sum(len(b[1]) for b in want) == n_lines
            monkeypatch.setenv("SEERHIP_ROUTE", "reader_slab=70000,reader_pad=32768,kmer_inflate=1")
            got, stats = read_blocks(path, names, bs, engine=HOST_RULE)
            assert_same_blocks(got, want, (member, bs))
            assert stats["members_host"] == 0 and stats["members_dev"] == len(ic.members_of(data)), (member, bs, stats)


def test_damaged_and_truncated_files_read_as_on_the_host_route(tmp_path, monkeypatch):
    names = sample_names(65)
    text, _ = corpus(names, n_lines=150, seed=2)
    data = bgzf_bytes(text, block=10000)
    for what, bad in (("flipped", ic.flip_member_byte(data, 2)), ("truncated", ic.truncate_last_member(data))):
        path = str(tmp_path / (what + ".bgzf"))
        open(path, "wb").write(bad)
        errs = []
        for route, engine in ((None, None), ("kmer_inflate=1", HOST_RULE)):
            if route:
                monkeypatch.setenv("SEERHIP_ROUTE", route)
            else:
                monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
            with pytest.raises(IOError) as ex:
                read_blocks(path, names, 3000, engine=engine)
            errs.append(str(ex.value))
        assert errs[0] == errs[1] and errs[0].startswith("BGZF"), (what, errs)
