"""A packed cache served to a subset or another order of its samples, without a device: the host restatement of k_rows_select
(sh_select_rows_host) against numpy, the iterator's `select="host"` against the native reader over the same samples, and the tool that
writes a cache over all isolates (python -m pyseer_amd.pack).  SEERHIP_ROUTE cache_select (csrc/route.h) is the route key of this path."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pyseer_amd import _abi
from pyseer_amd.engine import select_rows_host
from pyseer_amd.input import (check_packed_cache, iter_packed_blocks_cached, iter_packed_blocks_native, packed_cache_complete)
from pyseer_amd.packing import row_bytes_for

import _cache_select as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMERS = os.path.join(cs.CLI, "kmers.gz")


@pytest.mark.parametrize("n_src", cs.N_SRC)
def test_host_rule_equals_numpy(n_src):
    rng = np.random.default_rng(n_src)
    for V in cs.V_ROWS:
        bits, _ = cs.source_rows(V, n_src, rng)
        for n_dst in cs.n_dsts(n_src):
            for kind in cs.MAP_KINDS:
                m = cs.make_map(kind, n_src, n_dst, rng)
                got_bits, got_counts = select_rows_host(bits, n_src, m)
                cs.check_selected(got_bits, got_counts, bits, n_src, m)


def test_host_rule_takes_rows_wider_than_the_samples_need():
    rng = np.random.default_rng(5)
    bits, _ = cs.source_rows(9, 100, rng)
    wide = np.ascontiguousarray(np.concatenate([bits, np.full((9, 8), 0xFF, dtype=np.uint8)], axis=1))
    m = cs.make_map("permuted", 100, 65, rng)
    got_bits, got_counts = select_rows_host(wide, 100, m)
    cs.check_selected(got_bits, got_counts, bits, 100, m)


def test_bad_maps_are_refused():
    bits, _ = cs.source_rows(3, 64, np.random.default_rng(0))
    with pytest.raises(_abi.SeerHipError, match="selected twice"):
        select_rows_host(bits, 64, [3, 5, 3])
    with pytest.raises(_abi.SeerHipError, match="outside the source row"):
        select_rows_host(bits, 64, [0, 64])
    with pytest.raises(_abi.SeerHipError, match="outside the source row"):
        select_rows_host(bits, 64, [-1])
    with pytest.raises(_abi.SeerHipError):
        select_rows_host(bits[:0], 64, [1, 1])                                    # (also with no row to select)
    with pytest.raises(AssertionError):
        select_rows_host(bits, 65, [0])                                           # rows too narrow for n_src


def _pack(tmp_path, samples, name="all.seerpack", block=37, expect=0):
    listing = str(tmp_path / (name + ".samples.txt"))
    with open(listing, "w") as fh:
        fh.write("".join(s + "\n" for s in samples))
    out = str(tmp_path / name)
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", "pyseer_amd.pack", listing, "--kmers", KMERS, "-o", out, "--block", str(block)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == expect, r.stderr.decode()[-2000:]
    return out, r.stderr.decode()


@pytest.fixture(scope="module")
def all_cache(tmp_path_factory):
    samples = cs.all_samples()
    assert len(samples) == 1837
    path, err = _pack(tmp_path_factory.mktemp("pack"), samples)
    assert "200 variants over 1837 samples" in err
    return path, samples


def _flat(blocks):
    blocks = list(blocks)
    return ([n for b in blocks for n in b.names], [a for b in blocks for a in b.afs], [int(s) for b in blocks for s in b.status],
            np.concatenate([b.bits for b in blocks]))


def _no_obs(text):
    return [l for l in text.splitlines() if l.startswith("No observations of ")]


def test_pack_writes_a_complete_cache_and_refuses_duplicates(all_cache, tmp_path):
    path, samples = all_cache
    assert packed_cache_complete(path) and not os.path.exists(path + ".part")
    out, err = _pack(tmp_path, samples[:5] + samples[2:3], name="dup.seerpack", expect=1)
    assert "listed twice" in err and samples[2] in err and not os.path.exists(out) and not os.path.exists(out + ".part")


@pytest.mark.parametrize("which", ["subset", "subset_reversed", "supersubset"])
def test_iterator_selects_like_the_reader_reads(all_cache, which, capsys, monkeypatch):
    monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
    path, samples = all_cache
    p = cs.phenotype("supersubset.pheno" if which == "supersubset" else "subset.pheno")
    assert len(p) == (10 if which == "supersubset" else 50)
    if which == "subset_reversed":
        p = p.iloc[::-1]
    capsys.readouterr()
    want = _flat(iter_packed_blocks_native(p, KMERS, 0.01, 0.99, 37))
    want_said = _no_obs(capsys.readouterr().err)
    assert len(want[0]) == 200
    for bs in (37, 100000):
        got = _flat(iter_packed_blocks_cached(p, path, 0.01, 0.99, bs, select="host"))
        got_said = _no_obs(capsys.readouterr().err)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
        assert got[3].shape[1] == row_bytes_for(len(p)) and np.array_equal(got[3], want[3])
        assert got_said == want_said
        raw = list(iter_packed_blocks_cached(p, path, 0.01, 0.99, bs, raw=True, select="host"))       # the job stream's blocks: the same rows
        assert _no_obs(capsys.readouterr().err) == want_said
        assert np.array_equal(np.concatenate([b.bits for b in raw]), want[3]) and not any(b.dma for b in raw)
        assert np.array_equal(np.concatenate([b.counts for b in raw]), np.round(np.array(want[1]) * len(p)).astype(np.int32))
    # the header check alone accepts the same caches, and says which source bit every run sample is
    m = check_packed_cache(p, path, select="host")
    assert [samples[i] for i in m] == [str(x) for x in p.index]
    # without `select` nothing has changed: another list or order is another cache
    with pytest.raises(ValueError, match="different sample list / order"):
        list(iter_packed_blocks_cached(p, path, 0.01, 0.99, 37))
    with pytest.raises(ValueError, match="different sample list / order"):
        check_packed_cache(p, path)
    # ... and so it is under SEERHIP_ROUTE cache_select=0, whatever the caller asks for
    monkeypatch.setenv("SEERHIP_ROUTE", "cache_select=0")
    with pytest.raises(ValueError, match="different sample list / order"):
        list(iter_packed_blocks_cached(p, path, 0.01, 0.99, 37, select="host"))


def test_same_list_takes_the_old_path_and_a_missing_sample_the_old_message(tmp_path, monkeypatch):
    monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
    p = cs.phenotype("subset.pheno")
    own, _ = _pack(tmp_path, [str(x) for x in p.index], name="own.seerpack")
    assert check_packed_cache(p, own, select="host") is None
    want = _flat(iter_packed_blocks_cached(p, own, 0.01, 0.99, 64))
    got = _flat(iter_packed_blocks_cached(p, own, 0.01, 0.99, 64, select="host"))
    assert got[:3] == want[:3] and np.array_equal(got[3], want[3])
    fewer, _ = _pack(tmp_path, [str(x) for x in p.index[:-1]], name="fewer.seerpack")
    for kw in ({}, {"select": "host"}):
        with pytest.raises(ValueError) as ex:
            list(iter_packed_blocks_cached(p, fewer, 0.01, 0.99, 64, **kw))
        assert "packed cache was written for a different sample list / order (49 vs 50 samples)" in str(ex.value)
        with pytest.raises(ValueError) as ex:
            check_packed_cache(p, fewer, **kw)
        assert "(49 vs 50 samples)" in str(ex.value)
