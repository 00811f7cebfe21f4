"""The run-wide set of distinct presence patterns on the device (include/seerhip.h sh_patset_*; csrc/patset_kernels.hip, patset_api.inc): what the
reference's scripts/count_patterns.py counts with `sort -u | wc -l` over an --output-patterns file.  Through the ABI, with a table of 1024 slots
to begin with, so that the sizes used here cross several growths.  Check values are numpy's: distinct masked rows, distinct keys, distinct
md5 lines."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _engine(n):
    from pyseer_amd.engine import Engine
    return Engine(n)


def _set(e, slots=1024):
    from pyseer_amd.engine import PatternSet
    return PatternSet(e, slots)


def _masked(bits, n):
    m = bits.copy()
    full, rem = n // 8, n % 8
    if rem:
        m[:, full] &= np.uint8((1 << rem) - 1)
        full += 1
    m[:, full:] = 0
    return m


def _pool_rows(n, n_rows, n_distinct, seed):
    """n_rows packed rows drawn from n_distinct patterns (the all-zero and the all-ones row among them), random garbage in the padding"""
    from pyseer_amd.engine import pack_variants
    rng = np.random.default_rng(seed)
    K = np.unique((rng.random((4 * n_distinct, n)) < 0.4).astype(np.uint8), axis=0)
    K = K[(K.sum(axis=1) > 0) & (K.sum(axis=1) < n)][:n_distinct - 2]
    K = np.concatenate([K, np.zeros((1, n), np.uint8), np.ones((1, n), np.uint8)])
    assert K.shape[0] == n_distinct
    pick = np.concatenate([np.arange(n_distinct), rng.integers(0, n_distinct, n_rows - n_distinct)])
    bits = pack_variants(K[rng.permutation(pick)])
    bits = np.concatenate([bits, np.zeros((n_rows, 3), np.uint8)], axis=1)      # (a row width that is no multiple of eight bytes as well)
    noise = rng.integers(0, 256, size=bits.shape, dtype=np.uint8)
    bits = _masked(bits, n) | (noise & ~_masked(np.full_like(bits, 0xFF), n))
    return np.ascontiguousarray(bits)


@pytest.mark.parametrize("n", [130, 64, 65])
@pytest.mark.parametrize("trim", [False, True])
def test_rows_count_distinct_patterns(n, trim):
    """3000 rows from 41 patterns; trim: the rows cut to whole 64-bit words where that still holds n samples (the aligned read path)"""
    bits = _pool_rows(n, 3000, 41, n)
    if trim:
        w = (n + 63) // 64 * 8
        bits = np.ascontiguousarray(bits[:, :w]) if w <= bits.shape[1] else np.ascontiguousarray(np.concatenate([bits, np.zeros((3000, w - bits.shape[1]), np.uint8)], axis=1))
    want = len(np.unique(_masked(bits, n), axis=0))
    assert want == 41
    e = _engine(n); ps = _set(e)
    ps.add_rows(bits)
    assert ps.count() == want
    ps.add_rows(bits)
    assert ps.count() == want
    ps.add_rows(bits[::-1][:1])
    assert ps.count() == want
    ps.close(); e.close()


@pytest.mark.parametrize("n", [130, 64, 65])
def test_host_and_device_give_the_same_keys(n):
    from pyseer_amd.engine import hash_rows
    bits = _pool_rows(n, 3000, 41, 7 * n)
    e = _engine(n); ps = _set(e)
    ps.add_keys(hash_rows(bits, n))
    assert ps.count() == 41
    ps.add_rows(bits)
    assert ps.count() == 41
    import torch
    ps.add_rows_dev(torch.from_numpy(bits).cuda())
    assert ps.count() == 41
    ps.close(); e.close()


def test_keys_with_the_same_first_half():
    """random data never reaches the second word's compare-and-swap with a foreign key in the slot: 40 keys with equal word 0"""
    rng = np.random.default_rng(1)
    keys = np.empty((40, 2), dtype=np.uint64)
    keys[:, 0] = np.uint64(0x1234567890ABCDEF)
    keys[:, 1] = np.unique(rng.integers(1, 1 << 62, 80, dtype=np.uint64))[:40]
    e = _engine(10); ps = _set(e)
    ps.add_keys(keys)
    assert ps.count() == 40
    ps.add_keys(keys[::-1])
    assert ps.count() == 40
    ps.close(); e.close()


def test_probe_chains_through_a_growth():
    """300 keys with one home slot (low 24 bits of word 0 zero) in a 1024-slot table, found again after the table has grown"""
    rng = np.random.default_rng(2)
    keys = np.empty((300, 2), dtype=np.uint64)
    keys[:, 0] = np.unique(rng.integers(1, 1 << 38, 600, dtype=np.uint64))[:300] << np.uint64(24)
    keys[:, 1] = rng.integers(0, 1 << 62, 300, dtype=np.uint64)
    e = _engine(10); ps = _set(e)
    ps.add_keys(keys)
    assert ps.info() == (300, 1024, 0)
    ps.add_keys(keys)                                              # room for 300 + 300 keys at load 1/2 = 1200 slots: the table grows first
    assert ps.info() == (300, 2048, 1)
    more = rng.integers(0, 1 << 63, (2000, 2), dtype=np.uint64) | np.uint64(1)          # (odd word 0: none of the 300)
    n_more = len(np.unique(more, axis=0))
    ps.add_keys(more)
    d, slots, growths = ps.info()
    assert d == 300 + n_more and growths >= 1 and slots >= 2 * d
    ps.add_keys(keys)
    assert ps.count() == 300 + n_more
    ps.close(); e.close()


def test_one_key_65536_times_in_one_call():
    keys = np.tile(np.array([[0xDEADBEEF12345678, 0x0123456789ABCDEF]], dtype=np.uint64), (65536, 1))
    e = _engine(10); ps = _set(e)
    ps.add_keys(keys)
    assert ps.count() == 1
    ps.close(); e.close()


def test_growth_keeps_every_key():
    rng = np.random.default_rng(3)
    keys = np.unique(rng.integers(0, 1 << 63, (20500, 2), dtype=np.uint64), axis=0)
    keys = keys[rng.permutation(len(keys))[:20000]]
    assert len(keys) == 20000
    e = _engine(10); ps = _set(e)
    done = 0
    for lo in range(0, 20000, 3000):
        ps.add_keys(keys[lo:lo + 3000])
        done = min(20000, lo + 3000)
        d, slots, growths = ps.info()
        assert d == done and slots >= 2 * d, (lo, d, slots)
    assert growths >= 4
    ps.add_keys(keys[:3000])
    assert ps.count() == 20000
    ps.close(); e.close()


def test_marker_halves_are_accepted():
    """(~0, ~0) is a key like any other: stored as (0, 0), with which it therefore counts as one (include/seerhip.h)"""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    e = _engine(10); ps = _set(e)
    ps.add_keys(np.array([[full, full]], dtype=np.uint64))
    assert ps.count() == 1
    ps.add_keys(np.array([[full, full]], dtype=np.uint64))
    assert ps.count() == 1
    ps.add_keys(np.array([[full, 5], [7, full], [full, 5]], dtype=np.uint64))
    assert ps.count() == 3
    ps.add_keys(np.array([[0, 0], [0, 5], [7, 0]], dtype=np.uint64))
    assert ps.count() == 3
    ps.close(); e.close()


def test_set_is_needed_and_single():
    from pyseer_amd import _abi
    e = _engine(10)
    lib = _abi.load()
    assert lib.sh_patset_add_keys(e._h, np.zeros(2, np.uint64).ctypes.data_as(_abi.C.POINTER(_abi.C.c_uint64)), 1) == _abi.SH_EINVAL
    with pytest.raises(_abi.SeerHipError):
        _set(e, 1000)                                               # not a power of two
    ps = _set(e)
    with pytest.raises(_abi.SeerHipError):
        _set(e)
    ps.close()
    ps = _set(e, 0)
    assert ps.info() == (0, 1 << 20, 0)
    ps.close(); e.close()


# ---- the job stream ---------------------------------------------------------------------------------------------------------------------------
N_JOB = 50
SIZES = [1, 255, 256, 257, 1000]


@functools.lru_cache(maxsize=None)
def _job_blocks():
    from pyseer_amd.engine import pack_variants
    from pyseer_amd.sink import names_blob
    rng = np.random.default_rng(50)
    af = np.concatenate([rng.uniform(0.0, 0.08, 12), rng.uniform(0.15, 0.85, 40), rng.uniform(0.93, 1.0, 8)])
    pool = np.unique((rng.random((60, N_JOB)) < af[:, None]).astype(np.uint8), axis=0)
    blocks, at = [], 0
    for v in SIZES:
        K = pool[rng.integers(0, len(pool), v)]
        blob, off = names_blob(["K%06d" % (at + i) for i in range(v)])
        blocks.append((pack_variants(K), K.sum(axis=1).astype(np.int32), blob, off))
        at += v
    return pool, blocks


def _job_engine(lmm, dedup):
    from pyseer_amd.engine import Engine
    from pyseer_amd.model import fit_null
    rng = np.random.default_rng(8)
    e = Engine(N_JOB); e.set_af_filter(0.1, 0.9); e.set_dedup(dedup)
    y = (rng.random(N_JOB) < 0.4).astype(float)
    if lmm:
        from pyseer_amd.lmm import initialise_lmm_arrays
        G_ = (rng.random((200, N_JOB)) < 0.3).astype(float)
        U, S, h2, nll, Cc = initialise_lmm_arrays(G_.T @ G_, y)
        e.lmm_setup(U, S, y, Cc, h2)
    else:
        W = rng.standard_normal((N_JOB, 2)); W /= np.abs(W).max(axis=0)
        e0 = np.zeros((0, 0))
        e.glm_setup(y, W, False, fit_null(y, W, e0, False).llf, fit_null(y, W, e0, False, firth=True), 1.0, 1.0)
    return e


def _run_job(lmm, dedup, patterns, pattern_count):
    from pyseer_amd.engine import Job, PatternSet
    _, blocks = _job_blocks()
    e = _job_engine(lmm, dedup)
    ps = PatternSet(e, 1024) if pattern_count else None
    job = Job(e, lmm, False, patterns=patterns, pattern_count=pattern_count)
    lines, tested = set(), 0
    for b in blocks:
        job.submit(*b)
        while job.pending() >= job.depth:
            t, c, _ = job.collect(); tested += c[1]
            if patterns:
                text = bytes(job.patterns()); lines.update(text[i:i + 25] for i in range(0, len(text), 25))
    while job.pending():
        t, c, _ = job.collect(); tested += c[1]
        if patterns:
            text = bytes(job.patterns()); lines.update(text[i:i + 25] for i in range(0, len(text), 25))
    n = ps.count() if ps is not None else None
    job.close()
    if ps is not None:
        assert ps.count() == n
        ps.close()
    e.close()
    return n, len(lines), tested


@functools.lru_cache(maxsize=None)
def _md5_lines():
    """distinct 25-byte lines over all job.patterns() texts of the fixed-effects job, counting off"""
    _, n_lines, tested = _run_job(False, True, True, False)
    return n_lines, tested


@pytest.mark.parametrize("lmm,dedup,patterns", [(False, True, True), (False, True, False), (False, False, True), (True, True, True), (True, False, False)])
def test_job_counts_the_patterns_it_tests(lmm, dedup, patterns):
    pool, blocks = _job_blocks()
    want, want_tested = _md5_lines()
    # the same number from the rows themselves: distinct rows whose carrier frequency lies in the AF window
    rows = np.concatenate([b[0] for b in blocks]); cnt = np.concatenate([b[1] for b in blocks])
    keep = (cnt / N_JOB >= 0.1) & (cnt / N_JOB <= 0.9)
    assert 0 < keep.sum() < len(keep) and want_tested == int(keep.sum())
    assert want == len(np.unique(_masked(rows[keep], N_JOB), axis=0)) and 20 < want <= len(pool)
    n, n_lines, tested = _run_job(lmm, dedup, patterns, True)
    assert tested == want_tested
    assert n == want
    if patterns:
        assert n_lines == want


def test_job_without_a_set_is_refused():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Job
    e = _job_engine(False, True)
    with pytest.raises(_abi.SeerHipError):
        Job(e, False, False, pattern_count=True)
    e.close()
