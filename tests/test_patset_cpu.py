"""The host half of --count-patterns: the 128-bit key of a packed row (csrc/patset_hash.h through sh_patset_hash_rows -- the definition the
device shares) and `python -m pyseer_amd.count_patterns`, the reference's scripts/count_patterns.py for an existing pattern file.

tests/golden/patterns: patterns.txt is 200 hash_pattern lines over 37 distinct presence vectors; the expected_*.txt files are what the
reference's script printed for it (its `LC_ALL=C sort -u | wc -l`, '%.2E' % Decimal(alpha / count)): no arguments, --threshold, and
--alpha 0.01 --cores 2."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = os.path.join(ROOT, "tests", "golden", "patterns")


def _keys(bits, n):
    from pyseer_amd.engine import hash_rows
    k = hash_rows(bits, n)
    assert k.shape == (bits.shape[0], 2) and k.dtype == np.uint64
    return k


def _distinct_rows(rng, V, n):
    """V distinct random rows of n samples, packed, padding bits zero"""
    from pyseer_amd.engine import pack_variants
    K = (rng.random((V + V // 8 + 64, n)) < 0.5).astype(np.uint8)
    K = np.unique(K, axis=0)
    assert K.shape[0] >= V
    K = K[rng.permutation(K.shape[0])[:V]]
    return K, pack_variants(K)


def _garbage_padding(rng, bits, n):
    """the same rows with random bits from sample n on"""
    g = bits.copy()
    noise = rng.integers(0, 256, size=g.shape, dtype=np.uint8)
    full, rem = n // 8, n % 8
    if rem:
        g[:, full] |= noise[:, full] & np.uint8((0xFF << rem) & 0xFF)
        full += 1
    g[:, full:] = noise[:, full:]
    return g


@pytest.mark.parametrize("n", [50, 64, 65, 130])
def test_hash_rows_padding_boundary_and_distinctness(n):
    rng = np.random.default_rng(n)
    V = 100000
    K, bits = _distinct_rows(rng, V, n)
    assert bits.shape[1] * 8 >= n
    k = _keys(bits, n)
    # 10^5 distinct rows -> 10^5 distinct keys (and distinct in each half: 64 bits over 10^5 rows collide with probability 3e-10)
    assert np.unique(k, axis=0).shape[0] == V
    assert np.unique(k[:, 0]).shape[0] == V and np.unique(k[:, 1]).shape[0] == V
    # padding bits never matter: random garbage behind sample n - 1, and a wider row of the same samples
    garb = _garbage_padding(rng, bits, n)
    if bits.shape[1] * 8 > n:
        assert (garb != bits).any()
    assert (_keys(garb, n) == k).all()
    wide = np.concatenate([bits, rng.integers(0, 256, size=(V, 5), dtype=np.uint8)], axis=1)
    assert (_keys(_garbage_padding(rng, wide, n), n) == k).all()
    # the last sample's bit is part of the key
    flip = garb[:2000].copy()
    flip[:, (n - 1) // 8] ^= np.uint8(1 << ((n - 1) % 8))
    kf = _keys(flip, n)
    assert (kf[:, 0] != k[:2000, 0]).all() and (kf[:, 1] != k[:2000, 1]).all()
    # equal rows give equal keys, wherever they stand
    perm = rng.permutation(V)
    assert (_keys(bits[perm], n) == k[perm]).all()
    rep = np.repeat(bits[:50], 3, axis=0)
    assert (_keys(rep, n) == np.repeat(k[:50], 3, axis=0)).all()


def test_hash_rows_zero_and_full_rows_and_bad_shapes():
    from pyseer_amd import _abi
    n = 130
    bits = np.zeros((2, 17), dtype=np.uint8)
    bits[1] = 0xFF
    k = _keys(bits, n)
    assert (k[0] != k[1]).all()
    assert (_keys(np.zeros((1, 24), dtype=np.uint8), n) == k[0]).all()
    with pytest.raises(_abi.SeerHipError):
        _keys(np.zeros((1, 16), dtype=np.uint8), n)              # 128 bits < 130 samples


def _tool(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pyseer_amd.count_patterns"] + list(args), cwd=PAT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def test_count_patterns_tool_prints_what_the_reference_prints():
    lines = open(os.path.join(PAT, "patterns.txt"), "rb").read().splitlines()
    assert len(lines) == 200 and len(set(lines)) == 37
    want = open(os.path.join(PAT, "expected_default.txt"), "rb").read()
    assert want == b"Patterns:\t37\nThreshold:\t1.35E-03\n"
    assert _tool("patterns.txt") == want
    assert _tool("patterns.txt", "--threshold") == open(os.path.join(PAT, "expected_threshold.txt"), "rb").read() == b"1.35E-03\n"
    assert _tool("patterns.txt", "--alpha", "0.01", "--cores", "2", "--memory", "64", "--temp", "/nowhere") == \
        open(os.path.join(PAT, "expected_alpha001.txt"), "rb").read()


def test_threshold_goes_through_decimal_as_in_the_reference():
    from decimal import Decimal
    from pyseer_amd.count_patterns import result_text, threshold_text, digests_of_lines
    for alpha, n in ((0.05, 37), (0.05, 1), (0.01, 3), (0.05, 40000000), (1e-3, 7), (0.05, 8)):
        assert threshold_text(alpha, n) == '%.2E' % Decimal(alpha / float(n))
        assert result_text(n, alpha) == "Patterns:\t%d\nThreshold:\t%s\n" % (n, '%.2E' % Decimal(alpha / float(n)))
    assert result_text(0) == "Patterns:\t0\nThreshold:\tNA\n"
    # the digest bytes behind the lines (the keys of host-made patterns)
    import binascii
    text = open(os.path.join(PAT, "patterns.txt"), "rb").read()
    d = digests_of_lines(text)
    assert d.shape == (200, 16) and d.dtype == np.uint8
    for i, line in enumerate(text.splitlines()):
        assert d[i].tobytes() == binascii.a2b_base64(line)
