"""`--count-patterns FILE` on the command line (tests/golden/cli): the number of distinct presence patterns of the tested variants and the
Bonferroni threshold, as the reference's scripts/count_patterns.py prints them for the file --output-patterns writes.  The pattern file is
the yardstick (tests/test_cli_gpu.py and tests/test_job_gpu.py hold it to the reference's hashes): the count must be the number of its
distinct lines on every single-device route, and asking for the count must change nothing else of the run."""
import os
import subprocess
import sys
from decimal import Decimal

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
VCF = os.path.join(ROOT, "tests", "golden", "vcf")
ENET = os.path.join(ROOT, "tests", "golden", "enet")

KMERS = ["--kmers", "kmers.gz", "--phenotypes", "subset.pheno"]
FIXED = KMERS + ["--distances", "distances50.tsv"]
LMM = ["--similarity", "similarity50.tsv", "--lmm"]
ROUTES = {
    "fixed": FIXED,
    "lmm": KMERS + LMM,
    "python_sink": FIXED + ["--python-sink"],
    "serial_sink": KMERS + LMM + ["--serial-sink"],
    "no_dedup": FIXED + ["--no-dedup"],
    "rtab": ["--pres", "kmers120.Rtab", "--phenotypes", "subset.pheno", "--distances", "distances50.tsv", "--max-dimensions", "3"],
    "rtab_missing": ["--pres", os.path.join(ENET, "missing.Rtab"), "--phenotypes", "subset.pheno", "--no-distances", "--max-missing", "0.25"],
    "rtab_missing_lmm": ["--pres", os.path.join(ENET, "missing.Rtab"), "--phenotypes", "subset.pheno", "--max-missing", "0.25"] + LMM,
    "vcf": ["--vcf", os.path.join(VCF, "variants_missing.vcf.gz"), "--phenotypes", "subset.pheno", "--no-distances", "--max-missing", "0.5"],
}


def _cli(args, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pyseer_amd"] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r


def _want(pattern_file, alpha=0.05):
    lines = open(pattern_file, "rb").read().splitlines()
    n = len(set(lines))
    assert 0 < n <= len(lines)
    return "Patterns:\t%d\nThreshold:\t%s\n" % (n, '%.2E' % Decimal(alpha / float(n))), n, len(lines)


def _with_and_without(args, tmp_path, tag=""):
    """one run with --output-patterns and --count-patterns, one with --output-patterns only -> (count text, pattern file of the first)"""
    p1, p2, c = str(tmp_path / ("p1" + tag)), str(tmp_path / ("p2" + tag)), str(tmp_path / ("c" + tag))
    a = _cli(args + ["--output-patterns", p1, "--count-patterns", c])
    b = _cli(args + ["--output-patterns", p2])
    assert a.stdout == b.stdout and a.stderr == b.stderr
    assert open(p1, "rb").read() == open(p2, "rb").read()
    return open(c).read(), p1


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_count_equals_the_distinct_lines_of_the_pattern_file(route, tmp_path):
    got, p1 = _with_and_without(ROUTES[route], tmp_path)
    want, n, n_lines = _want(p1)
    assert got == want, (got, want)
    if route.startswith("rtab_missing"):
        # rows with missing calls were among the tested ones (they never reach the device: their host-made digests are the keys)
        rows = [l.rstrip("\n").split("\t")[1:] for l in open(os.path.join(ENET, "missing.Rtab")).read().splitlines()[1:]]
        assert n_lines > sum(1 for r in rows if "." not in r)


def test_count_through_a_packed_cache(tmp_path):
    """--save-packed counts while it writes the cache; --load-packed (the library's own block loop) counts the same"""
    cache = str(tmp_path / "k.seerpack")
    got_s, p_s = _with_and_without(FIXED + ["--save-packed", cache], tmp_path, "s")
    assert got_s == _want(p_s)[0]
    got_l, p_l = _with_and_without(FIXED + ["--load-packed", cache], tmp_path, "l")
    assert got_l == _want(p_l)[0] == got_s
    got_m, p_m = _with_and_without(KMERS + LMM + ["--load-packed", cache], tmp_path, "m")
    assert got_m == _want(p_m)[0]


def test_count_without_the_pattern_file_and_with_another_alpha(tmp_path):
    p, c0, c1, c2 = (str(tmp_path / x) for x in ("p", "c0", "c1", "c2"))
    a = _cli(FIXED + ["--output-patterns", p, "--count-patterns", c0])
    b = _cli(FIXED + ["--count-patterns", c1])                     # no md5 anywhere in this run
    assert a.stdout == b.stdout and a.stderr == b.stderr
    want, n, _ = _want(p)
    assert open(c0).read() == want and open(c1).read() == want
    d = _cli(FIXED + ["--count-patterns", c2, "--pattern-alpha", "0.01"])
    assert d.stdout == a.stdout and d.stderr == a.stderr
    assert open(c2).read() == _want(p, 0.01)[0]
    assert open(c2).read().splitlines()[0] == want.splitlines()[0] and open(c2).read().splitlines()[1] != want.splitlines()[1]
    # SEERHIP_ROUTE job=0: the same k-mers through the block sink, host-made digests as keys
    env = dict(os.environ, PYTHONPATH=ROOT, SEERHIP_ROUTE="job=0")
    c3 = str(tmp_path / "c3")
    r = subprocess.run([sys.executable, "-m", "pyseer_amd"] + FIXED + ["--count-patterns", c3], cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == a.stdout and open(c3).read() == want


@pytest.mark.parametrize("args,message", [
    (KMERS + ["--wg", "enet"], "Whole genome model does not produce patterns. Re-run without --count-patterns.\n"),
    (FIXED + ["--gpus", "0,0"], "--count-patterns counts on one device: it is not available with more than one device in --gpus\n"),
    (FIXED + ["--gpus", "2"], "--count-patterns counts on one device: it is not available with more than one device in --gpus\n"),
    (FIXED + ["--load-packed", "nothing.seerpack", "--packed-part", "0/2"], "--count-patterns counts one whole run: it is not available with --packed-part\n"),
])
def test_refusals(args, message, tmp_path):
    c = str(tmp_path / "c")
    r = _cli(args + ["--count-patterns", c], ok=False)
    assert r.returncode == 1
    assert r.stderr.decode() == message and r.stdout == b""
    assert not os.path.exists(c)
