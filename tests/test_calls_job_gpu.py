"""--device-calls (SEERHIP_ROUTE calls_job=1): the blocks of the native VCF / BCF and Rtab readers through the job stream (sh_job_submit_calls,
k_job_calls_mark, k_job_md5_calls in csrc/job_kernels.hip) against the route they leave -- input._vcf_packed_block, cli_run.rows_of_block /
BlockSink.sink_rows and utils.format_output, one Python loop per variant -- which the CLI tests hold to the reference's own output.  The command
line with the flag must write the bytes it writes without it; Job.submit_calls must give, row by row, what that host route gives for the same
arrays; the recorded runs of the reference (tests/golden/cli/expected, tests/golden/vcf) are compared as tests/test_cli_gpu.py and
tests/test_vcf_gpu.py compare them, with the route switched on by its key."""
import contextlib
import io
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

from _calls_ref import SIZES, V, f64_pattern, make_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
VCF = os.path.join(ROOT, "tests", "golden", "vcf")
PRET = 0.5                                                  # --filter-pvalue of the submit_calls cases: rows with missing calls fall on both sides


# ---- 1. the command line: the same bytes with and without the flag ---------------------------------------------------------------------------
# Every run is `python -m pyseer_amd` in a process of its own, as in tests/test_cli_gpu.py and tests/test_vcf_gpu.py: the command line chooses how
# the process waits for the device (sh_set_wait_mode) and sets that on the device at its first context, which is a program's business -- called
# as main() inside the suite's process it would change the mode of a device that the tests before it had been using.
INPUTS = {"vcf50": ["--vcf", os.path.join(VCF, "variants50.vcf.gz")],                  # skipped records, rows outside the AF window, fitted rows
          "vcf_missing": ["--vcf", os.path.join(VCF, "variants_missing.vcf.gz")],      # rows with missing calls
          "burden": ["--vcf", os.path.join(VCF, "variants_missing.vcf.gz"), "--burden", os.path.join(VCF, "burden_missing.txt")],
          "pres": ["--pres", "kmers120.Rtab"]}                                         # all of them
KINDS = {"vcf50": ("af-filter", "fitted"), "vcf_missing": ("missing",), "burden": (), "pres": ("af-filter", "missing", "fitted")}
VARIANTS = {"plain": [], "filtered": ["--print-filtered", "--max-missing", "0.5"], "samples": ["--print-samples"], "patterns": ["--output-patterns", "PAT"],
            "count": ["--count-patterns", "COUNT"], "lineage": ["--lineage", "--lineage-clusters", "clusters50.txt"], "blocks37": ["--block_size", "37"]}


def _cli(argv, env=None):
    r = subprocess.run([sys.executable, "-m", "pyseer_amd"] + argv, cwd=CLI, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode()


def _both_routes(argv, tmp_path):
    """-> [(stdout, stderr, pattern file, count file) without the flag, the same with it]"""
    runs = []
    for tag, extra in (("default", []), ("calls", ["--device-calls"])):
        files = {"PAT": str(tmp_path / (tag + ".patterns")), "COUNT": str(tmp_path / (tag + ".count"))}
        args = [files.get(a, a) for a in argv] + extra
        if "--lineage" in args:
            args += ["--lineage-file", str(tmp_path / "lineage.txt")]          # (its name is part of stderr: the same for both runs)
        out, err = _cli(args)
        runs.append((out, err) + tuple(open(f, "rb").read() if os.path.exists(f) else None for f in files.values()))
    return runs


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("model", ["fixed", "lmm"])
@pytest.mark.parametrize("source", sorted(INPUTS))
def test_cli_with_the_flag_writes_the_same_bytes(source, model, variant, tmp_path):
    argv = INPUTS[source] + ["--phenotypes", "subset.pheno"] + VARIANTS[variant]
    if model == "fixed":
        argv += ["--distances", "distances50.tsv"]
    else:                                                   # (--cpu-eigh, both runs: the 50 x 50 kinship needs no torch in the process)
        argv += ["--lmm", "--similarity", "similarity50.tsv", "--cpu-eigh"] + (["--distances", "distances50.tsv"] if "--lineage" in argv else [])
    want, got = _both_routes(argv, tmp_path)
    assert got[0] == want[0], "stdout"
    assert got[1] == want[1], "stderr"
    assert got[2] == want[2] and got[3] == want[3], "pattern file / count file"
    assert ("PAT" in argv) == (want[2] is not None and len(want[2]) > 0) and ("COUNT" in argv) == (want[3] is not None and len(want[3]) > 0)
    assert any(l.endswith(" printed variants") for l in want[1].splitlines())
    notes = [set(r.split("\t")[-1].split(",")) for r in want[0].splitlines()[1:]]
    assert len(notes) > 0 or (source == "vcf_missing" and variant != "filtered")     # (its two records are filtered rows: printed only on request)
    if variant == "filtered":                               # between them the two VCF fixtures show every kind of row, the Rtab alone does
        have = {"af-filter": any("af-filter" in n for n in notes),
                "missing": any(("lrt-filtering-failed" if model == "lmm" else "missing-data-error") in n for n in notes),
                "fitted": any(not (n & {"af-filter", "pre-filtering-failed", "lrt-filtering-failed", "missing-data-error"}) for n in notes)}
        assert all(have[k] for k in KINDS[source]), (have, KINDS[source])


def test_the_flag_takes_the_job_stream():
    """(the byte comparisons above would hold for a flag that did nothing)"""
    argv = INPUTS["vcf_missing"] + ["--phenotypes", "subset.pheno", "--distances", "distances50.tsv"]
    for extra, word in (([], '"job_path": false'), (["--device-calls"], '"job_path": true')):
        _, err = _cli(argv + extra, env={"SEERHIP_DEBUG": "cli"})
        assert word in err and ("(job stream)" in err) == bool(extra)


# ---- 2. the reference's recorded runs, with the route switched on by its key -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtab", "lmm_rtab"])
def test_rtab_goldens_through_the_route(name, tmp_path, monkeypatch):
    import test_cli_gpu
    monkeypatch.setenv("SEERHIP_ROUTE", "calls_job=1")
    monkeypatch.setenv("SEERHIP_DEBUG", "")
    test_cli_gpu.test_cli_matches_reference(name, tmp_path)


def test_vcf_lmm_golden_through_the_route(monkeypatch):
    """tests/golden/vcf/lmm50_expected.log with its counters (254 loaded ... 90 printed)"""
    import test_vcf_gpu
    monkeypatch.setenv("SEERHIP_ROUTE", "calls_job=1")
    test_vcf_gpu.test_cli_lmm_matches_the_reference_run()


# ---- 3. Job.submit_calls against the host route on the same arrays ---------------------------------------------------------------------------
def _engine(N, lmm, continuous, y, case):
    from pyseer_amd.engine import Engine
    from pyseer_amd.model import fit_null
    rng = np.random.default_rng(1000 + N)
    e = Engine(N)
    e.set_af_filter(case["min_af"], case["max_af"])
    if lmm:
        X = rng.standard_normal((N, 2 * N))
        S, U = np.linalg.eigh(X.dot(X.T) / (2 * N))
        e.lmm_setup(U, S, y, np.ones((N, 1)), 0.5, continuous, PRET, 0.5)
    else:
        W = rng.standard_normal((N, 1)); W /= np.abs(W).max(axis=0)
        e0 = np.zeros((0, 0))
        e.glm_setup(y, W, continuous, fit_null(y, W, e0, continuous).llf, None if continuous else fit_null(y, W, e0, False, firth=True), PRET, 0.5)
    return e


def _host_route(e, lmm, continuous, case, planes, print_filtered, print_samples):
    """(text, pattern text, (pre-filtered, tested, printed), the row objects in input order -- None for a skipped record --, the block)"""
    from pyseer_amd import cli_run, input as I
    from pyseer_amd.lmm import mask_like_fit_lmm
    N, samples = case["N"], case["samples"]
    order = sorted(range(N), key=lambda i: samples[i])
    with contextlib.redirect_stderr(io.StringIO()):
        blk = I._vcf_packed_block(N, samples, order, case["names"], case["skip"], planes[0], planes[1], case["n_present"], case["n_missing"],
                                  case["min_af"], case["max_af"], case["max_missing"], True)
    r = (e.lmm_batch(blk.bits) if lmm else e.glm_batch(blk.bits)) if blk.bits.shape[0] else None
    options = SimpleNamespace(lmm=lmm, continuous=continuous, filter_pvalue=PRET, print_filtered=print_filtered, print_samples=print_samples, lineage=False,
                              python_sink=True, serial_sink=False, lmm_lineage_per_variant=False)
    ctx = cli_run.RunContext(None, options, None, case["y"], 'lmm' if lmm else 'seer', None)
    out, pats = [], []
    sink = cli_run.BlockSink(ctx, out.append, pats.append, cli_run.new_tm())
    sink.sink_rows(blk, r, e)
    sink.close()
    rows = cli_run.rows_of_block(ctx, blk, mask_like_fit_lmm(r) if (lmm and r is not None) else r)
    return b"".join(out), b"".join(pats), (sink.n.prefilter, sink.n.tested, sink.n.printed), rows, blk


def _job_route(e, lmm, case, planes, print_filtered, print_samples):
    from pyseer_amd.engine import Job
    job = Job(e, lmm, print_filtered, patterns=True, sample_names=(case["samples"] if print_samples else None))
    try:
        job.submit_calls(planes[0], planes[1], case["n_present"], case["n_missing"], case["skip"], case["blob"], case["off"], case["max_missing"])
        text, counts, _ = job.collect()
        return bytes(text), bytes(job.patterns()), counts, job.records()
    finally:
        job.close()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("continuous", [False, True], ids=["binary", "continuous"])
@pytest.mark.parametrize("lmm", [False, True], ids=["fixed", "lmm"])
def test_submit_calls_equals_the_host_route(lmm, continuous, N):
    """No size is dropped: the existing route takes every N of SIZES.  No row is left out of any comparison."""
    from pyseer_amd.classes import FLAG_FILTER, FLAG_PREFILTER, notes_from_flags
    from pyseer_amd.engine import pack_variants
    from pyseer_amd.model import host_pre_filtering
    case = make_case(N, continuous, seed=11 * N + (1 if continuous else 0))
    planes = (pack_variants(case["P"]), pack_variants(case["M"]))
    y = case["y"]
    # the condition of the comparison, checked on the host: no filter-pvalue of a row with missing calls lies within 1e-6 (relative) of the threshold
    inside = (case["skip"] == 0) & (case["n_missing"] > 0)
    preps = {}
    for v in np.nonzero(inside)[0]:
        k = case["P"][v].astype(float); k[case["M"][v].astype(bool)] = np.nan
        preps[int(v)] = host_pre_filtering(y, k, continuous)
    assert all(not np.isfinite(pr) or abs(pr - PRET) > 1e-6 * PRET for pr, _ in preps.values())
    e = _engine(N, lmm, continuous, y, case)
    try:
        seen = set()
        for print_filtered in (True, False):
            want_text, want_pat, want_counts, rows, blk = _host_route(e, lmm, continuous, case, planes, print_filtered, print_filtered)
            text, pat, counts, (idx, flags, cols) = _job_route(e, lmm, case, planes, print_filtered, print_filtered)
            assert counts == want_counts, (counts, want_counts)
            assert pat == want_pat and len(pat) == 25 * want_counts[1]
            assert text == want_text, (text[:400], want_text[:400])
            # the order of the records: input order, the LMM with its pre-filtered rows first; skipped records are never rows
            real = [v for v in range(V) if rows[v] is not None]
            shown = [v for v in real if print_filtered or not (rows[v].prefilter or rows[v].filter)]
            if lmm:
                shown = [v for v in shown if rows[v].prefilter] + [v for v in shown if not rows[v].prefilter]
            assert idx.tolist() == shown and counts[2] == len(shown) and counts[0] == V - counts[1] == sum(1 for v in range(V) if rows[v] is None or rows[v].prefilter)
            for r_, v in enumerate(idx.tolist()):
                x, f = rows[v], int(flags[r_])
                assert notes_from_flags(f) == set(x.notes) and bool(f & FLAG_PREFILTER) == bool(x.prefilter) and bool(f & FLAG_FILTER) == bool(x.filter), (v, hex(f), x)
                if blk.status[v] == 2:                                   # filter-pvalue on the device against host_pre_filtering
                    want = preps[v][0]
                    got = cols[0, r_]
                    assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-6 * abs(want), (v, got, want)
                    assert np.isnan(cols[1:, r_]).all()
                    seen |= set(x.notes) | ({"nan"} if np.isnan(want) else set()) | ({"good-chisq"} if "bad-chisq" not in x.notes else set())
                if blk.status[v] == 1:
                    assert np.isnan(cols[:, r_]).all() and set(x.notes) == {"af-filter"}
            if print_filtered:
                assert sorted(idx.tolist()) == real and {int(s) for s in blk.status} == {0, 1, 2, 3}
                # the edges make_case places: the window is inclusive on both sides, with and without a missing call's help; so is max_missing
                status = {v: blk.status[v] for v in range(1, 15)}
                assert [status[v] for v in (1, 2, 3, 4)] == [0, 1, 0, 1] and [status[v] for v in (5, 6, 7, 8, 9, 10, 11, 12)] == [2, 2, 1, 2, 1, 1, 2, 2]
                assert np.isnan(preps[11][0]) and rows[11].prefilter and "pre-filtering-failed" in rows[11].notes
        assert {"pre-filtering-failed", "lrt-filtering-failed" if lmm else "missing-data-error", "nan"} <= seen
        if not continuous:
            assert "bad-chisq" in seen and (N < 127 or "good-chisq" in seen)       # tables that do and do not trip bad-chisq
    finally:
        e.close()


@pytest.mark.parametrize("N", SIZES)
def test_patterns_of_rows_with_missing_calls_are_float64_md5(N):
    """sh_job_patterns for rows with missing calls: base64(md5) of the float64 vector with NaN, from hashlib (tests/_calls_ref.py f64_pattern,
    held to input.hash_pattern by tests/test_calls_job_cpu.py); rows without one keep the int64 digest."""
    from pyseer_amd.classes import FLAG_PREFILTER
    from pyseer_amd.engine import pack_variants
    from pyseer_amd.input import hash_pattern
    case = make_case(N, False, seed=5 * N)
    planes = (pack_variants(case["P"]), pack_variants(case["M"]))
    e = _engine(N, False, False, case["y"], case)
    try:
        text, pat, counts, (idx, flags, cols) = _job_route(e, False, case, planes, True, False)
    finally:
        e.close()
    tested = [v for r_, v in enumerate(idx.tolist()) if not (int(flags[r_]) & FLAG_PREFILTER)]         # (fixed effects: input order)
    want = [f64_pattern(case["P"][v], case["M"][v]) if case["n_missing"][v] else hash_pattern(case["P"][v].astype(np.int64)) for v in tested]
    assert pat == b"".join(want) and counts[1] == len(tested)
    assert sum(1 for v in tested if case["n_missing"][v]) >= 20 and sum(1 for v in tested if not case["n_missing"][v]) >= 20


def test_submit_calls_refuses_what_it_cannot_take():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Job, pack_variants
    case = make_case(64, False, seed=3)
    planes = (pack_variants(case["P"]), pack_variants(case["M"]))
    e = _engine(64, False, False, case["y"], case)
    job = Job(e, False)
    try:
        narrow = np.zeros((V, 4), dtype=np.uint8)                            # 32 bits < 64 samples
        with pytest.raises(_abi.SeerHipError):
            job.submit_calls(narrow, narrow, case["n_present"], case["n_missing"], case["skip"], case["blob"], case["off"], 0.05)
        with pytest.raises(_abi.SeerHipError):
            job.submit_calls(planes[0], planes[1], case["n_present"], np.full(V, -1, np.int32), case["skip"], case["blob"], case["off"], 0.05)
        assert job.pending() == 0
        for _ in range(job.depth):
            job.submit_calls(planes[0], planes[1], case["n_present"], case["n_missing"], case["skip"], case["blob"], case["off"], case["max_missing"])
        with pytest.raises(_abi.SeerHipError):
            job.submit_calls(planes[0], planes[1], case["n_present"], case["n_missing"], case["skip"], case["blob"], case["off"], case["max_missing"])
        got = [job.collect()[1] for _ in range(job.depth)]
        assert len(set(got)) == 1 and got[0][0] + got[0][1] == V
    finally:
        job.close(); e.close()
