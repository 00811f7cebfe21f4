"""The call cache on the device: k_calls_select (csrc/select_kernels.hip) through RowSelector.select_calls / select_calls_dev against
the numpy yardstick of tests/_cache_select.py, at every launch shape's edges; Job.submit_calls_select against Job.submit_calls on the numpy-selected planes;
and the command line -- a run with --save-calls writes the bytes it writes without it, and a run with --load-calls, over the cache's own sample list,
another order of it or a subset, writes the bytes of the same run reading the text.  Every comparison is exact.  The text side is held to the
reference by tests/test_cli_gpu.py, tests/test_vcf_gpu.py and tests/test_calls_job_gpu.py; the recorded runs of the reference are repeated from a cache
at the end."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import _cache_select as cs  # noqa: E402
import test_calls_job_gpu as cj  # noqa: E402
from _calls_ref import SIZES, V, make_case  # noqa: E402

CLI, VCF, ROOT = cj.CLI, cj.VCF, cj.ROOT


def _proc(args, expect=0, route=None, module="pyseer_amd"):
    """a run that may fail, or of another module -> (stdout, stderr)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("SEERHIP_ROUTE", None)
    if route:
        env["SEERHIP_ROUTE"] = route
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout, r.stderr.decode()


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------------
# the launch shapes of k_calls_select by source row bytes (select_kernels.hip calls_select_shape): four rows a wavefront with 4, 2, 1 wavefronts up
# to 2048, 4096, 8192; one row a wavefront with 2, 1 wavefronts up to 16 384, 32 768 -- the widest row taken; 32 776 is the first refused
SHAPE_EDGES = (2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 32768)
FIRST_REFUSED = 32776


def _check_calls(got, present, missing, n_src, m):
    for bits, counts, src in ((got[0], got[2], present), (got[1], got[3], missing)):
        cs.check_selected(bits, counts, src, n_src, m)        # (whole rows equal, padding bits zero, int32 counts = the popcounts)


def _both_ways(sel, present, missing, n_src, m):
    import torch
    _check_calls(sel.select_calls(present, missing), present, missing, n_src, m)
    got = sel.select_calls_dev(torch.from_numpy(present).cuda(), torch.from_numpy(missing).cuda())
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.int32
    _check_calls(tuple(t.cpu().numpy() for t in got), present, missing, n_src, m)


@pytest.mark.parametrize("n_src", cs.N_SRC)
def test_kernel_equals_numpy(n_src):
    from pyseer_amd.engine import Engine, RowSelector
    rng = np.random.default_rng(n_src)
    rows = {v: (cs.source_rows(v, n_src, rng, 0.4)[0], cs.source_rows(v, n_src, rng, 0.1)[0]) for v in (0, 1, 5, 257)}    # (padding bits all ones)
    for n_dst in cs.n_dsts(n_src):
        eng = Engine(n_dst)
        for kind in cs.MAP_KINDS:
            m = cs.make_map(kind, n_src, n_dst, rng)
            sel = RowSelector(eng, n_src, m)
            for v in rows:
                _both_ways(sel, rows[v][0], rows[v][1], n_src, m)
            sel.close()
        eng.close()


@pytest.mark.parametrize("row_bytes", SHAPE_EDGES)
def test_both_sides_of_every_launch_shape(row_bytes):
    """5 rows: a ragged last group where a wavefront takes four, a lone wavefront behind the last row where a workgroup has several"""
    from pyseer_amd.engine import Engine, RowSelector
    n_src = row_bytes * 8 - 5
    assert cs.row_bytes_for(n_src) == row_bytes
    rng = np.random.default_rng(row_bytes)
    present, missing = cs.source_rows(5, n_src, rng, 0.4)[0], cs.source_rows(5, n_src, rng, 0.1)[0]
    for n_dst, kind in ((4161, "permuted"), (65, "reversed")):
        m = cs.make_map(kind, n_src, n_dst, rng)
        eng = Engine(n_dst)
        sel = RowSelector(eng, n_src, m)
        _both_ways(sel, present, missing, n_src, m)
        sel.close(); eng.close()


def test_many_rows_in_several_chunks():
    """sh_select_calls stages 16 MB of the two planes at a time through two slots: 30 000 rows of 656 bytes are three chunks, the last ragged"""
    from pyseer_amd.engine import Engine, RowSelector
    rng = np.random.default_rng(2)
    one_p, one_m = cs.source_rows(1000, 5200, rng, 0.4)[0], cs.source_rows(1000, 5200, rng, 0.1)[0]
    present, missing = np.ascontiguousarray(np.tile(one_p, (30, 1))), np.ascontiguousarray(np.tile(one_m, (30, 1)))
    present[:, 0] ^= (np.arange(30000) & 0xFF).astype(np.uint8)                    # (no two chunks alike)
    missing[:, 1] ^= ((np.arange(30000) >> 3) & 0xFF).astype(np.uint8)
    m = cs.make_map("permuted", 5200, 5000, rng)
    eng = Engine(5000)
    sel = RowSelector(eng, 5200, m)
    _check_calls(sel.select_calls(present, missing), present, missing, 5200, m)
    sel.close(); eng.close()


def test_the_first_width_too_wide_is_refused_not_launched():
    import torch
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine, RowSelector
    n_src = FIRST_REFUSED * 8 - 5
    rng = np.random.default_rng(5)
    m = cs.make_map("permuted", n_src, 65, rng)
    eng = Engine(65)
    sel = RowSelector(eng, n_src, m)                                               # (one plane of this width fits k_rows_select)
    rows = np.zeros((5, FIRST_REFUSED), dtype=np.uint8)
    with pytest.raises(_abi.SeerHipError, match="too wide for the two planes of one wavefront of k_calls_select"):
        sel.select_calls(rows, rows)
    t = torch.from_numpy(rows).cuda()
    with pytest.raises(_abi.SeerHipError, match="too wide for the two planes of one wavefront of k_calls_select"):
        sel.select_calls_dev(t, t)
    got_bits, got_counts = sel.select(rows)                                        # the selector still works
    assert not got_bits.any() and not got_counts.any()
    sel.close(); eng.close()


# ---- 2. Job.submit_calls_select against Job.submit_calls on the numpy-selected planes ---------------------------------------------------------
def _embedded(case, rng, extra=37):
    """The case's planes as columns map[j] of a wider source whose other columns, and whose padding bits, hold calls of their own"""
    from pyseer_amd.engine import pack_variants
    N = case["N"]
    n_src = N + extra
    m = rng.permutation(n_src)[:N].astype(np.int32)
    planes = []
    for dense, density in ((case["P"], 0.4), (case["M"], 0.2)):
        wide = (rng.random((V, cs.row_bytes_for(n_src) * 8)) < density).astype(np.uint8)
        wide[:, n_src:] = 1
        wide[:, m] = dense
        planes.append(np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")))
    want = [cs.numpy_select(pl, n_src, m) for pl in planes]
    assert np.array_equal(want[0][0], pack_variants(case["P"])) and np.array_equal(want[1][0], pack_variants(case["M"]))
    assert np.array_equal(want[0][1], case["n_present"]) and np.array_equal(want[1][1], case["n_missing"])
    return n_src, m, planes, (want[0][0], want[1][0], want[0][1], want[1][1])


def _collected(job):
    text, counts, _ = job.collect()
    return bytes(text), bytes(job.patterns()), counts, tuple(a.tolist() for a in job.records()[:2]), job.records()[2].tobytes()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("lmm", [False, True], ids=["fixed", "lmm"])
def test_submit_calls_select_equals_submit_calls(lmm, N):
    from pyseer_amd.engine import Job, RowSelector
    case = make_case(N, False, seed=13 * N)
    rng = np.random.default_rng(N)
    n_src, m, src, want = _embedded(case, rng)
    e = cj._engine(N, lmm, False, case["y"], case)
    sel = RowSelector(e, n_src, m)
    try:
        for listed in (False, True):                               # print-filtered and the sample lists, as tests/test_calls_job_gpu.py pairs them
            results = []
            for way in ("calls", "select", "rows"):
                job = Job(e, lmm, listed, patterns=True, sample_names=(case["samples"] if listed else None))
                try:
                    if way == "calls":
                        job.submit_calls(want[0], want[1], want[2], want[3], case["skip"], case["blob"], case["off"], case["max_missing"])
                    elif way == "select":
                        job.submit_calls_select(sel, src[0], src[1], case["skip"], case["blob"], case["off"], case["max_missing"])
                    else:                                          # what SEERHIP_ROUTE=calls_cache=rows does: selected to the host, submitted as a reader's
                        got = sel.select_calls(src[0], src[1])
                        job.submit_calls(got[0], got[1], got[2], got[3], case["skip"], case["blob"], case["off"], case["max_missing"])
                    results.append(_collected(job))
                    if way == "select":
                        n_p, n_m = job.calls_counts()
                        assert n_p.dtype == np.int32 and np.array_equal(n_p, want[2]) and np.array_equal(n_m, want[3])
                finally:
                    job.close()
            assert results[1] == results[0] and results[2] == results[0]
            text, pat, counts = results[0][:3]
            assert counts[0] + counts[1] == V and counts[2] > 0 and len(pat) == 25 * counts[1] and text.count(b"\n") == counts[2]
            assert (b"\ts" in text) == listed
    finally:
        sel.close(); e.close()


def test_blocks_in_flight_and_the_lmm_lineage_of_the_last_row():
    """Every slot of the job holds a selected block (the selector stages through two): each comes back as the first.  Then the LMM's per-block lineage,
    which a block has unless its last record was skipped or holds a missing call -- the latter known only from the counts the device made."""
    from pyseer_amd.engine import Job, RowSelector
    N = 65
    case = make_case(N, False, seed=4)
    rng = np.random.default_rng(9)
    n_src, m, src, want = _embedded(case, rng)
    lin = np.zeros((N, 2)); lin[np.arange(N) % 3 == 1, 0] = 1.0; lin[np.arange(N) % 3 == 2, 1] = 1.0
    e = cj._engine(N, True, False, case["y"], case)
    e.lineage_setup(lin, None)
    sel = RowSelector(e, n_src, m)
    try:
        job = Job(e, True, False)
        for _ in range(job.depth):
            job.submit_calls_select(sel, src[0], src[1], case["skip"], case["blob"], case["off"], case["max_missing"])
        got = [(bytes(t), c) for t, c, _ in (job.collect() for _ in range(job.depth))]
        job.close()
        assert len(set(got)) == 1 and got[0][1][2] > 0
        tail = [v for v in range(150, V) if case["skip"][v] == 0]
        holed, clean = [v for v in tail if case["n_missing"][v] > 0][0], [v for v in tail if case["n_missing"][v] == 0][0]
        assert case["skip"][V - 1] == 1
        seen = set()
        for rows in (holed + 1, clean + 1, V):                     # the last row: with missing calls, without, skipped
            texts = []
            for way in ("calls", "select"):
                job = Job(e, True, False, lineage_labels=["L1", "L2"])
                cut = lambda a: np.ascontiguousarray(a[:rows])
                off = np.ascontiguousarray(case["off"][:rows + 1])
                if way == "calls":
                    job.submit_calls(cut(want[0]), cut(want[1]), cut(want[2]), cut(want[3]), cut(case["skip"]), case["blob"], off, case["max_missing"])
                else:
                    job.submit_calls_select(sel, cut(src[0]), cut(src[1]), cut(case["skip"]), case["blob"], off, case["max_missing"])
                texts.append(bytes(job.collect()[0]))
                job.close()
            assert texts[0] == texts[1] and len(texts[0]) > 0
            seen.add((b"\tL1\t" in texts[0]) or (b"\tL2\t" in texts[0]))
        assert seen == {True, False}
    finally:
        sel.close(); e.close()


def test_submit_calls_select_refuses_what_it_cannot_take():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine, Job, RowSelector
    case = make_case(64, False, seed=3)
    rng = np.random.default_rng(3)
    n_src, m, src, want = _embedded(case, rng)
    e = cj._engine(64, False, False, case["y"], case)
    other = Engine(64)
    sel, foreign = RowSelector(e, n_src, m), RowSelector(other, n_src, m)
    job = Job(e, False)
    try:
        with pytest.raises(_abi.SeerHipError, match="the selector belongs to another context"):
            job.submit_calls_select(foreign, src[0], src[1], case["skip"], case["blob"], case["off"], 0.05)
        narrow = np.zeros((V, 8), dtype=np.uint8)                                  # 64 bits < 101 source samples
        with pytest.raises(_abi.SeerHipError, match="src_row_bytes\\*8 < n_src"):
            job.submit_calls_select(sel, narrow, narrow, case["skip"], case["blob"], case["off"], 0.05)
        assert job.pending() == 0
        for _ in range(job.depth):
            job.submit_calls_select(sel, src[0], src[1], case["skip"], case["blob"], case["off"], case["max_missing"])
        with pytest.raises(_abi.SeerHipError, match="every slot holds a block"):
            job.submit_calls_select(sel, src[0], src[1], case["skip"], case["blob"], case["off"], case["max_missing"])
        got = [job.collect()[1] for _ in range(job.depth)]
        assert len(set(got)) == 1 and got[0][0] + got[0][1] == V
    finally:
        job.close(); sel.close(); foreign.close(); other.close(); e.close()


# ---- 3. the command line: the same bytes ---------------------------------------------------------------------------------------------------------
# Every run is `python -m pyseer_amd` in a process of its own (tests/test_calls_job_gpu.py says why).
ANNOUNCE = "pyseer_amd: call cache holds %d samples; the run's %d are selected on the %s\n"


def _model(model, argv, fixed_extra=()):
    if model == "fixed":
        return ["--distances", "distances50.tsv"] + list(fixed_extra)
    return ["--lmm", "--similarity", "similarity50.tsv", "--cpu-eigh"] + (["--distances", "distances50.tsv"] if "--lineage" in argv else [])


def _run(argv, tmp_path, tag, env=None):
    """-> (stdout, stderr, pattern file, count file)"""
    files = {"PAT": str(tmp_path / (tag + ".patterns")), "COUNT": str(tmp_path / (tag + ".count"))}
    args = [files.get(a, a) for a in argv]
    if "--lineage" in args:
        args += ["--lineage-file", str(tmp_path / "lineage.txt")]                  # (its name is part of stderr: the same for every run)
    out, err = cj._cli(args, env=env)
    return (out, err) + tuple(open(f, "rb").read() if os.path.exists(f) else None for f in files.values())


def _without(line, run):
    """the run with the one announcing line taken out of its stderr (it must be there, once)"""
    assert run[1].count(line) == 1, run[1][-2000:]
    return (run[0], run[1].replace(line, "")) + run[2:]


@pytest.mark.parametrize("variant", sorted(cj.VARIANTS))
@pytest.mark.parametrize("model", ["fixed", "lmm"])
@pytest.mark.parametrize("source", sorted(cj.INPUTS))
def test_save_and_load_write_the_text_runs_bytes(source, model, variant, tmp_path):
    """the run's own list: the cache --save-calls writes over subset.pheno, read back by the same run"""
    rest = ["--phenotypes", "subset.pheno"] + cj.VARIANTS[variant]
    rest += _model(model, rest)
    cache = str(tmp_path / "own.seercalls")
    want = _run(cj.INPUTS[source] + rest, tmp_path, "text")
    saved = _run(cj.INPUTS[source] + rest + ["--save-calls", cache], tmp_path, "save")
    assert saved == want and os.path.exists(cache) and not os.path.exists(cache + ".part")
    loaded = _run(["--load-calls", cache] + rest, tmp_path, "load")
    assert loaded == want
    assert any(l.endswith(" printed variants") for l in want[1].splitlines())
    assert ("PAT" in rest) == bool(want[2]) and ("COUNT" in rest) == bool(want[3])


@pytest.fixture(scope="module")
def relations(tmp_path_factory):
    """shuffled.pheno: subset.pheno's 50 in another order; per source a cache over subset.pheno's own order (--save-calls) and one over samples50.txt
    (pyseer_amd.pack), each in stored blocks of 3000 and of 37"""
    d = tmp_path_factory.mktemp("relations")
    lines = open(os.path.join(CLI, "subset.pheno")).read().splitlines()
    shuffled = str(d / "shuffled.pheno")
    with open(shuffled, "w") as fh:
        fh.write("\n".join([lines[0]] + [lines[1 + i] for i in np.random.default_rng(7).permutation(50)]) + "\n")
    caches = {}
    for source, inp in cj.INPUTS.items():
        for block in (3000, 37):
            own, sup = str(d / ("%s_%d_own.seercalls" % (source, block))), str(d / ("%s_%d_super.seercalls" % (source, block)))
            cj._cli(inp + ["--phenotypes", "subset.pheno", "--no-distances", "--block_size", str(block), "--save-calls", own])
            _proc([os.path.join(CLI, "samples50.txt")] + inp + ["-o", sup, "--block", str(block)], module="pyseer_amd.pack")
            caches[source, block] = {"order": own, "superset": sup}
    return shuffled, caches


@pytest.mark.parametrize("variant", sorted(cj.VARIANTS))
@pytest.mark.parametrize("model", ["fixed", "lmm"])
@pytest.mark.parametrize("source", sorted(cj.INPUTS))
@pytest.mark.parametrize("relation", ["order", "superset"])
def test_a_cache_over_other_samples_writes_the_text_runs_bytes(relation, source, model, variant, relations, tmp_path):
    """the other two relations of a cache to its run, through the fused submit: every source, model and variant once more"""
    shuffled, caches = relations
    pheno, n_run = (shuffled, 50) if relation == "order" else ("supersubset.pheno", 10)
    variants = cj.VARIANTS[variant]
    if relation == "superset" and model == "lmm":
        # (--lmm --lineage over 10 of the similarity matrix's 50 samples is refused before any variant is read, whatever the input: "Lineage file and
        # similarity matrix contain different sets of samples"; the fixed-effects runs carry the lineage of this relation)
        variants = [a for a in variants if a not in cj.VARIANTS["lineage"]]
    rest = ["--phenotypes", pheno] + variants + (["--phenotype-column", "continuous"] if relation == "superset" else [])
    rest += _model(model, rest, ["--max-dimensions", "3"] if relation == "superset" else [])
    cache = caches[source, 37 if "--block_size" in rest else 3000][relation]
    want = _run(cj.INPUTS[source] + rest, tmp_path, "text")
    loaded = _run(["--load-calls", cache] + rest, tmp_path, "load")
    assert _without(ANNOUNCE % (50, n_run, "device"), loaded) == want
    assert any(l.endswith(" printed variants") for l in want[1].splitlines())
    # (the files exist where they were asked for; over the 10 samples a source may leave no tested variant, and its pattern file empty)
    assert ("PAT" in rest) == (want[2] is not None) and ("COUNT" in rest) == bool(want[3])


@pytest.fixture(scope="module")
def all_columns(tmp_path_factory):
    """a cache over all 1837 columns of variants_missing.vcf.gz, written by pyseer_amd.pack"""
    import gzip
    d = tmp_path_factory.mktemp("all_columns")
    with gzip.open(os.path.join(VCF, "variants_missing.vcf.gz"), "rt") as fh:
        names = next(l for l in fh if l.startswith("#CHROM")).rstrip("\n").split("\t")[9:]
    assert len(names) == 1837
    listing, cache = str(d / "all.txt"), str(d / "all.seercalls")
    with open(listing, "w") as fh:
        fh.write("".join(s + "\n" for s in names))
    _, err = _proc([listing, "--vcf", os.path.join(VCF, "variants_missing.vcf.gz"), "-o", cache], module="pyseer_amd.pack")
    assert "2 variants over 1837 samples written to" in err
    return cache


@pytest.mark.parametrize("model", ["fixed", "lmm"])
def test_a_cache_of_every_column_serves_the_fifty(model, all_columns, tmp_path):
    rest = ["--phenotypes", "subset.pheno"] + cj.VARIANTS["filtered"] + cj.VARIANTS["samples"]
    rest += _model(model, rest)
    want = _run(cj.INPUTS["vcf_missing"] + rest, tmp_path, "text")
    loaded = _run(["--load-calls", all_columns] + rest, tmp_path, "load")
    assert _without(ANNOUNCE % (1837, 50, "device"), loaded) == want and len(want[0].splitlines()) == 3


@pytest.mark.parametrize("how", ["--python-sink", "--serial-sink", "job=0", "cache_select=host", "calls_cache=rows"])
def test_the_other_routes_of_a_selected_cache_write_the_same_bytes(how, relations, tmp_path):
    shuffled, caches = relations
    rest = ["--phenotypes", shuffled, "--distances", "distances50.tsv"] + cj.VARIANTS["filtered"] + cj.VARIANTS["count"]
    want = _run(cj.INPUTS["pres"] + rest, tmp_path, "text")
    extra, env = ([how], None) if how.startswith("--") else ([], {"SEERHIP_ROUTE": how})
    loaded = _run(["--load-calls", caches["pres", 3000]["order"]] + rest + extra, tmp_path, "load", env=env)
    assert _without(ANNOUNCE % (50, 50, "host" if how == "cache_select=host" else "device"), loaded) == want and len(want[0].splitlines()) > 50


def test_load_calls_takes_the_job_stream(relations):
    """(the byte comparisons above would hold for a loader that read the text again)"""
    shuffled, caches = relations
    rest = ["--phenotypes", "subset.pheno", "--distances", "distances50.tsv"]
    _, err = cj._cli(cj.INPUTS["vcf_missing"] + rest, env={"SEERHIP_DEBUG": "cli"})
    assert '"job_path": false' in err and "(job stream)" not in err
    for cache in (caches["vcf_missing", 3000]["order"], caches["vcf_missing", 3000]["superset"]):
        _, err = cj._cli(["--load-calls", cache] + rest, env={"SEERHIP_DEBUG": "cli"})
        assert '"job_path": true' in err and "(job stream)" in err
    _, err = cj._cli(["--load-calls", cache] + rest + ["--python-sink"], env={"SEERHIP_DEBUG": "cli"})
    assert '"job_path": false' in err


def test_refusals_that_need_the_cache(relations, tmp_path):
    shuffled, caches = relations
    cache = caches["pres", 3000]["superset"]
    twice = str(tmp_path / "twice.pheno")
    lines = open(os.path.join(CLI, "supersubset.pheno")).read().splitlines()
    with open(twice, "w") as fh:
        fh.write("\n".join(lines[:4] + ["sample_x\t1\t0"]) + "\n")
    kmers = str(tmp_path / "k.seerpack")
    _proc(["--kmers", "kmers.gz", "--phenotypes", "subset.pheno", "--no-distances", "--save-packed", kmers])
    rest = ["--no-distances", "--phenotype-column", "continuous"]
    for argv, route, text in (
            (["--load-calls", cache, "--phenotypes", twice], None, "pyseer_amd: --load-calls: the call cache does not hold sample sample_x of the run\n"),
            (["--load-calls", cache, "--phenotypes", "supersubset.pheno"], "cache_select=0",
             "pyseer_amd: --load-calls: call cache was written for a different sample list / order (50 vs 10 samples)\n"),
            (["--load-calls", kmers, "--phenotypes", "supersubset.pheno"], None,
             "pyseer_amd: --load-calls: %s is a packed k-mer cache, not a call cache (it is read by --load-packed)\n" % kmers)):
        out, err = _proc(argv + rest, expect=1, route=route)
        assert out == b"" and err.endswith(text) and "Traceback" not in err
    out, err = _proc(["--kmers", "kmers.gz", "--load-packed", cache, "--phenotypes", "subset.pheno", "--no-distances"], expect=1)
    assert "is a call cache, not a packed k-mer cache (it is read by --load-calls)" in err


def _rtab(path, columns, lines):
    with open(path, "w") as fh:
        fh.write("Gene\t" + "\t".join(columns) + "\n" + "".join(l + "\n" for l in lines))
    return path


def test_save_calls_refuses_a_header_that_names_a_sample_twice(tmp_path):
    """by the native reader's own word, before the header line; pyseer_amd.pack likewise; neither leaves a file"""
    table = _rtab(str(tmp_path / "twice.Rtab"), ["sample_1", "sample_2", "sample_1"], ["g1\t1\t0\t1", "g2\t0\t1\t."])
    cache = str(tmp_path / "c.seercalls")
    out, err = _proc(["--pres", table, "--phenotypes", "subset.pheno", "--no-distances", "--save-calls", cache], expect=1)
    assert out == b"" and "Traceback" not in err
    assert err.endswith("--save-calls needs the native Rtab reader, which does not read %s (Rtab: duplicate sample column sample_1)\n" % table)
    out, err = _proc([os.path.join(CLI, "samples50.txt"), "--pres", table, "-o", cache], expect=1, module="pyseer_amd.pack")
    assert err.endswith("pyseer_amd.pack: Rtab: duplicate sample column sample_1: no call cache is written for such a table\n") and "Traceback" not in err
    assert not os.path.exists(cache) and not os.path.exists(cache + ".part")
    out, err = _proc(["--pres", table, "--phenotypes", "subset.pheno", "--no-distances", "--print-filtered"])       # (without the option: the line reader)
    assert len(out.splitlines()) == 3


@pytest.mark.parametrize("extra", [[], ["--device-calls"]], ids=["default", "device-calls"])
def test_a_malformed_rtab_line_leaves_no_cache(extra, tmp_path):
    columns = open(os.path.join(CLI, "samples50.txt")).read().split()
    good = ["g%d\t" % i + "\t".join("1" if (i + j) % 3 == 0 else "0" for j in range(50)) for i in range(5)]
    table = _rtab(str(tmp_path / "bad.Rtab"), columns, good + ["short\t1\t0"] + good)
    cache = str(tmp_path / "c.seercalls")
    out, err = _proc(["--pres", table, "--phenotypes", "subset.pheno", "--no-distances", "--print-filtered", "--block_size", "2", "--save-calls", cache] + extra, expect=1)
    assert "Unexpected mismatch between header and data row" in err
    assert not os.path.exists(cache) and not os.path.exists(cache + ".part")
    if not extra:
        out, err = _proc([os.path.join(CLI, "samples50.txt"), "--pres", table, "-o", cache, "--block", "2"], expect=1, module="pyseer_amd.pack")
        assert err.endswith("pyseer_amd.pack: Unexpected mismatch between header and data row\n") and "Traceback" not in err
        assert not os.path.exists(cache) and not os.path.exists(cache + ".part")
        table = _rtab(str(tmp_path / "good.Rtab"), columns, good)                                       # (the same table without the line: a cache)
        _proc([os.path.join(CLI, "samples50.txt"), "--pres", table, "-o", cache, "--block", "2"], module="pyseer_amd.pack")
        assert os.path.exists(cache)


# ---- 4. the reference's recorded runs, from a cache written first ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtab", "lmm_rtab"])
def test_rtab_goldens_from_a_cache(name, tmp_path, monkeypatch):
    import test_cli_gpu
    args = list(test_cli_gpu.CASES[name])
    i = args.index("--pres")
    cache = str(tmp_path / "golden.seercalls")
    cj._cli(args + ["--save-calls", cache])
    assert os.path.exists(cache)
    monkeypatch.setitem(test_cli_gpu.CASES, name, args[:i] + ["--load-calls", cache] + args[i + 2:])
    monkeypatch.setenv("SEERHIP_DEBUG", "")
    test_cli_gpu.test_cli_matches_reference(name, tmp_path)


def test_vcf_lmm_golden_from_a_cache(tmp_path, monkeypatch):
    """tests/golden/vcf/lmm50_expected.log with its counters (254 loaded ... 90 printed)"""
    import test_vcf_gpu
    real, cache = test_vcf_gpu._cli, str(tmp_path / "golden.seercalls")

    def from_cache(args, *a, **kw):
        i = args.index("--vcf")
        real(args + ["--save-calls", cache], *a, **kw)
        return real(args[:i] + ["--load-calls", cache] + args[i + 2:], *a, **kw)
    monkeypatch.setattr(test_vcf_gpu, "_cli", from_cache)
    test_vcf_gpu.test_cli_lmm_matches_the_reference_run()
