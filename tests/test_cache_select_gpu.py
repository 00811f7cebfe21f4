"""A packed cache served to a subset or another order of its samples, on the device: k_rows_select (csrc/select_kernels.hip) through
engine.RowSelector against numpy, and the command line reading a cache over all 1837 isolates of tests/golden/cli/kmers.gz -- or one
written by --save-packed over 50 -- for runs over fewer samples in another order: the bytes of the same command reading the text.
The text side is held to the reference by tests/test_cli_gpu.py::test_cli_matches_reference; identity carries that over."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _cache_select as cs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = cs.CLI
CASES = json.load(open(os.path.join(CLI, "cases.json")))
METER = re.compile(r"\r\d+variants \[[^\]]*\]")
OLD_ERROR = "packed cache was written for a different sample list / order"


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def _selector(n_src, m):
    from pyseer_amd.engine import Engine, RowSelector
    eng = Engine(len(m))
    return eng, RowSelector(eng, n_src, m)


def _both_ways(sel, bits, n_src, m):
    import torch
    got_bits, got_counts = sel.select(bits)
    cs.check_selected(got_bits, got_counts, bits, n_src, m)
    d_bits, d_counts = sel.select_dev(torch.from_numpy(bits).cuda())
    cs.check_selected(d_bits.cpu().numpy(), d_counts.cpu().numpy(), bits, n_src, m)


@pytest.mark.parametrize("n_src", cs.N_SRC)
def test_kernel_equals_numpy(n_src):
    rng = np.random.default_rng(n_src)
    rows = {V: cs.source_rows(V, n_src, rng)[0] for V in cs.V_ROWS}
    from pyseer_amd.engine import Engine, RowSelector
    for n_dst in cs.n_dsts(n_src):
        eng = Engine(n_dst)
        for kind in cs.MAP_KINDS:
            m = cs.make_map(kind, n_src, n_dst, rng)
            sel = RowSelector(eng, n_src, m)
            for V in cs.V_ROWS:
                _both_ways(sel, rows[V], n_src, m)
            sel.close()
        eng.close()


@pytest.mark.parametrize("n_src,n_dst,kind", [(5200, 5000, "subset"), (5000, 5000, "permuted")])
def test_kernel_equals_numpy_many_rows(n_src, n_dst, kind):
    """4097 rows: 257 workgroups of sixteen rows, the last with one row in one of its four wavefronts (the staging chunks of the host entry
    point are walked by test_host_rows_in_several_chunks)"""
    rng = np.random.default_rng(1)
    bits, _ = cs.source_rows(4097, n_src, rng)
    m = cs.make_map(kind, n_src, n_dst, rng)
    eng, sel = _selector(n_src, m)
    _both_ways(sel, bits, n_src, m)
    sel.close(); eng.close()


def test_host_rows_in_several_chunks():
    """sh_select_rows stages 16 MB of source rows at a time through two slots: 60 000 rows of 656 bytes are three chunks, the last ragged"""
    rng = np.random.default_rng(2)
    one, _ = cs.source_rows(1000, 5200, rng)
    bits = np.ascontiguousarray(np.tile(one, (60, 1)))
    bits[:, 0] ^= (np.arange(60000) & 0xFF).astype(np.uint8)                       # (no two chunks alike)
    m = cs.make_map("permuted", 5200, 5000, rng)
    eng, sel = _selector(5200, m)
    got_bits, got_counts = sel.select(bits)
    cs.check_selected(got_bits, got_counts, bits, 5200, m)
    sel.close(); eng.close()


@pytest.mark.parametrize("n_src", [40000, 140000])
def test_wide_source_rows_take_the_narrow_shapes(n_src):
    """a source row of more than 4 KB leaves no room for sixteen rows per workgroup in the LDS: one row per wavefront, four wavefronts (40 000
    samples: 5000 bytes) and, above 16 KB, one (140 000 samples: 17 500 bytes)"""
    rng = np.random.default_rng(n_src)
    bits, _ = cs.source_rows(9, n_src, rng)
    m = cs.make_map("permuted", n_src, 4161, rng)
    eng, sel = _selector(n_src, m)
    _both_ways(sel, bits, n_src, m)
    sel.close(); eng.close()


def test_selected_rows_count_patterns_like_host_rows():
    import torch
    from pyseer_amd.engine import PatternSet
    rng = np.random.default_rng(3)
    base, _ = cs.source_rows(300, 1837, rng)
    bits = np.ascontiguousarray(base[rng.integers(0, 300, 2000)])                  # 2000 rows, at most 300 distinct
    m = cs.make_map("permuted", 1837, 50, rng)
    eng, sel = _selector(1837, m)
    want_bits, _ = cs.numpy_select(bits, 1837, m)
    ps = PatternSet(eng)
    ps.add_rows(want_bits)
    want = ps.count()
    ps.close()
    assert want == len({r.tobytes() for r in want_bits})
    d_bits, _ = sel.select_dev(torch.from_numpy(bits).cuda())
    ps = PatternSet(eng)
    ps.add_rows_dev(d_bits)
    assert ps.count() == want
    ps.close(); sel.close(); eng.close()


def test_too_wide_a_source_row_is_refused_by_name():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine, RowSelector
    eng = Engine(100)
    with pytest.raises(_abi.SeerHipError, match="k_rows_select"):
        RowSelector(eng, 524288 + 1, np.arange(100))
    with pytest.raises(_abi.SeerHipError, match="another number of samples"):
        RowSelector(eng, 200, np.arange(99))
    with pytest.raises(_abi.SeerHipError, match="selected twice"):
        RowSelector(eng, 200, np.zeros(100, dtype=np.int32))
    sel = RowSelector(eng, 524288, np.arange(100))                                 # the widest row that fits is taken
    sel.close(); eng.close()


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def run(args, expect=0, route=None, module="pyseer_amd"):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    env.pop("SEERHIP_ROUTE", None)
    if route:
        env["SEERHIP_ROUTE"] = route
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout, r.stderr.decode()


def plain(err):
    """stderr without the lines this build adds (`pyseer_amd: ...`) and without the reference's progress meter"""
    return [l for l in METER.sub("", err).split("\n") if l != "" and not l.startswith("pyseer_amd:")]


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    """all.seerpack / all50.seerpack: every isolate of kmers.gz, stored in blocks of 3000 / 50 variants (no device: pyseer_amd.pack)"""
    d = tmp_path_factory.mktemp("caches")
    listing = str(d / "all.txt")
    with open(listing, "w") as fh:
        fh.write("".join(s + "\n" for s in cs.all_samples()))
    out = {}
    for name, block in (("all", 3000), ("all50", 50)):
        out[name] = str(d / (name + ".seerpack"))
        run([listing, "--kmers", "kmers.gz", "-o", out[name], "--block", str(block)], module="pyseer_amd.pack")
    return out


def _with_files(args, tmp_path):
    """the case's arguments with every output file under tmp_path; -> (args, the files)"""
    args, files = list(args), []
    for opt in ("--lineage-file", "--output-patterns", "--count-patterns"):
        if opt in args:
            i = args.index(opt)
            args[i + 1] = str(tmp_path / os.path.basename(args[i + 1]))
            files.append(args[i + 1])
    return args, files


def _take(files):
    """the files' bytes; the files are removed (the next run writes the same names: stderr names them)"""
    out = []
    for f in files:
        with open(f, "rb") as fh:
            out.append(fh.read())
        os.remove(f)
    return out


def _same_run(args, cache, tmp_path, route=None):
    args, files = _with_files(args, tmp_path)
    want_out, want_err = run(args)
    want_files = _take(files)
    got_out, got_err = run(args + ["--load-packed", cache], route=route)
    assert got_out == want_out and len(want_out.splitlines()) > 1
    assert plain(got_err) == plain(want_err)
    assert _take(files) == want_files and all(len(b) > 0 for b in want_files)
    return got_err


ENET = ["--kmers", "kmers.gz", "--phenotypes", "subset.pheno", "--min-af", "0.05", "--max-af", "0.95", "--phenotype-column", "binary", "--wg", "enet"]
CLI_CASES = {name: CASES[name] for name in ("fixed", "fixed_dim3_samples", "fixed_lineage_clusters", "cont", "lmm", "lmm_cov", "lmm_all")}
CLI_CASES["fixed_output_patterns"] = CASES["fixed"] + ["--output-patterns", "patterns.txt"]
CLI_CASES["fixed_count_patterns"] = CASES["fixed"] + ["--count-patterns", "count.txt"]
CLI_CASES["enet"] = ENET


@pytest.mark.parametrize("name", sorted(CLI_CASES))
def test_superset_cache_gives_the_text_runs_bytes(name, caches, tmp_path):
    # (lmm_all prints filtered rows and fits the lineage of each block's last variant: its blocks must end where the text run's do)
    cache = caches["all50"] if name == "lmm_all" else caches["all"]
    assert "--block_size" in CLI_CASES[name] or name != "lmm_all"
    err = _same_run(CLI_CASES[name], cache, tmp_path)
    assert "pyseer_amd: packed cache holds 1837 samples; the run's 50 are selected on the device\n" in err


@pytest.fixture(scope="module")
def shuffled(tmp_path_factory):
    """a cache written by --save-packed over the 50 samples of subset.pheno, and a phenotype file of 37 of them in another order"""
    d = tmp_path_factory.mktemp("shuffled")
    cache = str(d / "fifty.seerpack")
    run(["--kmers", "kmers.gz", "--phenotypes", "subset.pheno", "--no-distances", "--save-packed", cache])
    lines = open(os.path.join(CLI, "subset.pheno")).read().splitlines()
    order = np.random.default_rng(7).permutation(50)[:37]
    pheno = str(d / "shuffled37.pheno")
    with open(pheno, "w") as fh:
        fh.write("\n".join([lines[0]] + [lines[1 + i] for i in order]) + "\n")
    return cache, pheno


@pytest.mark.parametrize("route", [None, "cache_select=host"])
def test_save_packed_cache_serves_a_shuffled_subset(shuffled, route, tmp_path):
    cache, pheno = shuffled
    args = ["--kmers", "kmers.gz", "--phenotypes", pheno, "--distances", "distances50.tsv", "--print-filtered"]
    err = _same_run(args, cache, tmp_path, route=route)
    assert ("pyseer_amd: packed cache holds 50 samples; the run's 37 are selected on the %s\n" % ("host" if route else "device")) in err


def test_host_route_gives_the_same_bytes(caches, tmp_path):
    _same_run(CLI_CASES["fixed"], caches["all"], tmp_path, route="cache_select=host")


def test_python_sinks_take_the_select_route_too(caches, tmp_path):
    want_out, _ = run(CLI_CASES["fixed"])
    for sink in ("--python-sink", "--serial-sink"):
        got_out, err = run(CLI_CASES["fixed"] + [sink, "--load-packed", caches["all"]])
        assert got_out == want_out and "selected on the device" in err


def test_refusals(caches):
    # the route key turns the feature off: the error every cache of other samples has always met
    out, err = run(CLI_CASES["fixed"] + ["--load-packed", caches["all"]], expect=1, route="cache_select=0")
    assert "ValueError: " + OLD_ERROR + " (1837 vs 50 samples)" in err
    # several devices, or one part of the cache: one line, nothing on stdout
    for extra in (["--gpus", "0,0"], ["--packed-part", "0/2"]):
        out, err = run(CLI_CASES["fixed"] + ["--load-packed", caches["all"]] + extra, expect=1)
        assert out == b"" and "Traceback" not in err
        assert "pyseer_amd: a packed cache over other samples than the run's own list is read on one device" in err
