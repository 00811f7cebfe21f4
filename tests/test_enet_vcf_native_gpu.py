"""--wg enet fed by the native VCF reader, burden regions included: input.iter_call_blocks_vcf_native, enet.load_all_vars_calls (over
sh_enet_ingest_calls), selected_from_rows with missing calls, and the command line on top of them.

Every comparison is exact (bytes and integers): the route moves rows, it computes no floating-point figure of its own.  The yardstick is this
project's --python-reader run of the same input (read_variant line by line, twice over the file), and enet.load_all_vars for the matrix."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vcf_text  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
VCF = os.path.join(ROOT, "tests", "golden", "vcf")
V50 = os.path.join(VCF, "variants50.vcf.gz")
BASE = ["--phenotypes", "subset.pheno", "--min-af", "0.05", "--max-af", "0.95"]
WG = ["--wg", "enet"]

# a child that runs the command line with the fixed slope vector of tests/test_enet_ingest_gpu.py in place of the fit's (every seventh kept
# row is selected) and leaves the route the run took in the file ENET_ROUTE_FILE names
FIXED = ("import os, sys, numpy as np\n"
         "from pyseer_amd import enet\n"
         "def fixed_betas(n_cov, var_indices):\n"
         "    j = np.arange(len(var_indices))\n"
         "    return np.concatenate([[0.25], np.zeros(n_cov), np.where(j % 7 == 0, ((j * 37) % 11 - 5) / 10.0 + 0.05, 0.0)])\n"
         "enet.TEST_BETAS = fixed_betas\n"
         "from pyseer_amd.__main__ import main\n"
         "try:\n"
         "    main(sys.argv[1:])\n"
         "finally:\n"
         "    open(os.environ['ENET_ROUTE_FILE'], 'w').write(str(getattr(enet, 'LAST_LOAD_ROUTE', None)))\n")


def run(args, route_file, expect=0):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    env["ENET_ROUTE_FILE"] = str(route_file)
    r = subprocess.run([sys.executable, "-c", FIXED] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode(), open(str(route_file)).read()


def both_routes(args, tmp_path):
    """the default run and the --python-reader run: same bytes on both streams, routes "calls" and "lines"; returns the default run's"""
    native = run(args, tmp_path / "route_native")
    python = run(args + ["--python-reader"], tmp_path / "route_python")
    assert native[2] == "calls" and python[2] == "lines"
    assert native[0] == python[0]
    assert native[1] == python[1]
    return native


def _printed(out):
    return out.splitlines()[1:]


@pytest.mark.parametrize("extra", [["--phenotype-column", "binary"], ["--phenotype-column", "continuous"],
                                   ["--phenotype-column", "binary", "--distances", "distances50.tsv"],
                                   ["--phenotype-column", "continuous", "--distances", "distances50.tsv"],
                                   ["--phenotype-column", "binary", "--lineage-clusters", "clusters50.txt", "--sequence-reweighting"]])
def test_vcf_run_prints_what_the_python_reader_run_prints(extra, tmp_path):
    """variants50: of 254 records 15 are skipped, 47 pass the strict rule and 4 of those are stored flipped (Python reader on the CPU)."""
    out, err, _ = both_routes(["--vcf", V50] + BASE + WG + extra, tmp_path)
    assert len(_printed(out)) >= 1 and "254 loaded variants" in err   # (--cor-filter's default cuts the 47 at their 25th percentile)
    assert "Multiple alleles at FM211187_23. Skipping\n" in err


def test_burden_run_prints_what_the_python_reader_run_prints(tmp_path):
    out, err, _ = both_routes(["--vcf", V50, "--burden", os.path.join(VCF, "burden_regions_multiple.txt")] + BASE + WG + ["--phenotype-column", "binary"],
                              tmp_path)
    assert len(_printed(out)) == 1 and "3 loaded variants" in err and "2 tested variants" in err      # (3 pass the AF window, 2 the correlation cut)


def test_burden_messages_are_said_again_for_a_selected_line(tmp_path):
    """The first line holds a multi-allelic record (FM211187:4887) and an unparsable region and passes the AF window (its carriers come
    from 4908 and from 3910-3951), so the fixed slope vector selects it: the reference's second pass parses it again and says both lines a
    second time.  The second line's unparsable region and the third's empty region are said once, on the first pass."""
    regions = tmp_path / "regions.txt"
    regions.write_text("R1 FM211187:4885-4910,junk,FM211187:3910-3951\n"
                       "R2 nonsense,FM211187:4006-4057\n"
                       "R3 FM211187:9000-9100\n")
    out, err, _ = both_routes(["--vcf", V50, "--burden", str(regions)] + BASE + WG + ["--phenotype-column", "binary", "--cor-filter", "0"], tmp_path)
    assert [l.split("\t")[0] for l in _printed(out)] == ["R1"]
    assert err.count("Multiple alleles at FM211187_4887. Skipping\n") == 2
    assert err.count("Could not parse region None\n") == 3
    assert err.count("No observations of R3 in selected samples\n") == 1
    assert "3 loaded variants" in err and "2 tested variants" in err


def _generated(tmp_path, n_pheno, n_cols):
    text, pheno, _ = _vcf_text.generated_vcf(n_pheno=n_pheno, n_cols=n_cols, n_records=600, seed=7, missing=0.03)
    path = str(tmp_path / "generated.vcf.gz")
    _vcf_text.write_bgzf(path, text)
    y = np.random.RandomState(3).randint(0, 2, n_pheno)
    ph = str(tmp_path / "generated.pheno")
    with open(ph, "w") as f:
        f.write("samples\tbinary\n" + "".join("%s\t%d\n" % (s, b) for s, b in zip(pheno, y)))
    return path, ph


@pytest.mark.parametrize("n_pheno,n_cols,kept", [(200, 230, 458), (65, 70, 431)])
def test_missing_calls_synthetic(n_pheno, n_cols, kept, tmp_path):
    """600 generated records, 3 % missing calls (Python reader on the CPU): at 200 samples 78 are skipped, 458 kept (442 with a missing call,
    98 stored flipped, 95 of those with a missing call), 33 rejected by the missing rule alone, 31 by AF; at 65 samples 431 kept, 340 with a
    missing call, 83 flipped.  Every seventh kept row is selected: rows of each kind.
    --cor-filter 0: 61 (89) of the kept records have missing calls and no carrier, so their stored row is empty, its correlation NaN, and
    the reference's percentile cut then keeps nothing on either route ("No variants passed filters")."""
    path, ph = _generated(tmp_path, n_pheno, n_cols)
    out, err, _ = both_routes(["--vcf", path, "--phenotypes", ph, "--min-af", "0.01", "--max-af", "0.99"] + WG + ["--print-samples", "--cor-filter", "0"],
                              tmp_path)
    assert "600 loaded variants" in err and "%d tested variants" % kept in err and len(_printed(out)) == (kept + 6) // 7


@pytest.fixture(scope="module")
def line_by_line(tmp_path_factory):
    """enet.load_all_vars on the generated file, once: (path, phenotypes, var_indices, loaded, rows)"""
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import load_all_vars
    from pyseer_amd.input import load_phenotypes, open_variant_file
    path, ph = _generated(tmp_path_factory.mktemp("enet_vcf"), 200, 230)
    p = load_phenotypes(ph, None)
    e = Engine(len(p))
    infile, order = open_variant_file("vcf", path)
    M, var_indices, loaded = load_all_vars(e, "vcf", p, False, None, infile, set(p.index), order, 0.01, 0.99, 0.05, False)
    rows = M.get_rows(np.arange(M.rows))
    M.close()
    e.close()
    return path, p, np.asarray(var_indices), loaded, rows


@pytest.mark.parametrize("block", [7, 64, 4096])
def test_call_blocks_give_the_line_by_line_matrix(block, line_by_line):
    import io
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import load_all_vars_calls
    from pyseer_amd.input import iter_call_blocks_vcf_native
    path, p, want_idx, want_loaded, want_rows = line_by_line
    assert want_loaded == 600 and want_idx.size == 458
    n = len(p)
    e = Engine(n)
    err = io.StringIO()
    M, var_indices, loaded, kept = load_all_vars_calls(e, p, iter_call_blocks_vcf_native(p, path, e, block), 0.01, 0.99, 0.05, err, capacity=1)
    assert loaded == want_loaded and (np.asarray(var_indices) == want_idx).all()
    rows = M.get_rows(np.arange(M.rows))
    assert rows.shape == want_rows.shape and (rows == want_rows).all()
    # what the host keeps: t per row, a missing row exactly where there is a missing call, and the stored row follows from the two
    assert kept.counts.shape == (458,) and int(kept.has_missing.sum()) == 442 == kept.missing_rows.shape[0]
    flipped = 2 * kept.counts > n
    assert int(flipped.sum()) == 98 and int((flipped & kept.has_missing).sum()) == 95
    stored = np.unpackbits(rows, axis=1, bitorder="little")[:, :n].sum(axis=1)
    n_m = np.zeros(458, dtype=np.int64)
    n_m[kept.has_missing] = np.unpackbits(kept.missing_rows, axis=1, bitorder="little")[:, :n].sum(axis=1)
    assert (np.where(flipped, n - kept.counts, kept.counts - n_m) == stored).all()
    assert err.getvalue().count("Multiple alleles at ") > 0
    M.close()
    e.close()


def test_refusals_stay_on_the_vcf_route(tmp_path):
    words = "--gpus and the packed cache (--save-packed / --load-packed / --packed-cache / --packed-part) are not available with --vcf"
    wg = ["--vcf", V50] + BASE + WG
    burden = ["--burden", os.path.join(VCF, "burden_regions_multiple.txt")]
    for extra in (["--gpus", "2"], ["--load-packed", "x", "--packed-part", "0/2"], ["--save-packed", str(tmp_path / "c")],
                  ["--load-packed", str(tmp_path / "c")], ["--packed-cache"], burden + ["--gpus", "2"], burden + ["--packed-cache"]):
        _, err, route = run(wg + extra, tmp_path / "route", expect=1)
        assert words in err and route == "None"


def test_pres_stays_line_by_line(tmp_path):
    old = "the packed cache and several --kmers files are not available with it"
    _, err, _ = run(["--pres", "kmers120.Rtab"] + BASE + WG + ["--packed-cache"], tmp_path / "route", expect=1)
    assert old in err
    out, err, route = run(["--pres", "kmers120.Rtab"] + BASE + WG + ["--phenotype-column", "binary"], tmp_path / "route")
    assert route == "lines" and len(_printed(out)) > 0
