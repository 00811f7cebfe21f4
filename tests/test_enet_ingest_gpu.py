"""--wg enet fed by the native k-mer reader and the packed cache: sh_enet_ingest (k_enet_ingest_*), EnetMatrix.ingest,
enet.load_all_vars_blocks and the command line on top of them.

Every comparison is exact (bytes and integers): the feature moves rows, it computes no floating-point figure of its own.
Yardsticks: tests/golden/enet/ref_kmers_*.npz (the reference's own load_all_vars on tests/golden/cli/kmers.gz), ref_rows.json (its own
find_enet_selected + format_output for a fixed slope vector), numpy on the host, and this project's --python-reader run of the same input."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
GOLD = os.path.join(ROOT, "tests", "golden", "enet")
BASE = ["--phenotypes", "subset.pheno", "--min-af", "0.05", "--max-af", "0.95"]
KMERS = ["--kmers", "kmers.gz"] + BASE

# a child that runs the command line with the fixed slope vector of tests/test_enet_cli_gpu.py in place of the fit's
FIXED = ("import sys, numpy as np\n"
         "from pyseer_amd import enet\n"
         "def fixed_betas(n_cov, var_indices):\n"
         "    j = np.arange(len(var_indices))\n"
         "    return np.concatenate([[0.25], np.zeros(n_cov), np.where(j % 7 == 0, ((j * 37) % 11 - 5) / 10.0 + 0.05, 0.0)])\n"
         "enet.TEST_BETAS = fixed_betas\n"
         "from pyseer_amd.__main__ import main\n"
         "main(sys.argv[1:])\n")


def run(args, expect=0, fixed=False):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    head = [sys.executable, "-c", FIXED] if fixed else [sys.executable, "-m", "pyseer_amd"]
    r = subprocess.run(head + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode()


def _pheno(column="binary"):
    from pyseer_amd.input import load_phenotypes
    return load_phenotypes(os.path.join(CLI, "subset.pheno"), column)


def _host_counts(bits, n):
    return np.unpackbits(bits, axis=1, bitorder="little")[:, :n].sum(axis=1)


def _raw_kmers(p, block):
    from pyseer_amd.input import iter_packed_blocks_native
    return iter_packed_blocks_native(p, os.path.join(CLI, "kmers.gz"), 0.0, 1.0, block, raw=True)


@pytest.mark.parametrize("block", [7, 64, 4096])
def test_raw_blocks_give_the_references_matrix(block):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import load_all_vars_blocks, correlation_cut
    g = np.load(os.path.join(GOLD, "ref_kmers_binary.npz"))
    p = _pheno()
    assert [str(s) for s in g["samples"]] == list(p.index)
    e = Engine(len(p))
    M, var_indices, loaded, blob, off, counts = load_all_vars_blocks(e, p, _raw_kmers(p, block), 0.05, 0.95, 0.05, capacity=1)
    assert loaded == int(g["loaded"]) == 200
    assert (np.asarray(var_indices) == g["var_indices"]).all()
    assert M.rows == 176 and (M.get_rows(np.arange(M.rows)) == g["rows"]).all()
    cor = M.correlations(g["y"])
    for q, key in ((0.25, "kept25"), (0.5, "kept50")):
        assert (correlation_cut(cor, q) == g[key]).all()
    # names and counts are those of the kept lines of the file
    lines = gzip.open(os.path.join(CLI, "kmers.gz"), "rt").read().splitlines()
    names = [bytes(blob[off[i]:off[i + 1]]).decode() for i in range(M.rows)]
    assert names == [lines[i].split()[0] for i in g["var_indices"]]
    stored = _host_counts(g["rows"], len(p))
    assert (np.where(2 * counts > len(p), len(p) - counts, counts) == stored).all()
    M.close()
    e.close()


def test_the_rule_is_strict_at_its_boundaries():
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import load_all_vars, load_all_vars_blocks, count_bounds
    from pyseer_amd.input import open_variant_file
    p = _pheno()
    n = len(p)
    all_counts = np.concatenate([b.counts for b in _raw_kmers(p, 4096)])
    assert (all_counts == 5).sum() == 7 and (all_counts == 45).sum() == 2 and (all_counts == 0).sum() == 6 and (all_counts == 25).sum() == 3
    af = all_counts.astype(float) / n
    want = np.nonzero((af > 0.1) & (af < 0.9) & (0.0 < 0.05))[0]
    assert want.size == 153 and ((af >= 0.1) & (af <= 0.9)).sum() == 162
    assert count_bounds(n, 0.1, 0.9, 0.05) == (6, 44)
    e = Engine(n)
    M, var_indices, loaded, _, _, counts = load_all_vars_blocks(e, p, _raw_kmers(p, 64), 0.1, 0.9, 0.05)
    assert (np.asarray(var_indices) == want).all() and loaded == 200 and (counts == all_counts[want]).all()
    rows1 = M.get_rows(np.arange(M.rows))
    M.close()                                                         # (an engine holds one matrix at a time)
    infile, order = open_variant_file("kmers", os.path.join(CLI, "kmers.gz"))
    M2, vi2, loaded2 = load_all_vars(e, "kmers", p, False, None, infile, set(p.index), order, 0.1, 0.9, 0.05, False)
    assert list(vi2) == list(want) and loaded2 == 200
    rows2 = M2.get_rows(np.arange(M2.rows))
    M2.close()
    assert rows1.shape == rows2.shape and (rows1 == rows2).all()
    M3, vi3, _, _, _, _ = load_all_vars_blocks(e, p, _raw_kmers(p, 7), 0.1, 0.9, 0.05)
    assert (M3.get_rows(np.arange(M3.rows)) == rows2).all()
    M3.close()
    for mm in (0.0, -1.0):
        with pytest.raises(ValueError, match="No variants passed filters"):
            load_all_vars_blocks(e, p, _raw_kmers(p, 64), 0.05, 0.95, mm)
    e.close()


@pytest.mark.parametrize("n", [63, 64, 65, 1000, 5000])
def test_volume_and_shapes_against_numpy_and_append(n):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, count_bounds
    from pyseer_amd.packing import row_bytes_for
    rng = np.random.default_rng(1000 + n)
    rb = row_bytes_for(n)
    lo, hi = count_bounds(n, 0.02, 0.97, 0.05)
    blocks = []
    for V in (1, 5, 257, 3000, 1024, 4097):
        dens = rng.choice([0.0, 0.01, 0.03, 0.3, 0.5, 0.7, 0.96, 0.99, 1.0], size=V)
        K = rng.random((V, n)) < dens[:, None]
        if V >= 257:
            K[3] = False; K[3, :n // 2] = True                        # exactly n / 2 carriers (n even), or just below
            K[4] = False; K[4, :n // 2 + 1] = True                    # just above
            K[5] = False; K[5, :lo] = True; K[6] = False; K[6, :max(lo - 1, 0)] = True
            K[7] = False; K[7, :hi] = True; K[8] = False; K[8, :min(hi + 1, n)] = True
        bits = np.zeros((V, rb), dtype=np.uint8)
        pk = np.packbits(K, axis=1, bitorder="little")
        bits[:, :pk.shape[1]] = pk
        clean = bits.copy()
        # padding bits set on purpose: the decision and the stored words must not see them
        pad = np.zeros(rb * 8, dtype=np.uint8); pad[n:] = 1
        dirty = bits | (np.packbits(pad, bitorder="little")[None, :] * (rng.random((V, 1)) < 0.5).astype(np.uint8))
        blocks.append((K, clean, dirty))
    e1, e2 = Engine(n), Engine(n)
    M1, M2 = EnetMatrix(e1, 1), EnetMatrix(e2, sum(b[0].shape[0] for b in blocks))
    want_rows = []
    for K, clean, dirty in blocks:
        c = K.sum(axis=1)
        af = c.astype(float) / n
        keep = np.nonzero((af > 0.02) & (af < 0.97))[0]
        flip = af > 0.5
        idx, cnt = M1.ingest(dirty, lo, hi)
        assert idx.dtype == np.int32 and (idx == keep).all() and (cnt == c[keep]).all()
        M2.append(clean[keep], None, flip[keep].astype(np.uint8))
        Kc = np.where(flip[:, None], ~K, K)[keep]
        w = np.zeros((keep.size, rb), dtype=np.uint8)
        pk = np.packbits(Kc, axis=1, bitorder="little")
        w[:, :pk.shape[1]] = pk
        want_rows.append(w)
    want_rows = np.concatenate(want_rows)
    assert M1.rows == M2.rows == want_rows.shape[0] > 0
    got = M1.get_rows(np.arange(M1.rows))
    assert (got == want_rows).all()
    assert (M2.get_rows(np.arange(M2.rows)) == got).all()
    # an empty interval and an empty block keep nothing and leave the matrix alone
    idx, cnt = M1.ingest(blocks[2][2], 1, 0)
    assert idx.size == 0 and cnt.size == 0 and M1.rows == want_rows.shape[0]
    idx, cnt = M1.ingest(np.zeros((0, rb), dtype=np.uint8), lo, hi)
    assert idx.size == 0 and M1.rows == want_rows.shape[0]
    assert (M1.get_rows(np.arange(M1.rows)) == want_rows).all()
    # the solver is untouched: the same rows give the same bytes
    y = rng.standard_normal(n)
    fold = (np.arange(n) % 5).astype(np.int32)
    f1 = M1.fit(y, True, 0.5, fold_id=fold, n_folds=5, n_lambda=8)
    f2 = M2.fit(y, True, 0.5, fold_id=fold, n_folds=5, n_lambda=8)
    assert f1.n_lambda == f2.n_lambda and f1.beta.tobytes() == f2.beta.tobytes() and f1.beta0 == f2.beta0
    assert f1.cvm.tobytes() == f2.cvm.tobytes()
    M1.close(); M2.close()
    e1.close(); e2.close()


WG = ["--wg", "enet"]


@pytest.mark.parametrize("extra", [["--phenotype-column", "binary"], ["--phenotype-column", "continuous"],
                                   ["--phenotype-column", "binary", "--distances", "distances50.tsv"],
                                   ["--phenotype-column", "binary", "--lineage-clusters", "clusters50.txt", "--lineage"],
                                   ["--phenotype-column", "binary", "--print-samples"],
                                   ["--phenotype-column", "binary", "--min-af", "0.1", "--max-af", "0.9"]])
def test_native_run_prints_what_the_python_reader_run_prints(extra, tmp_path):
    if "--lineage" in extra:
        extra = extra + ["--lineage-file", str(tmp_path / "lin.txt")]
    native = run(KMERS + WG + extra)
    python = run(KMERS + WG + extra + ["--python-reader"])
    assert native[0] == python[0] and len(native[0].splitlines()) > 1
    assert native[1] == python[1]


def _halves(tmp_path):
    lines = gzip.open(os.path.join(CLI, "kmers.gz"), "rb").read().splitlines(True)
    a, b = str(tmp_path / "a.gz"), str(tmp_path / "b.gz")
    with gzip.open(a, "wb") as f:
        f.write(b"".join(lines[:93]))
    with gzip.open(b, "wb") as f:
        f.write(b"".join(lines[93:]))
    return a, b


TAGS = [("plain", ["--print-samples"]), ("distances", ["--distances", "distances50.tsv"]), ("lineage", ["--lineage-clusters", "clusters50.txt", "--lineage"])]


def _rows_are_the_references(tag, out, err):
    want = json.load(open(os.path.join(GOLD, "ref_rows.json")))[tag]
    out = out.splitlines()
    header = ['variant', 'af', 'filter-pvalue', 'lrt-pvalue', 'beta'] + (['lineage'] if tag == "lineage" else []) + \
        (['k-samples', 'nk-samples'] if tag == "plain" else []) + ['notes']
    assert out[0] == "\t".join(header)
    assert out[1:] == want
    assert "%d printed variants" % len(want) in err and "200 loaded variants" in err


@pytest.mark.parametrize("tag,extra", TAGS)
def test_fixed_beta_rows_from_two_files_and_from_caches_are_the_references(tag, extra, tmp_path):
    """On the commit before this feature each of these runs ends with status 1: "the packed cache and several --kmers files are not
    available with it"."""
    if tag == "lineage":
        extra = extra + ["--lineage-file", str(tmp_path / "lin.txt")]
    tail = BASE + ["--phenotype-column", "binary"] + WG + extra
    a, b = _halves(tmp_path)
    _rows_are_the_references(tag, *run(["--kmers", a, b] + tail, fixed=True))
    # (a) a cache an enet run wrote
    ca = str(tmp_path / "enet.seerpack")
    _rows_are_the_references(tag, *run(KMERS + ["--phenotype-column", "binary"] + WG + extra + ["--save-packed", ca], fixed=True))
    # (--kmers is a required argument; that the rows come from the cache shows in naming half the input beside it)
    _rows_are_the_references(tag, *run(["--kmers", b, "--load-packed", ca] + tail, fixed=True))
    # (b) a cache a plain per-variant run wrote (other AF window on purpose: the cache holds every parsed line)
    cb = str(tmp_path / "plain.seerpack")
    run(["--kmers", "kmers.gz", "--phenotypes", "subset.pheno", "--phenotype-column", "binary", "--no-distances", "--min-af", "0.2", "--max-af", "0.8",
         "--save-packed", cb])
    _rows_are_the_references(tag, *run(["--kmers", b, "--load-packed", cb] + tail, fixed=True))
    # and the reverse: the per-variant run reads the cache the enet run wrote, and prints what it prints from the text
    per = ["--phenotypes", "subset.pheno", "--phenotype-column", "binary", "--no-distances"]
    assert run(["--kmers", "kmers.gz", "--load-packed", ca] + per)[0] == run(["--kmers", "kmers.gz"] + per)[0]


def test_packed_cache_twice(tmp_path):
    import shutil
    k = str(tmp_path / "k.gz")
    shutil.copy(os.path.join(CLI, "kmers.gz"), k)
    args = ["--kmers", k] + BASE + ["--phenotype-column", "binary"] + WG
    plain = run(args)
    first = run(args + ["--packed-cache"])
    assert os.path.exists(k + ".seerpack") and os.path.exists(k + ".seerpack.stamp")
    stamp = os.stat(k + ".seerpack").st_mtime_ns
    second = run(args + ["--packed-cache"])
    assert os.stat(k + ".seerpack").st_mtime_ns == stamp, "the second run wrote the cache again"
    assert first == plain and second == plain
    # a real fit from two files is the fit from one
    a, b = _halves(tmp_path)
    assert run(["--kmers", a, b] + BASE + ["--phenotype-column", "binary"] + WG) == plain


def test_refusals_stay(tmp_path):
    wg = KMERS + WG
    for extra, word in ((["--gpus", "2"], "--gpus"), (["--load-packed", "x", "--packed-part", "0/2"], "--packed-part"), (["--save-vars", "x"], "--save-vars"),
                        (["--load-vars", "x"], "--load-vars"), (["--save-model", "x"], "--save-model"), (["--output-patterns", "x.txt"], "patterns")):
        _, err = run(wg + extra, expect=1)
        assert word in err
    for model in ("rf", "blup"):
        _, err = run(KMERS + ["--wg", model], expect=1)
        assert model in err
    _, err = run(wg + ["--lmm", "--similarity", "similarity50.tsv"], expect=1)
    assert "--lmm" in err
    old = "the packed cache and several --kmers files are not available with it"
    _, err = run(["--kmers", "kmers.gz", "kmers.gz"] + BASE + WG + ["--python-reader"], expect=1)
    assert old in err
    for cache in (["--save-packed", str(tmp_path / "c")], ["--load-packed", str(tmp_path / "c")], ["--packed-cache"]):
        _, err = run(wg + ["--python-reader"] + cache, expect=1)
        assert old in err
        _, err = run(["--vcf", os.path.join("..", "vcf", "variants50.vcf.gz")] + BASE + WG + cache, expect=1)
        assert "--vcf" in err
        _, err = run(["--pres", "kmers120.Rtab"] + BASE + WG + cache, expect=1)
        assert old in err
    _, err = run(["--kmers", "subset.pheno"] + BASE + WG, expect=1)
    assert "Not a gzipped file" in err
