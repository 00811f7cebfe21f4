"""python -m pyseer_amd.enet_predict, enet.EnetPredictor (sh_predict_*, k_enet_predict) and --save-enet-model.

Yardsticks: tests/golden/predict/ -- stdout and stderr of the reference's own pyseer.enet_predict on the models committed there
(tests/golden/make_predict_golden.py); a numpy loop `acc += k_r * beta_r` compared as 64-bit patterns; numpy on the host for the figures
the reference cannot give here (--true-values, a VCF).  Every comparison of printed text is of bytes."""
import collections
import gzip
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
GOLD = os.path.join(ROOT, "tests", "golden", "predict")
VCF = os.path.join(ROOT, "tests", "golden", "vcf", "variants_missing.vcf.gz")
VCF50 = os.path.join(ROOT, "tests", "golden", "vcf", "variants50.vcf.gz")
METER = re.compile(r"\r\d+variants \[[^\]]*\]")          # the reference's tqdm meter: the one thing of its stderr this build does not write
with open(os.path.join(GOLD, "cases.json")) as _fh:
    CASES = json.load(_fh, object_pairs_hook=collections.OrderedDict)


def run(module, args, expect=0):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode()


def predict(args, expect=0):
    return run("pyseer_amd.enet_predict", args, expect)


def without_meter(err):
    return "\n".join(line for line in METER.sub("", err).split("\n") if line != "")


def golden(case):
    with open(os.path.join(GOLD, case + ".out"), "rb") as fh:
        out = fh.read().decode()
    with open(os.path.join(GOLD, case + ".err"), "rb") as fh:
        err = fh.read().decode()
    return out, err


def as_pickle(model_path, tmp_path, numpy_scalars=False):
    """The reference's form of a committed text model: [dict, continuous], pickled."""
    from pyseer_amd.enet import read_model
    model, continuous = read_model(model_path)
    conv = np.float64 if numpy_scalars else float
    path = str(tmp_path / (os.path.basename(model_path) + ".pkl"))
    with open(path, "wb") as fh:
        pickle.dump([{k: (conv(a), conv(b)) for k, (a, b) in model.items()}, continuous], fh)
    return path


@pytest.mark.parametrize("case", list(CASES))
def test_bytes_are_the_references(case, tmp_path):
    want_out, want_err = golden(case)
    assert METER.search(want_err), "the golden holds the reference's meter"
    model = os.path.join(GOLD, case + ".model")
    args = ["samples50.txt"] + CASES[case]["args"]
    routes = [("text model", [model] + args), ("pickle", [as_pickle(model, tmp_path)] + args)]
    if "--kmers" in args:
        routes.append(("--python-reader", [model] + args + ["--python-reader"]))
    for label, a in routes:
        out, err = predict(a)
        assert out == want_out, label
        assert not METER.search(err), label
        assert without_meter(err) == without_meter(want_err), label


def _pheno_file(tmp_path, samples, name):
    with open(os.path.join(CLI, "subset.pheno")) as fh:
        rows = dict(line.rstrip("\n").split("\t", 1) for line in fh)
    path = str(tmp_path / name)
    with open(path, "w") as fh:
        fh.write("samples\t" + rows["samples"] + "\n")
        for s in samples:
            fh.write(s + "\t" + rows[s] + "\n")
    return path


def _samples50():
    with open(os.path.join(CLI, "samples50.txt")) as fh:
        return [line.rstrip() for line in fh]


def test_packed_caches_give_the_same_bytes(tmp_path):
    samples = _samples50()
    pheno = _pheno_file(tmp_path, samples, "all.pheno")
    per_variant, wg = str(tmp_path / "per_variant.seerpack"), str(tmp_path / "wg.seerpack")
    base = ["--kmers", "kmers.gz", "--phenotypes", pheno, "--phenotype-column", "binary", "--min-af", "0.05", "--max-af", "0.95"]
    run("pyseer_amd", base + ["--no-distances", "--save-packed", per_variant])
    run("pyseer_amd", base + ["--wg", "enet", "--save-packed", wg])
    for case in ("kmers_binary", "kmers_cov_continuous", "no_intercept"):
        want_out, want_err = golden(case)
        model = os.path.join(GOLD, case + ".model")
        rest = [x for x in CASES[case]["args"] if x not in ("--kmers", "kmers.gz")]
        for cache in (per_variant, wg):
            out, err = predict([model, "samples50.txt", "--load-packed", cache] + rest)
            assert out == want_out
            assert without_meter(err) == without_meter(want_err)
    # a cache over another sample list (here: one sample fewer) is refused with the cache reader's own message
    other = str(tmp_path / "other.seerpack")
    run("pyseer_amd", ["--kmers", "kmers.gz", "--phenotypes", _pheno_file(tmp_path, samples[:-1], "fewer.pheno"), "--phenotype-column", "binary",
                       "--no-distances", "--save-packed", other])
    out, err = predict([os.path.join(GOLD, "kmers_binary.model"), "samples50.txt", "--load-packed", other], expect=1)
    assert out == "" and "packed cache was written for a different sample list / order (49 vs 50 samples)" in err


@pytest.mark.parametrize("vcf", [VCF, VCF50])
def test_vcf_native_equals_python_reader(vcf, tmp_path):
    """variants_missing.vcf.gz: two records with missing calls, both in the model, one of them flipped.  variants50.vcf.gz: 254 records over 55
    samples (five are not in the samples file), among them records with several ALTs and filtered ones, which the model names too."""
    from pyseer_amd.enet import write_model
    from pyseer_amd.input import VCF_FILTERED, VCF_KEPT, VCF_MULTI, VcfFile
    recs = list(VcfFile(vcf))
    by_kind = {k: [r for r in recs if r.skip == k] for k in (VCF_KEPT, VCF_MULTI, VCF_FILTERED)}
    rng = np.random.default_rng(5)
    model = collections.OrderedDict([("intercept", (1, 0.125))])
    kept = [by_kind[VCF_KEPT][i] for i in rng.choice(len(by_kind[VCF_KEPT]), size=min(30, len(by_kind[VCF_KEPT])), replace=False)]
    for j, r in enumerate(kept):
        model[r.name] = (0.25 + 0.5 * (j % 2), 0.0 if j == 2 else float(rng.normal()))      # every other entry is flipped
    if vcf == VCF50:
        assert by_kind[VCF_MULTI] and by_kind[VCF_FILTERED], "the fixture holds multi-allelic and filtered records"
        model[by_kind[VCF_MULTI][0].name_all_alleles()] = (0.2, 0.5)   # named by the model: reported, never met
        model[by_kind[VCF_FILTERED][0].name] = (0.3, -0.5)             # filtered: never met either
    for continuous in (False, True):
        path = str(tmp_path / ("vcf%d.model" % continuous))
        write_model(path, model, continuous)
        native = predict([path, "samples50.txt", "--vcf", vcf])
        python = predict([path, "samples50.txt", "--vcf", vcf, "--python-reader"])
        assert native == python
        out, err = native
        assert len(out.split("\n")) == 52
        if vcf == VCF50:
            multi = by_kind[VCF_MULTI][0]
            assert err.count("Multiple alleles at") == 1 and ("Multiple alleles at %s_%d. Skipping\n" % (multi.contig, multi.pos)) in err
            assert ("Could not find covariate/variant " + multi.name_all_alleles()) in err
            assert ("Could not find covariate/variant " + by_kind[VCF_FILTERED][0].name) in err
            assert err.count("Could not find") == 2
        else:
            assert "Could not find" not in err and "nan" in out, "the fixture's missing calls reach the link"


# ---------------------------------------------------------------------------------------------------------------------------------------
def _case(n, rows, seed):
    """A block of `rows` packed rows over n samples with dirty padding bits, missing rows, flips, and slopes from 1e-300 to 1e300."""
    from pyseer_amd.packing import row_bytes_for
    rng = np.random.default_rng(seed)
    rb = row_bytes_for(n)
    present = rng.integers(0, 256, size=(rows, rb), dtype=np.uint8)            # (bits at and above n are dirty on purpose)
    missing = np.where(rng.random((rows, rb)) < 0.03, rng.integers(0, 256, size=(rows, rb), dtype=np.uint8), 0).astype(np.uint8)
    missing[:, (n + 7) // 8:] = 0xFF                                           # every padding bit says "missing"
    missing[rng.random(rows) < 0.5] &= 0                                       # half the rows have no missing call among the samples ...
    missing[:, (n + 7) // 8:] = 0xFF                                           # ... and dirty padding all the same
    flip = (rng.random(rows) < 0.4).astype(np.uint8)
    beta = rng.choice([-1.0, 1.0], size=rows) * 10.0 ** rng.uniform(-300, 300, size=rows)
    small = rng.random(rows) < 0.6
    beta[small] = rng.normal(size=int(small.sum()))
    beta[rng.random(rows) < 0.05] = 0.0
    beta[rng.random(rows) < 0.02] = -0.0
    start = rng.normal(size=n)
    start[::3] = -0.0
    return present, missing, flip, beta, start


def _numpy_sum(n, present, missing, flip, beta, start, idx):
    """The reference's loop (enet_predict.py:174-179) over rows idx[], fp64, in order."""
    acc = start.copy()
    dense_p = np.unpackbits(present, axis=1, bitorder="little")[:, :n]
    dense_m = np.unpackbits(missing, axis=1, bitorder="little")[:, :n].astype(bool) if missing is not None else None
    with np.errstate(all="ignore"):
        for j, r in enumerate(idx):
            k = dense_p[r].astype(np.float64)
            if dense_m is not None:
                k[dense_m[r]] = np.nan
            if flip[j]:
                k = np.array(~np.array(k, dtype=bool), dtype=np.int64)
            acc += k * beta[j]
    return acc


def _same_bits(a, b):
    nan = np.isnan(a)
    assert (nan == np.isnan(b)).all(), "NaN positions differ"
    assert (a[~nan].view(np.uint64) == b[~nan].view(np.uint64)).all(), "bit patterns differ"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 5000])
def test_predictor_is_the_numpy_loop_bit_for_bit(n):
    from pyseer_amd.enet import EnetPredictor
    from pyseer_amd.engine import Engine
    n_eng = max(n, 2)                                                          # (sh_create takes two samples at least: the case N = 1 runs as N = 2)
    rows = 9000 if n <= 1000 else 6000
    present, missing, flip_all, beta_all, start = _case(n_eng, rows, 1000 + n)
    rng = np.random.default_rng(n)
    subset = np.sort(rng.choice(rows, size=rows * 2 // 3, replace=False))      # a strict subset of the block, in block order
    engine = Engine(n_eng, device=0)
    try:
        for with_missing in (True, False):
            miss = missing if with_missing else None
            for idx in (np.arange(rows), subset):
                beta, flip = beta_all[idx], flip_all[idx]
                want = _numpy_sum(n_eng, present, miss, flip, beta, start, idx)
                for step in (None, 1, 7, 4096):
                    if step == 1 and idx.size > 2000:
                        cut = 2000                                                 # (one row a call over the first rows, the rest in one)
                        bounds = list(range(0, cut)) + [cut, idx.size]
                    else:
                        bounds = list(range(0, idx.size, step or idx.size)) + [idx.size]
                    pr = EnetPredictor(engine, start)
                    for a, b in zip(bounds[:-1], bounds[1:]):
                        pr.add(present, idx[a:b], beta[a:b], flip[a:b], missing=miss)
                    _same_bits(pr.finish(), want)
    finally:
        engine.close()


def test_predictor_refuses_bad_shapes():
    from pyseer_amd.enet import EnetPredictor
    from pyseer_amd.engine import Engine
    engine = Engine(100, device=0)
    try:
        pr = EnetPredictor(engine, np.zeros(100))
        block = np.zeros((4, 16), dtype=np.uint8)
        with pytest.raises(ValueError):
            pr.add(block, [4], [1.0], [0])
        with pytest.raises(ValueError):
            pr.add(block, [-1], [1.0], [0])
        with pytest.raises(ValueError):
            pr.add(np.zeros((4, 8), dtype=np.uint8), [0], [1.0], [0])
        with pytest.raises(ValueError):
            pr.add(block, [0, 1], [1.0], [0, 0])
        assert (pr.finish() == 0).all()
        with pytest.raises(ValueError):
            EnetPredictor(engine, np.zeros(99))
    finally:
        engine.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
def _kmer_columns(names, samples):
    """{name: 0/1 vector over samples} of the lines of kmers.gz named in `names` (first line of a name)."""
    pos = {s: i for i, s in enumerate(samples)}
    cols = {}
    with gzip.open(os.path.join(CLI, "kmers.gz"), "rt") as fh:
        for line in fh:
            name = line.split()[0]
            if name in names and name not in cols:
                k = np.zeros(len(samples))
                for x in line.rstrip().split("|")[1].split():
                    s = x.split(":")[0]
                    if s in pos:
                        k[pos[s]] = 1.0
                cols[name] = k
    return cols


def test_train_save_predict(tmp_path):
    from pyseer_amd.enet import read_model
    from pyseer_amd.input import load_covariates, load_phenotypes
    import pandas as pd
    samples = _samples50()
    model_path, pred_path = str(tmp_path / "m.txt"), str(tmp_path / "p.tsv")
    out, err = run("pyseer_amd", ["--kmers", "kmers.gz", "--phenotypes", "subset.pheno", "--phenotype-column", "continuous", "--continuous", "--min-af", "0.05",
                                  "--max-af", "0.95", "--wg", "enet", "--covariates", "covariates.txt", "--use-covariates", "2q",
                                  "--save-enet-model", model_path, "--save-predictions", pred_path])
    assert ("Saved enet model as " + model_path + "\n") in err
    model, continuous = read_model(model_path)
    assert continuous and list(model)[0] == "intercept" and model["intercept"][0] == 1.0
    printed = [line.split("\t") for line in out.split("\n")[1:] if line]
    variants = [k for k in model if k not in ("intercept", "quantitative")]
    assert variants == [f[0] for f in printed], "the model's variants are the printed rows, in their order"
    for f in printed:                                                           # (the rows print %.2E: the model keeps every digit of the same numbers)
        assert "%.2E" % model[f[0]][0] == f[1] and "%.2E" % model[f[0]][1] == f[4]
    link_out, _ = predict([model_path, "samples50.txt", "--kmers", "kmers.gz", "--covariates", "covariates.txt", "--use-covariates", "2q"])
    link = np.array([float(line.split("\t")[1]) for line in link_out.split("\n")[1:] if line])
    # ---- the same terms in numpy
    cols = _kmer_columns(set(variants), samples)
    p = load_phenotypes(os.path.join(CLI, "subset.pheno"), "continuous")
    cov = load_covariates(os.path.join(CLI, "covariates.txt"), ["2q"], pd.DataFrame(index=samples))
    x_cov = cov["quantitative"].values.astype(float)
    terms = [np.full(len(samples), model["intercept"][1])]
    if "quantitative" in model:
        assert model["quantitative"][0] == float(np.mean(x_cov))
        terms.append(x_cov * model["quantitative"][1])
    coded = {}
    for v in variants:
        af, beta = model[v]
        coded[v] = 1.0 - cols[v] if af > 0.5 else cols[v]
        assert af == cols[v].sum() / len(samples)
        terms.append(coded[v] * beta)
    terms = np.array(terms)
    S = len(model)
    bound = (S + 2) * 2.0 ** -52 * np.abs(terms).sum(axis=0)
    recomputed = terms.sum(axis=0)
    print("largest |link - numpy| / bound:", float(np.max(np.abs(link - recomputed) / bound)))
    assert (np.abs(link - recomputed) <= bound).all()
    # ---- against the fit's own predictions: eta on standardised columns against the model on the original scale, two algebraic forms;
    # numpy evaluates both from the same slopes, means and deviations, and their largest difference d_np is the yardstick
    X = np.array(([x_cov] if "quantitative" in model else []) + [coded[v] for v in variants])
    b = np.array(([model["quantitative"][1]] if "quantitative" in model else []) + [model[v][1] for v in variants])
    m = X.mean(axis=1)
    sd = np.sqrt(((X - m[:, None]) ** 2).mean(axis=1))
    original = model["intercept"][1] + (b[:, None] * X).sum(axis=0)
    standardised = (model["intercept"][1] + (b * m).sum()) + ((b * sd)[:, None] * ((X - m[:, None]) / sd[:, None])).sum(axis=0)
    d_np = float(np.max(np.abs(original - standardised)))
    print("d_np:", d_np)
    saved = pd.read_csv(pred_path, sep="\t", index_col=0)
    assert list(saved.index.astype(str)) == samples
    diff = np.abs(link - saved["predicted_value"].values.astype(float))
    print("largest |link - predicted_value|:", float(diff.max()))
    assert (diff <= 4 * d_np + bound).all()
    assert (saved["true_value"].values.astype(float) == p.loc[samples].values.astype(float)).all()


@pytest.mark.parametrize("case", ["kmers_binary", "kmers_continuous"])
@pytest.mark.parametrize("lineages", [False, True])
def test_true_values_summary(case, lineages, tmp_path):
    from pyseer_amd.input import load_lineage
    import pandas as pd
    samples = _samples50()
    continuous = CASES[case]["continuous"]
    column = "continuous" if continuous else "binary"
    truth = str(tmp_path / "truth.pheno")
    left_out = samples[7]
    with open(os.path.join(CLI, "subset.pheno")) as fh, open(truth, "w") as dst:
        for line in fh:
            if line.split("\t")[0] != left_out:                                 # one sample has no true value
                dst.write(line)
    args = [os.path.join(GOLD, case + ".model"), "samples50.txt", "--kmers", "kmers.gz", "--true-values", truth]
    # (load_phenotypes(file, None) takes the LAST column, as the reference does: the fixture's is `binary`)
    if continuous:
        with open(truth) as fh:
            lines = [line.rstrip("\n").split("\t") for line in fh]
        with open(truth, "w") as dst:
            for f in lines:
                dst.write("\t".join([f[0], f[2], f[1]]) + "\n")
    out, err = predict(args + (["--lineage-clusters", "clusters50.txt"] if lineages else []))
    assert out == golden(case)[0]
    rows = [line.split("\t") for line in out.split("\n")[1:] if line]
    pred = np.array([float(f[1]) for f in rows])                                # class (binary) or link (continuous)
    y = pd.read_csv(truth, sep="\t", index_col=0)
    y.index = y.index.astype(str)
    have = [i for i, s in enumerate(samples) if s in y.index]
    assert len(have) == 49
    y_true, y_pred = y.loc[[samples[i] for i in have]][column].values.astype(float), pred[have]

    def r2(t, q):
        return 1.0 - np.sum((t - q) ** 2) / np.sum((t - np.mean(t)) ** 2)
    want = ["Overall prediction accuracy", "R2: " + str(r2(y_true, y_pred))]
    if not continuous:
        want += ["tn: %d" % np.sum((y_true == 0) & (y_pred == 0)), "fp: %d" % np.sum((y_true == 0) & (y_pred == 1)),
                 "fn: %d" % np.sum((y_true == 1) & (y_pred == 0)), "tp: %d" % np.sum((y_true == 1) & (y_pred == 1))]
    if lineages:
        mat, labels = load_lineage(os.path.join(CLI, "clusters50.txt"), pd.DataFrame(index=samples))
        fold = np.where(mat == 1)[1][have]
        want += ["Predictions within each lineage", "\t".join(["Lineage", "Size", "R2"] + ([] if continuous else ["TP", "TN", "FP", "FN"]))]
        for f, label in enumerate(labels):
            t, q = y_true[fold == f], y_pred[fold == f]
            if t.size == 0:
                continue
            line = [label, str(t.size), "%.3f" % (np.nan if np.all(t == t[0]) else r2(t, q))]
            if not continuous:
                line += [str(int(np.sum((t == 1) & (q == 1)))), str(int(np.sum((t == 0) & (q == 0)))), str(int(np.sum((t == 0) & (q == 1)))),
                         str(int(np.sum((t == 1) & (q == 0))))]
            want.append("\t".join(line))
    tail = err[err.index("Overall prediction accuracy"):]
    assert tail == "\n".join(want) + "\n"
    assert without_meter(err[:err.index("Overall prediction accuracy")]) == without_meter(golden(case)[1])
