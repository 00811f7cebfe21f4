"""`python -m pyseer_amd --wg enet` end to end on the fixtures of tests/golden/cli.

Rows for a FIXED slope vector (injected through pyseer_amd.enet.TEST_BETAS, a test-only hook) are compared byte for byte with what the
reference's own find_enet_selected + format_output printed for that vector (tests/golden/enet/ref_rows.json, made by
tests/golden/make_enet_golden.py): everything but the solver.  For real fits the solver's part is held to the numpy yardstick
(tests/_enet_ref.py) run here on the reference's own matrix of the same input: the same variants selected, slopes within twice the
distance the numpy solver itself keeps from the optimum at the same threshold (plus half a unit of the printed '%.2E')."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _enet_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
GOLD = os.path.join(ROOT, "tests", "golden", "enet")
BASE = ["--phenotypes", "subset.pheno", "--min-af", "0.05", "--max-af", "0.95"]
KMERS = ["--kmers", "kmers.gz"] + BASE


def run(args, expect=0):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", "pyseer_amd"] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines(), r.stderr.decode()


def fixed_betas(n_cov, var_indices):
    j = np.arange(len(var_indices))
    return np.concatenate([[0.25], np.zeros(n_cov), np.where(j % 7 == 0, ((j * 37) % 11 - 5) / 10.0 + 0.05, 0.0)])


def run_in_process(args, capsys, monkeypatch):
    from pyseer_amd import enet
    from pyseer_amd.__main__ import main
    monkeypatch.chdir(CLI)
    monkeypatch.setattr(enet, "TEST_BETAS", fixed_betas)
    capsys.readouterr()
    main(args)
    cap = capsys.readouterr()
    return cap.out.splitlines(), cap.err


@pytest.mark.parametrize("tag,extra", [("plain", ["--print-samples"]), ("distances", ["--distances", "distances50.tsv"]),
                                       ("lineage", ["--lineage-clusters", "clusters50.txt", "--lineage"])])
def test_fixed_beta_rows_are_the_references(tag, extra, capsys, monkeypatch, tmp_path):
    want = json.load(open(os.path.join(GOLD, "ref_rows.json")))[tag]
    if tag == "lineage":
        extra = extra + ["--lineage-file", str(tmp_path / "lin.txt")]
    out, err = run_in_process(KMERS + ["--phenotype-column", "binary", "--wg", "enet"] + extra, capsys, monkeypatch)
    header = ['variant', 'af', 'filter-pvalue', 'lrt-pvalue', 'beta'] + (['lineage'] if tag == "lineage" else []) + \
        (['k-samples', 'nk-samples'] if tag == "plain" else []) + ['notes']
    assert out[0] == "\t".join(header)
    assert out[1:] == want
    assert "%d printed variants" % len(want) in err


def _yardstick(col, quantile, thresh, weights=None, folds=None):
    """The numpy solver on the reference's own matrix of kmers.gz: (names are not needed) slopes of the kept variants, in file order."""
    from pyseer_amd.enet import assign_folds
    g = np.load(os.path.join(GOLD, "ref_kmers_%s.npz" % col))
    n = int(g["n_samples"])
    K = np.unpackbits(g["rows"], axis=1, bitorder="little")[:, :n]
    keep = g["kept25"] if quantile == 0.25 else np.arange(K.shape[0])
    fold = assign_folds(n, 10, 1) if folds is None else folds
    case = dict(K=K[keep], y=g["y"], w=np.ones(n) if weights is None else weights, cov=np.zeros((n, 0)), fold=fold, n_folds=int(fold.max()) + 1)
    fam = R.GAUSSIAN if col == "continuous" else R.BINOMIAL
    probs = R.problems(case, fam, 0.0069)
    lam = R.lambda_sequence(probs[0], 100)
    runs = [R.fit_path(probs[0], lam, thresh, stop_early=True)]
    L = len(runs[0])
    runs += [R.fit_path(pr, lam[:L], thresh) for pr in probs[1:]]
    opt = [R.fit_path(pr, lam[:L], 1e-26, starts=runs[f]) for f, pr in enumerate(probs)]
    cvm, _, _ = R.cv_figures(case, probs, opt, fam)
    i_min = int(np.argmin(cvm))
    assert int(np.argmin(R.cv_figures(case, probs, runs, fam)[0])) == i_min, "the fixture does not decide lambda_min at this threshold"
    b_thr, b_opt = R.to_original(probs[0], *runs[0][i_min])[1], R.to_original(probs[0], *opt[0][i_min])[1]
    return b_opt, 2 * float(np.abs(b_thr - b_opt).max()), g


@pytest.mark.parametrize("col", ["binary", "continuous"])
def test_real_fit_selects_and_sizes_what_the_yardstick_does(col):
    b_opt, delta, g = _yardstick(col, 0.25, 1e-12)
    out, err = run(KMERS + ["--phenotype-column", col, "--wg", "enet", "--enet-thresh", "1e-12"])
    rows = [r.split("\t") for r in out[1:]]
    sel = np.nonzero(b_opt)[0]
    print("%s: %d selected, slopes allowed within %.3e" % (col, sel.size, delta))
    assert len(rows) == sel.size, "another number of variants is selected"
    for r, j in zip(rows, sel):
        assert abs(float(r[4]) - b_opt[j]) <= delta + 0.005 * 10 ** np.floor(np.log10(abs(b_opt[j]))) + 1e-300, (r[0], r[4], b_opt[j])
    assert "%d loaded variants" % int(g["loaded"]) in err and "%d tested variants" % g["kept25"].size in err
    assert "%d pre-filtered variants" % (int(g["loaded"]) - g["kept25"].size) in err
    assert "Best penalty (lambda) from cross-validation: " in err and "Best R^2 from cross-validation: " in err
    assert ("Best model deviance from cross-validation: " in err) == (col == "binary")
    # the other columns are what the per-variant path prints for these variants
    per, _ = run(KMERS + ["--phenotype-column", col, "--no-distances"])
    pv = {r.split("\t")[0]: r.split("\t") for r in per[1:]}
    for r in rows:
        assert r[1:3] == pv[r[0]][1:3], r[0]
        assert r[3] == ""                                             # no --distances: nan


def test_cor_filter_zero_keeps_every_variant_and_other_inputs_run(tmp_path):
    g = np.load(os.path.join(GOLD, "ref_kmers_binary.npz"))
    out, err = run(KMERS + ["--phenotype-column", "binary", "--wg", "enet", "--cor-filter", "0"])
    assert "%d tested variants" % g["rows"].shape[0] in err and "%d pre-filtered variants" % (int(g["loaded"]) - g["rows"].shape[0]) in err
    assert len(out) > 1
    g = np.load(os.path.join(GOLD, "ref_rtab_binary.npz"))
    out, err = run(["--pres", "kmers120.Rtab"] + BASE + ["--phenotype-column", "binary", "--wg", "enet"])
    assert "%d loaded variants" % int(g["loaded"]) in err and "%d tested variants" % g["kept25"].size in err and len(out) > 1
    out, err = run(["--vcf", os.path.join("..", "vcf", "variants50.vcf.gz")] + BASE + ["--phenotype-column", "binary", "--wg", "enet"])
    assert out[0].split("\t")[:5] == ['variant', 'af', 'filter-pvalue', 'lrt-pvalue', 'beta'] and len(out) > 1
    # --distances fills the lrt column from the fixed-effects fit; --save-predictions writes write_predictions' table
    pred = tmp_path / "pred.tsv"
    out, err = run(KMERS + ["--phenotype-column", "binary", "--wg", "enet", "--distances", "distances50.tsv", "--save-predictions", str(pred)])
    assert any(r.split("\t")[3] != "" for r in out[1:])
    lines = open(str(pred)).read().splitlines()
    assert lines[0] == "sample\ttrue_value\tpredicted_value" and len(lines) == 51


def test_clusters_with_reweighting(tmp_path):
    out, err = run(KMERS + ["--phenotype-column", "binary", "--wg", "enet", "--lineage-clusters", "clusters50.txt", "--sequence-reweighting"])
    assert out[0] == "\t".join(['variant', 'af', 'filter-pvalue', 'lrt-pvalue', 'beta', 'lineage', 'notes'])
    assert all(r.split("\t")[5] == "NA" for r in out[1:])
    assert "Predictions within each lineage\nLineage\tSize\tR2\tTP\tTN\tFP\tFN\n" in err
    sizes = dict(line.split("\t")[:2] for line in err.split("Lineage\tSize\tR2\tTP\tTN\tFP\tFN\n")[1].splitlines() if line.startswith("BAPS"))
    cl = [l.split()[1] for l in open(os.path.join(CLI, "clusters50.txt")).read().splitlines()]
    assert {k: int(v) for k, v in sizes.items()} == {c: cl.count(c) for c in set(cl)}


def test_prediction_texts_are_the_references(tmp_path):
    import io
    from pyseer_amd import enet
    want = json.load(open(os.path.join(GOLD, "ref_rows.json")))
    lines = want["write_predictions_lineage"].splitlines()[1:]
    samples = [l.split("\t")[0] for l in lines]
    labels = [l.split("\t")[1] for l in lines]
    fold = np.array([int(l.split("\t")[2]) for l in lines])
    lin_dict = [labels[list(fold).index(k)] for k in range(fold.max() + 1)]
    y = np.array([int(l.split("\t")[3]) for l in lines])
    preds = np.array(want["fixed_predictions"])
    enet.write_predictions(samples, y, preds, fold, lin_dict, str(tmp_path / "a.tsv"))
    assert open(str(tmp_path / "a.tsv")).read() == want["write_predictions_lineage"]
    enet.write_predictions(samples, y, preds, None, None, str(tmp_path / "b.tsv"))
    assert open(str(tmp_path / "b.tsv")).read() == want["write_predictions_plain"]
    buf = io.StringIO()
    enet.write_lineage_predictions(y.astype(float), preds, fold, lin_dict, False, buf)
    assert buf.getvalue() == want["write_lineage_predictions"]


@pytest.mark.parametrize("name", ["ref_missing_binary", "ref_missing_continuous"])
def test_load_all_vars_with_missing_calls_is_the_references(name):
    import pandas as pd
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import load_all_vars, correlation_cut
    from pyseer_amd.input import open_variant_file
    g = np.load(os.path.join(GOLD, name + ".npz"))
    p = pd.Series(g["y"], index=[str(s) for s in g["samples"]])
    infile, order = open_variant_file("Rtab", os.path.join(GOLD, "missing.Rtab"))
    e = Engine(len(p))
    M, var_indices, loaded = load_all_vars(e, "Rtab", p, False, None, infile, set(p.index), order, float(g["min_af"]), float(g["max_af"]),
                                           float(g["max_missing"]), False)
    assert loaded == int(g["loaded"]) and (np.array(var_indices) == g["var_indices"]).all()
    assert (M.get_rows(np.arange(M.rows)) == g["rows"]).all()
    cor = M.correlations(g["y"])
    for q, key in ((0.25, "kept25"), (0.5, "kept50")):
        assert (correlation_cut(cor, q) == g[key]).all()
    M.close()
    e.close()


def test_refusals():
    wg = KMERS + ["--wg", "enet"]
    _, err = run(wg + ["--lmm", "--similarity", "similarity50.tsv"], expect=1)
    assert err.endswith("Choose only one alternative model. Either --lmm, --wg or neither\n")
    for extra in (["--sequence-reweighting"], ["--sequence-reweighting", "--lineage-clusters", "clusters50.txt", "--lineage"]):
        _, err = run(wg + extra, expect=1)
        assert err.endswith("Using sequence reweighting requires clusters to weight with.\nProvide these with --lineage-clusters. Incompatible with --lineage.\n")
    _, err = run(wg + ["--output-patterns", "x.txt"], expect=1)
    assert err.endswith("Whole genome model does not produce patterns.\nRe-run without --output-patterns.\n")
    for extra, word in ((["--gpus", "2"], "--gpus"), (["--save-vars", "x"], "--save-vars"), (["--load-vars", "x"], "--load-vars"),
                        (["--save-model", "x"], "--save-model"), (["--alpha", "1.5"], "--alpha")):
        _, err = run(wg + extra, expect=1)
        assert word in err
    for model in ("rf", "blup"):
        _, err = run(KMERS + ["--wg", model], expect=1)
        assert model in err
    _, err = run(wg + ["--min-af", "0.6", "--max-af", "0.61"], expect=1)
    assert "No variants passed filters" in err
