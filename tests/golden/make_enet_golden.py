"""Yardsticks of the whole-genome elastic net, written to tests/golden/enet/.

  reference   (the reference's interpreter, glmnet stubbed):
              PYTHONPATH=_harness:_harness/stubs:<reference> python3.9 -W ignore make_enet_golden.py reference
              load_all_vars (pyseer/enet.py:33) and correlation_filter (:379) of the reference itself on the k-mer and Rtab
              fixtures of tests/golden/cli with the binary and the continuous phenotype: the matrix as packed rows,
              var_indices, loaded, the correlations and the kept indices at quantiles 0.25 and 0.5 -> ref_<input>_<phenotype>.npz
  solver      (any interpreter with numpy and scikit-learn; no reference needed):   python make_enet_golden.py solver [case ...]
              the reference cannot supply the solver (glmnet is not installed), so the yardstick is tests/_enet_ref.py, checked
              HERE against scikit-learn before anything is written: enet_path (gaussian; agreement asserted at 1e-10) and
              LogisticRegression(saga) within 1e-5 with the numpy solution's own KKT residual below 1e-12 as the certificate.
              Per case -> solver_<case>.npz: the lambda sequence, the optimum (threshold 1e-26) at six path points, its
              cross-validation figures, and the bounds MEASURED from the numpy solver stopped at glmnet's 1e-7 and at 1e-12
              (largest KKT residual, distance from the optimum, cvm / cvsd discrepancy; the tests double them).
The matrices are not committed: make_case(seed, ...) of tests/_enet_ref.py rebuilds them in the test."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "enet")
CLI = os.path.join(HERE, "cli")

# name: make_case arguments, family, alpha, n_lambda (the numpy solver is a Python loop: the large shapes take a short path).
# The P = 20 000 cases keep a FINE path (and few folds instead): what they are for is the strong rule and the KKT growth over a matrix
# much wider than the active set, and on a coarse path the strong rule admits every column (alpha (2 lambda_l - lambda_(l-1)) < 0 once
# the step is below 1/2), which also makes the dense numpy solver build a 20 000 x 20 000 Gram matrix.
CASES = {
    "g_n200_p500_a0069": dict(seed=101, N=200, P=500, continuous=True, n_cov=0, n_dup=50, reweight=True, n_folds=5, alpha=0.0069, n_lambda=100),
    "g_n200_p500_a5_cov": dict(seed=102, N=200, P=500, continuous=True, n_cov=3, n_dup=50, reweight=False, n_folds=5, alpha=0.5, n_lambda=100),
    "b_n200_p500_a0069_cov": dict(seed=103, N=200, P=500, continuous=False, n_cov=3, n_dup=50, reweight=True, n_folds=5, alpha=0.0069, n_lambda=40),
    "b_n200_p500_a5_const": dict(seed=104, N=200, P=500, continuous=False, n_cov=0, n_dup=50, reweight=False, n_folds=5, alpha=0.5, n_lambda=40,
                                 const_in_fold=True),
    "g_n200_p500_a1": dict(seed=105, N=200, P=500, continuous=True, n_cov=0, n_dup=0, reweight=False, n_folds=5, alpha=1.0, n_lambda=30),
    "g_n1000_p500_a5_const": dict(seed=106, N=1000, P=500, continuous=True, n_cov=3, n_dup=50, reweight=True, n_folds=4, alpha=0.5, n_lambda=25,
                                  const_in_fold=True),
    "b_n1000_p500_a0069": dict(seed=107, N=1000, P=500, continuous=False, n_cov=0, n_dup=50, reweight=False, n_folds=4, alpha=0.0069, n_lambda=20),
    "g_n5000_p500_a0069": dict(seed=110, N=5000, P=500, continuous=True, n_cov=0, n_dup=50, reweight=True, n_folds=3, alpha=0.0069, n_lambda=12),
    "b_n5000_p500_a5_cov": dict(seed=111, N=5000, P=500, continuous=False, n_cov=3, n_dup=50, reweight=False, n_folds=3, alpha=0.5, n_lambda=12),
    "b_n200_p20000_a5": dict(seed=118, N=200, P=20000, continuous=False, n_cov=0, n_dup=200, reweight=True, n_folds=3, alpha=0.5, n_lambda=100),
    "g_n1000_p20000_a5": dict(seed=109, N=1000, P=20000, continuous=True, n_cov=3, n_dup=200, reweight=False, n_folds=2, alpha=0.5, n_lambda=50),
    "g_n1000_p500_a0069_plain": dict(seed=119, N=1000, P=500, continuous=True, n_cov=0, n_dup=50, reweight=False, n_folds=4, alpha=0.0069, n_lambda=12),
    "b_n5000_p500_a0069": dict(seed=120, N=5000, P=500, continuous=False, n_cov=0, n_dup=50, reweight=False, n_folds=3, alpha=0.0069, n_lambda=8),
    # coarse paths over well-determined problems: the argmin of cvm is decided at glmnet's own threshold too
    "g_n1000_p200_a5_short": dict(seed=115, N=1000, P=200, continuous=True, n_cov=0, n_dup=20, reweight=False, n_folds=5, alpha=0.5, n_lambda=4),
    "b_n1000_p1200_a5_short": dict(seed=116, N=1000, P=1200, continuous=False, n_cov=0, n_dup=20, reweight=True, n_folds=5, alpha=0.5, n_lambda=4),
    "b_n2000_p200_a5_short": dict(seed=117, N=2000, P=200, continuous=False, n_cov=0, n_dup=20, reweight=False, n_folds=5, alpha=0.5, n_lambda=3),
    # the per-sample state no longer fits the LDS of a CU: the same bounds as the neighbours above
    "g_n8192_p500_a5": dict(seed=113, N=8192, P=500, continuous=True, n_cov=0, n_dup=50, reweight=True, n_folds=3, alpha=0.5, n_lambda=10),
    "b_n8192_p500_a0069": dict(seed=114, N=8192, P=500, continuous=False, n_cov=0, n_dup=50, reweight=False, n_folds=3, alpha=0.0069, n_lambda=8),
}
MAKE_KEYS = ("seed", "N", "P", "continuous", "n_cov", "n_dup", "reweight", "n_folds", "const_in_fold")


def case_of(name):
    import _enet_ref as R
    spec = CASES[name]
    return R.make_case(**{k: spec[k] for k in MAKE_KEYS if k in spec}), spec


# ------------------------------------------------------------------------------------------------------------------
def check_against_sklearn(R):
    """The numpy solver against scikit-learn, before anything is written; scikit-learn's own figures are kept (sklearn_figures.npz) so that
    tests/test_enet_cpu.py holds the numpy solver to them where scikit-learn is not installed."""
    from sklearn.linear_model import enet_path, LogisticRegression
    keep = {}
    for alpha in (0.0069, 0.5):
        c = R.make_case(1, 200, 300, True, n_dup=30, reweight=True)
        pr = R.problems(c, R.GAUSSIAN, alpha)[0]
        lam = R.lambda_sequence(pr, 10)
        opt = R.fit_path(pr, lam, 1e-26, starts=R.fit_path(pr, lam, 1e-12))
        Xs, sw = pr.cols(np.arange(pr.PT)), np.sqrt(200 * pr.w)
        _, coefs, _ = enet_path(Xs * sw[:, None], (c["y"] - pr.mu0) * sw, l1_ratio=alpha, alphas=lam, tol=1e-14, max_iter=10 ** 7)
        d = max(np.abs(coefs[:, l] - opt[l][1]).max() for l in range(10))
        print("sklearn enet_path, gaussian alpha %g: %.2e" % (alpha, d))
        assert d < 1e-10, d
        keep["gaussian_coefs_%g" % alpha], keep["gaussian_lambdas_%g" % alpha] = coefs, lam
    c = R.make_case(2, 200, 40, False, reweight=True)
    pr = R.problems(c, R.BINOMIAL, 0.5)[0]
    lam = R.lambda_sequence(pr, 10, ratio=1e-2)
    opt = R.fit_path(pr, lam, 1e-26, starts=R.fit_path(pr, lam, 1e-12))
    Xs = pr.cols(np.arange(pr.PT))
    for l in (2, 5, 9):
        kkt = R.kkt_residual(pr, lam[l], *opt[l])[0]
        lr = LogisticRegression(penalty="elasticnet", solver="saga", l1_ratio=0.5, C=1.0 / lam[l], tol=1e-12, max_iter=2000000)
        lr.fit(Xs, c["y"], sample_weight=pr.w)
        d = max(np.abs(lr.coef_[0] - opt[l][1]).max(), abs(lr.intercept_[0] - opt[l][0]))
        print("sklearn saga, binomial lambda %d: %.2e, numpy KKT residual %.1e" % (l, d, kkt))
        assert d < 1e-5 and kkt < 1e-12, (d, kkt)
        keep["binomial_coef_%d" % l], keep["binomial_b0_%d" % l] = lr.coef_[0], lr.intercept_[0]
    keep["binomial_lambdas"] = lam
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "sklearn_figures.npz"), **keep)


def pack_bool(a):
    return np.packbits(np.asarray(a, bool))


def solve_case(name):
    import _enet_ref as R
    case, spec = case_of(name)
    family = R.GAUSSIAN if spec["continuous"] else R.BINOMIAL
    alpha, n_cov = spec["alpha"], spec["n_cov"]
    probs = R.problems(case, family, alpha)
    lam = R.lambda_sequence(probs[0], spec["n_lambda"])
    # the full fit ends the path (glmnet's rule); every threshold must end it at the same place or the case is no yardstick
    runs = {}
    for thr in (1e-7, 1e-12):
        full = R.fit_path(probs[0], lam, thr, always_active=n_cov, stop_early=True)
        runs[thr] = [full]
    L = len(runs[1e-12][0])
    assert len(runs[1e-7][0]) == L, "the path ends at another lambda at 1e-7 (%d) than at 1e-12 (%d)" % (len(runs[1e-7][0]), L)
    dr = [1 - probs[0].deviance(*s) / probs[0].nulldev for s in runs[1e-12][0]]
    for l in range(1, L):                                             # no stopping decision within 1e-6 of its limit
        assert abs(dr[l] - 0.999) > 1e-6
        if l + 1 >= min(5, len(lam)):
            assert abs((dr[l] - dr[l - 1]) - 1e-5 * dr[l]) > 1e-7 * dr[l], (l, dr[l], dr[l - 1])
    lamL = lam[:L]
    for thr in (1e-7, 1e-12):
        for f in range(1, len(probs)):
            runs[thr].append(R.fit_path(probs[f], lamL, thr, always_active=n_cov))
    opt = [R.fit_path(probs[f], lamL, 1e-26, starts=runs[1e-12][f], always_active=n_cov) for f in range(len(probs))]
    kkt_opt = max(R.kkt_residual(probs[f], lamL[l], *opt[f][l])[0] for f in range(len(probs)) for l in range(L))
    assert kkt_opt < 1e-11, kkt_opt
    cvm_o, cvsd_o, _ = R.cv_figures(case, probs, opt, family)
    i_min = int(np.argmin(cvm_o))
    out = dict(spec=json.dumps(spec), lambdas=lam, L=L, cvm_opt=cvm_o, cvsd_opt=cvsd_o, i_min_opt=i_min, kkt_opt=kkt_opt)
    for thr, tag in ((1e-7, "d"), (1e-12, "t")):
        tau = max(R.kkt_residual(probs[f], lamL[l], *runs[thr][f][l])[0] for f in range(len(probs)) for l in range(L))
        delta = 0.0
        for f in range(len(probs)):
            for l in range(L):
                a0, a = R.to_original(probs[f], *runs[thr][f][l])
                o0, o = R.to_original(probs[f], *opt[f][l])
                delta = max(delta, abs(a0 - o0), float(np.abs(a - o).max()))
        cvm, cvsd, _ = R.cv_figures(case, probs, runs[thr], family)
        dc, ds = float(np.abs(cvm - cvm_o).max()), float(np.abs(cvsd - cvsd_o).max())
        gap = float(np.partition(cvm_o, 1)[1] - cvm_o[i_min]) if L > 1 else np.inf
        out.update({"tau_" + tag: tau, "delta_" + tag: delta, "cvm_bound_" + tag: dc, "cvsd_bound_" + tag: ds,
                    "imin_decided_" + tag: bool(gap >= (100 if tag == "d" else 4) * dc), "i_min_" + tag: int(np.argmin(cvm))})
        print("%s thr %g: tau %.2e delta %.2e cvm %.2e cvsd %.2e gap %.2e i_min %d/%d" % (name, thr, tau, delta, dc, ds, gap, int(np.argmin(cvm)), i_min))
    assert out["i_min_t"] == i_min, "the tight numpy run finds another lambda_min than the optimum: no yardstick"
    # six path points of the full fit: lambda_min and five spread over the path
    pts = sorted(set([i_min] + [int(round(x)) for x in np.linspace(0, L - 1, 6)]))[:7]
    out["points"] = np.array(pts)
    tau_t = 2 * out["tau_t"]
    n_dropped = n_selected = 0
    for k, l in enumerate(pts):
        o0, o = R.to_original(probs[0], *opt[0][l])
        nz = np.nonzero(o)[0]
        out["opt_b0_%d" % k], out["opt_idx_%d" % k], out["opt_val_%d" % k] = o0, nz.astype(np.int32), o[nz]
        # the tight solution's selected set, and the columns no solver at this threshold decides: |g_j| within tau of alpha lambda,
        # g_j taken with the column's own term out (u_j = g_j + xv_j b_j, what a coordinate step thresholds): for an unselected column
        # that is its gradient; for a selected one the plain gradient sits at alpha lambda + (1 - alpha) lambda |b_j| by the optimality
        # condition itself -- exactly alpha lambda at alpha = 1 -- and says nothing about how firmly the column is in
        tb = runs[1e-12][0][l][1]
        g = R.partial_gradient(probs[0], *runs[1e-12][0][l])
        und = (np.abs(np.abs(g) - alpha * lamL[l]) <= tau_t) & (probs[0].sinv > 0)
        und[:n_cov] = False
        sel = tb != 0
        n_selected += int(sel[n_cov:].sum())
        n_dropped += int((und & (sel | (opt[0][l][1] != 0))).sum())
        assert ((sel != (opt[0][l][1] != 0)) <= und).all(), "the tight numpy run itself selects another set than the optimum at lambda %d" % l
        out["sel_%d" % k], out["und_%d" % k] = pack_bool(sel), pack_bool(und)
    assert n_dropped <= 0.01 * n_selected, "more than 1 %% of the selected variants of this case are undecidable (%d of %d)" % (n_dropped, n_selected)
    out["n_dropped"], out["n_selected"] = n_dropped, n_selected
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "solver_%s.npz" % name), **out)
    return out


# ------------------------------------------------------------------------------------------------------------------
def reference_part():
    import shim  # noqa: F401
    import gzip
    from pyseer.input import load_phenotypes, open_variant_file
    from pyseer.enet import load_all_vars, correlation_filter
    os.makedirs(OUT, exist_ok=True)
    for tag, var_type, path in (("kmers", "kmers", "kmers.gz"), ("rtab", "Rtab", "kmers120.Rtab")):
        for col in ("binary", "continuous"):
            p = load_phenotypes(os.path.join(CLI, "subset.pheno"), col)
            infile, sample_order = open_variant_file(var_type, os.path.join(CLI, path), None, [], False)
            variants, var_indices, loaded = load_all_vars(var_type, p, False, [], infile, set(p.index), sample_order, 0.05, 0.95, 0.05, False)
            dense = np.asarray(variants.todense()).astype(np.uint8)
            b = p.values - np.mean(p.values)
            sb2 = np.sum(b ** 2)
            cors = []
            for r in range(dense.shape[0]):                           # correlation_filter's own arithmetic, kept value by value (:409-418)
                k = variants.getrow(r)
                km = k.mean()
                if km == 0:
                    cors.append(np.nan)
                    continue
                ab = k.dot(b) - np.sum(km * b)
                sa2 = k.dot(k.transpose()).data[0] - 2 * km * k.sum() + km ** 2 * variants.shape[1]
                cors.append(float(np.abs(ab / np.sqrt(sa2 * sb2))[0]))
            cors = np.array(cors)
            kept = {q: correlation_filter(p, variants, q) for q in (0.25, 0.5)}
            for q in kept:                                            # set equality must be decided by the data, not by rounding
                cut = np.percentile(cors, q * 100)
                assert (np.nonzero(cors > cut)[0] == kept[q]).all()
                near = np.abs(cors - cut) <= 1e-9
                assert not near.any() or np.all(cors[near] == cut), "a correlation lies within 1e-9 of the cut without being it"
            rows = np.zeros((dense.shape[0], ((dense.shape[1] + 63) // 64) * 8), np.uint8)
            pk = np.packbits(dense.astype(bool), axis=1, bitorder="little")
            rows[:, :pk.shape[1]] = pk
            np.savez_compressed(os.path.join(OUT, "ref_%s_%s.npz" % (tag, col)), rows=rows, n_samples=dense.shape[1], y=p.values.astype(float),
                                samples=np.array(list(p.index)), var_indices=np.array(var_indices), loaded=loaded, cor=cors,
                                kept25=kept[0.25], kept50=kept[0.5], min_af=0.05, max_af=0.95, max_missing=0.05)
            print(tag, col, dense.shape, "loaded", loaded, "kept", len(kept[0.25]), len(kept[0.5]), "nan", int(np.isnan(cors).sum()))


def fixed_betas(n_cov, var_indices):
    """The hand-made slope vector of the fixed-beta rows: intercept, covariates, then every seventh kept variant non-zero."""
    j = np.arange(len(var_indices))
    b = np.where(j % 7 == 0, ((j * 37) % 11 - 5) / 10.0 + 0.05, 0.0)
    return np.concatenate([[0.25], np.zeros(n_cov), b])


def reference_rows():
    """find_enet_selected + format_output of the reference for fixed_betas (k-mers, binary, quantile 0.25): without distances, with
    --distances (the fixed-effects p-value), and with --lineage-clusters --lineage; write_predictions / write_lineage_predictions text
    for fixed predictions.  -> ref_rows.json"""
    import shim  # noqa: F401
    import contextlib
    import io
    import tempfile
    import pandas as pd
    from pyseer.input import load_phenotypes, open_variant_file, load_structure, load_lineage
    from pyseer.enet import load_all_vars, correlation_filter, find_enet_selected, write_predictions, write_lineage_predictions
    from pyseer.model import fit_null
    from pyseer.utils import format_output
    out = {}
    cov = pd.DataFrame([])
    for tag in ("plain", "distances", "lineage"):
        p = load_phenotypes(os.path.join(CLI, "subset.pheno"), "binary")
        m, fit_seer, lin, lin_dict = np.empty((0, 0)), None, None, None
        if tag == "distances":
            md = load_structure(os.path.join(CLI, "distances50.tsv"), p, 10, "classic", 1, None)
            p = p.loc[p.index.intersection(md.index)]
            m = md.loc[p.index].values[:, :10]
            fit_seer = (m, fit_null(p.values, m, cov, False).llf, fit_null(p.values, m, cov, False, True))    # __main__.py:449-450
        if tag == "lineage":
            lin, lin_dict = load_lineage(os.path.join(CLI, "clusters50.txt"), p)
            wald = {}
            for name, design in zip(lin_dict, lin.T):
                lf = fit_null(p.values, design.reshape(-1, 1), cov, False)
                wald[name] = np.absolute(lf.params[1]) / lf.bse[1]
            drop = lin_dict.index(min(wald.items(), key=lambda kv: kv[1])[0])
            lin = np.delete(lin, drop, 1)
            del lin_dict[drop]
        infile, so = open_variant_file("kmers", os.path.join(CLI, "kmers.gz"), None, [], False)
        variants, var_indices, loaded = load_all_vars("kmers", p, False, [], infile, set(p.index), so, 0.05, 0.95, 0.05, False)
        keep = correlation_filter(p, variants, 0.25)
        var_indices = np.array(var_indices)[keep]
        betas = fixed_betas(0, var_indices)
        infile, so = open_variant_file("kmers", os.path.join(CLI, "kmers.gz"), None, [], False)
        rows = []
        for x in find_enet_selected(betas, var_indices, p, cov, "kmers", fit_seer, False, [], infile, set(p.index), so, False,
                                    tag == "lineage", lin, False):
            x = x._replace(notes=sorted(x.notes))
            rows.append(format_output(x, lin_dict, "enet", tag == "plain"))
        out[tag] = rows
        print(tag, len(rows), rows[:2])
    p = load_phenotypes(os.path.join(CLI, "subset.pheno"), "binary")
    lin, lin_dict = load_lineage(os.path.join(CLI, "clusters50.txt"), p)
    fold_ids = np.where(lin == 1)[1]
    rng = np.random.default_rng(4)
    preds = np.where(rng.random(len(p)) < 0.8, p.values, 1 - p.values).astype(float).reshape(-1, 1)
    out["fixed_predictions"] = preds.reshape(-1).tolist()
    with tempfile.TemporaryDirectory() as d:
        write_predictions(p.index, p.values, preds, fold_ids, lin_dict, os.path.join(d, "a.tsv"))
        out["write_predictions_lineage"] = open(os.path.join(d, "a.tsv")).read()
        write_predictions(p.index, p.values, preds, None, None, os.path.join(d, "b.tsv"))
        out["write_predictions_plain"] = open(os.path.join(d, "b.tsv")).read()
    buf = io.StringIO()
    with contextlib.redirect_stderr(buf):
        write_lineage_predictions(p.values, preds, fold_ids, lin_dict, False)
    out["write_lineage_predictions"] = buf.getvalue()
    json.dump(out, open(os.path.join(OUT, "ref_rows.json"), "w"), indent=0)


def reference_missing():
    """load_all_vars / correlation_filter of the reference on an Rtab with missing calls (cli/kmers120.Rtab with a seeded 4 % of its calls
    turned into '.', written next to the goldens): the missing-call side of the minor-allele coding.  (The harness has no pysam, so the
    reference cannot read the VCF fixtures itself.)  -> missing.Rtab, ref_missing_<phenotype>.npz"""
    import shim  # noqa: F401
    from pyseer.input import load_phenotypes, open_variant_file
    from pyseer.enet import load_all_vars, correlation_filter
    rng = np.random.default_rng(9)
    lines = open(os.path.join(CLI, "kmers120.Rtab")).read().split("\n")
    with open(os.path.join(OUT, "missing.Rtab"), "w") as fh:
        fh.write(lines[0] + "\n")
        for line in lines[1:]:
            if line:
                f = line.split("\t")
                fh.write("\t".join([f[0]] + ["." if rng.random() < 0.04 else c for c in f[1:]]) + "\n")
    for col in ("binary", "continuous"):
        p = load_phenotypes(os.path.join(CLI, "subset.pheno"), col)
        infile, so = open_variant_file("Rtab", os.path.join(OUT, "missing.Rtab"), None, [], False)
        variants, var_indices, loaded = load_all_vars("Rtab", p, False, [], infile, set(p.index), so, 0.05, 0.95, 0.2, False)
        dense = np.asarray(variants.todense()).astype(np.uint8)
        kept = {q: correlation_filter(p, variants, q) for q in (0.25, 0.5)}
        rows = np.zeros((dense.shape[0], ((dense.shape[1] + 63) // 64) * 8), np.uint8)
        pk = np.packbits(dense.astype(bool), axis=1, bitorder="little")
        rows[:, :pk.shape[1]] = pk
        np.savez_compressed(os.path.join(OUT, "ref_missing_%s.npz" % col), rows=rows, n_samples=dense.shape[1], y=p.values.astype(float),
                            samples=np.array(list(p.index)), var_indices=np.array(var_indices), loaded=loaded,
                            kept25=kept[0.25], kept50=kept[0.5], min_af=0.05, max_af=0.95, max_missing=0.2)
        print("missing", col, dense.shape, "loaded", loaded, "kept", len(kept[0.25]), len(kept[0.5]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "reference":
        reference_part()
        reference_rows()
        reference_missing()
    elif len(sys.argv) > 1 and sys.argv[1] in ("rows", "missing"):
        reference_rows() if sys.argv[1] == "rows" else reference_missing()
    else:
        sys.path.insert(0, os.path.dirname(HERE))
        import _enet_ref as R
        names = sys.argv[2:] or list(CASES)
        check_against_sklearn(R)
        for n in [x for x in names if x != "sklearn"]:
            solve_case(n)
        # at least one binary and one continuous committed case decide lambda_min at the default threshold as well
        decided = {True: False, False: False}
        for n in CASES:
            f = os.path.join(OUT, "solver_%s.npz" % n)
            if os.path.exists(f):
                decided[CASES[n]["continuous"]] |= bool(np.load(f)["imin_decided_d"])
        assert decided[True] and decided[False], "no committed case decides lambda_min at 1e-7: %r" % decided
