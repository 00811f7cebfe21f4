"""The whole-genome elastic net on the device (sh_enet_*, pyseer_amd/enet.py) against committed yardsticks only:
tests/golden/enet/ref_*.npz from the reference's own load_all_vars / correlation_filter, and solver_*.npz from the numpy
solver of tests/_enet_ref.py (checked against scikit-learn when the files were made, tests/golden/make_enet_golden.py).

The contract is the optimum of the stated objective, not a solver's trajectory, so the solver is held by the KKT conditions,
computed HERE in numpy fp64 from the returned slopes and the unpacked matrix, at two thresholds: 1e-12 (tight) and glmnet's
1e-7 (default).  tau (KKT residual), delta (distance from the optimum) and the cvm / cvsd bounds are not chosen: the golden
file holds what the numpy solver itself leaves when it stops by the same rule at the same threshold, and the test allows
twice that (same rule, other summation order: a factor, not an order of magnitude)."""
import json
import os

import numpy as np
import pytest

import _enet_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enet")
CASES = ["g_n200_p500_a0069", "g_n200_p500_a5_cov", "b_n200_p500_a0069_cov", "b_n200_p500_a5_const", "g_n200_p500_a1",
         "g_n1000_p500_a5_const", "b_n1000_p500_a0069", "g_n1000_p200_a5_short", "b_n1000_p1200_a5_short", "b_n2000_p200_a5_short",
         "g_n1000_p500_a0069_plain", "b_n200_p20000_a5", "g_n1000_p20000_a5", "b_n5000_p500_a0069", "g_n5000_p500_a0069", "b_n5000_p500_a5_cov", "g_n8192_p500_a5", "b_n8192_p500_a0069"]
MAKE_KEYS = ("seed", "N", "P", "continuous", "n_cov", "n_dup", "reweight", "n_folds", "const_in_fold")


def _load(name):
    g = np.load(os.path.join(GOLD, "solver_%s.npz" % name))
    spec = json.loads(str(g["spec"]))
    case = R.make_case(**{k: spec[k] for k in MAKE_KEYS if k in spec})
    return g, spec, case


def _device_fit(case, spec, thresh, **kw):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import pack_variants
    e = Engine(spec["N"])
    M = EnetMatrix(e, spec["P"])
    M.append(pack_variants(case["K"]))
    fit = M.fit(case["y"], spec["continuous"], spec["alpha"], weights=case["w"], covariates=case["cov"], fold_id=case["fold"],
                n_folds=spec["n_folds"], thresh=thresh, n_lambda=spec["n_lambda"], **kw)
    sols = [[fit.betas_at(l, f) for l in range(fit.n_lambda)] for f in range(spec["n_folds"] + 1)]
    M.close()
    e.close()
    return fit, sols


def _check(name, tag, thresh):
    g, spec, case = _load(name)
    family = R.GAUSSIAN if spec["continuous"] else R.BINOMIAL
    fit, sols = _device_fit(case, spec, thresh)
    L, lam, n_cov = int(g["L"]), g["lambdas"], spec["n_cov"]
    tau, delta = 2 * float(g["tau_" + tag]), 2 * float(g["delta_" + tag])
    assert fit.n_lambda == L, "the path ended at lambda %d, the yardstick's at %d" % (fit.n_lambda, L)
    assert np.max(np.abs(fit.lambdas / lam[:L] - 1)) <= 1e-12
    # the state is v and the residual, and the working response for binomial: fp64 vectors of ceil(N / 64) * 64 entries plus 64 doubles of
    # scratch, in the LDS while that fits the 160 KiB of a CU (binomial N = 8192: 192 KiB, in global memory)
    lds_bytes = (64 + (2 if spec["continuous"] else 3) * ((spec["N"] + 63) // 64) * 64) * 8
    assert fit.state_in_lds == (lds_bytes <= 160 * 1024), "where the per-sample state is kept"
    if name == "b_n8192_p500_a0069":
        assert not fit.state_in_lds
    probs = R.problems(case, family, spec["alpha"])
    # ---- KKT at every lambda of the path, for the full fit and every fold, from the returned slopes and the unpacked matrix
    worst = 0.0
    for f, prob in enumerate(probs):
        for l in range(L):
            assert not np.any(sols[f][l][1][prob.sinv == 0]), "a column that is constant in this problem has a slope"
            b0, beta = R.to_standardised(prob, *sols[f][l])
            worst = max(worst, R.kkt_residual(prob, lam[l], b0, beta)[0])
    print("%s thresh %g: largest KKT residual %.3e (allowed %.3e)" % (name, thresh, worst, tau))
    assert worst <= tau
    # ---- slopes at lambda_min and five other path points against the optimum
    far = 0.0
    for k, l in enumerate(g["points"]):
        b0, beta = sols[0][l]
        opt = np.zeros(beta.size)
        opt[g["opt_idx_%d" % k]] = g["opt_val_%d" % k]
        far = max(far, abs(b0 - float(g["opt_b0_%d" % k])), float(np.abs(beta - opt).max()))
        if tag == "t":                                                # the selected set, the undecidable columns dropped (at most 1 %: generator)
            sel = np.unpackbits(g["sel_%d" % k])[:beta.size].astype(bool)
            und = np.unpackbits(g["und_%d" % k])[:beta.size].astype(bool)
            # (variants: a covariate is always swept, and at lambda_max the column that sets lambda_max sits on the threshold by definition)
            assert ((beta != 0) == sel)[n_cov:][~und[n_cov:]].all(), "another set of variants is selected at lambda %d" % l
    print("%s thresh %g: slopes within %.3e of the optimum (allowed %.3e)" % (name, thresh, far, delta))
    assert far <= delta
    # ---- cross-validation figures
    dc, ds = np.abs(fit.cvm - g["cvm_opt"]).max(), np.abs(fit.cvsd - g["cvsd_opt"]).max()
    print("%s thresh %g: cvm within %.3e (allowed %.3e), cvsd within %.3e (allowed %.3e), i_min %d (optimum %d)"
          % (name, thresh, dc, 2 * float(g["cvm_bound_" + tag]), ds, 2 * float(g["cvsd_bound_" + tag]), fit.i_min, int(g["i_min_opt"])))
    assert dc <= 2 * float(g["cvm_bound_" + tag]) + 1e-14 and ds <= 2 * float(g["cvsd_bound_" + tag]) + 1e-14
    if tag == "t" or bool(g["imin_decided_d"]):
        assert fit.i_min == int(g["i_min_opt"])
    b0, beta = sols[0][fit.i_min]
    assert fit.beta0 == b0 and (fit.beta == beta).all(), "the slopes returned by the fit are the full fit's at lambda_min"
    assert (fit.nzero == [int(np.count_nonzero(sols[0][l][1][n_cov:])) for l in range(L)]).all()


@pytest.mark.parametrize("name", CASES)
def test_tight_run_meets_kkt_and_the_optimum(name):
    _check(name, "t", 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_default_run_meets_kkt_within_glmnets_own_slack(name):
    _check(name, "d", 1e-7)


def test_default_argmin_is_decided_in_a_binary_and_a_continuous_case():
    decided = {True: False, False: False}
    for name in CASES:
        g, spec, _ = np.load(os.path.join(GOLD, "solver_%s.npz" % name)), None, None
        decided[json.loads(str(g["spec"]))["continuous"]] |= bool(g["imin_decided_d"])
    assert decided[True] and decided[False]


@pytest.mark.parametrize("name", ["ref_kmers_binary", "ref_kmers_continuous", "ref_rtab_binary", "ref_rtab_continuous"])
def test_correlations_and_kept_sets_are_the_references(name):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, correlation_cut
    g = np.load(os.path.join(GOLD, name + ".npz"))
    e = Engine(int(g["n_samples"]))
    M = EnetMatrix(e, g["rows"].shape[0])
    M.append(g["rows"])
    cor = M.correlations(g["y"])
    assert (np.isnan(cor) == np.isnan(g["cor"])).all()
    ok = ~np.isnan(cor)
    assert np.max(np.abs(cor[ok] - g["cor"][ok])) <= 1e-11
    for q, key in ((0.25, "kept25"), (0.5, "kept50")):
        assert (correlation_cut(cor, q) == g[key]).all()
    # the kept rows, compacted on the device, are the rows
    M.keep(g["kept50"])
    assert M.rows == g["kept50"].size
    assert (M.get_rows(np.arange(M.rows)) == g["rows"][g["kept50"]]).all()
    M.close()
    e.close()


def test_minor_allele_coding_and_missing_calls():
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import pack_variants, unpack_variants
    rng = np.random.default_rng(5)
    N = 130
    K = (rng.random((6, N)) < np.array([0.1, 0.7, 0.9, 0.4, 0.6, 0.5])[:, None]).astype(np.uint8)
    miss = ((rng.random((6, N)) < 0.05) & (K == 0)).astype(np.uint8)
    flip = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    e = Engine(N)
    M = EnetMatrix(e, 6)
    M.append(pack_variants(K), pack_variants(miss), flip)
    got = unpack_variants(M.get_rows(np.arange(6)), N)
    want = np.where(flip[:, None] == 1, (K == 0) & (miss == 0), K == 1)   # enet.py:95-106: obs == pres, a missing call equals neither
    assert (got == want).all()
    assert not M.get_rows(np.arange(6))[:, (N + 7) // 8:].any() and not (M.get_rows(np.arange(6))[:, N // 8] >> (N % 8)).any()
    M.close()
    e.close()


def test_a_fold_is_the_problem_with_its_samples_removed():
    """Fold 0 fitted by physically removing its samples (repacked bits, no folds, the same penalties) gives the slopes of the zero-weight
    route within the bound on the slopes."""
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import pack_variants
    for name in ("g_n200_p500_a5_cov", "b_n200_p500_a5_const", "g_n200_p500_a0069"):
        g, spec, case = _load(name)
        fit, sols = _device_fit(case, spec, 1e-12)
        keep = case["fold"] != 0
        e = Engine(int(keep.sum()))
        M = EnetMatrix(e, spec["P"])
        M.append(pack_variants(case["K"][:, keep]))
        sub = M.fit(case["y"][keep], spec["continuous"], spec["alpha"], weights=case["w"][keep], covariates=case["cov"][keep], thresh=1e-12,
                    lambdas=fit.lambdas)
        delta, far = 2 * float(g["delta_t"]), 0.0
        assert sub.n_lambda >= min(5, fit.n_lambda)
        for l in range(sub.n_lambda):
            b0, beta = sub.betas_at(l)
            far = max(far, abs(b0 - sols[1][l][0]), float(np.abs(beta - sols[1][l][1]).max()))
        print("%s: removed samples against zero weights, slopes within %.3e (allowed %.3e)" % (name, far, delta))
        assert far <= delta
        M.close()
        e.close()


def test_two_runs_give_the_same_bytes():
    g, spec, case = _load("b_n200_p500_a0069_cov")
    a, sa = _device_fit(case, spec, 1e-7)
    b, sb = _device_fit(case, spec, 1e-7)
    for x, y in ((a.lambdas, b.lambdas), (a.cvm, b.cvm), (a.cvsd, b.cvsd), (a.beta, b.beta), (a.fold_dev, b.fold_dev)):
        assert x.tobytes() == y.tobytes()
    assert a.i_min == b.i_min and a.beta0 == b.beta0 and a.cd_sweeps == b.cd_sweeps
    for f in range(len(sa)):
        for l in range(a.n_lambda):
            assert sa[f][l][0] == sb[f][l][0] and sa[f][l][1].tobytes() == sb[f][l][1].tobytes()


def test_state_in_global_memory_gives_the_same_slopes_as_in_the_lds():
    g, spec, case = _load("g_n200_p500_a5_cov")
    a, sa = _device_fit(case, spec, 1e-12)
    b, sb = _device_fit(case, spec, 1e-12, state_in_global=True)
    assert a.state_in_lds and not b.state_in_lds
    for l in range(a.n_lambda):
        assert sa[0][l][1].tobytes() == sb[0][l][1].tobytes()


def test_refusals():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import pack_variants
    rng = np.random.default_rng(3)
    K = (rng.random((20, 64)) < 0.3).astype(np.uint8)
    y = rng.normal(size=64)
    e = Engine(64)
    M = EnetMatrix(e, 20)
    with pytest.raises(ValueError, match="No variants passed filters"):
        M.fit(y, True, 0.5)
    with pytest.raises(ValueError, match="No variants passed filters"):
        M.correlations(y)
    M.append(pack_variants(K))
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            M.fit(y, True, alpha)
    with pytest.raises(_abi.SeerHipError, match="reserved"):
        M.append(pack_variants(K))
    with pytest.raises(_abi.SeerHipError, match="0 or 1"):
        M.fit(y, False, 0.5)
    M.close()
    e.close()


def test_carrier_sums_of_sixteen_and_more_vectors_and_spare_words():
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import pack_variants
    rng = np.random.default_rng(8)
    N, P = 777, 300
    K = (rng.random((P, N)) < rng.uniform(0.01, 0.6, P)[:, None]).astype(np.uint8)
    V = rng.normal(size=(19, N))
    e = Engine(N)
    M = EnetMatrix(e, P)
    M.append(pack_variants(K))
    got = M.carrier_sums(V)
    want = V @ K.T.astype(float)
    # fp64 sums of at most N terms of magnitude ~4: N x 4 x 1.1e-16 = 3.5e-13
    assert np.abs(got - want).max() <= 1e-12
    M.close()
    e.close()


def test_a_changed_matrix_forgets_the_last_fit():
    from pyseer_amd import _abi
    g, spec, case = _load("g_n1000_p200_a5_short")
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import pack_variants
    e = Engine(spec["N"])
    M = EnetMatrix(e, spec["P"])
    M.append(pack_variants(case["K"]))
    fit = M.fit(case["y"], True, 0.5, n_lambda=3)
    fit.betas_at(1)
    M.keep(np.arange(10))
    with pytest.raises(_abi.SeerHipError):
        fit.betas_at(1)
    fit = M.fit(case["y"], True, 0.5, n_lambda=3)
    assert fit.betas_at(1)[1].size == 10
    with pytest.raises(_abi.SeerHipError):
        M.fit(case["y"], True, 0.5, lambdas=[1.0, 2.0])
    with pytest.raises(_abi.SeerHipError):
        M._betas_at(0, 0)
    M.close()
    e.close()
