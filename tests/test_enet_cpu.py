"""Host side of the whole-genome elastic net, no GPU: fold assignment, sample weights, the quantile cut of the correlation filter
against the reference's kept sets, the numpy yardstick solver (tests/_enet_ref.py) against scikit-learn's committed figures, and the
ABI surface of sh_enet_*."""
import ctypes as C
import os
import re

import numpy as np

import _enet_ref as R
from pyseer_amd import _abi
from pyseer_amd import enet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "enet")


def test_folds_are_balanced_seeded_and_follow_cvglmnets_rule():
    f = enet.assign_folds(103, 10, seed=1)
    assert f.dtype == np.int32 and f.min() == 0 and f.max() == 9
    counts = np.bincount(f)
    assert counts.max() - counts.min() <= 1 and counts.sum() == 103
    assert (f == enet.assign_folds(103, 10, seed=1)).all() and (f != enet.assign_folds(103, 10, seed=2)).any()
    perm = np.random.default_rng(1).permutation(103)                 # sample i of the random order goes to fold i mod F
    assert (f[perm] == np.arange(103) % 10).all()
    for bad in (1, 104):
        try:
            enet.assign_folds(103, bad)
        except ValueError:
            continue
        raise AssertionError("n_folds = %d accepted" % bad)


def test_sequence_weights_are_one_over_the_cluster_size():
    cl = np.array(["a", "b", "a", "c", "a", "b"])
    w = enet.sequence_weights(cl)
    assert np.allclose(w, [1 / 3, 1 / 2, 1 / 3, 1, 1 / 3, 1 / 2])
    # pyseer/__main__.py:651-652 on the one-hot matrix
    onehot = (cl[:, None] == np.unique(cl)[None, :]).astype(float)
    assert np.allclose(w, onehot @ (1 / onehot.sum(0)))


def test_quantile_cut_is_the_references():
    for name in ("ref_kmers_binary", "ref_kmers_continuous", "ref_rtab_binary", "ref_rtab_continuous"):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        for q, key in ((0.25, "kept25"), (0.5, "kept50")):
            assert (enet.correlation_cut(g["cor"], q) == g[key]).all()
    cor = np.array([0.1, 0.4, np.nan, 0.3])                          # one empty row: the percentile is NaN and nothing passes (enet.py:420)
    assert enet.correlation_cut(cor, 0.25).size == 0
    assert (enet.correlation_cut(np.array([0.1, 0.2, 0.2, 0.3]), 0.5) == [3]).all()   # strictly above the cut


def test_reference_matrices_are_minor_allele_coded_and_filtered_strictly():
    for name in ("ref_kmers_binary", "ref_rtab_continuous"):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        n = int(g["n_samples"])
        K = np.unpackbits(g["rows"], axis=1, bitorder="little")[:, :n]
        assert (K.sum(1) <= n / 2).all() and (K.sum(1) > 0).all()
        assert g["var_indices"].size == K.shape[0] and int(g["loaded"]) >= K.shape[0]
        assert (np.diff(g["var_indices"]) > 0).all() and g["var_indices"].max() < int(g["loaded"])


def test_numpy_solver_against_scikit_learn_figures():
    g = np.load(os.path.join(GOLD, "sklearn_figures.npz"))
    for alpha in (0.0069, 0.5):
        c = R.make_case(1, 200, 300, True, n_dup=30, reweight=True)
        pr = R.problems(c, R.GAUSSIAN, alpha)[0]
        lam = R.lambda_sequence(pr, 10)
        assert np.allclose(lam, g["gaussian_lambdas_%g" % alpha], rtol=1e-12, atol=0)
        opt = R.fit_path(pr, lam, 1e-26, starts=R.fit_path(pr, lam, 1e-12))
        coefs = g["gaussian_coefs_%g" % alpha]
        assert max(np.abs(coefs[:, l] - opt[l][1]).max() for l in range(10)) < 1e-10
    c = R.make_case(2, 200, 40, False, reweight=True)
    pr = R.problems(c, R.BINOMIAL, 0.5)[0]
    lam = R.lambda_sequence(pr, 10, ratio=1e-2)
    opt = R.fit_path(pr, lam, 1e-26, starts=R.fit_path(pr, lam, 1e-12))
    for l in (2, 5, 9):                                               # saga is the weaker party: 1e-5, and the KKT residual is the certificate
        assert R.kkt_residual(pr, lam[l], *opt[l])[0] < 1e-12
        assert max(np.abs(g["binomial_coef_%d" % l] - opt[l][1]).max(), abs(float(g["binomial_b0_%d" % l]) - opt[l][0])) < 1e-5


def test_numpy_solver_thresholds_order_and_zero_weight_folds():
    c = R.make_case(3, 120, 80, True, n_cov=2, n_dup=8, reweight=True, n_folds=3, const_in_fold=True)
    probs = R.problems(c, R.GAUSSIAN, 0.5)
    assert probs[1].sinv[2] == 0 and probs[0].sinv[2] > 0            # row 0 (column n_cov + 0) is constant once fold 0 is held out
    lam = R.lambda_sequence(probs[0], 8)
    res = {}
    for thr in (1e-7, 1e-12, 1e-26):
        sol = R.fit_path(probs[1], lam, thr, always_active=2)
        res[thr] = max(R.kkt_residual(probs[1], lam[l], *sol[l])[0] for l in range(8))
        assert all(s[1][2] == 0 for s in sol)
    assert res[1e-26] < 1e-12 and res[1e-26] <= res[1e-12] <= res[1e-7]
    # the zero-weight problem is the problem with the samples removed
    keep = c["fold"] != 0
    sub = R.Problem(R.design(c)[keep], c["y"][keep], c["w"][keep], R.GAUSSIAN, 0.5)
    a = R.fit_path(probs[1], lam, 1e-26, always_active=2)
    b = R.fit_path(sub, lam, 1e-26, always_active=2)
    assert max(np.abs(a[l][1] - b[l][1]).max() for l in range(8)) < 1e-10


def test_abi_declares_binds_and_exports_the_enet_surface():
    hdr = open(os.path.join(ROOT, "include", "seerhip.h")).read()
    names = ["sh_enet_begin", "sh_enet_append", "sh_enet_rows", "sh_enet_correlations", "sh_enet_carrier_sums", "sh_enet_keep", "sh_enet_get_rows", "sh_enet_fit",
             "sh_enet_betas_at", "sh_enet_eta_at", "sh_enet_end"]
    lib = _abi.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _abi.SIGNATURES and hasattr(lib, n)
    assert lib.sh_abi_version() == 2
    # the structs of the header and of the binding have the same layout (LP64)
    assert C.sizeof(_abi.EnetOpts) == 40 and _abi.EnetOpts.thresh.offset == 16 and _abi.EnetOpts.lambda_seq.offset == 32
    assert C.sizeof(_abi.EnetOut) == 112 and _abi.EnetOut.cd_sweeps.offset == 16 and _abi.EnetOut.lambda_.offset == 48 and _abi.EnetOut.nzero.offset == 104
    fields = re.search(r"typedef struct sh_enet_out \{(.*?)\} sh_enet_out;", hdr, re.S).group(1)
    assert re.findall(r"\*(\w+)", fields) == ["lambda", "cvm", "cvsd", "dev_ratio", "fold_dev", "fold_weight", "beta", "nzero"]
    # without a context every entry point refuses instead of touching a device
    assert lib.sh_enet_begin(None, 8, 1) == _abi.SH_EINVAL and lib.sh_enet_rows(None) == -1 and lib.sh_enet_end(None) == _abi.SH_EINVAL
