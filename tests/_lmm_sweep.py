"""Shared by the LMM sweeps (tests/test_lmm_widths_gpu.py, tests/test_lmm_refined_gpu.py) and their CPU check
(tests/test_lmm_sweep_helpers_cpu.py): the designs and rows of the sweeps, a numpy.longdouble restatement of the reference's fit_lmm_block
(pyseer/lmm.py:228-260, fastlmm/lmm_cov.py rotate :165-194, nLLcore :686-838) that the oracle is held to, and the deviation bookkeeping.

Designs follow tests/test_lmm_gpu.py:_random_lmm: U not orthonormal with k = N - D columns, gamma-distributed S, the intercept last."""
import numpy as np

LD = np.longdouble
FIELDS = ("beta", "bse", "frac_h2", "pvalue")


def design(N, D, seed, continuous=False, binary_col0=True, dup=(), indefinite=False):
    """(U, S, covar, y).  binary_col0: for D >= 2 column 0 of the panel is 0/1 with 35 % ones (a row can then equal it).
    dup: (dst, src, factor) triples, column dst = factor x column src (a numerically dependent column).
    indefinite: the five smallest eigenvalues become -(0.05, 0.1, 0.3, 0.6, 0.9): at h2 = 0.6 the smallest Sd = h2 S + 1 - h2 is -0.14."""
    rng = np.random.default_rng(seed)
    k = N - D
    U = rng.standard_normal((N, k)) / np.sqrt(N)
    S = np.sort(rng.gamma(0.5, 2.0, k))[::-1].copy()
    covar = np.ones((N, 1)) if D == 1 else np.c_[rng.standard_normal((N, D - 1)), np.ones((N, 1))]
    y = rng.standard_normal(N) if continuous else (rng.random(N) < 0.4).astype(float)
    if D >= 2 and binary_col0:
        covar[:, 0] = (rng.random(N) < 0.35).astype(float)
    for dst, src, f in dup:
        assert 0 <= src < dst < D - 1
        covar[:, dst] = f * covar[:, src]
    if indefinite:
        S[-5:] = -np.array([0.05, 0.1, 0.3, 0.6, 0.9])
    return U, S, covar, y


def rows(N, V, seed, covar=None, edges=True):
    """(Kv, special).  Allele frequencies uniform in 0.02 .. 0.98; the first V/8 rows at 0.9 (the engine stores them complemented).
    edges: one all-zero and one all-one row, and for a panel whose column 0 is 0/1 one row equal to it and one equal to its complement;
    special maps "zero" / "one" / "span" / "cospan" to their row indices."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.02, 0.98, V)
    Kv = (rng.random((V, N)) < af[:, None]).astype(np.uint8)
    Kv[: V // 8] = (rng.random((V // 8, N)) < 0.9).astype(np.uint8)
    special = {}
    if edges:
        base = V // 8 + 3
        special["zero"] = base; Kv[base] = 0
        special["one"] = base + 5; Kv[base + 5] = 1
        if covar is not None and covar.shape[1] >= 2 and np.isin(covar[:, 0], (0.0, 1.0)).all():
            special["span"] = base + 9; Kv[base + 9] = covar[:, 0].astype(np.uint8)
            special["cospan"] = base + 14; Kv[base + 14] = 1 - covar[:, 0].astype(np.uint8)
    return Kv, special


def covariate_basis(covar, plain_qr=False):
    """Orthonormal basis (longdouble) of the span of covar's numerically independent columns: modified Gram-Schmidt, every column
    orthogonalised twice; a column whose remainder is below 1e-10 of its norm is dropped (pinv drops it as well, lmm_cov.py:869).
    plain_qr (the CPU test's self-check only): numpy's QR of the whole panel, rank ignored -- wrong for a rank-deficient panel."""
    if plain_qr:
        return np.linalg.qr(np.asarray(covar, float))[0].astype(LD)
    C = np.asarray(covar, dtype=LD)
    Q = []
    for d in range(C.shape[1]):
        c = C[:, d].copy()
        n0 = np.sqrt(c @ c)
        for _ in range(2):
            for q in Q:
                c -= (q @ c) * q
        n1 = np.sqrt(c @ c)
        if n0 == 0 or n1 <= LD(1e-10) * n0:
            continue
        Q.append(c / n1)
    return np.stack(Q, axis=1)


def fit_lmm_block_longdouble(U, S, y, covar, h2, Kv, plain_qr=False):
    """beta, bse, frac_h2 of fit_lmm_block in numpy.longdouble; Kv (V, n) 0/1.  Degrees of freedom as the reference's: n - D - 1 with D
    the number of covariate columns, whatever their rank (Linreg.D = X.shape[1], lmm_cov.py:854)."""
    U = np.asarray(U, dtype=LD); S = np.asarray(S, dtype=LD); y = np.asarray(y, dtype=LD).reshape(-1)
    n = y.shape[0]; D = np.asarray(covar).reshape(n, -1).shape[1]
    Q = covariate_basis(np.asarray(covar).reshape(n, -1), plain_qr)

    def rotate(A):                                                  # lmm_cov.py:165-194
        A = A - Q @ (Q.T @ A)
        A = A - Q @ (Q.T @ A)
        A[:, A.std(0) <= 1e-10] = 0.0
        return U.T @ A

    Sd = LD(h2) * S + (LD(1.0) - LD(h2))
    uy = rotate(y.reshape(-1, 1))[:, 0]
    ux = rotate(np.asarray(Kv, dtype=LD).T.copy())
    yKy = np.sum(uy * uy / Sd)
    with np.errstate(divide="ignore", invalid="ignore"):
        sKs = np.sum(ux * ux / Sd[:, None], axis=0)
        sKy = np.sum(ux * (uy / Sd)[:, None], axis=0)
        beta = sKy / sKs
        beta[np.isnan(beta) & (sKy == 0)] = 0.0                    # lmm_cov.py:803-805
        veb = sKy * beta
        var = (yKy - veb) / LD(n - D - 1) / sKs                    # lmm_cov.py:813, N = n - D
        bse = np.sqrt(var)
        frac = np.sqrt(veb / yKy)
    return dict(beta=beta, bse=bse, frac_h2=frac)


def beta_error_of(beta, U, S, y, covar, h2, Kv):
    """Per row, the relative error of a float64 beta (the oracle's) itself.  beta's numerator x^T K^-1 y is the one cancelling sum of
    fit_lmm_block; it equals x^T w with w = P U Sd^-1 U^T P y, one n-vector, taken here in longdouble (V n operations, where the whole
    restatement takes V n k).  The denominator x^T K^-1 x is a sum of squares: float64 holds it to about 1e-14.  Rows the covariates
    explain are not meant (no zeroing here)."""
    n = np.asarray(y).reshape(-1).shape[0]
    Q = covariate_basis(np.asarray(covar).reshape(n, -1))
    Ul = np.asarray(U, dtype=LD); yl = np.asarray(y, dtype=LD).reshape(-1)
    Sd = LD(h2) * np.asarray(S, dtype=LD) + (LD(1.0) - LD(h2))
    proj = lambda a: a - Q @ (Q.T @ a)                             # noqa: E731
    w = Ul @ ((Ul.T @ proj(proj(yl))) / Sd)
    w = proj(proj(w))
    Q64 = Q.astype(float); U64 = np.asarray(U, float); Sd64 = Sd.astype(float)
    err = np.empty(Kv.shape[0])
    for a in range(0, Kv.shape[0], 2048):
        K = Kv[a:a + 2048]
        A = K.T.astype(float)
        A -= Q64 @ (Q64.T @ A)
        A -= Q64 @ (Q64.T @ A)
        ux = U64.T @ A
        sKs = np.sum(ux * ux / Sd64[:, None], axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):       # a row the covariates explain: 0 / 0, NaN
            exact = (K.astype(LD) @ w) / sKs
            err[a:a + 2048] = np.abs(np.asarray(beta[a:a + 2048], dtype=LD) - exact) / np.abs(exact)
    return err


def same_pattern(got, want, what=""):
    """NaN, +inf and -inf sit in the same rows."""
    got = np.asarray(got, dtype=float); want = np.asarray(want, dtype=float)
    for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        a, b = f(got), f(want)
        assert np.array_equal(a, b), "%s: %s pattern differs at rows %s" % (what, name, np.flatnonzero(a != b)[:8])


def deviation(got, want):
    """Maximum relative deviation over the rows where both sides are finite and non-zero (0.0 when there is none)."""
    got = np.asarray(got, dtype=LD); want = np.asarray(want, dtype=LD)
    ok = np.isfinite(got) & np.isfinite(want) & (got != 0) & (want != 0)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def deviations(r, want):
    """{field: deviation} of an engine result dict against the oracle's (beta, bse, frac_h2, p), patterns compared exactly first."""
    out = {}
    for f, w in zip(FIELDS, want):
        same_pattern(r[f], w, f)
        out[f] = deviation(r[f], w)
    return out


def fmt(devs):
    return "  ".join("%s %.3g" % (f, devs[f]) for f in FIELDS if f in devs)
