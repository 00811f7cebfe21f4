"""numpy yardsticks for fit_lineage_effect (pyseer/model.py:151-199) on a cluster-indicator design X = [1, indicators of l clusters], and the
inputs the count-route tests share (tests/test_lineage_counts_cpu.py, tests/test_lineage_counts_gpu.py).

wald_dense / argmax_dense: the reference's arithmetic as it stands -- statsmodels' Newton (zero start, ridge 1e-10 on the diagonal of
hessian/nobs, steps through np.linalg.inv, _check_perfect_pred after every step, at most 35 iterations, tolerance 1e-8 on the step), then
|params| / bse from inv(-hessian/nobs)/nobs without the ridge.  O(l^3) per iteration.
wald_counts / argmax_counts: the same iteration written on the carrier counts (n_c, s_c) of the clusters, O(l) per iteration: the form
k_glm_lineage_counts (csrc/glm_lineage.hip) runs.

The ridge: statsmodels adds 1e-10 to the diagonal of hessian/nobs, which is NEGATIVE definite for method='newton', so in terms of the
positive h_c = n_c mu_c (1 - mu_c) / n the regularised diagonal is h_c - 1e-10 (k_glm_lineage: H[a][a] -= 1e-10).  RHO below is that signed
value; the reduced step is
    d0  = (g_r + sum_c g_c RHO / (h_c + RHO)) / (h_r + RHO + sum_c h_c RHO / (h_c + RHO)),   d_c = (g_c - h_c d0) / (h_c + RHO).
"""
import os

import numpy as np

RHO = -1e-10
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(G, "lincounts_dense.npz")

# Largest relative difference between the Wald values of the two forms, over the clusters that can decide a row (FIXTURE_NEAR) of every
# well_conditioned row of YARDSTICK_CASES, as drawn and tame: measured 2.99e-6 (N = 200, l = 64; 2.52e-6 at l = 65, 2.0e-11 at N = 600,
# l = 200, 4.8e-14 at N = 1100, l = 1000).  tests/test_lineage_counts_cpu.py measures it again and holds it under 2 x MEASURED_WALD_DIFF.
# (Twice the measured figure is what the CPU test allows a run on another BLAS or libm.)
MEASURED_WALD_DIFF = 2.99e-6
DELTA = 10 * MEASURED_WALD_DIFF

YARDSTICK_CASES = [(200, 64), (200, 65), (600, 200), (1100, 1000)]
YARDSTICK_ROWS = 300
FIXTURE_NEAR = 0.5          # the fixture keeps a row's dense Wald values down to this share of its maximum: the values that can decide the answer


def _cdf(x):
    return 1.0 / (1.0 + np.exp(-x))


def design(cluster_of, l):
    """cluster_of[i] in 0..l (0: the reference cluster, no column) -> the n x l indicator matrix the command line passes."""
    cluster_of = np.asarray(cluster_of)
    lin = np.zeros((len(cluster_of), l))
    i = np.flatnonzero(cluster_of > 0)
    lin[i, cluster_of[i] - 1] = 1.0
    return lin


def wald_dense(lin, k):
    """|params| / bse of the l lineage columns as the reference computes them, or None (PerfectSeparationError / LinAlgError)."""
    with np.errstate(all="ignore"):
        k = np.asarray(k, dtype=float)
        n = len(k)
        X = np.concatenate([np.ones((n, 1)), np.asarray(lin, dtype=float)], axis=1)
        pc = X.shape[1]
        beta = np.zeros(pc); old = np.full(pc, np.inf); it = 0
        while it < 35 and np.any(np.abs(beta - old) > 1e-8):
            mu = _cdf(X @ beta)
            H = -(X.T * (mu * (1 - mu))) @ X / n
            H[np.diag_indices(pc)] += 1e-10
            try:
                Hinv = np.linalg.inv(H)
            except np.linalg.LinAlgError:
                return None
            old = beta
            beta = old - Hinv @ (X.T @ (k - mu) / n)
            it += 1
            if np.allclose(_cdf(X @ beta) - k, 0):
                return None
        mu = _cdf(X @ beta)
        try:
            cov = np.linalg.inv((X.T * (mu * (1 - mu))) @ X / n) / n
        except np.linalg.LinAlgError:
            return None
        return (np.abs(beta) / np.sqrt(np.diag(cov)))[1:]


def argmax_of(wald):
    """np.argmax as model.py:194 applies it (the first NaN wins), None for None."""
    return None if wald is None else int(np.argmax(wald))


def argmax_dense(lin, k):
    return argmax_of(wald_dense(lin, k))


def counts(cluster_of, l, k):
    """(n_c, s_c) for c = 0 (the reference cluster), 1..l."""
    cluster_of = np.asarray(cluster_of)
    n_c = np.bincount(cluster_of, minlength=l + 1).astype(float)
    s_c = np.bincount(cluster_of, weights=np.asarray(k, dtype=float), minlength=l + 1)
    return n_c, s_c


def wald_counts(n_c, s_c, rho=RHO):
    """The reduced form: the same Newton iteration on the counts.  Entry 0 is the reference cluster (its coefficient is fixed at 0)."""
    with np.errstate(all="ignore"):
        n_c = np.asarray(n_c, dtype=float); s_c = np.asarray(s_c, dtype=float)
        n = n_c.sum()
        b = np.zeros(len(n_c)); b0 = 0.0
        full = n_c > 0
        pure = (s_c == 0) | (s_c == n_c)
        y = (s_c > 0).astype(float)
        it = 0; moving = True
        while it < 35 and moving:
            mu = _cdf(b0 + b)
            h = n_c * mu * (1 - mu) / n
            g = (s_c - n_c * mu) / n
            den = h[1:] + rho
            d0den = h[0] + rho + np.sum(h[1:] * rho / den)
            if np.any(den == 0) or d0den == 0:
                return None
            d0 = (g[0] + np.sum(g[1:] * rho / den)) / d0den
            d = (g[1:] - h[1:] * d0) / den
            b0 += d0; b[1:] += d
            it += 1
            moving = bool(abs(d0) > 1e-8 or np.any(np.abs(d) > 1e-8))
            mu = _cdf(b0 + b)
            if np.all(pure[full]) and np.all(np.abs(mu - y)[full] <= 1e-8):
                return None
        mu = _cdf(b0 + b)
        h = n_c * mu * (1 - mu) / n
        if np.any(h == 0):
            return None
        return np.abs(b[1:]) / np.sqrt((1 / h[1:] + 1 / h[0]) / n)


def argmax_counts(n_c, s_c):
    return argmax_of(wald_counts(n_c, s_c))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def cluster_sizes(N, l, rng):
    """A quarter singletons, the rest 2-11, one large reference cluster of what remains.  Where N cannot hold those sizes (l = 1000 clusters
    in N = 1100 samples) the largest clusters shrink, down to singletons, until the reference cluster keeps at least max(N / 20, 2)."""
    sizes = np.where(np.arange(l) % 4 == 0, 1, rng.integers(2, 12, l))
    budget = N - max(N // 20, 2)
    assert budget >= l
    while sizes.sum() > budget:
        big = np.flatnonzero(sizes == sizes.max())
        sizes[big[rng.integers(len(big))]] -= 1
    return rng.permutation(sizes)


def break_full_clusters(cluster_of, l, K, rng):
    """Clears one carrier of every cluster (the reference cluster included) that holds nothing but carriers; an all-1 row stays as it is."""
    for k in K:
        if k.all():
            continue
        n_c, s_c = counts(cluster_of, l, k)
        for c in np.flatnonzero((s_c == n_c) & (n_c > 0)):
            i = np.flatnonzero(cluster_of == c)
            k[i[rng.integers(len(i))]] = 0
    return K


def well_conditioned(n_c, s_c):
    """False for the rows on which the reference's own answer is rounding noise: rows with a cluster of carriers only (s_c = n_c > 0) beside
    a cluster that is mixed.  Its coefficient runs to +infinity at a step of 1 per iteration until h_c = n_c mu_c (1 - mu_c) / n meets the
    ridge 1e-10; there the step -h_c / (h_c - 1e-10) has a pole, the iterate bounces around it for the remaining iterations, and every
    crossing multiplies the relative error of h_c -- 1e-16 / (1 - mu_c) ~ 1e-8 from the subtraction 1 - mu_c -- by 1 / |h_c / 1e-10 - 1|.
    Whether the fit ends with mu_c == 1.0 exactly (LinAlgError, None) or not is decided by that noise: np.linalg.inv, the oracle and the
    reduced form differ on such rows (tests/test_lineage_counts_cpu.py gives the counts).  A cluster without carriers is harmless: mu_c is
    small there, and mu_c (1 - mu_c) keeps its relative precision -- unless it is the reference cluster: then the intercept itself runs off,
    the corner h_r - 1e-10 + sum_c ... of the step crosses zero, and every coefficient is thrown about with it (Wald values ~ 1e-3, their
    order noise).  So: no cluster of carriers only, and a mixed reference cluster; or every cluster pure (PerfectSeparationError)."""
    n_c = np.asarray(n_c); s_c = np.asarray(s_c)
    full = (s_c == n_c) & (n_c > 0)
    pure = (s_c == 0) | (s_c == n_c)
    return bool((not full.any() and not pure[0]) or pure.all())


def yardstick_case(N, l, V=YARDSTICK_ROWS, tame=False):
    """-> cluster_of (N, uint16), K (V x N, uint8).  Per variant 60 % of the clusters have no carriers, the others a carrier rate in
    0.2-0.9; the reference cluster is mixed, and pure (all 0 / all 1 in turn) in every fourth variant.  tame: the same rows with every
    cluster of carriers only broken (break_full_clusters), so that every row is well_conditioned."""
    rng = np.random.default_rng(1000 * N + l)
    sizes = cluster_sizes(N, l, rng)
    cluster_of = np.zeros(N, dtype=np.uint16)
    cluster_of[:sizes.sum()] = np.repeat(np.arange(1, l + 1), sizes)
    cluster_of = cluster_of[rng.permutation(N)]
    K = np.zeros((V, N), dtype=np.uint8)
    for v in range(V):
        rate = np.where(rng.random(l + 1) < 0.6, 0.0, rng.uniform(0.2, 0.9, l + 1))
        rate[0] = ((v // 4) % 2) if v % 4 == 3 else rng.uniform(0.2, 0.9)
        K[v] = rng.random(N) < rate[cluster_of]
    if tame:
        break_full_clusters(cluster_of, l, K, np.random.default_rng(7))
    return cluster_of, K


def oracle_case(N, l, V, seed):
    """Cluster designs for the oracle comparisons: a reference cluster of about a quarter of the samples, the others spread over the l
    clusters (a column stays empty where N - 1 < l); rows with carrier rates per cluster as above, plus an all-0 and an all-1 row."""
    rng = np.random.default_rng(seed)
    nref = max(1, N // 4)
    rest = N - nref
    cluster_of = np.zeros(N, dtype=np.uint16)
    first = min(l, rest)
    cluster_of[nref:nref + first] = np.arange(1, first + 1)
    cluster_of[nref + first:] = rng.integers(1, l + 1, rest - first)
    cluster_of = cluster_of[rng.permutation(N)]
    K = np.zeros((V, N), dtype=np.uint8)
    for v in range(V):
        rate = np.where(rng.random(l + 1) < 0.4, 0.0, rng.uniform(0.2, 0.9, l + 1))
        rate[0] = ((v // 4) % 2) if v % 4 == 3 else rng.uniform(0.2, 0.9)
        K[v] = rng.random(N) < rate[cluster_of]
    break_full_clusters(cluster_of, l, K, rng)                       # (every row well_conditioned)
    K[0] = 0
    if V > 1:
        K[1] = 1
    return cluster_of, K


def check_rows(got, dense, cond=None, l=None, delta=None, cnt=None, loose_max=None):
    """The agreement rule.  got: the device's indices (-1: None); dense: per row None or (argmax, max, {index: wald} of the indices that
    reach FIXTURE_NEAR of the maximum, or the full array).  -1 matches None exactly; else wald_dense[g] >= max (1 - DELTA); at most 10 % of
    the rows may pass with g != argmax.  cond[i] False: a row that is not well_conditioned -- the answer only has to be None or one of the
    l columns, and in all no more of them than loose_max may differ from the yardstick about None.  cnt[i] = (n_c, s_c) of the row: clusters of the same size with the same carriers have the same Wald value in exact
    arithmetic (and bit for bit in the reduced form), so which of them an argmax names is rounding noise of the implementation; a row whose
    g is such a twin of the argmax is held to the bound but not counted among the 10 %.
    -> (rows that agree through the tolerance, ill-conditioned rows that differ from the yardstick)."""
    delta = DELTA if delta is None else delta
    tied = loose = nc = 0
    for i, (g, d) in enumerate(zip(got, dense)):
        g = int(g)
        if cond is not None and not cond[i]:
            assert -1 <= g < l, "row %d: got %d" % (i, g)
            loose += (d is None) != (g < 0)
            continue
        nc += 1
        if d is None or g < 0:
            assert d is None and g < 0, "row %d: got %r, want %r" % (i, g, d if d is None else d[0])
            continue
        am, mx, near = d
        if g == am:
            continue
        wg = near.get(g, -np.inf) if isinstance(near, dict) else near[g]
        assert wg >= mx * (1 - delta), "row %d: got %d (wald %r), argmax %d (wald %r)" % (i, g, wg, am, mx)
        twin = cnt is not None and cnt[i][0][g + 1] == cnt[i][0][am + 1] and cnt[i][1][g + 1] == cnt[i][1][am + 1]
        tied += not twin
    assert tied <= 0.1 * nc, "%d of %d rows agree only through the tolerance" % (tied, nc)
    assert loose_max is None or loose <= loose_max, "%d ill-conditioned rows differ from the yardstick about None, at most %g may" % (loose, loose_max)
    return tied, loose


def loose_bound(cnt, cond, dense):
    """On how many rows that are not well_conditioned an implementation may differ from `dense` (per row None or a tuple) about None.
    (Which column wins on such a row that does fit is noise altogether -- Wald values ~ 1e-3 thrown about by the pole, the two numpy forms
    name different columns on most of them -- so there only a column is asked for.)  None or not is decided by rounding noise on few of
    them: most hold several clusters of carriers only, and one that saturates is enough.  A third implementation differs from the yardstick
    about as often as the reduced numpy form -- the same arithmetic as the kernel, on the CPU -- does on the very same rows: that count,
    times 1.5, plus 3 for the spread of a small count (two standard deviations of a Poisson count of 2)."""
    n = 0
    for c, ok, d in zip(cnt, cond, dense):
        if not ok:
            a = argmax_counts(*c)
            n += (a is None) != (d is None)
    return 1.5 * n + 3


def dense_rows(lin, K):
    """check_rows' `dense` from wald_dense itself."""
    out = []
    for k in K:
        w = wald_dense(lin, k)
        out.append(None if w is None else (int(np.argmax(w)), float(w[int(np.argmax(w))]), w))
    return out


def fixture_rows(N, l, tame=False):
    """check_rows' `dense` for a case of YARDSTICK_CASES from tests/golden/lincounts_dense.npz (wald_dense of every row, made by
    `python -m tests._lineage_ref`; l = 1000 takes seconds per row), and the case's largest Wald difference between the forms."""
    d = np.load(FIXTURE)
    t = ("tame_" if tame else "") + "N%d_l%d_" % (N, l)
    none, am, mx, off, idx, val = (d[t + f] for f in ("none", "argmax", "max", "near_off", "near_idx", "near_val"))
    out = []
    for v in range(len(none)):
        if none[v]:
            out.append(None)
        else:
            out.append((int(am[v]), float(mx[v]), {int(a): float(b) for a, b in zip(idx[off[v]:off[v + 1]], val[off[v]:off[v + 1]])}))
    return out, float(d[t + "wald_diff"])


def wald_diff(wd, wc):
    """Largest relative difference of the two forms' Wald values over the clusters that can decide the answer: those whose dense value
    reaches FIXTURE_NEAR of the row's maximum.  wd: the dense values, an array or the fixture's {index: value}."""
    if wd is None or wc is None:
        return 0.0
    if isinstance(wd, dict):
        idx = np.array(sorted(wd)); wd = np.array([wd[i] for i in idx]); wc = np.asarray(wc)[idx]
    with np.errstate(all="ignore"):
        ok = np.isfinite(wd) & np.isfinite(wc) & (wd > 0)
        if not ok.any():
            return 0.0
        near = ok & (wd >= wd[ok].max() * FIXTURE_NEAR)
        return float(np.max(np.abs(wd[near] - wc[near]) / wd[near]))


def _make_row(args):
    N, l, v, tame = args
    cluster_of, K = yardstick_case(N, l, tame=tame)
    lin = design(cluster_of, l)
    wd = wald_dense(lin, K[v])
    n_c, s_c = counts(cluster_of, l, K[v])
    wc = wald_counts(n_c, s_c)
    if wd is None:
        return (N, l, v, True, -1, np.nan, np.zeros(0, int), np.zeros(0), 0.0, wc is None)
    am = int(np.argmax(wd)); mx = float(wd[am])
    near = np.flatnonzero(~(wd < mx * FIXTURE_NEAR))
    return (N, l, v, False, am, mx, near, wd[near], wald_diff(wd, wc), wc is not None)


def make_fixture(procs=8, kinds=(False, True)):
    import multiprocessing as mp
    out = dict(np.load(FIXTURE)) if os.path.exists(FIXTURE) else {}
    for tame in kinds:
        jobs = [(N, l, v, tame) for (N, l) in reversed(YARDSTICK_CASES) for v in range(YARDSTICK_ROWS)]
        with mp.Pool(procs) as pool:
            rows = pool.map(_make_row, jobs, chunksize=1)
        for (N, l) in YARDSTICK_CASES:
            t = ("tame_" if tame else "") + "N%d_l%d_" % (N, l)
            rs = sorted([r for r in rows if r[0] == N and r[1] == l], key=lambda r: r[2])
            print(t, "rows on which the forms differ in None:", [r[2] for r in rs if not r[9]], flush=True)
            out[t + "none"] = np.array([r[3] for r in rs])
            out[t + "argmax"] = np.array([r[4] for r in rs], dtype=np.int32)
            out[t + "max"] = np.array([r[5] for r in rs])
            out[t + "near_off"] = np.concatenate([[0], np.cumsum([len(r[6]) for r in rs])]).astype(np.int64)
            out[t + "near_idx"] = np.concatenate([r[6] for r in rs]).astype(np.int32)
            out[t + "near_val"] = np.concatenate([r[7] for r in rs]).astype(np.float64)
            out[t + "wald_diff"] = np.float64(max(r[8] for r in rs))
            print(t, "None rows", int(out[t + "none"].sum()), "near entries", len(out[t + "near_idx"]), "wald diff", out[t + "wald_diff"], flush=True)
        np.savez_compressed(FIXTURE, **out)


if __name__ == "__main__":
    make_fixture()
