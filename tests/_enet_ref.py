"""Test-side yardstick of the whole-genome elastic net: a plain numpy fp64 coordinate descent for

    gaussian:  1/2 sum_i w_i (y_i - b0 - x~_i.b)^2              + lambda [ (1-alpha)/2 |b|_2^2 + alpha |b|_1 ]
    binomial:  - sum_i w_i [ y_i eta_i - log(1 + exp(eta_i)) ]  + lambda [ (1-alpha)/2 |b|_2^2 + alpha |b|_1 ]

(weights normalised to sum 1, columns standardised with them, constant columns left out), with glmnet's stopping rule --
the largest xv_j delta_j^2 of a sweep below thresh x null deviance -- and the threshold as an argument: 1e-7 is glmnet's,
1e-12 the tight run, 1e-26 "the optimum".  Dense and slow on purpose; nothing of the product is used here.  The descent
runs on the Gram matrix of the active columns (covariance updates), so a coordinate step is one axpy over the active set;
the residual is rebuilt from the coefficients after every solve.

Also here: the seeded case generator that tests/golden/make_enet_golden.py and the GPU tests share (only seeds and
results are committed, never the matrices), the KKT residual, and the cross-validation figures of cv.glmnet (grouped)."""
import numpy as np

GAUSSIAN, BINOMIAL = 0, 1


# ------------------------------------------------------------------------------------------------------------------
def make_case(seed, N, P, continuous, n_cov=0, n_dup=0, reweight=False, n_folds=3, const_in_fold=False):
    """Seeded synthetic k-mer-like case: P 0/1 columns over N samples (rows of K are variants), n_dup of them copies of
    other columns with a few flipped bits (k-mers of one gene), a sparse true model, optional dense covariates, cluster
    weights, balanced folds; const_in_fold makes row 0 carried only by samples of fold 0 (constant once fold 0 is held out)."""
    rng = np.random.default_rng(seed)
    af = np.where(rng.random(P) < 0.7, rng.uniform(0.02, 0.15, P), rng.uniform(0.15, 0.5, P))
    K = (rng.random((P, N)) < af[:, None]).astype(np.uint8)
    for d in range(n_dup):
        src, dst = rng.integers(0, P // 2), P // 2 + d
        K[dst] = K[src]
        flip = rng.choice(N, size=max(1, N // 100), replace=False)
        K[dst, flip] ^= 1
    perm = rng.permutation(N)
    fold = np.empty(N, dtype=np.int32)
    fold[perm] = np.arange(N) % n_folds
    if const_in_fold:
        K[0] = 0
        K[0, np.nonzero(fold == 0)[0][:max(3, N // 50)]] = 1
    K[K.sum(1) == 0, 0] = 1                                           # no empty rows
    cov = rng.normal(size=(N, n_cov)) if n_cov else np.zeros((N, 0))
    truth = np.zeros(P)
    nz = rng.choice(P, size=min(10, P // 4), replace=False)
    truth[nz] = rng.normal(0, 1.0, nz.size)
    lin = K.T.astype(float) @ truth + (cov @ rng.normal(0, 0.5, n_cov) if n_cov else 0.0)
    if continuous:
        y = lin + rng.normal(0, 1.0, N)
    else:
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(lin - np.median(lin))))).astype(float)
    w = np.ones(N)
    if reweight:
        cl = rng.integers(0, max(2, N // 8), N)
        _, inv, cnt = np.unique(cl, return_inverse=True, return_counts=True)
        w = 1.0 / cnt[inv]
    return dict(K=K, y=y, w=w, cov=cov, fold=fold, n_folds=n_folds)


# ------------------------------------------------------------------------------------------------------------------
class Problem(object):
    """One weighted problem (the full fit, or a fold as its zero-weight form).  X: (N, PT) raw columns, covariates first."""

    def __init__(self, X, y, w, family, alpha):
        self.X, self.y, self.family, self.alpha = X, np.asarray(y, float), family, float(alpha)
        w = np.asarray(w, float)
        self.w = w / w.sum()
        self.m = self.w @ X
        tr = self.w > 0
        Xt = X[tr]
        const = (Xt == Xt[0]).all(axis=0)
        var = self.w @ (X * X) - self.m ** 2
        var = np.where(const, 0.0, np.maximum(var, 0.0))
        with np.errstate(divide="ignore"):
            self.sinv = np.where(var > 0, 1.0 / np.sqrt(var), 0.0)
        mu = float(self.w @ self.y)
        self.mu0 = mu
        if family == GAUSSIAN:
            self.b0_null = mu
            self.nulldev = float(self.w @ (self.y - mu) ** 2)
            self.thr_unit = self.nulldev
        else:
            self.b0_null = float(np.log(mu / (1 - mu)))
            self.nulldev = float(-2 * (mu * np.log(mu) + (1 - mu) * np.log(1 - mu)))
            self.thr_unit = 0.5 * self.nulldev                        # lognet's dev0 carries no factor 2
        self.PT = X.shape[1]

    def cols(self, A):
        return (self.X[:, A] - self.m[A]) * self.sinv[A]

    def eta(self, b0, beta):
        A = np.nonzero(beta)[0]
        return b0 + (self.cols(A) @ beta[A] if A.size else 0.0)

    def mu(self, eta):
        if self.family == GAUSSIAN:
            return eta
        return np.clip(1.0 / (1.0 + np.exp(-eta)), 1e-9, 1 - 1e-9)

    def grad(self, b0, beta):
        """x~_j . w (y - mu) for every column (0 for a left-out column), and the intercept's gradient."""
        q = self.w * (self.y - self.mu(self.eta(b0, beta)))
        return self.sinv * (q @ self.X - self.m * q.sum()), float(q.sum())

    def deviance(self, b0, beta):
        eta = self.eta(b0, beta)
        if self.family == GAUSSIAN:
            return float(self.w @ (self.y - eta) ** 2)
        return float(-2 * self.w @ (self.y * eta - np.logaddexp(0, eta)))

    def lambda_max(self):
        g, _ = self.grad(self.b0_null, np.zeros(self.PT))
        return float(np.max(np.abs(g))) / max(self.alpha, 1e-3)


def kkt_residual(prob, lam, b0, beta):
    """Largest violation of the optimality conditions at (b0, beta) on the standardised scale:
    b_j != 0: |g_j - lam (1-alpha) b_j - alpha lam sign(b_j)|;  b_j = 0: max(0, |g_j| - alpha lam);  the intercept: |sum w (y - mu)|."""
    g, g0 = prob.grad(b0, beta)
    al = prob.alpha
    nz = beta != 0
    res = np.where(nz, np.abs(g - lam * (1 - al) * beta - al * lam * np.sign(beta)), np.maximum(0.0, np.abs(g) - al * lam))
    res = np.where(prob.sinv > 0, res, 0.0)
    return max(float(res.max()), abs(g0)), g


def partial_gradient(prob, b0, beta):
    """u_j = g_j + xv_j b_j: the gradient of column j with its own term taken out, the quantity a coordinate step thresholds
    (j is selected iff |u_j| > alpha lambda; for b_j = 0 it is g_j itself).  xv_j = sum_i v_i x~_ij^2 at the solution's weights."""
    g, _ = prob.grad(b0, beta)
    if prob.family == GAUSSIAN:
        xv = (prob.sinv > 0).astype(float)
    else:
        p = prob.mu(prob.eta(b0, beta))
        v = prob.w * p * (1 - p)
        xv = prob.sinv ** 2 * (v @ (prob.X * prob.X) - 2 * prob.m * (v @ prob.X) + prob.m ** 2 * v.sum())
    return g + xv * beta


def _soft(u, t):
    a = abs(u) - t
    return (a if u > 0 else -a) if a > 0 else 0.0


def solve_point(prob, lam, lam_prev, b0, beta, active, thresh, max_sweeps=2000000):
    """Descend at one lambda from (b0, beta) with the ever-active set `active` (boolean, grown in place): strong rule,
    coordinate descent on the active list in index order, KKT check over all columns, until no column enters."""
    al = prob.alpha
    l1, l2 = al * lam, (1 - al) * lam
    thr = thresh * prob.thr_unit
    beta = beta.copy()
    usable = prob.sinv > 0
    g, _ = prob.grad(b0, beta)
    active |= usable & (np.abs(g) > al * (2 * lam - lam_prev))
    sweeps = 0
    while True:
        A = np.nonzero(active)[0]
        XA = prob.cols(A)
        b = beta[A].copy()
        for outer in range(100):
            eta = b0 + XA @ b
            if prob.family == BINOMIAL:
                p = prob.mu(eta)
                pq = p * (1 - p)
                v = prob.w * pq
                r = (prob.y - p) / pq
            else:
                v = prob.w
                r = prob.y - eta
            b0s, bs = b0, b.copy()
            if prob.family == BINOMIAL or outer == 0:
                G = XA.T @ (v[:, None] * XA)
                xv = np.diag(G).copy()
                sv = XA.T @ v
            SV = float(v.sum())
            q = XA.T @ (v * r)
            SVR = float(v @ r)
            conv = False
            while sweeps < max_sweeps:
                dlx = 0.0
                for k in range(A.size):
                    x = xv[k]
                    if not x > 0:
                        continue
                    bn = _soft(q[k] + x * b[k], l1) / (x + l2)
                    d = bn - b[k]
                    if d != 0.0:
                        b[k] = bn
                        q -= d * G[:, k]
                        SVR -= d * sv[k]
                        dlx = max(dlx, x * d * d)
                d = SVR / SV
                b0 += d
                q -= d * sv
                SVR = 0.0
                dlx = max(dlx, SV * d * d)
                sweeps += 1
                if dlx < thr:
                    conv = True
                    break
            if not conv:
                raise RuntimeError("no convergence")
            if prob.family == GAUSSIAN:
                break
            ch = max(SV * (b0 - b0s) ** 2, float(np.max(xv * (b - bs) ** 2)) if A.size else 0.0)
            if ch < thr:
                break
        else:
            raise RuntimeError("IRLS did not converge")
        beta[A] = b
        g, _ = prob.grad(b0, beta)
        viol = usable & ~active & (np.abs(g) > al * lam)
        if not viol.any():
            return b0, beta, sweeps
        active |= viol


def lambda_sequence(prob, n_lambda, ratio=None):
    lmax = prob.lambda_max()
    if ratio is None:
        ratio = 1e-2 if prob.X.shape[0] < prob.PT else 1e-4
    if n_lambda == 1:
        return np.array([lmax])
    return np.exp(np.log(lmax) + (np.log(lmax * ratio) - np.log(lmax)) * np.arange(n_lambda) / (n_lambda - 1))


def fit_path(prob, lambdas, thresh, starts=None, always_active=0, stop_early=False):
    """Solutions [(b0, beta)] down `lambdas` with warm starts (or from starts[l]: used to polish a looser path to the
    optimum, which does not depend on the start).  The first `always_active` columns (covariates) are always swept."""
    active = np.zeros(prob.PT, bool)
    active[:always_active] = prob.sinv[:always_active] > 0
    b0, beta = prob.b0_null, np.zeros(prob.PT)
    out, dr_prev = [], 0.0
    for l, lam in enumerate(lambdas):
        if starts is not None:
            b0, beta = starts[l]
            active |= beta != 0
        b0, beta, _ = solve_point(prob, lam, lambdas[l - 1] if l else lambdas[0], b0, beta, active, thresh)
        out.append((b0, beta.copy()))
        if stop_early:
            dr = 1 - prob.deviance(b0, beta) / prob.nulldev
            if l > 0 and (dr > 0.999 or (l + 1 >= min(5, len(lambdas)) and dr - dr_prev < 1e-5 * dr)):
                break
            dr_prev = dr
    return out


def design(case):
    """(N, n_cov + P) raw columns, covariates first."""
    return np.hstack([case["cov"], case["K"].T.astype(float)])


def problems(case, family, alpha, physically_removed=None):
    """The full problem and one per fold (zero weights for the held-out samples)."""
    X = design(case)
    out = [Problem(X, case["y"], case["w"], family, alpha)]
    for k in range(case["n_folds"]):
        out.append(Problem(X, case["y"], np.where(case["fold"] == k, 0.0, case["w"]), family, alpha))
    return out


def cv_figures(case, probs, sols, family):
    """cv.glmnet (grouped = TRUE): cvm[l] = weighted mean over folds of the fold's weighted mean held-out deviance,
    cvsd[l] = sqrt(weighted variance of the fold means / (F - 1)); binomial probabilities clamped to [1e-5, 1 - 1e-5]."""
    w = case["w"] / case["w"].sum()
    F, L = case["n_folds"], len(sols[0])
    fd, fw = np.zeros((F, L)), np.zeros(F)
    for k in range(F):
        held = case["fold"] == k
        fw[k] = w[held].sum()
        for l in range(L):
            b0, beta = sols[k + 1][l]
            eta = probs[k + 1].eta(b0, beta)
            if family == GAUSSIAN:
                dev = (case["y"] - eta) ** 2
            else:
                p = np.clip(1 / (1 + np.exp(-eta)), 1e-5, 1 - 1e-5)
                dev = -2 * (case["y"] * np.log(p) + (1 - case["y"]) * np.log(1 - p))
            fd[k, l] = (w[held] @ dev[held]) / fw[k]
    cvm = fw @ fd / fw.sum()
    cvsd = np.sqrt((fw @ (fd - cvm) ** 2 / fw.sum()) / (F - 1))
    return cvm, cvsd, fd


def to_original(prob, b0, beta):
    """Slopes b_j / s_j and the matching intercept."""
    bo = beta * prob.sinv
    return b0 - float(bo @ prob.m), bo


def to_standardised(prob, b0o, bo):
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = np.where(prob.sinv > 0, bo / prob.sinv, 0.0)
    return b0o + float(bo @ prob.m), beta
