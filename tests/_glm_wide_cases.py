"""Designs, rows and comparisons for the run-time-width fixed-effects kernels (15 <= q <= 32, csrc/glm_wide.hip) and the dense lineage fit
at its widest (17 <= 1 + lineages + covariates <= 50): tests/test_glm_wide_gpu.py runs them on the device, tests/test_glm_wide_cases_cpu.py
checks without one that the generator produces the row classes those tests rely on.  Test infrastructure.

Everything is a function of a seed; the seed of a case follows from its shape (seed_of), so no case depends on another.  Conditions a
case must meet -- the null model estimable, no Newton fit of the oracle on a numerically singular information matrix, Firth-routed rows
present, few oracle firth-fails, few rows on a halving tie -- are computed from the oracle's outputs alone and asserted by the CPU test;
where the default draw misses one, SEEDS or EDGE_ATTEMPT names another.

Row mix of a batch of V rows (rows_mix): 3/4 at uniform allele frequencies in [0.05, 0.95]; 1/8 rare, 0.4 % .. 2 % of the samples and never
fewer than one carrier (a binary phenotype routes some of those to Firth); 1/16 strong-effect rows; 1/16 of the tail rows of
tests/_glm_sweep.py (carriers exactly the last k samples, the last sample alone, every sample but the last few), spread evenly over its
kinds.  No row is empty or full."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _glm_sweep import FLOOR, STRONG, TAIL, rows as sweep_rows  # noqa: E402

UNIFORM, RARE = 0, 3                                   # row kinds beside _glm_sweep's STRONG and TAIL
FIELDS = ("kbeta", "intercept", "bse", "betas", "pvalue")

WIDTHS = tuple(range(15, 33))                          # every width of glm_wide.hip
EDGE_NS = (40, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 384)
EDGE_QS = (15, 32)
# (N, q, continuous) of the sample-count sweep that is left out: 33 covariate columns on 40 samples separate a binary phenotype on most draws
# (the Newton null fit ends in PerfectSeparation on 12 of 16 seeds).  The continuous case at N = 40 keeps 6 residual degrees of freedom and
# runs.  tests/test_glm_wide_cases_cpu.py shows for every (N, q, phenotype) whether the null model is estimable at the case's seed.
NOT_ESTIMABLE = ((40, 32, False),)
# binary cases whose first draw is no parity case: the null model's columns separate the phenotype (N = 64, 65 at q = 32), or quasi-separate
# it so that the oracle fits rows by Newton on a numerically singular information matrix (N = 40 at q = 15: numerically_singular_rows).  The
# first draw (seed + attempt) that is estimable and has no such row:
EDGE_ATTEMPT = {(40, 15, False): 1, (64, 32, False): 5, (65, 32, False): 1}
FORCED = ((130, 15, 192), (333, 23, 192), (320, 32, 192), (130, 15, 2304))       # (N, q, V) of the forced-Firth cases
DEGENERATE = tuple((200, q, cont) for q in EDGE_QS for cont in (False, True))
LINEAGE = ((15, 1), (16, 0), (44, 5), (49, 0), (46, 3))                          # (lineages, covariates): pc = 17, 17, 50, 50, 50
LINEAGE_REFUSED = (47, 3)                                                        # pc = 51
LINEAGE_N, LINEAGE_V = 600, 96

MAX_ORACLE_FAIL = 0.01       # share of a case's rows the oracle may call firth-fail
MAX_TIE = 0.05               # share of a case's Firth rows that may pass only through the tie detector
MAX_SEPARATED = 0.10         # share of a lineage case's rows the oracle may answer None

BASE = 20000
# case key -> seed where the default seed misses a condition.  The forced-Firth cases: the first seeds of a search (31000 + 100 a + q) at which
# the oracle fails at most MAX_ORACLE_FAIL of the rows and its own answers under its tie settings lie further apart than the tolerance on at
# most MAX_TIE of them -- both from the oracle's outputs alone.
SEEDS = {(3, 130, 15, 192): 31015, (3, 333, 23, 192): 35823, (3, 320, 32, 192): 31132, (3, 130, 15, 2304): 31016}


def seed_of(*key):
    if key in SEEDS:
        return SEEDS[key]
    s = BASE
    for k in key:
        s = s * 131 + int(k)
    return s % (1 << 31)


def threads():
    """The oracle's thread count, as the shapes sweep sets it, capped at 16."""
    from oracle import oracle as orc
    orc.set_threads(max(1, min(os.cpu_count() or 4, len(os.sched_getaffinity(0)), 16)))


def design(rng, N, q):
    """tests/test_glm_shapes_sweep_gpu.py _design for q >= 15: a 0/1 column (30 %), an age-like one (50 +- 10), a 6-level categorical
    one-hot encoded as the reference does it (columns 3..7), the rest standard normal."""
    assert q >= 15
    W = rng.standard_normal((N, q))
    W[:, 0] = rng.random(N) < 0.3
    W[:, 1] = 50 + 10 * W[:, 1]
    c = rng.integers(0, 6, N)
    W[:, 3:8] = (c[:, None] == np.arange(1, 6)[None, :])
    return W


def phenotype(rng, W, cont):
    N = W.shape[0]
    eta = -0.5 + 0.9 * W[:, 0] + 0.5 * W[:, 2]
    return eta + rng.standard_normal(N) if cont else (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(float)


def rows_mix(rng, V, N, y):
    """-> (K (V, N) uint8, kind (V,)): the mix of the module docstring, in the order uniform, rare, strong, tail."""
    assert V % 16 == 0
    nu, nr, ns, nt = 3 * V // 4, V // 8, V // 16, V // 16
    K = rng.random((nu, N)) < rng.uniform(0.05, 0.95, nu)[:, None]
    R = np.zeros((nr, N), bool)
    for r, af in zip(R, rng.uniform(0.004, 0.02, nr)):
        r[rng.choice(N, max(1, int(np.ceil(af * N))), replace=False)] = True
    hi = 0.05 + 0.8 * (y > np.median(y))
    S = rng.random((ns, N)) < hi[None, :] * rng.uniform(0.1, 1.0, ns)[:, None]
    T, tk = sweep_rows(rng, 0, N, y)
    assert (tk == TAIL).all()
    T = T[np.round(np.linspace(0, len(T) - 1, nt)).astype(int)].astype(bool)
    K = np.concatenate([K, R, S, T])
    kind = np.concatenate([np.full(nu, UNIFORM), np.full(nr, RARE), np.full(ns, STRONG), np.full(nt, TAIL)]).astype(np.int8)
    for i in np.flatnonzero(K.sum(axis=1) == 0):
        K[i, rng.integers(N)] = True
    for i in np.flatnonzero(K.sum(axis=1) == N):
        K[i, rng.integers(N)] = False
    return K.astype(np.uint8), kind


class Case(object):
    """One design with its phenotype, null fits and rows.  ok: the null model (and, binary, its Firth fit) could be estimated."""

    def __init__(self, seed, N, q, cont, V, pret=1.0, lrtt=1.0, force_firth=False):
        from pyseer_amd.model import fit_null
        self.seed, self.N, self.q, self.cont, self.V, self.pret, self.lrtt, self.force = seed, N, q, cont, V, pret, lrtt, force_firth
        rng = np.random.default_rng(seed)
        self.W = design(rng, N, q)
        self.y = phenotype(rng, self.W, cont)
        self.K, self.kind = rows_mix(rng, V, N, self.y)
        self.rng = rng
        e0 = np.zeros((0, 0))
        self.nl = self.nf = None
        self.ok = False
        if N <= q + 2 or (not cont and not 0 < self.y.sum() < N):
            return
        with np.errstate(all="ignore"):
            null = fit_null(self.y, self.W, e0, cont)
            if null is None or not np.isfinite(null.llf):
                return
            self.nl = null.llf
            self.nf = np.nan if cont else fit_null(self.y, self.W, e0, False, firth=True)
        self.ok = self.nf is not None

    def oracle(self, K=None):
        from oracle import oracle as orc
        K = self.K if K is None else K
        return orc.fixed_effects_batch(self.y, K.astype(float), self.W, self.cont, self.pret, self.lrtt, self.nl, self.nf)

    def oracle_variants(self, K):
        from oracle import oracle as orc
        return orc.firth_noise_variants(lambda: self.oracle(K))

    def firth_variants(self, K=None):
        from oracle import oracle as orc
        K = self.K if K is None else K
        return orc.firth_noise_variants(lambda: orc.firth_batch(self.y, K.astype(float), self.W))

    def engine(self):
        from pyseer_amd.engine import Engine
        e = Engine(self.N)
        e.set_dedup(False)
        e.glm_setup(self.y, self.W, self.cont, self.nl, self.nf, self.pret, self.lrtt, force_firth=self.force)
        return e


def width_case(q, cont, filtered=False):
    """Every width, N = 333 = 2 x 128 + 77 = 5 x 64 + 13: the last chunk of the workgroup kernels and the last word of the lane kernels ragged."""
    pret, lrtt = (0.3, 0.2) if filtered else (1.0, 1.0)
    return Case(seed_of(1, q, cont, filtered), 333, q, cont, 256, pret, lrtt)


def edge_case(N, q, cont, attempt=None):
    attempt = EDGE_ATTEMPT.get((N, q, cont), 0) if attempt is None else attempt
    return Case(seed_of(2, N, q, cont) + attempt, N, q, cont, 128)


def forced_case(N, q, V):
    """force_firth=True.  V = 2304 is longer than the grid of k_glm_wide_firth_blk (at most 2048 workgroups): rows 2048 .. 2303 are rows
    0 .. 255 in another order (case.perm: row 2048 + i is row case.perm[i])."""
    c = Case(seed_of(3, N, q, V), N, q, False, min(V, 2048), force_firth=True)
    c.perm = None
    if V > 2048:
        c.perm = np.random.default_rng(c.seed + 1).permutation(256)[:V - 2048]
        c.K = np.concatenate([c.K, c.K[c.perm]]); c.kind = np.concatenate([c.kind, c.kind[c.perm]]); c.V = V
    return c


# ---- degenerate rows -------------------------------------------------------------------------------------------------------------------

SINGULAR = ("covariate", "covariate complement", "one-hot column", "one-hot sum")
# Singular through the intercept (k = 1 - covariate, k = the sum of the one-hot columns): the duplicate of a column leaves the oracle's LU an
# exactly zero pivot (`matrix-inversion-error`, as the kernels' 4e-16 pivot rule has it), these leave it a pivot of rounding noise -- it then
# inverts, and reports `high-bse` or no note with a NaN standard error as the noise falls (numpy's inv on LAPACK would, too).  On these rows
# the note of the Newton fit is no parity target; the Firth fit behind it (pinv) is, wherever the oracle routes the row there.
COLLINEAR = ("covariate complement", "one-hot sum")


def degenerate_case(N, q, cont):
    """-> (case, names): case.K holds the named rows (rank-deficient designs first: SINGULAR), then eight ordinary ones."""
    c = Case(seed_of(4, N, q, cont), N, q, cont, 16)
    rng, y, W = c.rng, c.y, c.W
    hi = y > np.median(y) if cont else y == 1
    named = [("covariate", W[:, 0] == 1), ("covariate complement", W[:, 0] == 0), ("one-hot column", W[:, 4] == 1),
             ("one-hot sum", W[:, 3:8].sum(axis=1) == 1)]
    if not cont:
        named += [("phenotype", y == 1), ("phenotype complement", y == 0)]
    for cls, label in ((hi, "cases only"), (~hi, "controls only")):
        for m in (1, 2, 3):
            k = np.zeros(N, bool); k[rng.choice(np.flatnonzero(cls), m, replace=False)] = True
            named.append(("%s, %d" % (label, m), k))
    k = np.zeros(N, bool); k[rng.integers(N)] = True; named.append(("one carrier", k))
    k = np.ones(N, bool); k[rng.integers(N)] = False; named.append(("N - 1 carriers", k))
    ordinary = c.K[c.kind == UNIFORM][:8]
    c.K = np.concatenate([np.array([k for _, k in named]).astype(np.uint8), ordinary])
    c.V = c.K.shape[0]
    c.kind = np.full(c.V, UNIFORM, np.int8)
    return c, [n for n, _ in named] + ["ordinary"] * len(ordinary)


def design_rank(c, v):
    X = np.concatenate([np.ones((c.N, 1)), c.K[v][:, None].astype(float), c.W], axis=1)
    return int(np.linalg.matrix_rank(X)), X.shape[1]


# ---- wide lineage ----------------------------------------------------------------------------------------------------------------------

def lineage_case(nl, j, N=LINEAGE_N, V=LINEAGE_V):
    """MDS-like lineage columns (scaled to a largest magnitude of 1 as the reference scales them), not cluster indicators: the count route
    cannot take them.  Rows follow a logistic model on the columns, weak to strong.  -> (lin, cov or None, K)"""
    rng = np.random.default_rng(seed_of(5, nl, j))
    lin = rng.standard_normal((N, nl)); lin /= np.abs(lin).max(axis=0)
    cov = rng.standard_normal((N, j)) if j else None
    w = rng.standard_normal((V, nl)) * rng.uniform(0, 2, (V, 1))
    K = (rng.random((V, N)) < 1 / (1 + np.exp(-(lin @ w.T).T - rng.uniform(-1, 1, (V, 1))))).astype(np.uint8)
    return lin, cov, K


def lineage_oracle(lin, cov, K):
    from oracle import oracle as orc
    return [orc.lineage_effect(lin, cov, k.astype(float)) for k in K]


# ---- comparisons -----------------------------------------------------------------------------------------------------------------------

def close(a, b, rtol=1e-6, atol=0.0, what=""):
    a = np.atleast_1d(np.asarray(a, dtype=float)); b = np.atleast_1d(np.asarray(b, dtype=float))
    assert a.shape == b.shape, (a.shape, b.shape)
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))) | \
             (np.abs(a - b) <= atol + rtol * np.abs(b))
    assert ok.all(), "%s mismatch at %s: got %s want %s" % (what, np.argwhere(~ok)[:5].tolist(), a[~ok][:5], b[~ok][:5])


def oracle_classes(c, want):
    """Row classes from the oracle's notes alone: ofail (the oracle's firth-fail), firth (Firth-routed and fitted), plain (Newton / OLS
    fitted), and for each Firth row whether the tie detector fires on it (the oracle's own answer moves under its tie settings)."""
    notes = want["notes"]
    ofail = (notes & 0x40) != 0
    firth = ((notes & 0x7C) != 0) & ~ofail
    plain = ~firth & ~ofail & np.isfinite(want["kbeta"]) & np.isfinite(want["bse"])
    return ofail, firth, plain


COND_MAX = 1e13


def numerically_singular_rows(c, want):
    """Rows the oracle fits by Newton (binary phenotype) although the information matrix X^T W X at its solution has a 2-norm condition
    number above COND_MAX: a quasi-separated fit whose weights underflowed within the 35 iterations.  numpy's inv of such a matrix raises
    LinAlgError only on an exactly zero pivot, so whether the reference reports `matrix-inversion-error` there is LAPACK rounding; the
    oracle has its own LU, and the kernels call a final matrix singular once a pivot falls below 4e-16 of its largest entry (2.5e15 as a
    condition number; COND_MAX leaves two decades).  The cases are draws without such rows, so that notes can be held bit for bit."""
    from oracle import oracle as orc
    out = np.zeros(c.V, bool)
    if c.cont or c.force:
        return out
    _, _, plain = oracle_classes(c, want)
    start = np.zeros(c.q + 2); start[0] = np.log(c.y.mean() / (1 - c.y.mean()))
    for v in np.flatnonzero(plain):
        X = orc.design(c.K[v].astype(float), c.W)
        beta = orc.logit_newton(X, c.y, start)[1]
        mu = 1 / (1 + np.exp(-X @ beta))
        with np.errstate(all="ignore"):
            out[v] = not np.linalg.cond((X.T * (mu * (1 - mu))) @ X) <= COND_MAX
    return out


def tie_rows(variants, rows, rtol=1e-9, atol=1e-13):
    """Rows (of the mask `rows`) on which some tie setting moves one of the oracle's own statistics by more than rtol |value| + atol, or its
    status.  The defaults are the tie detector's (tests/_firth_tol.py); with rtol = 1e-6, atol = 1e-12 these are the rows on which the
    reference's own legitimate answers lie further apart than the tolerance, the rows that can need the detector at all."""
    base = variants[0]
    sens = np.zeros(int(rows.sum()), bool)
    with np.errstate(invalid="ignore"):
        for v in variants[1:]:
            for f in ("kbeta", "bse", "intercept"):
                b, w = base[f][rows], v[f][rows]
                sens |= ~((np.isnan(w) & np.isnan(b)) | (np.abs(w - b) <= rtol * np.abs(b) + atol))
            for f in ("notes", "status"):
                if f in base:
                    sens |= base[f][rows] != v[f][rows]
    return sens


def hold_fixed_effects(c, r, want=None, skip_pvalue=None, exclude=None):
    """Holds the engine's rows r of case c to the oracle:
      * notes (bits 0..8), prefilter and filter bits bit-exact -- except on rows the oracle calls firth-fail, its rounding-noise failures
        that this library fits: each of those must carry SH_FLAG_FIRTH_SENSITIVE, and their share is capped (MAX_ORACLE_FAIL);
      * Newton / OLS rows and prefiltered rows: prep, p-value, kbeta, bse, intercept, betas at rtol 1e-6 with atol 1e-12;
      * Firth-routed rows: kbeta, bse, intercept through firth_rows_close (1e-6 relative, the halving-tie slack only where the tie detector
        fires), prep and the p-value at 1e-6 relative -- the p-value not on the rows of skip_pvalue.
    Rows of `exclude` are the caller's: only their prep and prefilter bit are held here.
    -> dict(mx = the largest relative deviation per field over the Newton / OLS rows (as tests/_glm_sweep.py measures them), counts)."""
    from scipy.special import erfcinv
    from _firth_tol import firth_rows_close
    want = c.oracle() if want is None else want
    fl = r["flags"]
    ofail, firth, plain = oracle_classes(c, want)
    ex = np.zeros(c.V, bool) if exclude is None else exclude
    close(r["prep"][ex], want["prep"][ex], rtol=1e-6, atol=1e-300, what="prep")
    firth = firth & ~ex; plain = plain & ~ex
    diff = ((fl & 0x1FF) != want["notes"]) & ~ex
    bad = diff & ~ofail
    assert not bad.any(), ("notes differ", np.flatnonzero(bad)[:5], fl[bad][:5] & 0x1FF, want["notes"][bad][:5])
    assert (((fl >> 18) & 1)[ofail & diff] == 1).all(), "a row the oracle fails and this library fits does not carry SH_FLAG_FIRTH_SENSITIVE"
    assert ofail.sum() <= MAX_ORACLE_FAIL * c.V, ("oracle firth-fails", int(ofail.sum()), c.V)
    assert (((fl >> 16) & 1) == want["prefilter"]).all(), ("prefilter bits differ", np.flatnonzero(((fl >> 16) & 1) != want["prefilter"])[:5])
    fdiff = (((fl >> 17) & 1) != want["filter"]) & ~(ofail & diff) & ~ex
    assert not fdiff.any(), ("filter bits differ", np.flatnonzero(fdiff)[:5])
    rest = ~firth & ~(ofail & diff) & ~ex                                  # Newton / OLS rows, and the rows nobody fitted (NaN on both sides)
    for f in ("prep", "pvalue", "kbeta", "bse", "intercept"):
        close(r[f][rest], want[f][rest], rtol=1e-6, atol=1e-12, what=f)
    close(r["betas"][rest], want["betas"][rest], rtol=1e-6, atol=1e-12, what="betas")
    mx = {f: 0.0 for f in FIELDS}
    if plain.any():
        for f in ("kbeta", "intercept", "bse", "betas"):
            a, b = r[f][plain], want[f][plain]
            assert np.isfinite(a).all(), f
            mx[f] = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), FLOOR[f])))
        pg, pw = r["pvalue"][plain], want["pvalue"][plain]
        big = 2 * erfcinv(np.clip(pw, 1e-300, 1.0)) ** 2 > 1e-6           # (a statistic below that is compared through atol above)
        if big.any():
            mx["pvalue"] = float(np.max(np.abs(pg[big] - pw[big]) / np.maximum(pw[big], 1e-300)))
    ties = 0
    if firth.any():
        vs = c.oracle_variants(c.K[firth])
        allr = np.ones(int(firth.sum()), bool)
        need = np.zeros(int(firth.sum()), bool)
        for f in ("kbeta", "bse", "intercept"):
            good, _ = firth_rows_close(r[f][firth], vs, f, allr)
            assert good.all(), ("firth " + f, np.flatnonzero(firth)[~good][:5], r[f][firth][~good][:5], vs[0][f][~good][:5])
            strict, _ = firth_rows_close(r[f][firth], vs[:1], f, allr)
            need |= ~strict
        ties = int(need.sum())
        pf = firth.copy()
        if skip_pvalue is not None:
            pf &= ~skip_pvalue
        close(r["prep"][firth], want["prep"][firth], rtol=1e-6, atol=1e-300, what="prep (firth)")
        close(r["pvalue"][pf], want["pvalue"][pf], rtol=1e-6, atol=1e-300, what="pvalue (firth)")
    return dict(mx=mx, plain=int(plain.sum()), firth=int(firth.sum()), ofail=int(ofail.sum()), ties=ties,
                tail_plain=int((plain & (c.kind == TAIL)).sum()), prefiltered=int((want["prefilter"] != 0).sum()),
                filtered=int((want["filter"] != 0).sum()))


def hold_forced_firth(c, r, vs=None):
    """Every row through fit_firth, held to oracle.firth_batch as tests/test_fuzz_gpu.py test_forced_firth_random_configurations holds it,
    with tests/_firth_tol.py for the values: the failure bit equals status != 0; where the oracle converged, intercept, kbeta and bse
    through firth_rows_close, and the p-value recomputed from fitll and the Firth null at 5e-6 relative.  A row on which the oracle's own
    status or fitll moves under its tie settings may match any of them; such rows count as tie rows, and both caps are asserted."""
    from oracle import oracle as orc
    from _firth_tol import firth_rows_close
    vs = c.firth_variants() if vs is None else vs
    want = vs[0]
    V = c.V
    allr = np.ones(V, bool)
    failed = ((r["flags"] >> 6) & 1) == 1
    ofail = want["status"] != 0
    assert ofail.sum() <= MAX_ORACLE_FAIL * V, ("oracle firth-fails", int(ofail.sum()), V)
    sens = tie_rows(vs, allr)
    need = np.zeros(V, bool)

    def pvalue(w):
        with np.errstate(invalid="ignore"):
            lr = -2 * (c.nf - w["fitll"])
        return np.array([orc.chi2_sf1(x) if x > 0 else 1.0 for x in lr])

    def p_close(w):
        ok = (w["status"] == 0) & np.isfinite(w["fitll"])
        p = pvalue(w)
        with np.errstate(invalid="ignore"):
            return ~ok | (np.abs(r["pvalue"] - p) <= 5e-6 * p + 1e-300)
    st_ok = failed == ofail
    p_ok = p_close(want)
    for w in vs[1:]:
        alt_st = failed == (w["status"] != 0)
        need |= sens & ~st_ok & alt_st; st_ok = st_ok | (sens & alt_st)
        alt_p = p_close(w)
        need |= sens & ~p_ok & alt_p; p_ok = p_ok | (sens & alt_p)
    assert st_ok.all(), ("failure bit", np.flatnonzero(~st_ok)[:5], failed[~st_ok][:5], want["status"][~st_ok][:5])
    conv = ~failed & ~ofail & np.isfinite(want["fitll"])
    for f in ("intercept", "kbeta", "bse"):
        good, _ = firth_rows_close(r[f], vs, f, conv)
        assert good.all(), (f, np.flatnonzero(conv)[~good][:5], r[f][conv][~good][:5], want[f][conv][~good][:5])
        strict, _ = firth_rows_close(r[f], vs[:1], f, conv)
        need[np.flatnonzero(conv)[~strict]] = True
    assert (p_ok | ~conv).all(), ("pvalue", np.flatnonzero(~p_ok & conv)[:5], r["pvalue"][~p_ok & conv][:5], pvalue(want)[~p_ok & conv][:5])
    ties = int(need.sum())
    assert ties <= MAX_TIE * V, ("Firth rows that pass only through the tie detector", ties, V)
    mx = {}
    if conv.any():
        for f in ("kbeta", "intercept", "bse"):
            mx[f] = float(np.max(np.abs(r[f][conv & ~need] - want[f][conv & ~need]) / np.maximum(np.abs(want[f][conv & ~need]), FLOOR[f])))
        mx["betas"] = float(np.max(np.abs(r["betas"][conv & ~need] - want["betas"][conv & ~need])
                                   / np.maximum(np.abs(want["betas"][conv & ~need]), FLOOR["betas"])))
        p = pvalue(want)[conv & ~need]
        mx["pvalue"] = float(np.max(np.abs(r["pvalue"][conv & ~need] - p) / np.maximum(p, 1e-300)))
    return dict(mx=mx, firth=int(conv.sum()), ofail=int(ofail.sum()), ties=ties, sens=int(sens.sum()))


def summary(label, s):
    return "%s: %s; max relative deviation %s" % (label, ", ".join("%s %d" % (k, v) for k, v in s.items() if k != "mx"),
                                                  {k: float("%.3g" % v) for k, v in s["mx"].items()})


class OracleEngine(object):
    """Stands in for the engine with the oracle's own answers in the engine's layout (the CPU test runs the comparisons above on it)."""

    def __init__(self, c):
        self.c = c

    def glm_batch(self, bits):
        c = self.c
        K = np.unpackbits(bits, axis=1, bitorder="little")[:, :c.N]
        if c.force:
            from oracle import oracle as orc
            w = dict(orc.firth_batch(c.y, K.astype(float), c.W))
            with np.errstate(invalid="ignore"):
                lr = -2 * (c.nf - w["fitll"])
            w["pvalue"] = np.array([orc.chi2_sf1(x) if x > 0 else (1.0 if x == x else np.nan) for x in lr])
            w["flags"] = ((w["status"] != 0).astype(np.uint32) << 6)
            return w
        w = dict(c.oracle(K))
        w["flags"] = w["notes"].astype(np.uint32) | (w["prefilter"].astype(np.uint32) << 16) | (w["filter"].astype(np.uint32) << 17)
        return w
