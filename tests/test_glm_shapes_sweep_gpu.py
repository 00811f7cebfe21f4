"""The fixed-effects engine against the oracle away from the tuned shape of tests/test_glm_sweep_gpu.py (q = 10, N = 1000 / 5000): every
layout of the product table (q = 0 .. 14: which z columns fit behind the q(q+1)/2 products in the 32-column blocks; q = 0 has no chord
rounds), odd sample counts and sample counts one past / at a power of two (the packed records' odd last sample, the partial last 16-sample
group of the f16 MFMA operands, the partial last 64-bit word), a covariate offset by thousands (the fast phase iterates on standardised
columns), the OLS path (k_glm_ols_tab) with and without the prefilter, and the run-time-width designs (15 <= q <= 32, glm_wide.hip).
Rows: tests/_glm_sweep.py (uniform, U-shaped and strong-effect rows + the tail rows whose carriers are the last samples); default routes.

What is asserted for each configuration (tests/_glm_sweep.py): notes bit-exact (the oracle's firth-fails excepted, each of them carrying
SH_FLAG_FIRTH_SENSITIVE), prefilter and filter bits bit-exact, the p-value within 1e-6 relative (through the statistic inside the
log-likelihoods' noise), Firth-routed rows by tests/_firth_tol.py; and over the Newton-fitted (or OLS) rows the maximum relative deviation
of kbeta, intercept, bse, betas and the p-value held to a ceiling of its own, and the tail and strong-effect rows present.

Measured maxima of the first GPU run (relative; the ceilings in CEIL are 10x these rounded up, never above 1e-6; the run's output:
profiles/r06/glm_shapes_sweep.txt):
  bin-N1999-q0             kbeta 1.44e-10  intercept 3.51e-12  bse 2.74e-07  pvalue 3.57e-08
  bin-N1999-q1             kbeta 4.49e-09  intercept 2.02e-09  bse 2.17e-07  betas 7.48e-12  pvalue 1.2e-08
  bin-N1999-q2             kbeta 1.58e-10  intercept 4.05e-11  bse 8.2e-08  betas 1.19e-11  pvalue 1.77e-09
  bin-N1999-q3             kbeta 3.76e-10  intercept 4.03e-10  bse 6.62e-08  betas 8.47e-11  pvalue 1.2e-09
  bin-N1999-q7             kbeta 1.07e-10  intercept 2.12e-10  bse 1.02e-07  betas 3.97e-10  pvalue 1.15e-09
  bin-N1999-q8             kbeta 1.81e-10  intercept 1.28e-10  bse 8.67e-08  betas 1.07e-09  pvalue 1.18e-09
  bin-N1999-q11            kbeta 1.77e-10  intercept 2.52e-10  bse 8.87e-08  betas 8.93e-10  pvalue 1.34e-09
  bin-N1999-q14            kbeta 1.84e-10  intercept 1.45e-10  bse 8.32e-08  betas 1.58e-09  pvalue 1.55e-09
  bin-N1025-q10            kbeta 2.94e-10  intercept 2.92e-10  bse 1.44e-07  betas 2.58e-09  pvalue 4.68e-10
  bin-N2048-q10            kbeta 2.29e-10  intercept 1.48e-10  bse 9.65e-08  betas 2.25e-09  pvalue 1.99e-09
  bin-N4097-q10            kbeta 7.4e-10  intercept 4.95e-12  bse 1.21e-07  betas 1.26e-10  pvalue 3.99e-09
  bin-N5001-q3             kbeta 3.71e-10  intercept 2.21e-11  bse 1.02e-07  betas 1.39e-11  pvalue 4.6e-09
  bin-N5001-q14            kbeta 3.98e-10  intercept 1.28e-11  bse 1.11e-07  betas 1.38e-10  pvalue 4.93e-09
  bin-N3001-q6-offset      kbeta 6e-10  intercept 1.04e-09  bse 8.94e-08  betas 7.53e-11  pvalue 2.86e-09
  ols-N1999-q0             kbeta 2.82e-10  intercept 2.77e-12  bse 9.56e-14  pvalue 2.41e-11
  ols-N1999-q3             kbeta 1.75e-10  intercept 6.26e-12  bse 1.19e-14  betas 1.5e-12  pvalue 4.78e-12
  ols-N1999-q10            kbeta 1.25e-10  intercept 4.93e-12  bse 1.55e-14  betas 1.07e-12  pvalue 1.09e-11
  ols-N1999-q14            kbeta 1.73e-11  intercept 5.07e-13  bse 1.06e-14  betas 9.82e-13  pvalue 7.41e-12
  ols-N5001-q0             kbeta 9.1e-10  intercept 1.7e-12  bse 2.31e-13  pvalue 9.96e-11
  ols-N5001-q3             kbeta 5.89e-11  intercept 8.28e-13  bse 1.35e-14  betas 1.52e-12  pvalue 1.28e-11
  ols-N5001-q10            kbeta 1.18e-10  intercept 2.04e-12  bse 1.05e-14  betas 9.47e-13  pvalue 1.12e-10
  ols-N5001-q14            kbeta 1.66e-10  intercept 3.94e-12  bse 1.37e-14  betas 2.53e-12  pvalue 1.28e-10
  ols-N1999-q10-prefilter  kbeta 1.64e-11  intercept 3.95e-12  bse 1.43e-14  betas 9.69e-13  pvalue 1.08e-11
  wide-bin-N1999-q15       kbeta 4.64e-12  intercept 2.94e-13  bse 3.43e-14  betas 7.28e-13  pvalue 4e-10
  wide-bin-N1999-q20       kbeta 7.81e-12  intercept 4.96e-13  bse 4.03e-14  betas 5.59e-13  pvalue 6.03e-10
  wide-bin-N1999-q32       kbeta 2.14e-11  intercept 1.23e-13  bse 3.98e-14  betas 7.34e-13  pvalue 4.76e-10
  wide-ols-N1999-q15       kbeta 2.91e-11  intercept 2.77e-12  bse 6.63e-15  betas 3.49e-12  pvalue 1.02e-11
  wide-ols-N1999-q20       kbeta 3.16e-11  intercept 1.01e-12  bse 8.88e-15  betas 1.91e-12  pvalue 3.62e-12
  wide-ols-N1999-q32       kbeta 2.93e-11  intercept 3.16e-13  bse 7.63e-15  betas 1.48e-12  pvalue 1.03e-11
  wide-bin-N5001-q20       kbeta 5.4e-12  intercept 2.83e-13  bse 6.65e-14  betas 6.36e-13  pvalue 1.01e-09"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIELDS = ("kbeta", "intercept", "bse", "betas", "pvalue")

# id: (continuous, N, q, rows, offset column, pret, lrtt, seed)
CONFIGS = {
    "bin-N1999-q0": (False, 1999, 0, 1 << 16, False, 1.0, 1.0, 101),
    "bin-N1999-q1": (False, 1999, 1, 1 << 16, False, 1.0, 1.0, 102),
    "bin-N1999-q2": (False, 1999, 2, 1 << 16, False, 1.0, 1.0, 103),
    "bin-N1999-q3": (False, 1999, 3, 1 << 16, False, 1.0, 1.0, 104),
    "bin-N1999-q7": (False, 1999, 7, 1 << 16, False, 1.0, 1.0, 105),
    "bin-N1999-q8": (False, 1999, 8, 1 << 16, False, 1.0, 1.0, 106),
    "bin-N1999-q11": (False, 1999, 11, 1 << 16, False, 1.0, 1.0, 107),
    "bin-N1999-q14": (False, 1999, 14, 1 << 16, False, 1.0, 1.0, 108),
    "bin-N1025-q10": (False, 1025, 10, 1 << 16, False, 1.0, 1.0, 111),
    "bin-N2048-q10": (False, 2048, 10, 1 << 16, False, 1.0, 1.0, 112),
    "bin-N4097-q10": (False, 4097, 10, 1 << 16, False, 1.0, 1.0, 113),
    "bin-N5001-q3": (False, 5001, 3, 1 << 17, False, 1.0, 1.0, 121),
    "bin-N5001-q14": (False, 5001, 14, 1 << 17, False, 1.0, 1.0, 122),
    "bin-N3001-q6-offset": (False, 3001, 6, 1 << 16, True, 1.0, 1.0, 131),
    "ols-N1999-q0": (True, 1999, 0, 1 << 16, False, 1.0, 1.0, 141),
    "ols-N1999-q3": (True, 1999, 3, 1 << 16, False, 1.0, 1.0, 142),
    "ols-N1999-q10": (True, 1999, 10, 1 << 16, False, 1.0, 1.0, 143),
    "ols-N1999-q14": (True, 1999, 14, 1 << 16, False, 1.0, 1.0, 144),
    "ols-N5001-q0": (True, 5001, 0, 1 << 16, False, 1.0, 1.0, 145),
    "ols-N5001-q3": (True, 5001, 3, 1 << 16, False, 1.0, 1.0, 146),
    "ols-N5001-q10": (True, 5001, 10, 1 << 16, False, 1.0, 1.0, 147),
    "ols-N5001-q14": (True, 5001, 14, 1 << 16, False, 1.0, 1.0, 148),
    "ols-N1999-q10-prefilter": (True, 1999, 10, 1 << 16, False, 0.3, 0.2, 151),
    "wide-bin-N1999-q15": (False, 1999, 15, 1 << 14, False, 1.0, 1.0, 161),
    "wide-bin-N1999-q20": (False, 1999, 20, 1 << 14, False, 1.0, 1.0, 162),
    "wide-bin-N1999-q32": (False, 1999, 32, 1 << 14, False, 1.0, 1.0, 163),
    "wide-ols-N1999-q15": (True, 1999, 15, 1 << 14, False, 1.0, 1.0, 164),
    "wide-ols-N1999-q20": (True, 1999, 20, 1 << 14, False, 1.0, 1.0, 165),
    "wide-ols-N1999-q32": (True, 1999, 32, 1 << 14, False, 1.0, 1.0, 166),
    "wide-bin-N5001-q20": (False, 5001, 20, 1 << 14, False, 1.0, 1.0, 171),
}

# OLS at q >= 10: the oracle's pinv (a one-sided Jacobi SVD per row) fits ~300 rows/s there.  Every row is held to
# tests/_glm_sweep.py:ols_reference (prefilter p-value, notes, prefilter and filter bits, values); the oracle sees the tail rows, every 16th
# other row and the rows within 1e-9 of a threshold, and on the rows both see the reference must give its notes and bits and its values to 1e-10
ORACLE_EVERY = 16

# per configuration and field: 10x the first measured maximum, rounded up, never above 1e-6
CEIL = {
    "bin-N1999-q0": {"kbeta": 2e-09, "intercept": 4e-11, "bse": 1e-06, "pvalue": 4e-07},
    "bin-N1999-q1": {"kbeta": 5e-08, "intercept": 3e-08, "bse": 1e-06, "betas": 8e-11, "pvalue": 2e-07},
    "bin-N1999-q2": {"kbeta": 2e-09, "intercept": 5e-10, "bse": 9e-07, "betas": 2e-10, "pvalue": 2e-08},
    "bin-N1999-q3": {"kbeta": 4e-09, "intercept": 5e-09, "bse": 7e-07, "betas": 9e-10, "pvalue": 2e-08},
    "bin-N1999-q7": {"kbeta": 2e-09, "intercept": 3e-09, "bse": 1e-06, "betas": 4e-09, "pvalue": 2e-08},
    "bin-N1999-q8": {"kbeta": 2e-09, "intercept": 2e-09, "bse": 9e-07, "betas": 2e-08, "pvalue": 2e-08},
    "bin-N1999-q11": {"kbeta": 2e-09, "intercept": 3e-09, "bse": 9e-07, "betas": 9e-09, "pvalue": 2e-08},
    "bin-N1999-q14": {"kbeta": 2e-09, "intercept": 2e-09, "bse": 9e-07, "betas": 2e-08, "pvalue": 2e-08},
    "bin-N1025-q10": {"kbeta": 3e-09, "intercept": 3e-09, "bse": 1e-06, "betas": 3e-08, "pvalue": 5e-09},
    "bin-N2048-q10": {"kbeta": 3e-09, "intercept": 2e-09, "bse": 1e-06, "betas": 3e-08, "pvalue": 2e-08},
    "bin-N4097-q10": {"kbeta": 8e-09, "intercept": 5e-11, "bse": 1e-06, "betas": 2e-09, "pvalue": 4e-08},
    "bin-N5001-q3": {"kbeta": 4e-09, "intercept": 3e-10, "bse": 1e-06, "betas": 2e-10, "pvalue": 5e-08},
    "bin-N5001-q14": {"kbeta": 4e-09, "intercept": 2e-10, "bse": 1e-06, "betas": 2e-09, "pvalue": 5e-08},
    "bin-N3001-q6-offset": {"kbeta": 6e-09, "intercept": 2e-08, "bse": 9e-07, "betas": 8e-10, "pvalue": 3e-08},
    "ols-N1999-q0": {"kbeta": 3e-09, "intercept": 3e-11, "bse": 1e-12, "pvalue": 3e-10},
    "ols-N1999-q3": {"kbeta": 2e-09, "intercept": 7e-11, "bse": 2e-13, "betas": 2e-11, "pvalue": 5e-11},
    "ols-N1999-q10": {"kbeta": 2e-09, "intercept": 5e-11, "bse": 2e-13, "betas": 2e-11, "pvalue": 2e-10},
    "ols-N1999-q14": {"kbeta": 2e-10, "intercept": 6e-12, "bse": 2e-13, "betas": 1e-11, "pvalue": 8e-11},
    "ols-N5001-q0": {"kbeta": 1e-08, "intercept": 2e-11, "bse": 3e-12, "pvalue": 1e-09},
    "ols-N5001-q3": {"kbeta": 6e-10, "intercept": 9e-12, "bse": 2e-13, "betas": 2e-11, "pvalue": 2e-10},
    "ols-N5001-q10": {"kbeta": 2e-09, "intercept": 3e-11, "bse": 2e-13, "betas": 1e-11, "pvalue": 2e-09},
    "ols-N5001-q14": {"kbeta": 2e-09, "intercept": 4e-11, "bse": 2e-13, "betas": 3e-11, "pvalue": 2e-09},
    "ols-N1999-q10-prefilter": {"kbeta": 2e-10, "intercept": 4e-11, "bse": 2e-13, "betas": 1e-11, "pvalue": 2e-10},
    "wide-bin-N1999-q15": {"kbeta": 5e-11, "intercept": 3e-12, "bse": 4e-13, "betas": 8e-12, "pvalue": 4e-09},
    "wide-bin-N1999-q20": {"kbeta": 8e-11, "intercept": 5e-12, "bse": 5e-13, "betas": 6e-12, "pvalue": 7e-09},
    "wide-bin-N1999-q32": {"kbeta": 3e-10, "intercept": 2e-12, "bse": 4e-13, "betas": 8e-12, "pvalue": 5e-09},
    "wide-ols-N1999-q15": {"kbeta": 3e-10, "intercept": 3e-11, "bse": 7e-14, "betas": 4e-11, "pvalue": 2e-10},
    "wide-ols-N1999-q20": {"kbeta": 4e-10, "intercept": 2e-11, "bse": 9e-14, "betas": 2e-11, "pvalue": 4e-11},
    "wide-ols-N1999-q32": {"kbeta": 3e-10, "intercept": 4e-12, "bse": 8e-14, "betas": 2e-11, "pvalue": 2e-10},
    "wide-bin-N5001-q20": {"kbeta": 6e-11, "intercept": 3e-12, "bse": 7e-13, "betas": 7e-12, "pvalue": 2e-08},
}


def _design(rng, N, q, offset):
    """One binary column (30 %), one age-like (50 +- 10) or -- offset -- a year (2000 +- 10), for q >= 15 a 6-level categorical one-hot
    encoded as the reference does it (5 columns), the rest standard normal."""
    W = rng.standard_normal((N, q))
    if q >= 1:
        W[:, 0] = rng.random(N) < 0.3
    if q >= 2:
        W[:, 1] = (2000 if offset else 50) + 10 * W[:, 1]
    if q >= 15:
        c = rng.integers(0, 6, N)
        W[:, 3:8] = (c[:, None] == np.arange(1, 6)[None, :])
    return W


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fixed_effects_shapes_against_the_oracle_with_asserted_maxima(cfg):
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine
    from pyseer_amd.model import fit_null
    from _glm_sweep import Sweep
    cont, N, q, V0, offset, pret, lrtt, seed = CONFIGS[cfg]
    V = int(os.environ.get("SEERHIP_SWEEP_ROWS", V0))
    orc.set_threads(max(1, min(os.cpu_count() or 4, len(os.sched_getaffinity(0)), 64)))
    rng = np.random.default_rng(seed)
    W = _design(rng, N, q, offset)
    eta = -0.5 + (0.9 * W[:, 0] if q >= 1 else 0.0) + (0.5 * W[:, 2] if q >= 3 else 0.0)
    y = eta + rng.standard_normal(N) if cont else (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(float)
    e0 = np.zeros((0, 0))
    Wn = W if q else e0
    nl = fit_null(y, Wn, e0, cont).llf
    nf = np.nan if cont else fit_null(y, Wn, e0, False, firth=True)
    e = Engine(N); e.glm_setup(y, W, cont, nl, nf, pret, lrtt)
    s = Sweep(e, y, W, cont, nl, nf, pret, lrtt, oracle_every=ORACLE_EVERY if cont and q >= 10 else 1).run(rng, V)
    e.close()
    print(s.summary("%s (N=%d q=%d %s)" % (cfg, N, q, "continuous" if cont else "binary")))
    assert s.rows >= V
    nchunks = -(-V // 32768)
    # the tail rows are there, and fitted by Newton / OLS (with the prefilter on, most of them are prefiltered)
    assert s.tail >= 80 * nchunks and s.tail_newton >= (40 if pret == 1.0 else 4) * nchunks, (s.tail, s.tail_newton)
    assert s.effect_rows >= 0.1 * (s.newton + s.firth_rows), (s.effect_rows, s.newton)
    if not cont:
        assert s.strong >= 0.1 * s.newton, (s.strong, s.newton)
    if pret < 1.0:
        assert 0 < s.prefiltered < s.rows
    assert s.oracle_fail <= 1e-4 * s.rows
    for f in FIELDS:
        if f == "betas" and q == 0:
            continue
        assert s.mx[f] <= CEIL[cfg][f], (f, s.mx[f], CEIL[cfg][f])
