"""The LMM's per-variant linear kernels at every covariate width, in the shipped configuration (automatic limb count, default tolerance).
sh_lmm_setup pads the rank r of the covariate panel (intercept included) to DP in {0, 4, 8, 16, 32} and shk_lmm_linear picks a kernel from
(DP, continuous): k_lmm_linear_tab, k_lmm_linear_tabn<4 .. 12>, k_lmm_linear<16>, k_lmm_linear<32>.  Every reachable instantiation runs
here at both ends of its rank range, at sample counts that are no multiple of 4 or 64, on V = 300 rows (tests/_lmm_sweep.py): allele
frequencies 0.02 .. 0.98, an eighth of them majority-carrier rows (stored complemented), a row equal to the binary covariate and one equal to
its complement (rotate() zeroes them, lmm_cov.py:179-181: the table kernels' cancellation re-walk, the per-sample kernels' direct residual),
an all-zero and an all-one row.

Asserted per case: beta, bse, frac_h2, p against the oracle at the tolerances of tests/test_lmm_gpu.py; NaN and inf patterns exactly; the
edge rows bit-equal to the oracle's (beta 0, bse inf, p 1); the prefilter p-value and the bad-chisq note of EVERY row (the Welch sums ride in
the same tables); and the maximum relative deviation of every field under a ceiling of its own.  The oracle is held to a longdouble
restatement at these widths by tests/test_lmm_sweep_helpers_cpu.py (beta 1.5e-12, bse 1.6e-15).

Set-up edges (N = 300): 33 independent columns refused, 34 columns of rank 32 fitted; a numerically dependent column dropped with the
degrees of freedom still from the column count; an indefinite Sd (k_syrk_f64's sgn = -1 branch); h2 = 0.

Measured maxima of the first GPU run (relative; CEIL = 10x these rounded up, never above 1e-6; the run's lines: profiles/r17/lmm_sweep.txt):
  N65-D1-bin           beta 6.81e-10  bse 3.1e-10  frac_h2 3.41e-10  pvalue 3.08e-09
  N130-D1-cont         beta 3.42e-10  bse 1.7e-10  frac_h2 1.71e-10  pvalue 1.17e-09
  N257-D4-bin          beta 2.18e-10  bse 1.09e-10  frac_h2 1.09e-10  pvalue 7.98e-10
  N203-D3-cont         beta 2.96e-10  bse 1.48e-10  frac_h2 1.48e-10  pvalue 1.57e-09
  N301-D5-bin          beta 1.11e-11  bse 5.03e-13  frac_h2 1.11e-11  pvalue 6.38e-12
  N333-D8-bin          beta 2.04e-10  bse 1.02e-10  frac_h2 1.02e-10  pvalue 7.59e-10
  N190-D5-cont         beta 1.83e-12  bse 8.74e-13  frac_h2 9.14e-13  pvalue 8.31e-12
  N333-D8-cont         beta 2.05e-10  bse 1.02e-10  frac_h2 1.03e-10  pvalue 9.22e-10
  N200-D9-bin          beta 1.85e-12  bse 9.21e-13  frac_h2 9.92e-13  pvalue 3.94e-12
  N391-D16-cont        beta 8.33e-13  bse 4.13e-13  frac_h2 5.53e-13  pvalue 3.55e-12
  N391-D17-bin         beta 8.34e-13  bse 4.22e-13  frac_h2 6.58e-13  pvalue 6.63e-12
  N515-D24-bin         beta 3.1e-12  bse 5.16e-13  frac_h2 3.19e-12  pvalue 4.13e-12
  N640-D32-cont        beta 1.09e-12  bse 5.57e-13  frac_h2 6.04e-13  pvalue 3.48e-12
  N300-D34-rank32      beta 1.7e-12  bse 6.57e-13  frac_h2 1.69e-12  pvalue 3.66e-12
  N300-D6-rank5        beta 7.99e-12  bse 4.18e-13  frac_h2 7.84e-12  pvalue 5.04e-12
  N300-D3-indefinite   beta 2.12e-12  bse 1.06e-12  frac_h2 1.06e-12  pvalue 9.51e-12
  N300-D3-h2-0         beta 1.48e-12  bse 5.73e-13  frac_h2 1.25e-12  pvalue 5.58e-12"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _lmm_sweep import FIELDS, deviations, design, fmt, rows  # noqa: E402
from test_lmm_gpu import close  # noqa: E402

V = 300
H2 = 0.37

# id: (N, D, continuous)
CASES = {
    "N65-D1-bin": (65, 1, False),          # k_lmm_linear_tab
    "N130-D1-cont": (130, 1, True),        # k_lmm_linear_tabn<4>
    "N257-D4-bin": (257, 4, False),        # k_lmm_linear_tabn<6>
    "N203-D3-cont": (203, 3, True),        # k_lmm_linear_tabn<8>
    "N301-D5-bin": (301, 5, False),        # k_lmm_linear_tabn<10>
    "N333-D8-bin": (333, 8, False),        # k_lmm_linear_tabn<10>
    "N190-D5-cont": (190, 5, True),        # k_lmm_linear_tabn<12>
    "N333-D8-cont": (333, 8, True),        # k_lmm_linear_tabn<12>
    "N200-D9-bin": (200, 9, False),        # k_lmm_linear<16>
    "N391-D16-cont": (391, 16, True),      # k_lmm_linear<16>
    "N391-D17-bin": (391, 17, False),      # k_lmm_linear<32>
    "N515-D24-bin": (515, 24, False),      # k_lmm_linear<32>; the ragged-tile route under covariates (N = 4 x 128 + 3)
    "N640-D32-cont": (640, 32, True),      # k_lmm_linear<32>
}

# id: (D, h2, design keywords)
EDGES = {
    "N300-D34-rank32": (34, H2, dict(dup=((31, 1, 1.0), (32, 2, 2.0)))),
    "N300-D6-rank5": (6, H2, dict(dup=((2, 1, 3.0),))),
    "N300-D3-indefinite": (3, 0.6, dict(indefinite=True)),
    "N300-D3-h2-0": (3, 0.0, {}),
}

# per case and field: 10x the first measured maximum, rounded up, never above 1e-6
CEIL = {
    "N65-D1-bin": {"beta": 7e-9, "bse": 4e-9, "frac_h2": 4e-9, "pvalue": 4e-8},
    "N130-D1-cont": {"beta": 4e-9, "bse": 2e-9, "frac_h2": 2e-9, "pvalue": 2e-8},
    "N257-D4-bin": {"beta": 3e-9, "bse": 2e-9, "frac_h2": 2e-9, "pvalue": 8e-9},
    "N203-D3-cont": {"beta": 3e-9, "bse": 2e-9, "frac_h2": 2e-9, "pvalue": 2e-8},
    "N301-D5-bin": {"beta": 2e-10, "bse": 6e-12, "frac_h2": 2e-10, "pvalue": 7e-11},
    "N333-D8-bin": {"beta": 3e-9, "bse": 2e-9, "frac_h2": 2e-9, "pvalue": 8e-9},
    "N190-D5-cont": {"beta": 2e-11, "bse": 9e-12, "frac_h2": 1e-11, "pvalue": 9e-11},
    "N333-D8-cont": {"beta": 3e-9, "bse": 2e-9, "frac_h2": 2e-9, "pvalue": 1e-8},
    "N200-D9-bin": {"beta": 2e-11, "bse": 1e-11, "frac_h2": 1e-11, "pvalue": 4e-11},
    "N391-D16-cont": {"beta": 9e-12, "bse": 5e-12, "frac_h2": 6e-12, "pvalue": 4e-11},
    "N391-D17-bin": {"beta": 9e-12, "bse": 5e-12, "frac_h2": 7e-12, "pvalue": 7e-11},
    "N515-D24-bin": {"beta": 4e-11, "bse": 6e-12, "frac_h2": 4e-11, "pvalue": 5e-11},
    "N640-D32-cont": {"beta": 2e-11, "bse": 6e-12, "frac_h2": 7e-12, "pvalue": 4e-11},
}


def _fit_and_compare(tag, N, D, cont, h2, kw):
    """One engine run against the oracle: everything that is asserted for every configuration; returns the deviations."""
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine, pack_variants
    orc.set_threads(min(16, len(os.sched_getaffinity(0))))
    U, S, covar, y = design(N, D, 1000 + N + D, cont, **kw)
    Kv, special = rows(N, V, 2000 + N + D, covar)
    assert set(special) == ({"zero", "one", "span", "cospan"} if D >= 2 else {"zero", "one"})
    want = orc.LmmOracle(U, S, y, covar).block(h2, Kv.astype(float))
    e = Engine(N)
    e.lmm_setup(U, S, y, covar, h2, continuous=cont)
    r = e.lmm_batch(pack_variants(Kv)); info = e.lmm_info()
    e.close()
    devs = deviations(r, want)                                     # NaN and inf patterns exactly, on every row
    print("LMM-SWEEP widths %-20s %s  n_limbs %d extra_limbs %d bound_typical %.3g bound_max %.3g refined %d"
          % (tag, fmt(devs), info["n_limbs"], info["extra_limbs"], info["bound_rel_typical"], info["bound_rel_max_last_batch"],
             info["refined_last_batch"]))
    wb, ws, wf, wp = want
    close(r["beta"], wb, atol=1e-12, what="beta"); close(r["bse"], ws, what="bse")
    close(r["frac_h2"], wf, atol=1e-9, what="frac_h2"); close(r["pvalue"], wp, atol=1e-300, what="pvalue")
    edge = sorted(special.values())
    assert (wb[edge] == 0).all() and np.isposinf(ws[edge]).all() and (wp[edge] == 1.0).all()       # what the reference makes of a zeroed column
    for f, w in zip(FIELDS, want):
        assert np.array_equal(r[f][edge], w[edge]), (f, r[f][edge], w[edge])
    ordinary = np.setdiff1d(np.arange(V), edge)
    assert np.isfinite(ws[ordinary]).all() and np.isfinite(r["bse"][ordinary]).all()
    for v in range(V):
        pr, bad = orc.pre_filtering(y, Kv[v].astype(float), cont)
        close(r["prep"][v], pr, what="prep of row %d" % v); assert bool(r["flags"][v] & 4) == bad, v
    return devs, S


@pytest.mark.parametrize("cfg", list(CASES))
def test_every_linear_kernel_against_the_oracle_with_asserted_maxima(cfg):
    N, D, cont = CASES[cfg]
    devs, _ = _fit_and_compare(cfg, N, D, cont, H2, {})
    assert cfg in CEIL, "no ceilings for %s: measured %s" % (cfg, fmt(devs))
    for f in FIELDS:
        assert CEIL[cfg][f] <= 1e-6 and devs[f] <= CEIL[cfg][f], (cfg, f, devs[f], CEIL[cfg][f])


def test_more_than_32_independent_covariates_are_refused():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine
    U, S, covar, y = design(300, 33, 1333, False)
    e = Engine(300)
    with pytest.raises(_abi.SeerHipError, match="more than 32 independent covariates"):
        e.lmm_setup(U, S, y, covar, H2)
    e.close()


@pytest.mark.parametrize("cfg", list(EDGES))
def test_setup_edges_against_the_oracle(cfg):
    D, h2, kw = EDGES[cfg]
    devs, S = _fit_and_compare(cfg, 300, D, False, h2, kw)
    if kw.get("indefinite"):
        assert (h2 * S + 1.0 - h2).min() < -0.1                    # an eigenvalue of the rotated covariance is negative
    if kw.get("dup"):
        # the dependent columns are really dependent: the panel's rank is below its column count, which the degrees of freedom keep
        covar = design(300, D, 1000 + 300 + D, False, **kw)[2]
        assert np.linalg.matrix_rank(covar) == D - len(kw["dup"])
