"""The run-time-width fixed-effects kernels (15 <= q <= 32, csrc/glm_wide.hip) and the dense lineage fit at its widest, against the CPU
oracle in fp64 at their edges.  The workgroup kernels split their 256 threads by pc = q + 2 (the `tid < pc` loops, the sample groups G, the
3 x 3 tiles), walk the samples in chunks of WB_CH = 128, and stride a grid of at most 2048 workgroups over their lists; the lane kernels read
64-bit words with nb = min(64, N - sb * 64).  Cases and comparisons: tests/_glm_wide_cases.py (checked without a GPU by
tests/test_glm_wide_cases_cpu.py).

  test_every_wide_width_vs_oracle         every q = 15 .. 32, binary and continuous, N = 333 (ragged last chunk, ragged last word), and
                                          q = 19 with the prefilter and the LRT filter on: k_glm_wide (routing lists),
                                          k_glm_wide_newton_blk, k_glm_wide_firth_blk (the routed rows), k_glm_wide_ols
  test_wide_sample_count_edges_vs_oracle  q = 15 and 32 at N = 40 .. 384: no ragged chunk, a chunk of one sample, a single partial chunk,
                                          N just above pc; random bits behind sample N in the last word: the same kernels
  test_wide_forced_firth_vs_oracle        force_firth: whole batches through k_glm_wide_firth_blk, one of them (2304 rows) longer than its
                                          grid; its last 256 rows repeat the first 256 in another order and must equal them bit for bit
  test_wide_degenerate_rows_vs_oracle     variants that duplicate a 0/1 covariate, its complement, a one-hot column or the one-hot sum,
                                          the phenotype, carriers in one class only, one carrier, N - 1 carriers: k_glm_wide_firth_blk's
                                          hand-over of near-singular fits to k_glm_wide_firth (Jacobi pinv), k_glm_wide_ols' rank-deficient
                                          branch
  test_wide_lineage_limits_vs_oracle      k_glm_wide_lineage_blk at pc = 17 (the first width past the templates) and pc = 50 (the last),
                                          with covariates; pc = 51 is refused

Measured maxima of the first GPU run (relative, over the Newton / OLS rows; the run's output: profiles/r20/glm_wide_edges.txt): CEIL below
lists them per configuration and field next to their ceilings, 10x the measured figure rounded up, never above 1e-6.  Over all of them:
kbeta <= 1.65e-11, intercept <= 1.84e-12, bse <= 2.15e-13, betas <= 3.67e-11, p-value <= 5.43e-11.  bin-N64-q32 has no Newton row (33
columns on 64 samples: every row is routed to Firth), so no ceiling.  The forced-Firth cases have none either -- their rows are held by
tests/_firth_tol.py --; measured over their converged rows that needed no tie slack: kbeta <= 1.25e-11, bse <= 5.53e-14, p-value <=
2.88e-12, and 2 of 192 rows (N = 130, q = 15) passed only through the tie detector, none in the other three cases.
Singular designs (test_wide_degenerate_rows_vs_oracle): the duplicate of a column agrees with the oracle in its note and its Firth fit; a
variant singular through the intercept is `matrix-inversion-error` here and `high-bse` or no note (NaN standard error) in the oracle, whose
LU keeps a pivot of rounding noise; its Firth fit agrees to 3e-8 on three rows, on the one-hot sum at q = 32 kbeta is -0.01896635 here and
-0.01897019 in the oracle (3.8e-6, inside fit_firth's stop rule of 1e-4: the halvings there compare log-determinants of a singular matrix)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _glm_wide_cases as G  # noqa: E402

# per configuration and field: (ceiling, first measured maximum); a field that is not listed is held to 1e-6
CEIL = {
    "bin-N333-q15": {"kbeta": (7e-13, 6.16e-14), "intercept": (2e-12, 1.31e-13), "bse": (5e-14, 4.88e-15), "betas": (7e-13, 6.66e-14), "pvalue": (9e-11, 8.56e-12)},
    "ols-N333-q15": {"kbeta": (4e-11, 3.01e-12), "intercept": (5e-13, 4.22e-14), "bse": (1e-13, 9.69e-15), "betas": (2e-11, 1.75e-12), "pvalue": (3e-12, 2.54e-13)},
    "bin-N333-q16": {"kbeta": (2e-12, 1.23e-13), "intercept": (2e-12, 1.11e-13), "bse": (7e-14, 6.81e-15), "betas": (3e-12, 2.92e-13), "pvalue": (8e-11, 7.16e-12)},
    "ols-N333-q16": {"kbeta": (7e-12, 6.68e-13), "intercept": (4e-13, 3.76e-14), "bse": (2e-13, 1.01e-14), "betas": (4e-12, 3.61e-13), "pvalue": (2e-12, 1.94e-13)},
    "bin-N333-q17": {"kbeta": (2e-12, 1.48e-13), "intercept": (3e-12, 2.58e-13), "bse": (9e-14, 8.24e-15), "betas": (2e-12, 1.07e-13), "pvalue": (2e-10, 1.85e-11)},
    "ols-N333-q17": {"kbeta": (4e-12, 3.66e-13), "intercept": (5e-12, 4.45e-13), "bse": (2e-13, 1.03e-14), "betas": (3e-12, 2.46e-13), "pvalue": (3e-12, 2.16e-13)},
    "bin-N333-q18": {"kbeta": (3e-12, 2.34e-13), "intercept": (2e-12, 1.05e-13), "bse": (2e-13, 1.35e-14), "betas": (5e-13, 4.55e-14), "pvalue": (4e-10, 3.23e-11)},
    "ols-N333-q18": {"kbeta": (2e-11, 1.59e-12), "intercept": (6e-13, 5.02e-14), "bse": (9e-14, 8.29e-15), "betas": (6e-12, 5.8e-13), "pvalue": (2e-12, 1.65e-13)},
    "bin-N333-q19": {"kbeta": (5e-13, 4.63e-14), "intercept": (8e-13, 7.36e-14), "bse": (4e-14, 3.73e-15), "betas": (2e-12, 1.19e-13), "pvalue": (2e-10, 1.04e-11)},
    "ols-N333-q19": {"kbeta": (4e-11, 3.09e-12), "intercept": (2e-12, 1.28e-13), "bse": (9e-14, 8.37e-15), "betas": (6e-12, 5.6e-13), "pvalue": (3e-12, 2.19e-13)},
    "bin-N333-q20": {"kbeta": (2e-11, 1.04e-12), "intercept": (5e-13, 4.16e-14), "bse": (5e-14, 4.18e-15), "betas": (2e-12, 1.6e-13), "pvalue": (4e-11, 3.12e-12)},
    "ols-N333-q20": {"kbeta": (1e-11, 9.28e-13), "intercept": (2e-12, 1.53e-13), "bse": (9e-14, 8.05e-15), "betas": (3e-11, 2.38e-12), "pvalue": (2e-12, 1.59e-13)},
    "bin-N333-q21": {"kbeta": (2e-12, 1.62e-13), "intercept": (2e-13, 1.48e-14), "bse": (6e-14, 5.44e-15), "betas": (2e-11, 1.35e-12), "pvalue": (4e-11, 3.64e-12)},
    "ols-N333-q21": {"kbeta": (4e-11, 3.52e-12), "intercept": (2e-12, 1.14e-13), "bse": (1e-13, 9.24e-15), "betas": (9e-12, 8.74e-13), "pvalue": (2e-12, 1.52e-13)},
    "bin-N333-q22": {"kbeta": (2e-12, 1.59e-13), "intercept": (5e-14, 4.69e-15), "bse": (5e-14, 4.97e-15), "betas": (8e-12, 7.22e-13), "pvalue": (8e-11, 7.73e-12)},
    "ols-N333-q22": {"kbeta": (2e-11, 1.14e-12), "intercept": (4e-13, 3.55e-14), "bse": (1e-13, 9.37e-15), "betas": (8e-12, 7.46e-13), "pvalue": (3e-12, 2.37e-13)},
    "bin-N333-q23": {"kbeta": (1e-12, 9.07e-14), "intercept": (3e-13, 2.72e-14), "bse": (7e-14, 6.63e-15), "betas": (3e-12, 2.21e-13), "pvalue": (5e-11, 4.84e-12)},
    "ols-N333-q23": {"kbeta": (2e-11, 1.5e-12), "intercept": (3e-12, 2.61e-13), "bse": (1e-13, 9.44e-15), "betas": (2e-11, 1.38e-12), "pvalue": (2e-11, 1.26e-12)},
    "bin-N333-q24": {"kbeta": (2e-12, 1.65e-13), "intercept": (5e-14, 4.56e-15), "bse": (7e-14, 6.08e-15), "betas": (2e-12, 1.37e-13), "pvalue": (6e-11, 5.78e-12)},
    "ols-N333-q24": {"kbeta": (2e-11, 1.39e-12), "intercept": (2e-12, 1.66e-13), "bse": (9e-14, 8.79e-15), "betas": (8e-12, 7.09e-13), "pvalue": (2e-11, 1.17e-12)},
    "bin-N333-q25": {"kbeta": (6e-12, 5.13e-13), "intercept": (3e-13, 2.58e-14), "bse": (7e-14, 6.86e-15), "betas": (2e-12, 1.67e-13), "pvalue": (3e-10, 2.53e-11)},
    "ols-N333-q25": {"kbeta": (4e-12, 3.46e-13), "intercept": (6e-13, 5.86e-14), "bse": (1e-13, 9.72e-15), "betas": (2e-11, 1.9e-12), "pvalue": (2e-11, 1.31e-12)},
    "bin-N333-q26": {"kbeta": (3e-12, 2.17e-13), "intercept": (2e-12, 1.3e-13), "bse": (8e-14, 7.16e-15), "betas": (2e-12, 1.26e-13), "pvalue": (2e-10, 1.61e-11)},
    "ols-N333-q26": {"kbeta": (7e-12, 6.53e-13), "intercept": (5e-13, 4.58e-14), "bse": (9e-14, 8.31e-15), "betas": (4e-11, 3.4e-12), "pvalue": (3e-11, 2.42e-12)},
    "bin-N333-q27": {"kbeta": (9e-12, 8.34e-13), "intercept": (4e-12, 3.04e-13), "bse": (2e-13, 1.05e-14), "betas": (6e-12, 5.05e-13), "pvalue": (4e-10, 3.81e-11)},
    "ols-N333-q27": {"kbeta": (2e-11, 1.81e-12), "intercept": (3e-13, 2.6e-14), "bse": (1e-13, 1e-14), "betas": (5e-12, 4.31e-13), "pvalue": (2e-11, 1.26e-12)},
    "bin-N333-q28": {"kbeta": (2e-12, 1.45e-13), "intercept": (3e-12, 2.98e-13), "bse": (2e-13, 1.04e-14), "betas": (3e-12, 2.03e-13), "pvalue": (2e-10, 1.04e-11)},
    "ols-N333-q28": {"kbeta": (4e-12, 3.53e-13), "intercept": (7e-13, 6.28e-14), "bse": (1e-13, 9.11e-15), "betas": (3e-11, 2.2e-12), "pvalue": (2e-11, 1.33e-12)},
    "bin-N333-q29": {"kbeta": (4e-13, 3.24e-14), "intercept": (2e-13, 1.86e-14), "bse": (9e-14, 8.55e-15), "betas": (4e-12, 3.98e-13), "pvalue": (6e-10, 5.43e-11)},
    "ols-N333-q29": {"kbeta": (2e-11, 1.4e-12), "intercept": (8e-13, 7.23e-14), "bse": (2e-13, 1.04e-14), "betas": (6e-12, 5.79e-13), "pvalue": (2e-12, 1.86e-13)},
    "bin-N333-q30": {"kbeta": (2e-12, 1.6e-13), "intercept": (5e-12, 4.06e-13), "bse": (6e-14, 5.54e-15), "betas": (5e-12, 4.79e-13), "pvalue": (2e-10, 1.56e-11)},
    "ols-N333-q30": {"kbeta": (9e-11, 8.18e-12), "intercept": (2e-11, 1.47e-12), "bse": (2e-13, 1.15e-14), "betas": (2e-11, 1.89e-12), "pvalue": (3e-11, 2.34e-12)},
    "bin-N333-q31": {"kbeta": (2e-12, 1.81e-13), "intercept": (4e-14, 3.35e-15), "bse": (4e-14, 3.78e-15), "betas": (2e-12, 1.76e-13), "pvalue": (2e-10, 1.43e-11)},
    "ols-N333-q31": {"kbeta": (7e-12, 6.68e-13), "intercept": (4e-13, 3.61e-14), "bse": (8e-14, 7.95e-15), "betas": (1e-11, 9.29e-13), "pvalue": (2e-11, 1.22e-12)},
    "bin-N333-q32": {"kbeta": (2e-11, 1.3e-12), "intercept": (2e-12, 1.92e-13), "bse": (7e-14, 6.71e-15), "betas": (2e-12, 1.32e-13), "pvalue": (5e-10, 4.31e-11)},
    "ols-N333-q32": {"kbeta": (2e-11, 1.42e-12), "intercept": (2e-12, 1.64e-13), "bse": (8e-14, 7.56e-15), "betas": (7e-12, 6.24e-13), "pvalue": (2e-12, 1.44e-13)},
    "bin-N333-q19-filtered": {"kbeta": (3e-14, 2.21e-15), "intercept": (3e-13, 2.53e-14), "bse": (3e-14, 2.54e-15), "betas": (4e-12, 3.96e-13), "pvalue": (4e-12, 3.67e-13)},
    "ols-N333-q19-filtered": {"kbeta": (6e-13, 5.96e-14), "intercept": (8e-13, 7.67e-14), "bse": (3e-14, 2.34e-15), "betas": (9e-12, 8.15e-13), "pvalue": (3e-12, 2.45e-13)},
    "bin-N40-q15": {"kbeta": (3e-12, 2.17e-13), "intercept": (2e-13, 1.36e-14), "bse": (9e-13, 8.35e-14), "betas": (2e-11, 1.29e-12), "pvalue": (2e-12, 1.92e-13)},
    "ols-N40-q15": {"kbeta": (2e-12, 1.4e-13), "intercept": (5e-12, 4.78e-13), "bse": (4e-14, 3.32e-15), "betas": (5e-12, 4.99e-13), "pvalue": (2e-13, 1.59e-14)},
    "ols-N40-q32": {"kbeta": (2e-11, 1.77e-12), "intercept": (1e-11, 9.44e-13), "bse": (4e-13, 3.54e-14), "betas": (4e-10, 3.67e-11), "pvalue": (1e-12, 9.74e-14)},
    "bin-N64-q15": {"kbeta": (6e-13, 5.08e-14), "intercept": (7e-14, 6.08e-15), "bse": (7e-14, 6.26e-15), "betas": (7e-13, 6.07e-14), "pvalue": (5e-12, 4.13e-13)},
    "ols-N64-q15": {"kbeta": (7e-12, 6.59e-13), "intercept": (4e-12, 3.53e-13), "bse": (2e-14, 1.81e-15), "betas": (2e-11, 1.79e-12), "pvalue": (2e-13, 1.63e-14)},
    "ols-N64-q32": {"kbeta": (2e-10, 1.12e-11), "intercept": (5e-13, 4.89e-14), "bse": (7e-14, 6.06e-15), "betas": (2e-11, 1.99e-12), "pvalue": (9e-13, 8.14e-14)},
    "bin-N65-q15": {"kbeta": (3e-12, 2.97e-13), "intercept": (4e-13, 3.16e-14), "bse": (1e-13, 9.81e-15), "betas": (3e-12, 2.45e-13), "pvalue": (2e-10, 1.11e-11)},
    "ols-N65-q15": {"kbeta": (6e-12, 5.99e-13), "intercept": (5e-13, 4.7e-14), "bse": (3e-14, 2.32e-15), "betas": (2e-12, 1.9e-13), "pvalue": (3e-13, 2.83e-14)},
    "bin-N65-q32": {"kbeta": (1e-11, 9.87e-13), "intercept": (9e-14, 8.97e-15), "bse": (3e-12, 2.15e-13), "betas": (8e-12, 7.97e-13), "pvalue": (3e-11, 2.26e-12)},
    "ols-N65-q32": {"kbeta": (3e-12, 2.6e-13), "intercept": (7e-12, 6.92e-13), "bse": (2e-13, 1.21e-14), "betas": (2e-11, 1.34e-12), "pvalue": (2e-13, 1.74e-14)},
    "bin-N127-q15": {"kbeta": (3e-13, 2.43e-14), "intercept": (8e-14, 7.23e-15), "bse": (4e-14, 3.24e-15), "betas": (2e-12, 1.5e-13), "pvalue": (3e-12, 2.5e-13)},
    "ols-N127-q15": {"kbeta": (7e-12, 6.89e-13), "intercept": (2e-12, 1.67e-13), "bse": (2e-14, 1.53e-15), "betas": (6e-12, 5.08e-13), "pvalue": (5e-13, 4.32e-14)},
    "bin-N127-q32": {"kbeta": (3e-13, 2.94e-14), "intercept": (4e-13, 3.67e-14), "bse": (6e-14, 5.24e-15), "betas": (9e-12, 8.28e-13), "pvalue": (5e-12, 4.42e-13)},
    "ols-N127-q32": {"kbeta": (5e-12, 4.11e-13), "intercept": (3e-13, 2.34e-14), "bse": (3e-14, 2.7e-15), "betas": (2e-11, 1.34e-12), "pvalue": (4e-13, 3.41e-14)},
    "bin-N128-q15": {"kbeta": (2e-13, 1.98e-14), "intercept": (6e-12, 5.38e-13), "bse": (5e-14, 4.47e-15), "betas": (3e-12, 2.07e-13), "pvalue": (5e-12, 4.78e-13)},
    "ols-N128-q15": {"kbeta": (2e-12, 1.12e-13), "intercept": (6e-14, 5.92e-15), "bse": (2e-14, 1.97e-15), "betas": (6e-12, 5.31e-13), "pvalue": (4e-13, 3.04e-14)},
    "bin-N128-q32": {"kbeta": (2e-13, 1.94e-14), "intercept": (5e-13, 4.45e-14), "bse": (4e-14, 3.07e-15), "betas": (2e-12, 1.53e-13), "pvalue": (3e-11, 2.26e-12)},
    "ols-N128-q32": {"kbeta": (2e-10, 1.65e-11), "intercept": (6e-12, 5.06e-13), "bse": (4e-14, 3.48e-15), "betas": (2e-11, 1.08e-12), "pvalue": (6e-13, 5.76e-14)},
    "bin-N129-q15": {"kbeta": (2e-13, 1.56e-14), "intercept": (2e-12, 1.29e-13), "bse": (4e-14, 3.08e-15), "betas": (2e-12, 1.6e-13), "pvalue": (7e-12, 6.22e-13)},
    "ols-N129-q15": {"kbeta": (7e-13, 6.22e-14), "intercept": (6e-13, 5.78e-14), "bse": (2e-14, 1.76e-15), "betas": (2e-11, 1.12e-12), "pvalue": (5e-13, 4.72e-14)},
    "bin-N129-q32": {"kbeta": (2e-13, 1.39e-14), "intercept": (7e-14, 6.42e-15), "bse": (9e-14, 8.54e-15), "betas": (2e-11, 1.96e-12), "pvalue": (3e-12, 2.04e-13)},
    "ols-N129-q32": {"kbeta": (1e-11, 9.4e-13), "intercept": (2e-13, 1.94e-14), "bse": (4e-14, 3.26e-15), "betas": (7e-12, 6.65e-13), "pvalue": (8e-13, 7.13e-14)},
    "bin-N191-q15": {"kbeta": (4e-13, 3.64e-14), "intercept": (2e-13, 1.15e-14), "bse": (6e-14, 5.23e-15), "betas": (5e-13, 4.7e-14), "pvalue": (3e-11, 2.29e-12)},
    "ols-N191-q15": {"kbeta": (8e-12, 7.36e-13), "intercept": (7e-13, 6.96e-14), "bse": (3e-14, 2.15e-15), "betas": (2e-12, 1.14e-13), "pvalue": (2e-12, 1.16e-13)},
    "bin-N191-q32": {"kbeta": (2e-13, 1.79e-14), "intercept": (5e-13, 4.09e-14), "bse": (6e-14, 5.31e-15), "betas": (2e-12, 1.66e-13), "pvalue": (9e-12, 8.31e-13)},
    "ols-N191-q32": {"kbeta": (3e-12, 2.52e-13), "intercept": (2e-12, 1.6e-13), "bse": (3e-14, 2.15e-15), "betas": (1e-11, 9.92e-13), "pvalue": (7e-13, 6.69e-14)},
    "bin-N192-q15": {"kbeta": (4e-12, 3.58e-13), "intercept": (3e-12, 2.32e-13), "bse": (3e-14, 2.15e-15), "betas": (1e-12, 9.24e-14), "pvalue": (2e-10, 1.66e-11)},
    "ols-N192-q15": {"kbeta": (3e-12, 2.81e-13), "intercept": (6e-13, 5.28e-14), "bse": (2e-14, 1.97e-15), "betas": (4e-12, 3.86e-13), "pvalue": (7e-13, 6.58e-14)},
    "bin-N192-q32": {"kbeta": (5e-13, 4.41e-14), "intercept": (3e-12, 2.99e-13), "bse": (6e-14, 5.98e-15), "betas": (9e-13, 8.48e-14), "pvalue": (2e-11, 1.01e-12)},
    "ols-N192-q32": {"kbeta": (7e-12, 6.49e-13), "intercept": (2e-13, 1.98e-14), "bse": (3e-14, 2.57e-15), "betas": (1e-11, 9.42e-13), "pvalue": (7e-13, 6.76e-14)},
    "bin-N193-q15": {"kbeta": (2e-12, 1.15e-13), "intercept": (5e-13, 4.4e-14), "bse": (5e-14, 4.43e-15), "betas": (2e-12, 1.03e-13), "pvalue": (2e-11, 1.1e-12)},
    "ols-N193-q15": {"kbeta": (9e-13, 8.2e-14), "intercept": (3e-13, 2.36e-14), "bse": (3e-14, 2.3e-15), "betas": (2e-11, 1.19e-12), "pvalue": (8e-13, 7.98e-14)},
    "bin-N193-q32": {"kbeta": (4e-13, 3.2e-14), "intercept": (2e-12, 1.26e-13), "bse": (5e-14, 4.9e-15), "betas": (2e-12, 1.36e-13), "pvalue": (3e-11, 2.59e-12)},
    "ols-N193-q32": {"kbeta": (4e-12, 3.4e-13), "intercept": (9e-12, 8.14e-13), "bse": (3e-14, 2.28e-15), "betas": (2e-11, 1.03e-12), "pvalue": (6e-12, 5.05e-13)},
    "bin-N255-q15": {"kbeta": (2e-12, 1.63e-13), "intercept": (7e-12, 6.26e-13), "bse": (5e-14, 4.51e-15), "betas": (2e-12, 1.28e-13), "pvalue": (2e-11, 1.63e-12)},
    "ols-N255-q15": {"kbeta": (5e-12, 4.66e-13), "intercept": (2e-11, 1.84e-12), "bse": (2e-14, 1.92e-15), "betas": (3e-12, 2.59e-13), "pvalue": (6e-12, 5.56e-13)},
    "bin-N255-q32": {"kbeta": (4e-13, 3.49e-14), "intercept": (3e-12, 2.41e-13), "bse": (6e-14, 5.57e-15), "betas": (7e-13, 6.73e-14), "pvalue": (3e-11, 2.52e-12)},
    "ols-N255-q32": {"kbeta": (3e-12, 2.99e-13), "intercept": (3e-13, 2.49e-14), "bse": (3e-14, 2.22e-15), "betas": (1e-11, 9.38e-13), "pvalue": (2e-12, 1.35e-13)},
    "bin-N256-q15": {"kbeta": (7e-13, 6.12e-14), "intercept": (2e-13, 1.22e-14), "bse": (6e-14, 5.35e-15), "betas": (8e-13, 7.55e-14), "pvalue": (2e-10, 1.45e-11)},
    "ols-N256-q15": {"kbeta": (3e-11, 2.21e-12), "intercept": (5e-13, 4.4e-14), "bse": (2e-14, 1.62e-15), "betas": (7e-12, 6.97e-13), "pvalue": (6e-12, 5.73e-13)},
    "bin-N256-q32": {"kbeta": (3e-12, 2.18e-13), "intercept": (4e-14, 3.92e-15), "bse": (6e-14, 5.06e-15), "betas": (3e-12, 2.19e-13), "pvalue": (2e-10, 1.03e-11)},
    "ols-N256-q32": {"kbeta": (8e-12, 7.84e-13), "intercept": (3e-13, 2.77e-14), "bse": (3e-14, 2.64e-15), "betas": (2e-11, 1.53e-12), "pvalue": (7e-13, 6.64e-14)},
    "bin-N257-q15": {"kbeta": (3e-13, 2.6e-14), "intercept": (4e-14, 3.7e-15), "bse": (9e-14, 8.77e-15), "betas": (3e-12, 2.71e-13), "pvalue": (7e-11, 6.81e-12)},
    "ols-N257-q15": {"kbeta": (3e-12, 2.1e-13), "intercept": (6e-13, 5.43e-14), "bse": (3e-14, 2.84e-15), "betas": (1e-11, 9.24e-13), "pvalue": (6e-12, 5.99e-13)},
    "bin-N257-q32": {"kbeta": (3e-12, 2.94e-13), "intercept": (8e-12, 7.61e-13), "bse": (5e-14, 4.23e-15), "betas": (2e-12, 1.07e-13), "pvalue": (3e-10, 2.81e-11)},
    "ols-N257-q32": {"kbeta": (6e-12, 5.47e-13), "intercept": (7e-13, 6.29e-14), "bse": (3e-14, 2.53e-15), "betas": (2e-11, 1.66e-12), "pvalue": (6e-12, 5.68e-13)},
    "bin-N384-q15": {"kbeta": (6e-13, 5.81e-14), "intercept": (1e-12, 9.41e-14), "bse": (7e-14, 6.89e-15), "betas": (5e-13, 4.03e-14), "pvalue": (6e-11, 5.08e-12)},
    "ols-N384-q15": {"kbeta": (2e-11, 1.16e-12), "intercept": (5e-12, 4.69e-13), "bse": (3e-14, 2.24e-15), "betas": (2e-11, 1.41e-12), "pvalue": (3e-12, 2.31e-13)},
    "bin-N384-q32": {"kbeta": (9e-12, 8.96e-13), "intercept": (1e-12, 9.48e-14), "bse": (6e-14, 5.36e-15), "betas": (2e-12, 1.24e-13), "pvalue": (4e-10, 3.41e-11)},
    "ols-N384-q32": {"kbeta": (1e-11, 9.13e-13), "intercept": (5e-13, 4.28e-14), "bse": (4e-14, 3.36e-15), "betas": (2e-11, 1.02e-12), "pvalue": (2e-12, 1.8e-13)},
}


def _ceilings(cfg, s, fields=G.FIELDS):
    print(G.summary(cfg, s))
    for f in fields:
        if f in s["mx"]:
            ceil = CEIL.get(cfg, {}).get(f, (1e-6, None))[0]
            assert s["mx"][f] <= ceil, (cfg, f, s["mx"][f], ceil)


def _name(cont, N, q, extra=""):
    return "%s-N%d-q%d%s" % ("ols" if cont else "bin", N, q, extra)


def _run(c, bits=None):
    from pyseer_amd.engine import pack_variants
    e = c.engine()
    try:
        r = e.glm_batch(pack_variants(c.K) if bits is None else bits)
        return r, e.glm_info()
    finally:
        e.close()


WIDTH_CASES = [(q, cont, False) for q in G.WIDTHS for cont in (False, True)] + [(19, False, True), (19, True, True)]


@pytest.mark.parametrize("q,cont,filtered", WIDTH_CASES, ids=[_name(c, 333, q, "-filtered" if f else "") for q, c, f in WIDTH_CASES])
def test_every_wide_width_vs_oracle(q, cont, filtered):
    G.threads()
    c = G.width_case(q, cont, filtered)
    assert c.ok
    r, _ = _run(c)
    s = G.hold_fixed_effects(c, r)
    assert s["plain"] >= 64 and s["tail_plain"] >= 2, s
    if not cont:
        assert s["firth"] >= 8, s                                           # the rare rows did route to k_glm_wide_firth_blk
    if filtered:
        assert 32 <= s["prefiltered"] <= c.V - 32 and s["filtered"] >= 8, s
    _ceilings(_name(cont, 333, q, "-filtered" if filtered else ""), s)


EDGE_CASES = [(N, q, cont) for N in G.EDGE_NS for q in G.EDGE_QS for cont in (False, True) if (N, q, cont) not in G.NOT_ESTIMABLE]


@pytest.mark.parametrize("N,q,cont", EDGE_CASES, ids=[_name(c, N, q) for N, q, c in EDGE_CASES])
def test_wide_sample_count_edges_vs_oracle(N, q, cont):
    """The rows go in at the canonical width with random bits behind sample N in the last word: a tail read past N changes the answer."""
    from pyseer_amd.engine import pack_variants
    from pyseer_amd.packing import row_bytes_for
    from test_row_layout_gpu import relayout
    G.threads()
    c = G.edge_case(N, q, cont)
    assert c.ok
    rb = row_bytes_for(N)
    bits = relayout(pack_variants(c.K), N, rb, True, np.random.default_rng(c.seed + 7))
    assert np.array_equal(np.unpackbits(bits, axis=1, bitorder="little")[:, :N], c.K)
    if rb * 8 > N:
        assert not np.array_equal(bits, pack_variants(c.K)[:, :rb])
    r, _ = _run(c, bits)
    s = G.hold_fixed_effects(c, r)
    assert s["plain"] + s["firth"] >= c.V // 2, s
    _ceilings(_name(cont, N, q), s)


@pytest.mark.parametrize("N,q,V", G.FORCED)
def test_wide_forced_firth_vs_oracle(N, q, V):
    G.threads()
    c = G.forced_case(N, q, V)
    assert c.ok
    r, _ = _run(c)
    if c.perm is not None:
        # rows past the grid's 2048 workgroups repeat rows 0 .. 255 in another order: the same bits, whichever workgroup fits them
        assert V > 2048 and sorted(c.perm.tolist()) == list(range(256))
        for f in ("prep", "pvalue", "kbeta", "bse", "intercept", "betas", "flags"):
            assert np.array_equal(r[f][2048:], r[f][c.perm], equal_nan=(f != "flags")), ("rows past the grid differ from their originals", f)
    s = G.hold_forced_firth(c, r)
    assert s["firth"] >= 0.9 * V, s
    _ceilings("forced-N%d-q%d-V%d" % (N, q, V), s, fields=())


@pytest.mark.parametrize("N,q,cont", G.DEGENERATE, ids=[_name(c, N, q) for N, q, c in G.DEGENERATE])
def test_wide_degenerate_rows_vs_oracle(N, q, cont):
    G.threads()
    c, names = G.degenerate_case(N, q, cont)
    assert c.ok
    want = c.oracle()
    r, info = _run(c)
    singular = np.array([n in G.SINGULAR for n in names])
    assert info["pinv_routed"] > 0, info
    got = r["flags"] & 0x1FF
    differ = [(n, hex(a), hex(b)) for n, a, b in zip(names, got, want["notes"]) if a != b]
    if cont:
        # rank-deficient rows follow numpy's pinv: the minimum-norm coefficients, their standard errors, a t-test at N - rank
        assert not differ, ("notes differ", differ)
        for f in ("prep", "pvalue", "kbeta", "bse", "intercept", "betas"):
            G.close(r[f], want[f], rtol=1e-6, atol=1e-9, what=f)
        assert np.isfinite(r["kbeta"][singular]).all()
        return
    col = np.array([n in G.COLLINEAR for n in names])
    assert (got[~col] == want["notes"][~col]).all(), ("notes differ", differ)
    # singular through the intercept (_glm_wide_cases.COLLINEAR): a singular matrix here, as for the duplicate of a column; the oracle's note
    # of its Newton fit is rounding there (high-bse, or none beside a NaN standard error) -- every other bit as the oracle has it
    assert ((got[col] & 0x28) == 0x20).all() and ((got[col] & 0x1D7) == (want["notes"][col] & 0x1D7)).all(), ("notes differ", differ)
    # exactly singular designs: the reference's Firth log-determinant is LAPACK rounding, so its p-value is no parity target there
    print(G.summary(_name(cont, N, q, "-degenerate"), G.hold_fixed_effects(c, r, want, skip_pvalue=singular, exclude=col)))
    assert (((r["flags"] >> 17) & 1)[col] == 0).all() and np.isfinite(r["kbeta"][col]).all() and np.isfinite(r["bse"][col]).all()
    # Where the oracle routes such a row to Firth as well, it is the same fit -- but one whose step halvings compare two log-determinants of
    # a singular matrix (numpy's slogdet there halves until fit_firth gives up).  Held to the resolution of fit_firth's own stop rule: two
    # runs of the iteration that stop a step apart differ by less than convergence_limit = 1e-4 in the norm of beta.  (Measured: 3e-8 and
    # less on three of the four rows, 3.8e-6 in kbeta on the one-hot sum at q = 32: -0.01896635 here, -0.01897019 the oracle.)
    routed = col & ((want["notes"] & 0x7C) != 0) & ((want["notes"] & 0x40) == 0)
    for f in ("kbeta", "intercept"):
        print("%s of the rows singular through the intercept: here %s, the oracle %s" % (f, r[f][routed], want[f][routed]))
        assert (np.abs(r[f][routed] - want[f][routed]) <= 1e-4).all(), (f, r[f][routed], want[f][routed])


@functools.lru_cache(maxsize=None)
def _lineage(nl, j):
    lin, cov, K = G.lineage_case(nl, j)
    return lin, cov, K, G.lineage_oracle(lin, cov, K)


@pytest.mark.parametrize("nl,j", G.LINEAGE)
def test_wide_lineage_limits_vs_oracle(nl, j):
    from pyseer_amd.engine import Engine, pack_variants
    from test_oracle_golden import _same_or_tied
    lin, cov, K, want = _lineage(nl, j)
    e = Engine(G.LINEAGE_N)
    try:
        e.lineage_setup(lin, cov)
        got = e.lineage_batch(pack_variants(K))
    finally:
        e.close()
    # a row the oracle answers None on MDS-like columns is quasi-separated (whether the weights underflow to a singular Hessian within the
    # 35 iterations is rounding): no parity target, but few, and the answer still None or a column
    sep = np.array([w is None for w in want])
    assert sep.sum() <= G.MAX_SEPARATED * len(want)
    assert ((got >= -1) & (got < nl)).all()
    keep = np.flatnonzero(~sep)
    g = [None if x < 0 else int(x) for x in got]
    _same_or_tied([g[v] for v in keep], [want[v] for v in keep], lin, cov, K[keep])
    assert len(set(g[v] for v in keep)) >= nl // 2                         # the rows name many different columns


def test_wide_lineage_past_the_limit_is_refused():
    from pyseer_amd._abi import SeerHipError
    from pyseer_amd.engine import Engine
    nl, j = G.LINEAGE_REFUSED
    lin, cov, _ = G.lineage_case(nl, j, V=1)
    e = Engine(G.LINEAGE_N)
    try:
        with pytest.raises(SeerHipError, match="1 \\+ lineages \\+ covariates must be <= 50 in this build unless the design is cluster "
                                               "indicators without covariates: this one has covariates"):
            e.lineage_setup(lin, cov)
    finally:
        e.close()
