"""A million random + strong-effect logistic rows per sample count against the oracle, with ASSERTED maxima per field ("next
round" 1b): fixed_effects_regression (model.py:202-394) through sh_glm_batch at N = 1000 and N = 5000, 10 covariates (one binary, one
age-like: mean 50, sd 10), half of the rows at uniform allele frequencies, half from a U-shaped distribution, 15 % with real / near-separating effects
(|kbeta| 2 .. 6), and in every chunk the tail rows whose carriers are the last samples (the generator and the comparison: tests/_glm_sweep.py;
the other design widths, sample counts, OLS and the wide designs: tests/test_glm_shapes_sweep_gpu.py).  One timed bench step is 2^20 (N = 1000) / 2^18 (N = 5000) rows; the fixtures the reference made hold 64 .. 256 rows each.

What is asserted (measured values in profiles/r06/glm_sweep_2e20.txt):
  * notes bit-exact, except rows the ORACLE calls firth-fail (its rounding-noise failures, DESIGN.md section 6: the HIP path fits them) --
    every one of those must carry SH_FLAG_FIRTH_SENSITIVE (bit 18), and there are at most 1e-4 of them; prefilter and filter bits likewise;
  * Newton-fitted rows: kbeta <= 5e-8, intercept <= 1e-7, bse <= 2e-7 relative (north_star: 1e-6; kbeta against max(|kbeta|, 1e-4) -- a
    five-hundredth of the smallest bse --, the intercept against max(|intercept|, 1e-2): in a million rows one cancels to 1e-4).  bse is the thin one: the final
    information matrix carries single-precision DIFFERENCES from the exact null-model matrix (csrc/glm_kernels.hip: eta_const, weight_even,
    GLM_DIRECT_ROW); before round 6 this sweep measured 2.3e-7 .. 3.0e-7 on a tenth of the rows;
  * p-value <= 1e-6 relative, where a likelihood-ratio statistic below the noise of its two log-likelihoods (32 ulp of |llf|: 2e-11 at
    N = 5000) is compared as a statistic, not as its tail (p = 1 - 2e-6 against p = 1 is lr = 1e-11 against lr <= 0);
  * Firth-routed rows (bad-chisq / high-bse / separation): 1e-6 relative + the 3e-7 halving-tie slack on the rows the tie detector names
    (tests/_firth_tol.py).  (The covariate is age-like, not offset by thousands: with a column 2000 +- 10 the reference's own Firth answers move by
    4e-6 under a 2e-13 |F| bias of its halving test on half of the routed rows -- its output there is noise; the Newton rows do not care.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CEIL = {"kbeta": 5e-8, "intercept": 1e-7, "bse": 2e-7}


@pytest.mark.parametrize("N,q,seed", [(1000, 10, 12), (5000, 10, 11)])
def test_a_million_logistic_rows_against_the_oracle_with_asserted_maxima(N, q, seed):
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine
    from pyseer_amd.model import fit_null
    from _glm_sweep import Sweep          # the row generator (with the tail rows) and the per-chunk comparison
    V = int(os.environ.get("SEERHIP_SWEEP_ROWS", 1 << 20))
    orc.set_threads(max(1, min(os.cpu_count() or 4, len(os.sched_getaffinity(0)), 64)))
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((N, q)); W[:, 0] = rng.random(N) < 0.3; W[:, 1] = 50 + 10 * W[:, 1]
    eta = -0.5 + 0.9 * W[:, 0] + 0.5 * W[:, 2]
    y = (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(float)
    e0 = np.zeros((0, 0))
    nl = fit_null(y, W, e0, False).llf; nf = fit_null(y, W, e0, False, firth=True)
    e = Engine(N); e.glm_setup(y, W, False, nl, nf)
    s = Sweep(e, y, W, False, nl, nf).run(rng, V)
    e.close()
    print(s.summary("N=%d q=%d" % (N, q)))
    mx = s.mx
    assert s.rows >= V and s.strong >= 0.1 * s.newton
    for f, c in CEIL.items():
        assert mx[f] <= c, (f, mx[f], c)
    assert mx["pvalue"] <= 1e-6 and mx["betas"] <= 1e-6
    assert s.oracle_fail <= 1e-4 * s.rows
