"""What licenses the tight ceilings of the LMM sweeps (tests/test_lmm_widths_gpu.py, tests/test_lmm_refined_gpu.py), without a GPU: the
oracle's fit_lmm_block agrees with a numpy.longdouble restatement of the reference (tests/_lmm_sweep.py) at the covariate widths, ranks and
spectra the sweeps feed -- beta and frac_h2 to 1e-11, bse to 1e-13 (measured: 1.5e-12 and 1.6e-15), NaN and inf patterns exactly --, the rows
the covariates explain and the all-zero / all-one rows give (beta 0, bse inf, p 1), and the restatement itself notices a projector that
ignores the panel's rank."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _lmm_sweep import beta_error_of, design, deviation, fit_lmm_block_longdouble, rows, same_pattern  # noqa: E402

V = 96
# id: (N, D, continuous, h2, design keywords)
CASES = {
    "N333-D8-cont": (333, 8, True, 0.37, {}),
    "N200-D16-bin": (200, 16, False, 0.37, {}),
    "N391-D17-cont": (391, 17, True, 0.37, {}),
    "N640-D32-bin": (640, 32, False, 0.37, {}),
    "N300-D6-rank5": (300, 6, False, 0.37, dict(dup=((2, 1, 3.0),))),
    "N300-D3-indefinite": (300, 3, False, 0.6, dict(indefinite=True)),
    "N300-D3-h2-0": (300, 3, False, 0.0, {}),
    "N300-D34-rank32": (300, 34, False, 0.37, dict(dup=((31, 1, 1.0), (32, 2, 2.0)))),
}


def _case(cfg):
    N, D, cont, h2, kw = CASES[cfg]
    U, S, covar, y = design(N, D, 1000 + N + D, cont, **kw)
    Kv, special = rows(N, V, 2000 + N + D, covar)
    return U, S, covar, y, h2, Kv, special


@pytest.mark.parametrize("cfg", list(CASES))
def test_oracle_equals_the_longdouble_restatement(cfg):
    from oracle import oracle as orc
    orc.set_threads(min(16, len(os.sched_getaffinity(0))))
    U, S, covar, y, h2, Kv, special = _case(cfg)
    assert set(special) == {"zero", "one", "span", "cospan"}
    if cfg.endswith("indefinite"):
        assert (h2 * S + 1 - h2).min() < -0.1
    wb, ws, wf, wp = orc.LmmOracle(U, S, y, covar).block(h2, Kv.astype(float))
    ref = fit_lmm_block_longdouble(U, S, y, covar, h2, Kv)
    for f, w, lim in (("beta", wb, 1e-11), ("frac_h2", wf, 1e-11), ("bse", ws, 1e-13)):
        same_pattern(w, ref[f].astype(float), cfg + " " + f)
        d = deviation(w, ref[f])
        print("%s %s %.3g" % (cfg, f, d))
        assert d <= lim, (cfg, f, d)
    edge = sorted(special.values())
    ordinary = np.setdiff1d(np.arange(V), edge)
    # the cheap measure of the oracle's own beta error (longdouble numerator only), which the refined sweep draws its rows by, says
    # what the whole restatement says: its float64 denominator is good to 1e-13, far below the 1e-11 it is used at
    full = np.abs(wb.astype(np.longdouble) - ref["beta"])[ordinary] / np.abs(ref["beta"][ordinary])
    cheap = beta_error_of(wb, U, S, y, covar, h2, Kv)[ordinary]
    print("%s beta_error_of against the restatement %.3g" % (cfg, float(np.abs(cheap - full).max())))
    assert np.abs(cheap - full).max() <= 1e-12
    assert np.isfinite(ws[ordinary]).all() and (ws[ordinary] > 0).all()
    assert (wb[edge] == 0).all() and np.isposinf(ws[edge]).all() and (wp[edge] == 1.0).all() and (wf[edge] == 0).all()


def test_restatement_needs_the_rank_aware_projector():
    """A plain QR of the rank-deficient panel spans directions that are not in the covariate space: the restatement then no longer
    agrees with the oracle, by far."""
    from oracle import oracle as orc
    U, S, covar, y, h2, Kv, special = _case("N300-D6-rank5")
    wb, ws, wf, wp = orc.LmmOracle(U, S, y, covar).block(h2, Kv.astype(float))
    bad = fit_lmm_block_longdouble(U, S, y, covar, h2, Kv, plain_qr=True)
    ordinary = np.setdiff1d(np.arange(V), sorted(special.values()))
    assert deviation(wb[ordinary], bad["beta"][ordinary]) > 1e-3


def test_bookkeeping():
    a = np.array([1.0, np.nan, np.inf, 0.0, 2.0]); b = np.array([1.0 + 1e-9, np.nan, np.inf, 0.0, 2.0])
    same_pattern(a, b)
    assert abs(deviation(a, b) - 1e-9) < 1e-15                      # zero, NaN and inf rows do not enter
    with pytest.raises(AssertionError):
        same_pattern(a, np.array([1.0, 0.0, np.inf, 0.0, 2.0]))
    with pytest.raises(AssertionError):
        same_pattern(a, np.array([1.0, np.nan, -np.inf, 0.0, 2.0]))
