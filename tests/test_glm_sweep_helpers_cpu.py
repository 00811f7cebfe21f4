"""The volume sweeps' own machinery (tests/_glm_sweep.py), without a GPU: the generator's tail rows are there and inside the frequency
window; the vectorised OLS reference that holds the rows the oracle does not see equals the oracle's statsmodels-pinv OLS, notes and
prefilter / filter bits included; and a sweep with the oracle on a sixteenth of the rows still fails on a wrong bit in the others."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _glm_sweep import FLOOR, REF_FLOOR, STRONG, TAIL, ols_reference, rows  # noqa: E402


@pytest.mark.parametrize("N", [1025, 1999, 2048, 5001])
def test_generator_holds_the_tail_rows(N):
    rng = np.random.default_rng(N)
    y = (rng.random(N) < 0.4).astype(float)
    K, kind = rows(rng, 2000, N, y)
    m = K.mean(axis=1)
    assert ((m >= 0.01) & (m <= 0.99)).all()
    t = K[kind == TAIL]
    kmin = -(-N // 100)
    last_k = [k for k in range(kmin, kmin + 49) if (t == np.r_[np.zeros(N - k, np.uint8), np.ones(k, np.uint8)]).all(axis=1).any()]
    assert last_k == list(range(kmin, kmin + 49))                                    # exactly the last k samples, every k
    assert (t[:, N - 1] == 1).sum() >= 49 + 32 and (t[:, N - 1] == 0).sum() >= 8     # the last sample in, and out
    assert (kind == STRONG).mean() > 0.1


def _ols_case(N, q, seed):
    from pyseer_amd.model import fit_null
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((N, q))
    if q:
        W[:, 0] = rng.random(N) < 0.3
    y = (0.5 * W[:, 0] if q else 0.0) + rng.standard_normal(N)
    K, kind = rows(rng, 200, N, y)
    nl = fit_null(y, W if q else np.zeros((0, 0)), np.zeros((0, 0)), True).llf
    return W if q else None, y, K, kind, nl


@pytest.mark.parametrize("N,q,pret,lrtt", [(301, 0, 1.0, 1.0), (301, 3, 1.0, 1.0), (512, 16, 1.0, 1.0), (301, 10, 0.3, 0.2)])
def test_ols_reference_equals_the_oracle(N, q, pret, lrtt):
    """Values to 1e-10, and the prefilter / filter bits and notes exactly, wherever the reference does not hand the row to the oracle."""
    from oracle import oracle as orc
    W, y, K, _, nl = _ols_case(N, q, 7 * N + q)
    want = orc.fixed_effects_batch(y, K.astype(float), W, True, pret, lrtt, nl, np.nan)
    got = ols_reference(y, K, W, pret, lrtt)
    mine = ~got["oracle_only"]
    assert mine.mean() > 0.99
    for f in ("notes", "prefilter", "filter"):
        assert (got[f][mine] == want[f][mine]).all(), f
    if pret < 1.0:
        assert 0.2 < want["prefilter"].mean() < 0.8 and want["filter"].sum() > 5       # both kinds of rows, and both bits, are there
    for f in ("prep", "kbeta", "intercept", "bse", "pvalue"):
        a, b = got[f][mine], want[f][mine]
        assert (np.isnan(a) == np.isnan(b)).all(), f
        ok = ~np.isnan(b)
        rel = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), REF_FLOOR.get(f) or FLOOR[f])
        assert rel.max() <= 1e-10, (f, rel.max())
    if q:
        a, b = got["betas"][mine], want["betas"][mine]
        ok = ~np.isnan(b)
        assert (np.abs(a[ok] - b[ok]) <= 1e-10 * np.maximum(np.abs(b[ok]), FLOOR["betas"])).all()


class _OracleEngine(object):
    """Stands in for the engine with the oracle's own answers in the engine's layout (flags: notes | prefilter << 16 | filter << 17);
    `flip` toggles the prefilter bit of one row."""

    def __init__(self, y, W, pret, lrtt, nl, flip=None):
        self.a, self.flip = (y, W, pret, lrtt, nl), flip

    def glm_batch(self, bits):
        from oracle import oracle as orc
        y, W, pret, lrtt, nl = self.a
        K = np.unpackbits(bits, axis=1, bitorder="little")[:, :y.shape[0]]
        w = dict(orc.fixed_effects_batch(y, K.astype(float), W, True, pret, lrtt, nl, np.nan))
        w["flags"] = w["notes"].astype(np.uint32) | (w["prefilter"].astype(np.uint32) << 16) | (w["filter"].astype(np.uint32) << 17)
        if self.flip is not None:
            w["flags"][self.flip] ^= 1 << 16
        return w


def test_sweep_holds_every_row_the_oracle_does_not_see():
    """With the oracle on a sixteenth of the rows, a wrong prefilter bit on one of the others still fails the chunk."""
    from _glm_sweep import Sweep
    pret, lrtt = 0.3, 0.2
    W, y, K, kind, nl = _ols_case(301, 10, 5)
    Sweep(_OracleEngine(y, W, pret, lrtt, nl), y, W, True, nl, np.nan, pret, lrtt, oracle_every=16).chunk(K, kind)
    unseen = np.flatnonzero((kind != TAIL) & (np.arange(K.shape[0]) % 16 != 0))
    with pytest.raises(AssertionError, match="prefilter bits differ"):
        Sweep(_OracleEngine(y, W, pret, lrtt, nl, flip=unseen[3]), y, W, True, nl, np.nan, pret, lrtt, oracle_every=16).chunk(K, kind)
