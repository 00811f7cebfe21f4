"""Seeded random sweep of small configurations through both engines against the oracle: sample counts around word and tile
edges, few and many covariates, binary and continuous phenotypes, rare and near-fixed variants, random thresholds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu


def _close(a, b, rtol=1e-6, atol=0.0):
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    return (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))) | \
        (np.abs(a - b) <= atol + rtol * np.abs(b))


# FUZZ_SEEDS=n widens the sweep, FUZZ_OFFSET=k starts it at seed k (defaults: 12 seeds from 0), FUZZ_WIDE=1 draws wide designs only
_SEEDS = range(int(os.environ.get("FUZZ_OFFSET", 0)), int(os.environ.get("FUZZ_OFFSET", 0)) + int(os.environ.get("FUZZ_SEEDS", 12)))


def _variants(rng, N, V):
    af = np.concatenate([rng.uniform(0.03, 0.97, V - 8), [1.5 / N, 2.5 / N, 1 - 1.5 / N, 0.5, 0.5, 0.02, 0.98, 0.5]])
    K = (rng.random((V, N)) < af[:, None]).astype(np.uint8)
    K[-1] = 0; K[-1, :max(1, N // 50)] = 1                      # a handful of carriers at the front
    return K


def _rescale(W, seed):
    """One seed in three: covariates on their natural, badly matched scales (shifted, 1e-2 .. 30x), as users supply them."""
    if W.shape[1] == 0 or seed % 3 != 1:
        return W
    rng = np.random.default_rng(5000 + seed)
    scale = 10.0 ** rng.uniform(-2.0, 1.5, W.shape[1])
    return W * scale + rng.uniform(-2, 2, W.shape[1]) * scale


def _fixed_case(seed):
    rng = np.random.default_rng(2000 + seed)
    N = int(rng.choice([40, 63, 64, 65, 100, 128, 129, 250, 300]))
    q = int(rng.choice([0, 1, 2, 3, 5, 8, 11, 14, 16]))
    cont = bool(rng.integers(0, 2))
    if os.environ.get("FUZZ_WIDE"):                                # FUZZ_WIDE=1: only wide designs (workgroup-per-variant kernels)
        N = int(rng.choice([250, 300, 640])); q = int(rng.choice([15, 20, 27, 32]))
    V = 72
    W = rng.standard_normal((N, q))
    if q:
        W /= np.abs(W).max(axis=0)
    eta = -0.2 + (1.0 * W[:, 0] if q else 0.0)
    y = eta + rng.standard_normal(N) if cont else (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(float)
    pret, lrtt = (1.0, 1.0) if seed % 3 == 0 else (float(rng.uniform(0.3, 0.9)), float(rng.uniform(0.3, 0.9)))
    K = _variants(rng, N, V)
    af = K.mean(axis=1)
    K = K[(af >= 0.01) & (af <= 0.99)]
    return N, q, cont, _rescale(W, seed), y, pret, lrtt, K


def _firth_case(seed):
    rng = np.random.default_rng(3000 + seed)
    N = int(rng.choice([60, 64, 100, 129, 200, 320]))
    q = int(rng.choice([0, 1, 3, 6, 10, 14, 15]))
    if os.environ.get("FUZZ_WIDE"):
        N = int(rng.choice([320, 640])); q = int(rng.choice([15, 20, 27, 32]))
    V = 40
    W = rng.standard_normal((N, q))
    if q:
        W /= np.abs(W).max(axis=0)
    eta = -0.2 + (1.0 * W[:, 0] if q else 0.0)
    y = (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(float)
    K = _variants(rng, N, V)
    af = K.mean(axis=1)
    K = K[(af >= 0.01) & (af <= 0.99)]
    return N, q, _rescale(W, seed), y, K


def _lineage_case(seed):
    rng = np.random.default_rng(4000 + seed)
    N = int(rng.choice([90, 128, 200, 333, 600]))
    nl = int(rng.choice([1, 2, 3, 5, 9, 13, 14, 15, 18, 25]))
    j = int(rng.choice([0, 0, 1, 3]))
    nl = max(1, min(nl, N // 12 - 1 - j))                          # 19 columns on 90 samples separate almost every k-mer: not a parity case
    V = 48
    clusters = bool(rng.integers(0, 2)) and nl >= 2
    cl = None
    if clusters:
        cl = rng.integers(0, nl + 1, N)
        lin = np.zeros((N, nl)); lin[np.arange(N)[cl > 0], cl[cl > 0] - 1] = 1.0
        base = rng.uniform(0.25, 0.75, (V, nl + 1))
        K = (rng.random((V, N)) < base[:, cl]).astype(np.uint8)
    else:
        lin = rng.standard_normal((N, nl)); lin /= np.abs(lin).max(axis=0)           # scale_fix=False MDS columns, input.py:135
        w = rng.standard_normal((V, nl)) * rng.uniform(0, 2, (V, 1))
        K = (rng.random((V, N)) < 1 / (1 + np.exp(-(lin @ w.T).T - rng.uniform(-1, 1, (V, 1))))).astype(np.uint8)
    cov = _rescale(rng.standard_normal((N, j)), seed) if j else None
    return N, nl, j, V, clusters, cl, lin, cov, K


@pytest.mark.parametrize("seed", _SEEDS)
def test_lmm_random_configurations(seed):
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine, pack_variants
    from pyseer_amd.lmm import mask_like_fit_lmm
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.choice([31, 63, 64, 65, 127, 128, 129, 200, 257, 383]))
    D = int(rng.integers(1, 6))
    cont = bool(rng.integers(0, 2))
    V = 72
    k = N - D
    U = rng.standard_normal((N, k)) / np.sqrt(N)
    S = np.sort(rng.gamma(0.5, 2.0, k))[::-1].copy()
    covar = np.ones((N, 1)) if D == 1 else np.c_[_rescale(rng.standard_normal((N, D - 1)), seed), np.ones((N, 1))]
    y = rng.standard_normal(N) if cont else (rng.random(N) < 0.4).astype(float)
    h2 = float(rng.uniform(0.0, 0.95))
    if seed % 5 == 2:                                             # rank-deficient kinship: numerically zero eigenvalues of either sign
        nz = max(2, k // 6); S[-nz:] = np.random.default_rng(6000 + seed).uniform(-1, 1, nz) * 1e-13
    elif seed % 5 == 4:                                           # a similarity matrix that is not PSD: negative eigenvalues, Sd still > 0
        S[-3:] = -np.array([0.5, 0.3, 0.1]) * min(1.0, (1 - h2) / max(h2, 1e-3))
    fp, lp = (1.0, 1.0) if seed % 3 == 0 else (float(rng.uniform(0.2, 0.9)), float(rng.uniform(0.2, 0.9)))
    Kv = _variants(rng, N, V)
    af = Kv.mean(axis=1)
    afm = (~((af >= 0.01) & (af <= 0.99))).astype(np.uint8)      # 1 = af-filtered (load_var_block leaves pattern None)
    want = orc.LmmOracle(U, S, y, covar).fit_lmm(h2, Kv.astype(float), afm, cont, fp, lp)
    e = Engine(N)
    e.set_af_filter(0.01, 0.99)
    e.lmm_setup(U, S, y, covar, h2, continuous=cont, filter_pvalue=fp, lrt_pvalue=lp)
    r = mask_like_fit_lmm(e.lmm_batch(pack_variants(Kv)))
    e.close()
    noise = np.zeros(V, bool) if cont else ((Kv == y).all(axis=1) | (Kv == 1 - y).all(axis=1))
    for f, g in (("prep", "prep"), ("pvalue", "pvalue"), ("beta", "kbeta"), ("bse", "bse"), ("frac_h2", "frac_h2")):
        ok = _close(r[f], want[g], atol=1e-12 if f in ("beta", "frac_h2") else 1e-300) | noise
        assert ok.all(), (f, N, D, cont, np.argwhere(~ok)[:4].tolist(), r[f][~ok][:4], want[g][~ok][:4])
    assert (((r["flags"] & 0x1FF) == want["notes"]) | noise).all()
    assert ((((r["flags"] >> 16) & 1) == want["prefilter"])).all()
    assert (((((r["flags"] >> 17) & 1) == want["filter"])) | noise).all()


@pytest.mark.parametrize("seed", _SEEDS)
def test_fixed_effects_random_configurations(seed):
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine, pack_variants
    from pyseer_amd.model import fit_null
    N, q, cont, W, y, pret, lrtt, K = _fixed_case(seed)
    e0 = np.zeros((0, 0))
    null = fit_null(y, W, e0, cont)
    if null is None:
        pytest.skip("null model not estimable for this draw")
    nf = np.nan if cont else fit_null(y, W, e0, False, firth=True)
    if nf is None:
        pytest.skip("Firth null model did not converge for this draw")
    want = orc.fixed_effects_batch(y, K.astype(float), W if q else None, cont, pret, lrtt, null.llf, nf)
    e = Engine(N)
    e.glm_setup(y, W, cont, null.llf, nf, pret, lrtt)
    r = e.glm_batch(pack_variants(K))
    e.close()
    firth = (want["notes"] & 0x7C) != 0

    def rows_matching(w):
        m = ((r["flags"] & 0x1FF) == w["notes"]) & (((r["flags"] >> 16) & 1) == w["prefilter"]) & (((r["flags"] >> 17) & 1) == w["filter"])
        for f in ("prep", "pvalue", "kbeta", "bse", "intercept"):
            m &= _close(r[f], w[f], rtol=np.where(firth, 2e-6, 1e-6), atol=np.where(firth, 1e-6 if f != "pvalue" else 1e-300, 1e-12))
        if q:
            both_nan = ~np.isfinite(w["kbeta"])
            m &= both_nan | _close(r["betas"], w["betas"], rtol=2e-6, atol=1e-6).all(axis=1)
        return m
    good = rows_matching(want)
    if not good.all() and firth[~good].all():
        # Firth fits whose step-halving comparisons the reference decides on last-bit ties of F have more than one legitimate
        # answer (case 1): such a row must equal the oracle under one of its documented tie settings.
        for w in orc.firth_noise_variants(lambda: orc.fixed_effects_batch(y, K.astype(float), W if q else None, cont, pret, lrtt,
                                                                          null.llf, nf))[1:]:
            good |= rows_matching(w) & firth
    bad = np.flatnonzero(~good)
    assert bad.size == 0, (N, q, cont, bad[:4].tolist(), [(f, r[f][bad[:4]], want[f][bad[:4]]) for f in ("pvalue", "kbeta", "bse")],
                           r["flags"][bad[:4]], want["notes"][bad[:4]])


@pytest.mark.parametrize("seed", _SEEDS)
def test_forced_firth_random_configurations(seed):
    """Every variant through fit_firth (BASELINE config C4 shape, small): state-machine kernels, and the run-time-width kernel for
    q > 14, against the oracle's fit_firth."""
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine, pack_variants
    from pyseer_amd.model import fit_null
    N, q, W, y, K = _firth_case(seed)
    e0 = np.zeros((0, 0))
    null = fit_null(y, W, e0, False)
    nf = fit_null(y, W, e0, False, firth=True)
    if null is None or nf is None:
        pytest.skip("null model not estimable for this draw")
    want = orc.firth_batch(y, K.astype(float), W if q else None)
    e = Engine(N)
    e.glm_setup(y, W, False, null.llf, nf, force_firth=True)
    r = e.glm_batch(pack_variants(K))
    e.close()
    failed = ((r["flags"] >> 6) & 1) == 1

    def rows_matching(w):
        ok = (w["status"] == 0) & np.isfinite(w["fitll"])
        m = failed == (w["status"] != 0)
        for f in ("intercept", "kbeta", "bse"):
            m &= ~ok | _close(r[f], w[f], rtol=2e-6, atol=1e-6)
        with np.errstate(invalid="ignore"):
            lr = -2 * (nf - w["fitll"])
        want_p = np.array([orc.chi2_sf1(x) if x > 0 else 1.0 for x in lr])
        return m & (~ok | _close(r["pvalue"], want_p, rtol=5e-6, atol=1e-300))
    good = rows_matching(want)
    if not good.all():                                            # last-bit ties of the halving test: see the test above
        for w in orc.firth_noise_variants(lambda: orc.firth_batch(y, K.astype(float), W if q else None))[1:]:
            good |= rows_matching(w)
    assert good.all(), (N, q, np.argwhere(~good)[:4].tolist())


_WIDE_SEEDS = (0, 1, 2)       # their wide draws have estimable null models: tests/test_glm_wide_cases_cpu.py


@pytest.mark.parametrize("kind", ["fixed", "firth"])
@pytest.mark.parametrize("seed", _WIDE_SEEDS)
def test_wide_random_configurations(seed, kind, monkeypatch):
    """The wide draw of the two case builders (FUZZ_WIDE: q in 15 .. 32 on the run-time-width kernels of glm_wide.hip, forced Firth
    included) in the default suite, held as the two tests above hold their cases."""
    monkeypatch.setenv("FUZZ_WIDE", "1")
    (test_fixed_effects_random_configurations if kind == "fixed" else test_forced_firth_random_configurations)(seed)


@pytest.mark.parametrize("seed", _SEEDS)
def test_lineage_random_configurations(seed):
    """fit_lineage_effect (pyseer/model.py:151-199) for random sample counts, lineage widths on both sides of the fixed-width /
    run-time-width kernel split, MDS-like or cluster-indicator lineage columns, and covariates on unmatched scales."""
    from oracle import oracle as orc
    from pyseer_amd.engine import Engine, pack_variants
    from test_oracle_golden import _same_or_tied
    N, nl, j, V, clusters, cl, lin, cov, K = _lineage_case(seed)
    e = Engine(N)
    e.lineage_setup(lin, cov)
    got = e.lineage_batch(pack_variants(K))
    e.close()
    want = [orc.lineage_effect(lin, cov, K[v].astype(float)) for v in range(V)]
    # quasi-separated clusters (every member, or none, carries the k-mer) are not a parity target: DESIGN.md section 6, case 5
    sep = np.zeros(V, bool)
    if clusters:
        sep = np.array([any(K[v][cl == c].sum() in (0, (cl == c).sum()) for c in range(nl + 1) if (cl == c).any()) for v in range(V)])
    g = [None if x < 0 else int(x) for x in got]
    keep = np.flatnonzero(~sep)
    _same_or_tied([g[v] for v in keep], [want[v] for v in keep], lin, cov, K[keep])
