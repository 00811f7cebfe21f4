"""The generator and the comparisons of tests/test_glm_wide_gpu.py (tests/_glm_wide_cases.py), without a GPU: every case's null model is
estimable except the listed ones; the row classes the GPU tests rely on are there -- uniform, rare, strong-effect and tail rows, Newton / OLS
rows and Firth-routed rows, prefiltered and LRT-filtered rows, rank-deficient rows that numpy's pinv decides, singular rows routed to Firth,
rows past the Firth grid that repeat earlier ones --; the three caps (oracle firth-fails, rows that can need the tie detector, quasi-separated
lineage rows) hold from the oracle's outputs alone; and the comparisons pass on the oracle's own answers and fail on a wrong bit or value."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _glm_wide_cases as G  # noqa: E402
from _glm_sweep import STRONG, TAIL  # noqa: E402


def _oracle_rows(c):
    from pyseer_amd.engine import pack_variants
    return G.OracleEngine(c).glm_batch(pack_variants(c.K))


def _mix(c):
    V, N, K, kind = c.V, c.N, c.K, c.kind
    assert K.shape == (V, N) and set(np.unique(K)) <= {0, 1}
    assert [(kind == k).sum() for k in (G.UNIFORM, G.RARE, STRONG, TAIL)] == [3 * V // 4, V // 8, V // 16, V // 16]
    m = K.sum(axis=1)
    assert (m >= 1).all() and (m <= N - 1).all()
    r = m[kind == G.RARE]
    assert (r >= max(1, int(np.ceil(0.004 * N)))).all() and (r <= max(1, int(np.ceil(0.02 * N)))).all()
    t = K[kind == TAIL]
    assert (t[:, N - 1] == 1).any() and (t[:, N - 1] == 0).any()                       # the last sample in, and out
    k0 = t[0]
    assert k0[N - int(k0.sum()):].all()                                                # carriers exactly the last k samples


@pytest.mark.parametrize("q", G.WIDTHS)
@pytest.mark.parametrize("cont", [False, True])
def test_width_cases_hold_every_row_class(q, cont):
    G.threads()
    c = G.width_case(q, cont)
    assert c.ok and (c.N, c.V) == (333, 256)
    assert c.W.shape == (333, q) and set(np.unique(c.W[:, 0])) == {0.0, 1.0} and 30 < c.W[:, 1].mean() < 70
    assert set(np.unique(c.W[:, 3:8])) == {0.0, 1.0} and (c.W[:, 3:8].sum(axis=1) <= 1).all()
    _mix(c)
    s = G.hold_fixed_effects(c, _oracle_rows(c))
    assert s["plain"] >= 64 and s["tail_plain"] >= 2 and s["ofail"] <= G.MAX_ORACLE_FAIL * c.V, s
    assert not G.numerically_singular_rows(c, c.oracle()).any()
    assert max(s["mx"].values()) == 0.0
    if not cont:
        assert s["firth"] >= 8, s
        want = c.oracle()
        assert ((want["notes"][c.kind == G.RARE] & 0x7C) != 0).sum() >= 4              # the rare rows are among the Firth-routed ones
        assert (np.abs(want["kbeta"][c.kind == STRONG]) >= 1).any()


@pytest.mark.parametrize("cont", [False, True])
def test_filtered_width_cases_hold_both_filters(cont):
    G.threads()
    c = G.width_case(19, cont, True)
    assert c.ok and (c.pret, c.lrtt) == (0.3, 0.2)
    s = G.hold_fixed_effects(c, _oracle_rows(c))
    assert 32 <= s["prefiltered"] <= c.V - 32 and s["filtered"] >= 8 and s["plain"] >= 32, s


def test_the_sample_count_cases_that_cannot_run_are_the_listed_ones():
    """Estimable: the null model of the case's draw fits (binary: by Newton and by Firth).  Every (N, q, phenotype) is, at its seed, except
    the listed one -- which is not on most of sixteen draws."""
    table = {(N, q, cont): G.edge_case(N, q, cont).ok for N in G.EDGE_NS for q in G.EDGE_QS for cont in (False, True)}
    print("\n".join("N=%d q=%d %s: %s" % (N, q, "continuous" if cont else "binary", "estimable" if ok else "NOT estimable")
                    for (N, q, cont), ok in table.items()))
    assert sorted(k for k, ok in table.items() if not ok) == sorted(G.NOT_ESTIMABLE)
    assert len(table) - len(G.NOT_ESTIMABLE) == 51
    def parity_case(c):
        return c.ok and not G.numerically_singular_rows(c, c.oracle()).any()
    for key, a in G.EDGE_ATTEMPT.items():                                              # a later draw only where the first is no parity case
        assert a == min(i for i in range(16) if parity_case(G.edge_case(*key, attempt=i))) > 0
    for key in G.NOT_ESTIMABLE:
        assert sum(G.edge_case(*key, attempt=i).ok for i in range(16)) <= 4


@pytest.mark.parametrize("N", G.EDGE_NS)
def test_sample_count_cases_hold_fitted_rows(N):
    G.threads()
    for q in G.EDGE_QS:
        for cont in (False, True):
            if (N, q, cont) in G.NOT_ESTIMABLE:
                continue
            c = G.edge_case(N, q, cont)
            assert c.ok and c.V == 128
            _mix(c)
            s = G.hold_fixed_effects(c, _oracle_rows(c))
            assert s["plain"] + s["firth"] >= c.V // 2 and s["ofail"] <= G.MAX_ORACLE_FAIL * c.V, (N, q, cont, s)
            assert not G.numerically_singular_rows(c, c.oracle()).any(), (N, q, cont)


@pytest.mark.parametrize("N,q,V", G.FORCED)
def test_forced_firth_cases_meet_their_caps(N, q, V):
    """From the oracle alone: at most 1 % of the rows are its firth-fails, and on at most 5 % do its own answers under its tie settings
    lie further apart than the tolerance -- the rows that can need the tie detector at all."""
    G.threads()
    c = G.forced_case(N, q, V)
    assert c.ok and c.V == V == c.K.shape[0]
    vs = c.firth_variants()
    assert (vs[0]["status"] != 0).sum() <= G.MAX_ORACLE_FAIL * V
    assert G.tie_rows(vs, np.ones(V, bool), rtol=1e-6, atol=1e-12).sum() <= G.MAX_TIE * V
    if V > 2048:
        assert sorted(c.perm.tolist()) == list(range(256)) and not np.array_equal(c.perm, np.arange(256))
        assert np.array_equal(c.K[2048:], c.K[c.perm])
    r = _oracle_rows(c)
    s = G.hold_forced_firth(c, r, vs)
    assert s["firth"] >= 0.9 * V and s["ties"] == 0, s
    bad = dict(r); bad["flags"] = r["flags"].copy(); bad["flags"][5] ^= 1 << 6
    with pytest.raises(AssertionError, match="failure bit"):
        G.hold_forced_firth(c, bad, vs)
    quiet = np.flatnonzero(~G.tie_rows(vs, np.ones(V, bool)) & (vs[0]["status"] == 0))[0]
    bad = dict(r); bad["kbeta"] = r["kbeta"].copy(); bad["kbeta"][quiet] += 3e-6 * max(1.0, abs(r["kbeta"][quiet]))
    with pytest.raises(AssertionError, match="kbeta"):
        G.hold_forced_firth(c, bad, vs)


def test_the_comparison_fails_on_a_wrong_bit_or_value():
    G.threads()
    c = G.width_case(19, False, True)
    want = c.oracle()
    r = _oracle_rows(c)
    _, firth, plain = G.oracle_classes(c, want)
    for bit, what in ((16, "prefilter bits differ"), (17, "filter bits differ"), (3, "notes differ")):
        bad = dict(r); bad["flags"] = r["flags"].copy(); bad["flags"][np.flatnonzero(plain)[3]] ^= 1 << bit
        with pytest.raises(AssertionError, match=what):
            G.hold_fixed_effects(c, bad, want)
    for f in ("kbeta", "bse", "intercept", "pvalue", "prep"):
        bad = dict(r); bad[f] = r[f] * np.where(np.arange(c.V) == np.flatnonzero(plain)[-1], 1 + 2e-6, 1.0)
        with pytest.raises(AssertionError, match=f):
            G.hold_fixed_effects(c, bad, want)
    bad = dict(r); bad["betas"] = r["betas"].copy(); bad["betas"][np.flatnonzero(plain)[0], c.q - 1] *= 1 + 2e-6
    with pytest.raises(AssertionError, match="betas"):
        G.hold_fixed_effects(c, bad, want)
    fitted = np.isfinite(want["kbeta"][firth])                                         # (a prefiltered bad-chisq row has no statistics)
    quiet = np.flatnonzero(firth)[fitted & ~G.tie_rows(c.oracle_variants(c.K[firth]), np.ones(int(firth.sum()), bool))][0]
    bad = dict(r); bad["kbeta"] = r["kbeta"].copy(); bad["kbeta"][quiet] *= 1 + 3e-6
    with pytest.raises(AssertionError, match="firth kbeta"):
        G.hold_fixed_effects(c, bad, want)


@pytest.mark.parametrize("N,q,cont", G.DEGENERATE)
def test_degenerate_cases_hold_their_classes(N, q, cont):
    G.threads()
    c, names = G.degenerate_case(N, q, cont)
    assert c.ok and N == 200
    want = c.oracle()
    singular = np.array([n in G.SINGULAR for n in names])
    assert singular.sum() == 4
    for v in range(c.V):
        rank, pc = G.design_rank(c, v)
        assert pc == q + 2 and rank == pc - int(singular[v]), (names[v], rank, pc)
    at = {n: v for v, n in enumerate(names)}
    assert np.array_equal(c.K[at["covariate"]], c.W[:, 0]) and np.array_equal(c.K[at["covariate complement"]], 1 - c.W[:, 0])
    assert np.array_equal(c.K[at["one-hot sum"]], c.W[:, 3:8].sum(axis=1))
    assert c.K[at["one carrier"]].sum() == 1 and c.K[at["N - 1 carriers"]].sum() == N - 1
    for label, cls in (("cases only", 1), ("controls only", 0)):
        for m in (1, 2, 3):
            k = c.K[at["%s, %d" % (label, m)]]
            assert k.sum() == m
            if not cont:
                assert (c.y[k == 1] == cls).all()
    notes = want["notes"]
    if cont:
        # pinv-routed: rank-deficient rows the oracle still fits (minimum-norm coefficients, N - rank degrees of freedom)
        assert np.isfinite(want["kbeta"][singular]).all() and np.isfinite(want["bse"][singular]).all() and (notes[singular] == 0).all()
        assert (want["prefilter"] != 0).any()                                      # one carrier: Welch's test has no variance
    else:
        assert np.array_equal(c.K[at["phenotype"]], c.y) and np.array_equal(c.K[at["phenotype complement"]], 1 - c.y)
        col = np.array([n in G.COLLINEAR for n in names])
        assert col.sum() == 2 and (singular[col]).all()
        assert ((notes[singular & ~col] & 0x7C) == 0x20).all()                     # a duplicated column: matrix-inversion-error, Firth by pinv
        assert ((notes[col] & 0x20) == 0).all()                                    # singular through the intercept: a pivot of rounding noise,
        assert (((notes[col] & 0x08) != 0) | np.isnan(want["bse"][col])).all()     # high-bse or a NaN standard error as the noise falls
        assert ((notes & 0x04) != 0).sum() >= 8                                    # bad-chisq
        assert (notes & 0x40).sum() == 0                                           # no oracle firth-fail among them
        G.hold_fixed_effects(c, _oracle_rows(c), want, skip_pvalue=singular, exclude=col)


@pytest.mark.parametrize("nl,j", G.LINEAGE + (G.LINEAGE_REFUSED,))
def test_lineage_cases_sit_at_the_limits(nl, j):
    lin, cov, K = G.lineage_case(nl, j)
    pc = 1 + nl + j
    assert pc == 51 if (nl, j) == G.LINEAGE_REFUSED else pc in (17, 50)
    assert lin.shape == (G.LINEAGE_N, nl) and K.shape == (G.LINEAGE_V, G.LINEAGE_N) and (cov is None) == (j == 0)
    assert len(np.unique(lin)) > 100 and np.abs(lin).max() == 1.0                      # not cluster indicators: no count route
    if (nl, j) == G.LINEAGE_REFUSED:
        return
    want = G.lineage_oracle(lin, cov, K)
    assert sum(w is None for w in want) <= G.MAX_SEPARATED * len(want)
    assert len(set(w for w in want if w is not None)) >= nl // 2
    assert sorted(set(1 + a + b for a, b in G.LINEAGE)) == [17, 50]


def test_the_wide_fuzz_seeds_are_estimable(monkeypatch):
    """tests/test_fuzz_gpu.py test_wide_random_configurations: its three seeds draw wide designs whose null models fit (no run-time skip)."""
    import test_fuzz_gpu as F
    from pyseer_amd.model import fit_null
    monkeypatch.setenv("FUZZ_WIDE", "1")
    e0 = np.zeros((0, 0))
    for seed in F._WIDE_SEEDS:
        N, q, cont, W, y, pret, lrtt, K = F._fixed_case(seed)
        assert q > 14 and fit_null(y, W, e0, cont) is not None and (cont or fit_null(y, W, e0, False, firth=True) is not None)
        N, q, W, y, K = F._firth_case(seed)
        assert q > 14 and fit_null(y, W, e0, False) is not None and fit_null(y, W, e0, False, firth=True) is not None
