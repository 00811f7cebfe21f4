"""The LMM contraction at the fp64 level, limb by limb.  G is held as int8 limbs of weight 256^-l; the fourth carries about 6e-8 of x^T G x, so
a limb dropped or misplaced in one row-tile shape hides below the 1e-6 of every other oracle comparison, and the contraction routes are
only ever compared with each other.  Here the extra-limb pass (shk_lmm_refine: k_gather_T_list, the contraction over the gathered image,
k_lmm_refine_fix) contracts EVERY row down to the last stored limb and the result is held to the oracle at 1e-10 or better, at every
row-tile shape of the main pass (the two-wave kernel below four row tiles, N <= 256, where the pass itself is k_lmm_quadform_i8<64>; the wide
kernel with a ragged tile, a narrow last tile with 1 / 2 / 4 valid 32-row sub-tiles, the last tile all padding), with covariates, at every limb count, behind the AF compaction's gathered image, and on more listed
variants than one sweep of the pass' grid-stride loops covers (64 x 256).  The oracle is held to a longdouble restatement by
tests/test_lmm_sweep_helpers_cpu.py (beta 1.5e-12, bse 1.6e-15).

Rows: V = 513 (a 512-variant block plus one), allele frequencies 0.02 .. 0.98, V/8 majority-carrier rows (stored complemented); every row
is fitted (how the rows are kept to those the reference is good on: below).  Each case runs three times on one engine:
  set_lmm_tol(0)      never refine: refined count 0, and wherever the measured bse deviation d0 is above the oracle's own noise (1e-12)
                      the certificate covers it: 2 d0 <= 1.01 bound_rel_max_last_batch (x^T K^-1 x enters bse as a square root);
  set_lmm_tol(1e-13)  refine every row (1e-16 at n_limbs = 6, where every bound is below 1e-13 already): refined count = fitted rows
                      (0 at n_limbs = 7, which has no extra limbs: the main pass itself meets the ceilings); every field under its
                      ceiling; for n_limbs <= 4 the bse deviation at most 1/100 of d0;
  a tolerance halfway between bound_rel_typical and the unrefined run's maximum: every row's bse bit-equal to one of the two other
                      runs', at least refined_last_batch of them to the refined run's.
Route independence: the main partial sums are exact integers, so the refined run is bit-identical under SEERHIP_ROUTE ragged=0 and qf=0, and
with the AF compaction forced or off; AF-filtered rows stay NaN behind the refinement.

Measured maxima of the first GPU run on these rows (relative, against the oracle; d0 = unrefined bse; CEIL = 10x the refined run's rounded up, never
above 1e-10; the run's lines: profiles/r17/lmm_sweep.txt):
  N200-L4            d0 1.86e-10  refined: beta 4.16e-12  bse 2.95e-15  frac_h2 4.16e-12  pvalue 8.81e-14
  N200-L5            d0 5.82e-13  refined: beta 4.01e-13  bse 8.76e-16  frac_h2 4e-13  pvalue 8.58e-14
  N300-L4            d0 1.74e-10  refined: beta 1.14e-12  bse 2.52e-15  frac_h2 1.14e-12  pvalue 2.02e-13
  N385-L4            d0 1.44e-10  refined: beta 1.8e-13  bse 1.81e-15  frac_h2 1.8e-13  pvalue 2.53e-13
  N392-L0            d0 6.62e-13  refined: beta 1.66e-12  bse 4.64e-15  frac_h2 1.66e-12  pvalue 2.4e-13
  N520-L0            d0 6.27e-13  refined: beta 4.57e-12  bse 2.34e-15  frac_h2 4.57e-12  pvalue 2.74e-12
  N660-L4            d0 1.65e-10  refined: beta 4.05e-12  bse 6.64e-15  frac_h2 4.05e-12  pvalue 4.34e-13
  N680-L4            d0 1.42e-10  refined: beta 2.6e-12  bse 2.26e-15  frac_h2 2.6e-12  pvalue 2.45e-12
  N760-L5            d0 3.92e-13  refined: beta 3.12e-12  bse 9.55e-15  frac_h2 3.12e-12  pvalue 5.37e-13
  N1032-L4           d0 1.49e-10  refined: beta 2.03e-12  bse 1.79e-15  frac_h2 2.03e-12  pvalue 7.38e-13
  N515-D3-L4         d0 9.92e-11  refined: beta 5.71e-13  bse 1.92e-15  frac_h2 5.71e-13  pvalue 4.28e-13
  N520-L3            d0 3.42e-08  refined: beta 9.39e-12  bse 4.89e-13  frac_h2 9.49e-12  pvalue 3.96e-12
  N520-L6            d0 2.11e-15  refined: beta 2.4e-12  bse 1.88e-15  frac_h2 2.4e-12  pvalue 2.41e-12
  N520-L7            d0 1.57e-15  refined: beta 4.51e-13  bse 1.57e-15  frac_h2 4.51e-13  pvalue 2.51e-12
  N648-L4-afcompact  d0 1.2e-10  refined: beta 2.21e-13  bse 1.79e-15  frac_h2 2.21e-13  pvalue 3.6e-13
  N520-L4-V20000     d0 1.54e-10  refined: beta 8.66e-12  bse 2.73e-15  frac_h2 8.66e-12  pvalue 2.83e-12

Rows the reference is good on.  beta's numerator x^T K^-1 y is a cancelling fp64 sum in the oracle as well: on a row whose beta is 2e-4 / 2e-6
of the median |beta| (one in 513 / two in 20 000 as first drawn) the oracle's own beta is 9.4e-11 / 2.1e-9 off a longdouble numerator, the
engine's 9.1e-11 / 3.0e-9 (1e-14 of the median |beta| each; bse on those rows 1.6e-15 / 2.7e-15), and the deviation read 1.85e-10 at
N520-L7 and 8.87e-10 at N520-L4-V20000: not a measure of the contraction.  A 1e-10 ceiling needs a reference ten times better, so a row on
which the oracle's beta is off by more than REF_ERR = 1e-11 (tests/_lmm_sweep.py beta_error_of, itself held to the whole restatement by the
CPU test) is drawn again by the same recipe before anything runs on the device -- 0 to 3 rows per case, never more than one in a hundred;
every row of the final set is fitted and compared."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _lmm_sweep import FIELDS, beta_error_of, deviations, design, fmt, rows  # noqa: E402

H2 = 0.37
# what the reference's own beta may be off by on a row that is compared: a tenth of the 1e-10 that no ceiling may exceed
REF_ERR = 1e-11
OUT = ("prep", "beta", "bse", "pvalue", "frac_h2")

# id: (N, D, n_limbs, route, AF window, V)
CASES = {
    "N200-L4": (200, 1, 4, "", None, 513),                 # two row tiles: the two-wave kernel, main pass and extra-limb pass
    "N200-L5": (200, 1, 5, "", None, 513),
    "N300-L4": (300, 1, 4, "", None, 513),                 # four row tiles, the wide kernel: three full segments, last tile all padding
    "N385-L4": (385, 1, 4, "", None, 513),                 # ragged tile, 1 valid row
    "N392-L0": (392, 1, 0, "", None, 513),                 # ragged tile, 8 valid rows
    "N520-L0": (520, 1, 0, "", None, 513),                 # last row tile all padding
    "N660-L4": (660, 1, 4, "", None, 513),                 # 1 valid 32-row sub-tile in the last tile
    "N680-L4": (680, 1, 4, "", None, 513),                 # 2 valid 32-row sub-tiles
    "N760-L5": (760, 1, 5, "", None, 513),                 # 4 valid 32-row sub-tiles
    "N1032-L4": (1032, 1, 4, "", None, 513),               # ragged tile at nf = 8
    "N515-D3-L4": (515, 3, 4, "", None, 513),              # covariates and ragged tile
    "N520-L3": (520, 1, 3, "", None, 513),
    "N520-L6": (520, 1, 6, "", None, 513),
    "N520-L7": (520, 1, 7, "", None, 513),
    "N648-L4-afcompact": (648, 1, 4, "afcompact=2", (0.17, 0.83), 513),      # the pass after the gathered image
    "N520-L4-V20000": (520, 1, 4, "", None, 20000),        # more than 16 384 listed variants
}

# per case and field, the run with every row refined: 10x the first measured maximum, rounded up, never above 1e-10
CEIL = {
    "N200-L4": {"beta": 5e-11, "bse": 3e-14, "frac_h2": 5e-11, "pvalue": 9e-13},
    "N200-L5": {"beta": 5e-12, "bse": 9e-15, "frac_h2": 5e-12, "pvalue": 9e-13},
    "N300-L4": {"beta": 2e-11, "bse": 3e-14, "frac_h2": 2e-11, "pvalue": 3e-12},
    "N385-L4": {"beta": 2e-12, "bse": 2e-14, "frac_h2": 2e-12, "pvalue": 3e-12},
    "N392-L0": {"beta": 2e-11, "bse": 5e-14, "frac_h2": 2e-11, "pvalue": 3e-12},
    "N520-L0": {"beta": 5e-11, "bse": 3e-14, "frac_h2": 5e-11, "pvalue": 3e-11},
    "N660-L4": {"beta": 5e-11, "bse": 7e-14, "frac_h2": 5e-11, "pvalue": 5e-12},
    "N680-L4": {"beta": 3e-11, "bse": 3e-14, "frac_h2": 3e-11, "pvalue": 3e-11},
    "N760-L5": {"beta": 4e-11, "bse": 1e-13, "frac_h2": 4e-11, "pvalue": 6e-12},
    "N1032-L4": {"beta": 3e-11, "bse": 2e-14, "frac_h2": 3e-11, "pvalue": 8e-12},
    "N515-D3-L4": {"beta": 6e-12, "bse": 2e-14, "frac_h2": 6e-12, "pvalue": 5e-12},
    "N520-L3": {"beta": 1e-10, "bse": 5e-12, "frac_h2": 1e-10, "pvalue": 4e-11},
    "N520-L6": {"beta": 3e-11, "bse": 2e-14, "frac_h2": 3e-11, "pvalue": 3e-11},
    "N520-L7": {"beta": 5e-12, "bse": 2e-14, "frac_h2": 5e-12, "pvalue": 3e-11},
    "N648-L4-afcompact": {"beta": 3e-12, "bse": 2e-14, "frac_h2": 3e-12, "pvalue": 4e-12},
    "N520-L4-V20000": {"beta": 9e-11, "bse": 3e-14, "frac_h2": 9e-11, "pvalue": 3e-11},
}

# the tolerance that refines every row: below every row's bound.  Six main limbs leave every bound under 1e-13 already (4.3e-14 at most, measured),
# so 1e-13 would refine nothing there
TOL_ALL = {0: 1e-13, 3: 1e-13, 4: 1e-13, 5: 1e-13, 6: 1e-16, 7: 1e-13}

_inputs, _runs = {}, {}


def _macs(N, L, wide=True):
    """int8 MACs per variant of the main pass as shk_lmm_quadform issues them without the ragged route: NR = 2 ceil(N / 256) row tiles of 128; the
    two-wave kernel (NR < 4, or SEERHIP_ROUTE qf=0) contracts every tile, the wide one NR - 1 full segments and the 32-row sub-tiles of the last
    tile that hold samples (4 of them: a full segment)."""
    NR = 2 * ((N + 255) // 256)
    last = N - (NR - 1) * 128
    nit = 4 if not (wide and NR >= 4) else 0 if last <= 0 else 1 if last <= 32 else 2 if last <= 64 else 4
    nfull, nit = (NR, 0) if nit == 4 else (NR - 1, nit)
    return L * (nfull * (nfull + 1) * 128 * 64 + 2 * (nfull + 1) * 32 * nit * 64)


def _ragged(N):
    """the sample counts whose last 1 .. 8 rows go to k_lmm_ragged_i8 (lmm_params.h lmm_ragged_shape)"""
    return N // 128 >= 3 and 1 <= N % 128 <= 8


def _case(cfg):
    """inputs and the oracle's answers of a case, made once"""
    if cfg not in _inputs:
        from oracle import oracle as orc
        orc.set_threads(min(16, len(os.sched_getaffinity(0))))
        N, D, limbs, route, af, V = CASES[cfg]
        U, S, covar, y = design(N, D, 3000 + N + D + limbs, False, binary_col0=False)
        Kv, _ = rows(N, V, 4000 + N + D + limbs, edges=False)
        o = orc.LmmOracle(U, S, y, covar)
        rng = np.random.default_rng(5000 + N + D + limbs)
        redrawn = 0
        for _ in range(6):                                         # rows the reference itself is poor on are drawn again, same recipe
            want = o.block(H2, Kv.astype(float))
            poor = np.flatnonzero(~(beta_error_of(want[0], U, S, y, covar, H2, Kv) <= REF_ERR))
            if poor.size == 0:
                break
            redrawn += poor.size
            for v in poor:
                Kv[v] = rng.random(N) < (0.9 if v < V // 8 else rng.uniform(0.02, 0.98))
        else:
            raise AssertionError("%s: the reference is still above %g on rows %s" % (cfg, REF_ERR, poor[:8]))
        print("LMM-SWEEP refined %-18s rows drawn again %d of %d" % (cfg, redrawn, V))
        assert redrawn <= V // 100 + 1, (cfg, redrawn)             # a handful: the rows stay the recipe's
        m = Kv.sum(axis=1)
        assert ((m > 0) & (m < N)).all()
        kept = np.ones(V, bool)
        if af:
            f = Kv.mean(axis=1); kept = (f >= af[0]) & (f <= af[1])
            assert 0.2 < 1.0 - kept.mean() < 0.45
            want = o.block(H2, Kv[kept].astype(float))
        assert all(np.isfinite(w).all() for w in want)
        _inputs[cfg] = (U, S, covar, y, Kv, kept, want)
    return _inputs[cfg]


def _run(cfg, route=None):
    """the three runs of a case under a route (default: the case's own), made once: [(outputs, info)] for tol = 0, 1e-13, in between"""
    N, D, limbs, own, af, V = CASES[cfg]
    route = own if route is None else route
    if (cfg, route) not in _runs:
        from pyseer_amd.engine import Engine, pack_variants
        U, S, covar, y, Kv, kept, want = _case(cfg)
        bits = pack_variants(Kv)
        saved = os.environ.get("SEERHIP_ROUTE")
        try:
            if route:
                os.environ["SEERHIP_ROUTE"] = route
            else:
                os.environ.pop("SEERHIP_ROUTE", None)
            e = Engine(N)
            if af:
                e.set_af_filter(*af)
            e.lmm_setup(U, S, y, covar, H2, n_limbs=limbs)
            out = []
            e.set_lmm_tol(0.0); out.append((e.lmm_batch(bits), e.lmm_info()))
            e.set_lmm_tol(TOL_ALL[limbs]); out.append((e.lmm_batch(bits), e.lmm_info()))
            tol = 0.5 * (out[0][1]["bound_rel_typical"] + out[0][1]["bound_rel_max_last_batch"])
            e.set_lmm_tol(tol); out.append((e.lmm_batch(bits), e.lmm_info()))
            e.close()
        finally:
            if saved is None:
                os.environ.pop("SEERHIP_ROUTE", None)
            else:
                os.environ["SEERHIP_ROUTE"] = saved
        _runs[(cfg, route)] = out
    return _runs[(cfg, route)]


def _identical(a, b, what):
    assert np.array_equal(a["flags"], b["flags"]), what
    for f in OUT:
        assert np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64)), (what, f)


@pytest.mark.parametrize("cfg", list(CASES))
def test_every_limb_reaches_the_statistics(cfg):
    N, D, limbs, route, af, V = CASES[cfg]
    U, S, covar, y, Kv, kept, want = _case(cfg)
    (r0, i0), (r1, i1), (r2, i2) = _run(cfg)
    nfit = int(kept.sum())
    sub = lambda r: {f: r[f][kept] for f in FIELDS}                # noqa: E731
    dev0, dev1 = deviations(sub(r0), want), deviations(sub(r1), want)
    L, E = i0["n_limbs"], i0["extra_limbs"]
    print("LMM-SWEEP refined %-18s n_limbs %d->%d extra_limbs %d  unrefined: %s  refined: %s  bound_typical %.3g bound_max %.3g -> %.3g  "
          "refined rows %d / %d / %d of %d" % (cfg, limbs, L, E, fmt(dev0), fmt(dev1), i0["bound_rel_typical"], i0["bound_rel_max_last_batch"],
                                               i1["bound_rel_max_last_batch"], i0["refined_last_batch"], i1["refined_last_batch"],
                                               i2["refined_last_batch"], nfit))
    assert (L == limbs or limbs == 0) and E == min(2, 7 - L)
    # the kernel the main pass took: every tile below four row tiles (the two-wave kernel), the wide kernel's segments above, fewer with the ragged route
    macs = {i["int8_macs_per_variant"] for i in (i0, i1, i2)}
    assert len(macs) == 1
    if _ragged(N):
        assert macs.pop() < _macs(N, L)
    else:
        assert macs.pop() == _macs(N, L) and (N > 256 or _macs(N, L) == L * 2 * 3 * 128 * 64)
    for r in (r0, r1, r2):                                         # AF-filtered rows: no statistics, before and after the refinement
        assert all(np.isnan(r[f][~kept]).all() for f in FIELDS) and ((r["flags"][~kept] & 0x10001) == 0x10001).all()
    # never refine: the certificate covers what is measured
    assert i0["refined_last_batch"] == 0
    d0 = dev0["bse"]
    if d0 > 1e-12:
        assert 2 * d0 <= 1.01 * i0["bound_rel_max_last_batch"], (d0, i0["bound_rel_max_last_batch"])
    # refine every row
    assert i1["refined_last_batch"] == (nfit if E > 0 else 0), i1
    if L <= 4:
        assert d0 > 1e-12 and dev1["bse"] <= d0 / 100, (d0, dev1["bse"])
    # in between: only the rows above the tolerance are refined, and those land exactly where the all-refined run lands
    same = r2["bse"][kept] == r0["bse"][kept]; refined = r2["bse"][kept] == r1["bse"][kept]
    assert (same | refined).all() and refined.sum() >= i2["refined_last_batch"]
    if E > 0:
        assert 0 < i2["refined_last_batch"] < nfit, i2
    # every field of the all-refined run under its ceiling
    assert cfg in CEIL, "no ceilings for %s: measured %s" % (cfg, fmt(dev1))
    for f in FIELDS:
        assert CEIL[cfg][f] <= 1e-10 and dev1[f] <= CEIL[cfg][f], (cfg, f, dev1[f], CEIL[cfg][f])


@pytest.mark.parametrize("cfg", ["N385-L4", "N680-L4"])
@pytest.mark.parametrize("route", ["ragged=0", "qf=0"])
def test_refined_run_does_not_depend_on_the_route(cfg, route):
    N, L = CASES[cfg][0], CASES[cfg][2]
    for (a, ia), (b, ib) in zip(_run(cfg), _run(cfg, route)):
        _identical(a, b, (cfg, route))
        assert ia["refined_last_batch"] == ib["refined_last_batch"]
        # the route ran something else: qf=0 the two-wave kernel over every tile, ragged=0 the wide kernel's narrow segment instead of the ragged
        # kernel -- where there is a ragged tile (N = 680 has 40 rows in its last tile: the key changes nothing there)
        assert ib["int8_macs_per_variant"] == _macs(N, L, wide=route != "qf=0")
        assert (ib["int8_macs_per_variant"] > ia["int8_macs_per_variant"]) == (route == "qf=0" or _ragged(N))


def test_refined_run_behind_the_af_compaction_is_bit_identical():
    cfg = "N648-L4-afcompact"
    for (a, ia), (b, ib) in zip(_run(cfg), _run(cfg, "afcompact=0")):
        _identical(a, b, cfg)
        assert ia["refined_last_batch"] == ib["refined_last_batch"]
