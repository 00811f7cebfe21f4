"""The ragged row tile of the LMM contraction.  With N = 128 nf + r and 1 <= r <= LMM_RAGGED_MAX the wide kernel
(k_lmm_quadform_i8w) stops at the last full 128-row tile and k_lmm_ragged_i8 contracts the r remaining rows, all limbs stacked, adding its exact
integers to the wide kernel's per-limb partial sums.  Nothing downstream may see a difference: every output double is compared bit for bit
against the one-kernel route (SEERHIP_ROUTE ragged=0) and the two-wave kernel (qf=0), with the AF compaction's gathered image as well, and
against the oracle at the tolerances of test_lmm_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lmm_gpu import RTOL, _random_lmm, close, engine_mod  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MAX = int(re.search(r"#define LMM_RAGGED_MAX (\d+)", open(os.path.join(ROOT, "pyseer_amd", "csrc", "lmm_params.h")).read()).group(1))
FIELDS = ("prep", "beta", "bse", "pvalue", "frac_h2")
H2 = 0.33

# (N, V, limbs): r = 1 with three segments, the smallest wide case | r = 8 | the ragged tile is not the last one (NR = 2 ceil(N / 256) row tiles) |
# five limbs: 40 stacked rows, two MFMA row tiles | several variant tiles | r = 1, ragged tile not the last | both sides of the threshold
SHAPES = [(385, 513, 4), (392, 700, 0), (520, 700, 0), (648, 512, 5), (1032, 1536, 4), (2049, 600, 4), (384 + R_MAX, 513, 0), (384 + R_MAX + 1, 513, 0)]

_inputs, _runs = {}, {}


def _case(N, V):
    """inputs of a shape, made once: random rows, V/8 majority-carrier rows (stored complemented), rows whose ragged samples are all 0 / all 1"""
    if (N, V) not in _inputs:
        U, S, covar, y, Kv = _random_lmm(N, 1, 77 + N, V)
        Kv[: V // 8] = (np.random.default_rng(3).random((V // 8, N)) < 0.9).astype(np.uint8)
        r0 = N // 128 * 128
        Kv[V // 8: V // 8 + 8, r0:] = 0; Kv[V // 8 + 8: V // 8 + 16, r0:] = 1       # minority-carrier rows: stored as given
        Kv[0:4, r0:] = 1; Kv[4:8, r0:] = 0                                          # majority-carrier rows: stored complemented
        _inputs[(N, V)] = (U, S, covar, y, Kv)
    return _inputs[(N, V)]


def _run(engine_mod, monkeypatch, N, V, limbs, route):
    key = (N, V, limbs, route)
    if key not in _runs:
        Engine, pack = engine_mod
        U, S, covar, y, Kv = _case(N, V)
        if route:
            monkeypatch.setenv("SEERHIP_ROUTE", route)
        else:
            monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
        e = Engine(N)
        e.lmm_setup(U, S, y, covar, H2, n_limbs=limbs)
        out = e.lmm_batch(pack(Kv)); info = e.lmm_info(); e.close()
        monkeypatch.delenv("SEERHIP_ROUTE", raising=False)
        _runs[key] = (out, info)
    return _runs[key]


def _identical(a, b, what):
    assert np.array_equal(a["flags"], b["flags"]), what
    for f in FIELDS:
        assert np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64)), (what, f)


@pytest.mark.parametrize("N,V,limbs", SHAPES)
def test_ragged_route_is_bit_identical_to_both_other_routes(engine_mod, monkeypatch, N, V, limbs):
    new, _ = _run(engine_mod, monkeypatch, N, V, limbs, "")
    assert np.isfinite(new["bse"]).sum() > V // 2
    _identical(new, _run(engine_mod, monkeypatch, N, V, limbs, "ragged=0")[0], (N, "ragged=0"))
    _identical(new, _run(engine_mod, monkeypatch, N, V, limbs, "qf=0")[0], (N, "qf=0"))


@pytest.mark.parametrize("N,V,limbs", [(392, 700, 0), (648, 512, 5)])
def test_ragged_route_vs_oracle(engine_mod, monkeypatch, N, V, limbs):
    from oracle import oracle as orc
    U, S, covar, y, Kv = _case(N, V)
    r, info = _run(engine_mod, monkeypatch, N, V, limbs, "")
    assert info["int8_macs_per_variant"] < _run(engine_mod, monkeypatch, N, V, limbs, "ragged=0")[1]["int8_macs_per_variant"]   # the new route ran
    wb, ws, wf, wp = orc.LmmOracle(U, S, y, covar).block(H2, Kv.astype(float))
    close(r["beta"], wb, atol=1e-12, what="beta"); close(r["bse"], ws, what="bse")
    close(r["frac_h2"], wf, atol=1e-9, what="frac"); close(r["pvalue"], wp, atol=1e-300, what="p")


def test_ragged_route_through_the_af_compaction(engine_mod, monkeypatch):
    """afcompact=2 contracts a gathered image of the kept columns (its own T and q): the ragged kernel reads and adds to whatever the launcher was
    given.  An AF window that filters about 30 % of the rows; identical outputs with the compaction forced and off."""
    Engine, pack = engine_mod
    N, V = 648, 1500
    U, S, covar, y, Kv = _random_lmm(N, 1, 31, V)                  # allele frequencies uniform in 0.02 .. 0.98
    bits = pack(Kv)
    af = Kv.mean(axis=1); kept = (af >= 0.17) & (af <= 0.83)
    assert 0.2 < 1.0 - kept.mean() < 0.4
    res = []
    for on in ("2", "0"):
        monkeypatch.setenv("SEERHIP_ROUTE", "afcompact=" + on)
        e = Engine(N); e.set_af_filter(0.17, 0.83)
        e.lmm_setup(U, S, y, covar, 0.41)
        res.append(e.lmm_batch(bits)); res.append(e.lmm_batch(bits)); e.close()
    monkeypatch.delenv("SEERHIP_ROUTE")
    for other in res[1:]:
        assert np.array_equal(res[0]["flags"], other["flags"])
        for f in FIELDS:
            assert np.array_equal(res[0][f].view(np.uint64), other[f].view(np.uint64)), f
    assert np.isnan(res[0]["pvalue"][~kept]).all() and np.isfinite(res[0]["pvalue"][kept]).mean() > 0.9


@pytest.mark.parametrize("N,V,limbs", [(648, 512, 5), (392, 700, 0), (520, 700, 0)])
def test_lmm_info_counts_the_macs_as_issued(engine_mod, monkeypatch, N, V, limbs):
    """int8 MACs per variant: the wide kernel's full 128-row segments (segment I spans 2 (I + 1) tiles of 128 x 64) for every limb, plus the ragged
    kernel's padded rows x columns (L rows-rounded-up-to-8 stacked, rounded up to 32-row MFMA tiles -- an even number when more than one -- against
    2 nf + 1 sample blocks of 64).  Fewer than the one-kernel route issues for the same rows."""
    _, new = _run(engine_mod, monkeypatch, N, V, limbs, "")
    _, old = _run(engine_mod, monkeypatch, N, V, limbs, "ragged=0")
    L, nf, r = new["n_limbs"], N // 128, N % 128
    assert 1 <= r <= R_MAX
    mt = -(-L * ((r + 7) // 8 * 8) // 32)
    mt += mt & 1 if mt > 1 else 0
    assert new["int8_macs_per_variant"] == L * nf * (nf + 1) * 128 * 64 + mt * 32 * (2 * nf + 1) * 64
    NR = 2 * ((N + 255) // 256)
    last = N - (NR - 1) * 128                                      # the one-kernel route: a narrow last tile, or a full one in front of a padding tile
    nit = 0 if last <= 0 else 1 if last <= 32 else 2 if last <= 64 else 4
    assert old["int8_macs_per_variant"] == L * ((NR - 1) * NR * 128 * 64 + 2 * NR * 32 * nit * 64)
    assert new["int8_macs_per_variant"] < old["int8_macs_per_variant"]
