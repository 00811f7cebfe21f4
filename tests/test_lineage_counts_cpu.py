"""The numpy yardsticks of the count route (tests/_lineage_ref.py; SEERHIP_ROUTE lin_counts, csrc/route.h), without a device: the dense form
-- the reference's arithmetic through np.linalg.inv -- is held to oracle.lineage_effect where the oracle reaches (63 columns), the reduced
form on the clusters' carrier counts (what k_glm_lineage_counts runs) to the dense one on the inputs of tests/test_lineage_counts_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lineage_ref as R
from test_oracle_golden import _same_or_tied


@pytest.mark.parametrize("l", [3, 49, 63])
def test_dense_form_vs_oracle(l):
    from oracle import oracle as orc
    N, V = 200, 40
    cluster_of, K = R.oracle_case(N, l, V, 5 + l)
    lin = R.design(cluster_of, l)
    got = [R.argmax_dense(lin, k) for k in K]
    want = [orc.lineage_effect(lin, None, k.astype(float)) for k in K]
    assert any(w is not None for w in want) and any(w is None for w in want)
    _same_or_tied(got, want, lin, None, K)


def test_fixture_is_the_dense_form():
    """tests/golden/lincounts_dense.npz holds wald_dense of the yardstick cases' rows: recomputed here for a few rows of the cases
    that take milliseconds per row."""
    for (N, l) in R.YARDSTICK_CASES[:2]:
        tame = l == 65
        cluster_of, K = R.yardstick_case(N, l, tame=tame)
        lin = R.design(cluster_of, l)
        rows, _ = R.fixture_rows(N, l, tame)
        for v in list(range(0, R.YARDSTICK_ROWS, 25)) + [3, 7, 11]:
            wd = R.wald_dense(lin, K[v])
            if not R.well_conditioned(*R.counts(cluster_of, l, K[v])):
                continue                                                # (rounding noise decides those: another LAPACK, another answer)
            assert (wd is None) == (rows[v] is None), (N, l, v)
            if wd is not None:
                am, mx, near = rows[v]
                assert np.isclose(mx, np.max(wd), rtol=R.DELTA, atol=0) and wd[am] >= np.max(wd) * (1 - R.DELTA)
                assert all(np.isclose(wd[i], x, rtol=R.DELTA, atol=0) for i, x in near.items())


@pytest.mark.parametrize("tame", [False, True])
@pytest.mark.parametrize("N,l", R.YARDSTICK_CASES)
def test_reduced_form_vs_dense(N, l, tame):
    """On the GPU test's own rows, where the reference is well conditioned (_lineage_ref.well_conditioned): identical Nones, argmax equal
    or tied within DELTA (for clusters that are not twins, in at most 10 % of the rows), and the largest relative difference between the
    two forms' Wald values -- over the clusters that can decide a row, FIXTURE_NEAR -- under twice MEASURED_WALD_DIFF = DELTA / 10, the figure
    DELTA was set from.  On the other rows the two forms, like any two implementations, may differ: counted and printed."""
    cluster_of, K = R.yardstick_case(N, l, tame=tame)
    rows, _ = R.fixture_rows(N, l, tame)
    cnt = [R.counts(cluster_of, l, k) for k in K]
    cond = [R.well_conditioned(*c) for c in cnt]
    got, worst = [], 0.0
    for v in range(R.YARDSTICK_ROWS):
        wc = R.wald_counts(*cnt[v])
        got.append(-1 if wc is None else int(np.argmax(wc)))
        if cond[v] and wc is not None and rows[v] is not None:
            worst = max(worst, R.wald_diff(rows[v][2], wc))
    tied, loose = R.check_rows(got, rows, cond, l, cnt=cnt, loose_max=0.05 * (len(cond) - sum(cond)) + 3)   # (measured: at most 8 of 300)
    print("N %d l %d tame %d: %d rows None, %d well-conditioned, %d of them tied, largest Wald difference %.3g; %d of the others differ about None" %
          (N, l, tame, sum(r is None for r in rows), sum(cond), tied, worst, loose))
    assert worst <= 2 * R.MEASURED_WALD_DIFF
    assert not tame or sum(cond) >= 150
