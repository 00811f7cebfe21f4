"""sh_enet_ingest_calls (k_enet_ingest_calls_count / _scan / _scatter) through the ABI: load_all_vars' rule for a block of parsed rows with
missing calls, decided and stored on the device.

Every comparison is exact (integers and bytes).  The yardstick is numpy on the host plus the existing sh_enet_append(present, missing,
flip), never the new code: c = present, m = missing and not present, t = c + m over the first n bits; kept iff not skipped,
lo <= t <= hi and m <= mm; stored by its absences iff 2 t > n."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pack(K, rb):
    out = np.zeros((K.shape[0], rb), dtype=np.uint8)
    pk = np.packbits(K, axis=1, bitorder="little")
    out[:, :pk.shape[1]] = pk
    return out


def _pad_mask(n, rb):
    pad = np.zeros(rb * 8, dtype=np.uint8)
    pad[n:] = 1
    return np.packbits(pad, bitorder="little")


def _rule(P, Mi, skip, n, lo, hi, mm):
    """numpy: (kept indices, c, m, flip) of dense present / missing matrices (Mi may be None)"""
    c = P.sum(axis=1)
    m = np.zeros_like(c) if Mi is None else (Mi & ~P).sum(axis=1)
    t = c + m
    keep = (t >= lo) & (t <= hi) & (m <= mm)
    if skip is not None:
        keep &= skip == 0
    return np.nonzero(keep)[0], c, m, 2 * t > n


def _block(rng, V, n, rb, with_pad=True):
    dens = rng.choice([0.001, 0.01, 0.05, 0.3, 0.5, 0.7, 0.9, 0.98], size=V)
    mrate = rng.choice([0.0, 0.0, 0.01, 0.03, 0.1], size=V)
    u = rng.random((V, n))
    Mi = u < mrate[:, None]                                           # disjoint by construction: missing first, carriers among the rest
    P = ~Mi & (rng.random((V, n)) < dens[:, None])
    skip = (rng.random(V) < 0.15).astype(np.int32) * rng.integers(1, 3, V).astype(np.int32)
    clean_p, clean_m = _pack(P, rb), _pack(Mi, rb)
    dirty_p, dirty_m = clean_p, clean_m
    if with_pad:                                                      # random bits in the padding of both rows: neither counted nor stored
        pad = _pad_mask(n, rb)[None, :]
        dirty_p = clean_p | (rng.integers(0, 256, (V, rb)).astype(np.uint8) & pad)
        dirty_m = clean_m | (rng.integers(0, 256, (V, rb)).astype(np.uint8) & pad)
    return P, Mi, skip, clean_p, clean_m, dirty_p, dirty_m


CASES = [(63, (1, 64)), (64, (7, 1025)), (65, (1, 7, 64)), (127, (64, 4097)), (1000, (7, 1025)), (4097, (1, 1025, 4097))]


@pytest.mark.parametrize("n,Vs", CASES)
def test_random_blocks_against_numpy_and_append(n, Vs):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, call_bounds
    from pyseer_amd.packing import row_bytes_for
    rng = np.random.default_rng(7000 + n)
    rb = row_bytes_for(n)
    lo, hi, mm = call_bounds(n, 0.02, 0.97, 0.05)
    e1, e2 = Engine(n), Engine(n)
    M1, M2 = EnetMatrix(e1, 1), EnetMatrix(e2, sum(Vs))
    total = 0
    for V in Vs:
        P, Mi, skip, cp, cm, dp, dm = _block(rng, V, n, rb)
        want, c, m, flip = _rule(P, Mi, skip, n, lo, hi, mm)
        idx, n_p, n_m = M1.ingest_calls(dp, dm, skip, lo, hi, mm)
        assert idx.dtype == np.int32 and (idx == want).all()
        assert (n_p == c[want]).all() and (n_m == m[want]).all()
        M2.append(cp[want], cm[want], flip[want].astype(np.uint8))
        total += want.size
    assert M1.rows == M2.rows == total
    if total:
        got = M1.get_rows(np.arange(total))
        assert (got == M2.get_rows(np.arange(total))).all()
        assert not (got & _pad_mask(n, rb)[None, :]).any()
    M1.close(); M2.close()
    e1.close(); e2.close()


def test_overlapping_rows_agree_with_append():
    """The readers never set a sample in both rows; where a caller does, the sample is present (m counts missing & ~present), which is what
    k_enet_store makes of the same two rows."""
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import row_bytes_for
    n, V = 130, 40
    rng = np.random.default_rng(5)
    rb = row_bytes_for(n)
    P = rng.random((V, n)) < rng.choice([0.2, 0.6], size=V)[:, None]
    Mi = rng.random((V, n)) < 0.2                                      # overlaps P freely
    want, c, m, flip = _rule(P, Mi, None, n, 0, n, n)
    assert want.size == V and flip.any() and not flip.all()
    e1, e2 = Engine(n), Engine(n)
    M1, M2 = EnetMatrix(e1, 1), EnetMatrix(e2, V)
    idx, n_p, n_m = M1.ingest_calls(_pack(P, rb), _pack(Mi, rb), None, 0, n, n)
    assert (idx == want).all() and (n_p == c).all() and (n_m == m).all()
    M2.append(_pack(P, rb), _pack(Mi, rb), flip.astype(np.uint8))
    assert (M1.get_rows(np.arange(V)) == M2.get_rows(np.arange(V))).all()
    M1.close(); M2.close()
    e1.close(); e2.close()


def _one_row(n, rb, t, m):
    """a row with t - m carriers and m missing calls, disjoint"""
    P = np.zeros((1, n), dtype=bool); Mi = np.zeros((1, n), dtype=bool)
    P[0, :t - m] = True
    Mi[0, n - m:] = m > 0
    return P, Mi, _pack(P, rb), _pack(Mi, rb)


def test_boundaries_one_row_each():
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, call_bounds
    from pyseer_amd.packing import row_bytes_for
    n = 200
    rb = row_bytes_for(n)
    lo, hi, mm = call_bounds(n, 0.05, 0.95, 0.05)
    assert (lo, hi, mm) == (11, 189, 9)
    e1, e2 = Engine(n), Engine(n)
    M, R = EnetMatrix(e1, 1), EnetMatrix(e2, 64)
    n_ref = 0

    def one(t, m, kept, flipped=None, skip=None, lo_=lo):
        nonlocal n_ref
        P, Mi, bp, bm = _one_row(n, rb, t, m)
        before = M.rows
        idx, n_p, n_m = M.ingest_calls(bp, bm, skip, lo_, hi, mm)
        assert idx.size == (1 if kept else 0) and M.rows == before + idx.size
        if kept:
            assert idx[0] == 0 and n_p[0] == t - m and n_m[0] == m
            R.append(bp, bm, np.array([1 if flipped else 0], dtype=np.uint8))
            n_ref += 1
            got = M.get_rows([M.rows - 1])
            assert (got == R.get_rows([n_ref - 1])).all()
            want = (~P & ~Mi) if flipped else P
            assert (got == _pack(want, rb)).all()
    one(lo - 1, 0, False); one(lo, 0, True, False); one(hi, 0, True, True); one(hi + 1, 0, False)
    one(lo - 1, 3, False); one(lo, 3, True, False); one(hi, 3, True, True); one(hi + 1, 3, False)
    one(50, mm, True, False); one(50, mm + 1, False)
    one(n // 2, 0, True, False); one(n // 2, 4, True, False)          # 2 t = n: not flipped
    one(150, mm, True, True); one(150, mm + 1, False)
    one(n, n, False)                                                  # all missing
    one(0, 0, False)
    one(50, 0, False, skip=np.array([1], dtype=np.int32), lo_=0)     # skipped although it passes, lo = 0
    one(0, 0, False, skip=np.array([2], dtype=np.int32), lo_=0)
    one(0, 0, True, False, skip=np.array([0], dtype=np.int32), lo_=0)
    M.close(); R.close()
    e1.close(); e2.close()
    # 2 t = n + 1 is flipped (n odd)
    n = 201
    rb = row_bytes_for(n)
    e1 = Engine(n)
    M = EnetMatrix(e1, 1)
    for t, m, flipped in ((100, 0, False), (101, 0, True), (101, 5, True), (100, 5, False)):
        P, Mi, bp, bm = _one_row(n, rb, t, m)
        idx, _, _ = M.ingest_calls(bp, bm, None, 1, n, n)
        assert idx.size == 1
        assert (M.get_rows([M.rows - 1]) == _pack((~P & ~Mi) if flipped else P, rb)).all()
    M.close()
    e1.close()


@pytest.mark.parametrize("n", [65, 1000])
def test_without_missing_and_skip_it_is_sh_enet_ingest(n):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, count_bounds
    from pyseer_amd.packing import row_bytes_for
    rng = np.random.default_rng(n)
    rb = row_bytes_for(n)
    lo, hi = count_bounds(n, 0.02, 0.97, 0.05)
    _, _, _, _, _, dp, _ = _block(rng, 1500, n, rb)
    e1, e2 = Engine(n), Engine(n)
    M1, M2 = EnetMatrix(e1, 1), EnetMatrix(e2, 1)
    idx1, n_p, n_m = M1.ingest_calls(dp, None, None, lo, hi, 0)
    idx2, cnt = M2.ingest(dp, lo, hi)
    assert idx1.size > 0 and (idx1 == idx2).all() and (n_p == cnt).all() and not n_m.any()
    assert M1.rows == M2.rows and (M1.get_rows(np.arange(M1.rows)) == M2.get_rows(np.arange(M2.rows))).all()
    M1.close(); M2.close()
    e1.close(); e2.close()


def test_nothing_everything_growth_and_arguments():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix
    from pyseer_amd.packing import row_bytes_for
    n = 127
    rng = np.random.default_rng(11)
    rb = row_bytes_for(n)
    e1, e2 = Engine(n), Engine(n)
    M, R = EnetMatrix(e1, 1), EnetMatrix(e2, 4000)
    blocks = [_block(rng, V, n, rb) for V in (700, 1025, 300)]
    # nothing: an empty interval, a negative missing bound, every row skipped, an empty block
    P, Mi, skip, cp, cm, dp, dm = blocks[0]
    for args in ((None, 1, 0, n), (None, 0, n, -1), (np.ones(700, dtype=np.int32), 0, n, n)):
        idx, n_p, n_m = M.ingest_calls(dp, dm, *args)
        assert idx.size == 0 and n_p.size == 0 and n_m.size == 0 and M.rows == 0
    idx, _, _ = M.ingest_calls(np.zeros((0, rb), dtype=np.uint8), np.zeros((0, rb), dtype=np.uint8), None, 0, n, n)
    assert idx.size == 0 and M.rows == 0
    # everything, three calls into a matrix begun with capacity 1: the earlier rows stay
    total = 0
    for P, Mi, skip, cp, cm, dp, dm in blocks:
        want, c, m, flip = _rule(P, Mi, None, n, 0, n, n)
        idx, n_p, n_m = M.ingest_calls(dp, dm, None, 0, n, n)
        assert idx.size == P.shape[0] and (idx == np.arange(P.shape[0])).all() and (n_p == c).all() and (n_m == m).all()
        R.append(cp, cm, flip.astype(np.uint8))
        total += P.shape[0]
        assert M.rows == total and (M.get_rows(np.arange(total)) == R.get_rows(np.arange(total))).all()
    # a call forgets the last fit; the argument checks are sh_enet_ingest's
    y = rng.standard_normal(n)
    fit = M.fit(y, True, 0.5, fold_id=(np.arange(n) % 3).astype(np.int32), n_folds=3, n_lambda=4)
    fit.betas_at(0)
    M.ingest_calls(blocks[0][5][:1], blocks[0][6][:1], None, 1, 0, 0)
    with pytest.raises(_abi.SeerHipError):
        fit.betas_at(0)
    lib, h = e1._lib, e1._h
    assert lib.sh_enet_ingest_calls(h, None, None, None, 5, 0, n, n, None, None, None) < 0         # null argument
    assert lib.sh_enet_ingest_calls(h, None, None, None, -1, 0, n, n, None, None, None) < 0
    assert M.rows == total and (M.get_rows(np.arange(total)) == R.get_rows(np.arange(total))).all()
    M.close(); R.close()
    assert lib.sh_enet_ingest_calls(h, None, None, None, 0, 0, n, n, None, None, None) < 0        # before sh_enet_begin
    e1.close(); e2.close()


def test_call_bounds_are_the_literal_expressions():
    """No device: the bounds against the reference's float expressions (enet.py:95) at every count."""
    from pyseer_amd.enet import call_bounds, count_bounds
    for n in (50, 200):
        for min_af, max_af, max_missing in ((0.05, 0.95, 0.05), (0.0, 1.0, 0.05), (0.0, 0.95, 0.0), (0.1, 0.9, 0.1), (0.01, 0.99, 1.0),
                                            (0.5, 0.5, 0.05), (0.3, 0.1, 0.05), (0.05, 0.95, -1.0), (0.07, 0.93, 0.031)):
            lo, hi, mm = call_bounds(n, min_af, max_af, max_missing)
            for t in range(n + 1):
                af = float(t) / n
                assert (af > min_af and af < max_af) == (lo <= t <= hi), (n, min_af, max_af, t)
            for m in range(n + 1):
                assert (float(m) / n < max_missing) == (m <= mm), (n, max_missing, m)
            if max_missing > 0:
                assert (lo, hi) == count_bounds(n, min_af, max_af, max_missing)
    assert call_bounds(200, 0.05, 0.95, 0.05) == (11, 189, 9)        # m = 10 fails, m = 9 passes
    assert call_bounds(200, 0.05, 0.95, 0.0)[2] == -1
    assert call_bounds(50, 0.0, 0.95, 0.05) == (1, 47, 2)            # min_af = 0: af > 0 needs one carrier
    assert call_bounds(50, 0.5, 0.5, 0.05)[:2] == (1, 0)
