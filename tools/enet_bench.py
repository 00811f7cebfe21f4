#!/usr/bin/env python
"""Times the whole-genome elastic net on synthetic k-mers (the benchmark's AF mix): upload, the correlation pass (k_enet_moments: it reads
every row once, so its rate against the HBM roof is the yardstick of the streaming kernels), and the cross-validated fit (k_enet_cd
coordinate steps per second, KKT rounds).  One JSON line per measurement; warm-up run first, then --repeats timed runs (median, min, max).

    python tools/enet_bench.py --variants 100000 --samples 5000 --n-lambda 5"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(P, N, seed):
    rng = np.random.default_rng(seed)
    af = np.where(rng.random(P) < 0.7, rng.uniform(0.01, 0.1, P), rng.uniform(0.1, 0.5, P))
    rows = np.zeros((P, ((N + 63) // 64) * 8), np.uint8)
    for s in range(0, P, 20000):                                     # in slabs: the unpacked matrix of 1e7 rows does not fit a host
        K = rng.random((min(20000, P - s), N)) < af[s:s + 20000, None]
        pk = np.packbits(K, axis=1, bitorder="little")
        rows[s:s + pk.shape[0], :pk.shape[1]] = pk
    return rows


def stats(ts):
    return dict(median_s=float(np.median(ts)), min_s=float(np.min(ts)), max_s=float(np.max(ts)), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--n-folds", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.0069)
    ap.add_argument("--n-lambda", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=1e-7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true", help="the streaming kernels only")
    ap.add_argument("--continuous", action="store_true")
    o = ap.parse_args()
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, assign_folds
    P, N = o.variants, o.samples
    rows = synth(P, N, 1)
    rng = np.random.default_rng(2)
    K10 = np.unpackbits(rows[:10], axis=1, bitorder="little")[:, :N].astype(float)
    lin = K10.T @ rng.normal(0, 1, 10)
    y = lin + rng.normal(0, 1, N) if o.continuous else (rng.random(N) < 1 / (1 + np.exp(-(lin - np.median(lin))))).astype(float)
    e = Engine(N)
    ts = []
    for r in range(o.repeats + 1):
        M = EnetMatrix(e, P)
        t = time.perf_counter(); M.append(rows); dt = time.perf_counter() - t
        if r:
            ts.append(dt)
        if r < o.repeats:
            M.close()
    print(json.dumps(dict(what="upload", variants=P, samples=N, bytes=int(rows.nbytes), gb_per_s=rows.nbytes / np.median(ts) / 1e9, **stats(ts))), flush=True)
    M.correlations(y)
    ts = []
    for r in range(o.repeats):
        t = time.perf_counter(); M.correlations(y); ts.append(time.perf_counter() - t)
    print(json.dumps(dict(what="correlations (k_enet_moments + copy of the result)", variants=P, samples=N, row_bytes_read=int(rows.nbytes),
                          gb_per_s=rows.nbytes / np.median(ts) / 1e9, hbm_roof_gb_per_s=8000, **stats(ts))), flush=True)
    V = rng.normal(size=(o.n_folds + 1, N))
    M.carrier_sums(V)
    ts = []
    for r in range(o.repeats):
        t = time.perf_counter(); M.carrier_sums(V); ts.append(time.perf_counter() - t)
    print(json.dumps(dict(what="carrier sums of %d vectors (k_enet_grad + upload of the vectors + copy of the %d x P result)" % (V.shape[0], V.shape[0]),
                          variants=P, samples=N, row_bytes_read=int(rows.nbytes), result_bytes=int(8 * V.shape[0] * P),
                          gb_per_s_of_rows=rows.nbytes / np.median(ts) / 1e9, hbm_roof_gb_per_s=8000, **stats(ts))), flush=True)
    if not o.no_fit:
        fold = assign_folds(N, o.n_folds, 1)
        t = time.perf_counter()
        fit = M.fit(y, o.continuous, o.alpha, fold_id=fold, n_folds=o.n_folds, thresh=o.thresh, n_lambda=o.n_lambda)
        dt = time.perf_counter() - t
        print(json.dumps(dict(what="fit", variants=P, samples=N, n_folds=o.n_folds, alpha=o.alpha, thresh=o.thresh, n_lambda_asked=o.n_lambda,
                              n_lambda_fitted=fit.n_lambda, seconds=dt, kkt_rounds=fit.kkt_rounds, cd_sweeps=int(fit.cd_sweeps),
                              cd_steps=int(fit.cd_steps), cd_steps_per_s_of_the_whole_fit=fit.cd_steps / dt, state_in_lds=fit.state_in_lds,
                              nzero_last=int(fit.nzero[-1]), i_min=fit.i_min)), flush=True)
    M.close()
    e.close()


if __name__ == "__main__":
    main()
