"""Throughput of fit_lineage_effect on designs of cluster indicators at N = 5000: the dense kernels (glm_wide.hip) against the count kernel
(k_glm_lineage_counts, SEERHIP_ROUTE lin_counts) on the same rows in one process, then the count kernel alone beyond the dense kernels'
50 columns.  Prints one JSON line per measurement (variants/s through Engine.lineage_batch: upload, repack, kernel, download)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyseer_amd import _route
from pyseer_amd.engine import Engine, pack_variants


def run(N, l, V, lin_counts, reps=3):
    rng = np.random.default_rng(3)
    cl = rng.integers(0, l + 1, N)
    lin = np.zeros((N, l)); lin[np.arange(N)[cl > 0], cl[cl > 0] - 1] = 1.0
    base = rng.uniform(0.3, 0.7, (256, l + 1))
    K = (rng.random((256, N)) < base[:, cl]).astype(np.uint8)
    bits = np.tile(pack_variants(K), (V // 256, 1))
    os.environ["SEERHIP_ROUTE"] = _route.with_route(os.environ.get("SEERHIP_ROUTE"), lin_counts=lin_counts)
    e = Engine(N)
    e.lineage_setup(lin, None)
    first = e.lineage_batch(bits[:256])
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter(); e.lineage_batch(bits); best = min(best, time.perf_counter() - t0)
    e.close()
    print(json.dumps({"N": N, "clusters": l, "V": V, "route": "counts" if lin_counts == 1 or l + 1 > 50 else "dense", "seconds": round(best, 6),
                      "variants_per_s": round(V / best, 1), "fitted": int((first >= 0).sum())}), flush=True)
    return first


if __name__ == "__main__":
    a = run(5000, 30, 8192, 0, reps=2)
    b = run(5000, 30, 8192, 1)
    print(json.dumps({"N": 5000, "clusters": 30, "rows_compared": len(a), "same_answer": int((a == b).sum())}), flush=True)
    run(5000, 30, 1 << 20, 1)
    run(5000, 200, 1 << 20, 1)
    run(5000, 1000, 1 << 18, 1)
