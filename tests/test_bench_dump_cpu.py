"""bench.py --dump-outputs: the arrays of the last timed step as float64 .npy files, the variants with a finite value in every array,
at most 64 MB in all; a larger step's output is written as a fixed, seeded sample of those variants (variant_index.npy says which), the
same on every run.  Host helpers only: the GPU run of the flag is tests/test_bench_inputs_gpu.py::test_bench_dump_outputs_repeat."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _glm_step(V, q, seed=5):
    rng = np.random.default_rng(seed)
    out = torch.from_numpy(rng.standard_normal((5 + q, V)))
    fl = torch.from_numpy(rng.integers(0, 1 << 19, V).astype(np.int32))
    return out, fl


def test_output_arrays_are_the_callers_fields():
    out, fl = _glm_step(300, 3)
    a = dict(bench.output_arrays(out, fl, False, 3))
    assert list(a) == ["prep", "pvalue", "kbeta", "bse", "intercept", "betas", "flags"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["kbeta"], out[2].numpy()) and np.array_equal(a["betas"], out[5:8].numpy().T)
    assert np.array_equal(a["flags"], fl.numpy().astype(np.float64))
    lm = dict(bench.output_arrays(out[:5], fl, True, 0))
    assert list(lm) == ["prep", "pvalue", "beta", "bse", "frac_h2", "flags"]
    assert np.array_equal(lm["frac_h2"], out[4].numpy())


def test_small_output_is_written_whole(tmp_path):
    out, fl = _glm_step(1000, 2)
    arrs = bench.output_arrays(out, fl, False, 2)
    info = bench.dump_outputs(str(tmp_path), arrs)
    assert info["variants"] == info["of_variants"] == 1000 and info["not_finite_left_out"] == 0
    assert np.array_equal(np.load(tmp_path / "variant_index.npy"), np.arange(1000, dtype=np.float64))
    for name, a in arrs:
        b = np.load(tmp_path / (name + ".npy"))
        assert b.dtype == np.float64 and np.array_equal(b, a)


def test_variants_without_finite_results_are_left_out(tmp_path):
    """Filtered rows (prep NaN; bse inf, as the LMM gives a monomorphic variant; a NaN in one covariate's beta) are not written."""
    out, fl = _glm_step(1000, 2)
    out[0, 3] = np.nan; out[3, 10] = np.inf; out[6, 500] = np.nan; out[1, 999] = -np.inf
    arrs = bench.output_arrays(out, fl, False, 2)
    info = bench.dump_outputs(str(tmp_path), arrs)
    keep = np.setdiff1d(np.arange(1000), [3, 10, 500, 999])
    assert info["variants"] == 996 and info["not_finite_left_out"] == 4
    assert np.array_equal(np.load(tmp_path / "variant_index.npy"), keep.astype(np.float64))
    for name, a in arrs:
        b = np.load(tmp_path / (name + ".npy"))
        assert np.isfinite(b).all() and np.array_equal(b, a[keep])


def test_large_output_is_a_fixed_sample_within_the_cap(tmp_path):
    out, fl = _glm_step(20000, 10)
    out[2, ::7] = np.nan
    arrs = bench.output_arrays(out, fl, False, 10)
    cap = 1 << 20
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        info = bench.dump_outputs(str(d), arrs, max_bytes=cap)
        files = sorted(os.listdir(d))
        assert files == sorted(n + ".npy" for n in info["arrays"])
        assert sum(os.path.getsize(d / f) for f in files) == info["bytes"] <= cap
        assert 0 < info["variants"] < 20000
        idx = np.load(d / "variant_index.npy")
        assert (np.diff(idx) > 0).all() and idx.dtype == np.float64 and (idx % 7 != 0).all()
        assert info["not_finite_left_out"] == len(range(0, 20000, 7))
        got = {f: np.load(d / f) for f in files}
        for name, a in arrs:
            assert np.array_equal(got[name + ".npy"], a[idx.astype(np.int64)])
        runs.append(got)
    assert all(np.array_equal(runs[0][f], runs[1][f]) for f in runs[0])
