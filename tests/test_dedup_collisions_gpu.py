"""Pattern de-duplication (csrc/dedup_kernels.hip, api.hip dedup_wrap) on the inputs random data never gives it: rows that share all 64 bits
of the hash, rows whose probe runs off the end of the table, a table reused across batches of other sizes, batch sizes at the launch edges,
and the de-duplication nested inside the AF / prefilter compactions.  tests/_dd_hash.py restates the hash and models the table; it builds
the rows.  None of these inputs is out of the ordinary for a correct table: a collision costs one extra test of a row, a wrap one more probe.

Every sample count here is a multiple of 64 (128, 192) wherever rows are constructed from the hash: the solved last word of a colliding row
uses all 64 of its bits, and a row's last word is masked to the sample count before it is hashed.

What is held: outputs with de-duplication on are bit for bit those with it off (np.array_equal, NaN equal to NaN), sh_dedup_info reports the
model's count, and the outputs agree with the CPU oracle at the tolerances of tests/test_glm_gpu.py test_af_compaction_changes_nothing and
tests/test_lmm_gpu.py test_lmm_many_covariates_and_continuous_vs_oracle."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dd_hash as H

pytestmark = pytest.mark.gpu

GLM_FIELDS = ("prep", "pvalue", "kbeta", "bse", "intercept", "betas", "flags")
LMM_FIELDS = ("prep", "pvalue", "beta", "bse", "frac_h2", "flags")
H2 = 0.6


def close(a, b, rtol=1e-6, atol=0.0, what=""):
    a = np.atleast_1d(np.asarray(a, dtype=float)); b = np.atleast_1d(np.asarray(b, dtype=float))
    assert a.shape == b.shape, (a.shape, b.shape)
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))) | \
             (np.abs(a - b) <= atol + rtol * np.abs(b))
    assert ok.all(), "%s mismatch at %s: got %s want %s" % (what, np.argwhere(~ok)[:5].tolist(), a[~ok][:5], b[~ok][:5])


def same(got, want, fields, what=""):
    for f in fields:
        if not np.array_equal(got[f], want[f], equal_nan=True):
            g = np.asarray(got[f]).reshape(len(want["flags"]), -1); w = np.asarray(want[f]).reshape(g.shape)
            bad = np.flatnonzero(~((g == w) | ((g != g) & (w != w))).all(axis=1))
            raise AssertionError("%s: %s differs on %d rows, first %s: got %s want %s" % (what, f, len(bad), bad[:8], g[bad[:3]], w[bad[:3]]))


class Problem(object):
    """One sample count's phenotypes, covariates, null fits and LMM decomposition.  `assoc` (rows of 0/1, or None): rows the binary and the
    continuous phenotype are made to depend on, so that they pass a --filter-pvalue of 0.05."""

    def __init__(self, N, seed, assoc=None):
        from pyseer_amd.model import fit_null
        rng = np.random.default_rng(seed)
        self.N = N
        W = rng.standard_normal((N, 2)); self.W = W / np.abs(W).max(axis=0)
        noise = 0.3 * self.W[:, 0] + 0.3 * rng.standard_normal(N)
        score = np.zeros(N)
        if assoc is not None:                                          # a weighted vote of the rows; the weakest row's weight grows until
            wgt = np.ones(assoc.shape[0])                              # every row's correlation with the vote's outcome reaches 0.25
            for _ in range(200):
                score = wgt.dot(assoc - 0.5)
                r = np.array([np.corrcoef(a, score + noise > 0)[0, 1] for a in assoc])
                if r.min() >= 0.25:
                    break
                wgt[np.argmin(r)] *= 1.1
            assert r.min() >= 0.25, r
        self.y_bin = (score + noise > 0).astype(float)
        self.y_cont = 0.5 * score + self.W[:, 0] + rng.standard_normal(N)
        e0 = np.zeros((0, 0))
        self.null = {False: (fit_null(self.y_bin, self.W, e0, False).llf, fit_null(self.y_bin, self.W, e0, False, firth=True)),
                     True: (fit_null(self.y_cont, self.W, e0, True).llf, np.nan)}
        k = N - 1
        self.U = rng.standard_normal((N, k)) / np.sqrt(N)
        self.S = np.sort(rng.gamma(0.5, 2.0, k))[::-1].copy()
        self.covar = np.ones((N, 1))                                   # D = 1

    def y(self, cont):
        return self.y_cont if cont else self.y_bin

    def glm_engine(self, cont, dedup, pret=1.0):
        from pyseer_amd.engine import Engine
        e = Engine(self.N)
        e.set_af_filter(0.01, 0.99); e.set_dedup(dedup)
        e.glm_setup(self.y(cont), self.W, cont, self.null[cont][0], self.null[cont][1], pret, 1.0)
        return e

    def lmm_engine(self, dedup):
        from pyseer_amd.engine import Engine
        e = Engine(self.N)
        e.set_dedup(dedup)
        e.lmm_setup(self.U, self.S, self.y_bin, self.covar, H2)
        return e

    def engine(self, kind, dedup, pret=1.0):
        return self.lmm_engine(dedup) if kind == "lmm" else self.glm_engine(kind == "glm_cont", dedup, pret)

    def run(self, kind, bits, dedup, pret=1.0):
        """one batch on a fresh engine -> (outputs, sh_dedup_info)"""
        e = self.engine(kind, dedup, pret)
        try:
            r = e.lmm_batch(bits) if kind == "lmm" else e.glm_batch(bits)
            return r, e.dedup_info()
        finally:
            e.close()

    def check_oracle(self, kind, r, K):
        from oracle import oracle as orc
        if kind == "lmm":
            wb, ws, wf, wp = orc.LmmOracle(self.U, self.S, self.y_bin, self.covar).block(H2, K.astype(float))
            close(r["beta"], wb, atol=1e-12, what="beta"); close(r["bse"], ws, what="bse")
            close(r["frac_h2"], wf, atol=1e-9, what="frac_h2"); close(r["pvalue"], wp, atol=1e-300, what="pvalue")
            for v in range(0, K.shape[0], 17):
                pr, bad = orc.pre_filtering(self.y_bin, K[v].astype(float), False)
                close(r["prep"][v], pr, what="prep"); assert bool(r["flags"][v] & 4) == bad
            return
        cont = kind == "glm_cont"
        af = K.mean(axis=1); kept = (af >= 0.01) & (af <= 0.99)
        assert ((r["flags"][~kept] & 0x101FF) == 0x10001).all() and np.isnan(r["pvalue"][~kept]).all()
        want = orc.fixed_effects_batch(self.y(cont), K[kept].astype(float), self.W, cont, 1.0, 1.0, self.null[cont][0], self.null[cont][1])
        firth = (want["notes"] & 0x7C) != 0
        assert (~firth).sum() > 0.5 * kept.sum()
        for f in ("prep", "pvalue", "kbeta", "bse", "intercept"):
            close(r[f][kept][~firth], want[f][~firth], rtol=1e-6, atol=1e-12, what=f)
        assert ((r["flags"][kept] & 0x1FF) == want["notes"]).all()


def fields(kind):
    return LMM_FIELDS if kind == "lmm" else GLM_FIELDS


def ordinary_rows(rng, N, n_rows, n_patterns):
    """n_rows rows drawn from n_patterns random patterns with carrier rates across 0.1 .. 0.9 (so some are duplicated)"""
    base = (rng.random((n_patterns, N)) < rng.uniform(0.1, 0.9, (n_patterns, 1))).astype(np.uint8)
    return base[np.concatenate([np.arange(n_patterns), rng.integers(0, n_patterns, n_rows - n_patterns)])] if n_rows >= n_patterns \
        else base[rng.integers(0, n_patterns, n_rows)]


@functools.lru_cache(maxsize=None)
def family_case(N):
    """(a)'s batch: six distinct rows with one hash, each three to five times, among 200 ordinary rows (150 patterns), shuffled."""
    rng = np.random.default_rng(1000 + N)
    fam = H.dense_of(H.colliding_rows(rng, N // 64, 6), N)
    copies = rng.integers(3, 6, 6)
    K = np.concatenate([np.repeat(fam, copies, axis=0), ordinary_rows(rng, N, 200, 150)])
    K = K[rng.permutation(K.shape[0])]
    is_fam = (K[:, None, :] == fam[None, :, :]).all(axis=2)          # (V, 6): which member a row is
    return Problem(N, 2000 + N, assoc=fam), K, is_fam, fam


def model_count(K):
    return H.expected_representatives(H.words_of(K))[1]


def n_unique(K):
    return len(np.unique(K, axis=0))


@pytest.mark.parametrize("kind", ["glm_bin", "glm_cont", "lmm"])
@pytest.mark.parametrize("N", [128, 192])
def test_collision_family(N, kind):
    """Rows that share a 64-bit hash and differ: k_dd_resolve must compare the rows and let all but the owner's copies stand alone.  The count
    is the model's, and larger than the number of distinct rows -- which it could not be if the device hash were not the restatement's (no
    collision, count == distinct rows) or if the compare were skipped (count < distinct rows, and wrong outputs)."""
    from pyseer_amd.engine import pack_variants
    p, K, is_fam, _ = family_case(N)
    assert is_fam.any(axis=0).all() and len(np.unique(H.hash_rows(H.words_of(K[is_fam.any(axis=1)])))) == 1
    assert n_unique(K[is_fam.any(axis=1)]) == 6
    bits = pack_variants(K)
    off, _ = p.run(kind, bits, False)
    on, count = p.run(kind, bits, True)
    same(on, off, fields(kind), kind)
    want = model_count(K)
    print("N %d %s: %d rows, %d distinct, model count %d, device count %d" % (N, kind, K.shape[0], n_unique(K), want, count))
    assert want > n_unique(K)
    assert count == want
    # the members are different variants: no two of them may have been given one result
    first = [int(np.flatnonzero(is_fam[:, j])[0]) for j in range(6)]
    assert len(set(on["pvalue"][first].tolist())) == 6
    p.check_oracle(kind, on, K)


@pytest.mark.parametrize("kind", ["glm_bin", "glm_cont", "lmm"])
@pytest.mark.parametrize("N", [128, 192])
def test_probe_wraps_around_the_table(N, kind):
    """At most 512 rows on a fresh engine: a table of 1024 slots.  Eight patterns whose home is its last slot and four each at 1022, 0 and 1:
    the probes of k_dd_insert and k_dd_resolve run off the end and displace the rows at home in the first slots.  Nothing collides in all 64
    bits, so the count is the number of distinct rows."""
    from pyseer_amd.engine import pack_variants
    rng = np.random.default_rng(3000 + N)
    w, homes = H.rows_with_home_slot(rng, N // 64, 1024, [1023, 1022, 0, 1], [8, 4, 4, 4])
    assert len(np.unique(H.hash_rows(w[homes == 1023]))) == 8        # eight keys for one last slot: seven must wrap
    special = np.repeat(H.dense_of(w, N), rng.integers(2, 4, len(w)), axis=0)
    K = np.concatenate([special, ordinary_rows(rng, N, 480 - special.shape[0], 300)])
    K = K[rng.permutation(K.shape[0])]
    assert K.shape[0] <= 512
    slot_of, wrapped = H.table_slots(H.hash_rows(H.words_of(K)), 1024)
    assert wrapped >= 7                                               # keys that only a probe past the table's end can place, and find again
    assert any(slot_of[int(h)] != hm for h, hm in zip(H.hash_rows(w), homes) if hm in (0, 1))      # a row at home in slot 0 or 1 is displaced
    p = family_case(N)[0]
    bits = pack_variants(K)
    off, _ = p.run(kind, bits, False)
    on, count = p.run(kind, bits, True)
    same(on, off, fields(kind), kind)
    assert model_count(K) == n_unique(K)
    assert count == n_unique(K)
    p.check_oracle(kind, on, K)


@pytest.mark.parametrize("kind", ["glm_bin", "lmm"])
def test_table_reused_across_batches(kind):
    """One engine, batches of 100, 3000, 100 (the first again) and 1 rows: the table and its index array are cleared per batch over the
    capacity the largest batch so far has set, whatever the batch's own size."""
    from pyseer_amd.engine import pack_variants
    N = 128
    p, Kfam, _, fam = family_case(N)
    rng = np.random.default_rng(77)
    pool = np.concatenate([Kfam, ordinary_rows(rng, N, 1200, 1200)])
    batches = [pool[rng.integers(0, 60, 100)], pool[rng.integers(0, len(pool), 3000)]]
    batches += [batches[0], batches[1][1234:1235]]
    e_on, e_off = p.engine(kind, True), p.engine(kind, False)
    try:
        res = []
        for K in batches:
            bits = pack_variants(K)
            on = e_on.lmm_batch(bits) if kind == "lmm" else e_on.glm_batch(bits)
            count = e_on.dedup_info()
            off = e_off.lmm_batch(bits) if kind == "lmm" else e_off.glm_batch(bits)
            same(on, off, fields(kind), "%s V=%d" % (kind, K.shape[0]))
            assert count == model_count(K), K.shape[0]
            res.append(on)
        same(res[2], res[0], fields(kind), "first batch again")
        assert model_count(batches[3]) == 1 and model_count(batches[0]) < 100 and model_count(batches[1]) > 1024
    finally:
        e_on.close(); e_off.close()


@functools.lru_cache(maxsize=None)
def edge_case():
    N = 130
    rng = np.random.default_rng(130)
    pool = np.unique((rng.random((60, N)) < rng.uniform(0.1, 0.9, (60, 1))).astype(np.uint8), axis=0)[:38]
    pool = np.concatenate([np.zeros((1, N), np.uint8), np.ones((1, N), np.uint8), pool])
    assert n_unique(pool) == 40
    return Problem(N, 131), pool


@pytest.mark.parametrize("V", [1, 63, 64, 65, 255, 256, 257, 513])
def test_batch_sizes_at_the_launch_edges(V):
    """One row, one wavefront and one block of rows, and one more or less of each (the kernels run 256 threads, a row per thread or a row per
    wavefront; the repack takes 64 rows per block), at N = 130: a ragged last word.  40 patterns, the all-zero and the all-one row among them."""
    from pyseer_amd.engine import pack_variants
    p, pool = edge_case()
    rng = np.random.default_rng(V)
    K = pool[rng.integers(0, 40, V)]
    K[-1] = pool[V % 2]                                               # the last row of the batch is the all-zero or the all-one row
    bits = pack_variants(K)
    off, _ = p.run("glm_bin", bits, False)
    on, count = p.run("glm_bin", bits, True)
    same(on, off, GLM_FIELDS, "V=%d" % V)
    assert count == n_unique(K)


@pytest.mark.parametrize("kind,pret", [("glm_bin", 1.0), ("glm_cont", 1.0), ("glm_bin", 0.05)])
@pytest.mark.parametrize("N", [128, 192])
def test_dedup_inside_the_compactions(N, kind, pret, monkeypatch):
    """test_collision_family's batch among rare rows (no carrier or one: AF < 0.01), 1100 rows in all, with the compaction forced: rows are
    classified (k_af_rows / k_pf_rows), the kept ones gathered, de-duplicated and gathered again, fitted, and scattered back twice.  Against
    the plain path: no compaction, no de-duplication.  The family's members are associated with the phenotype, so they pass the prefilter."""
    from pyseer_amd import _route
    from pyseer_amd.engine import pack_variants
    p, Kfam, _, fam = family_case(N)
    rng = np.random.default_rng(5000 + N)
    rare = np.zeros((1100 - Kfam.shape[0], N), dtype=np.uint8)
    one = rng.random(rare.shape[0]) < 0.7
    rare[np.flatnonzero(one), rng.integers(0, N, int(one.sum()))] = 1
    K = np.concatenate([Kfam, rare])
    K = K[rng.permutation(K.shape[0])]
    assert K.shape[0] >= 1100 and (K.mean(axis=1) < 0.01).sum() == rare.shape[0]
    fam_rows = np.flatnonzero((K[:, None, :] == fam[None, :, :]).all(axis=2).any(axis=1))
    bits = pack_variants(K)
    monkeypatch.setenv("SEERHIP_ROUTE", _route.with_route(os.environ.get("SEERHIP_ROUTE"), afcompact=0))
    plain, _ = p.run(kind, bits, False, pret)
    monkeypatch.setenv("SEERHIP_ROUTE", _route.with_route(os.environ.get("SEERHIP_ROUTE"), afcompact=2))
    got, _ = p.run(kind, bits, True, pret)
    same(got, plain, GLM_FIELDS, "%s pret=%g" % (kind, pret))
    # the family went through the fit, and its six members kept six results
    assert len(fam_rows) == Kfam.shape[0] - 200
    assert ((got["flags"][fam_rows] >> 16) & 1 == 0).all() and np.isfinite(got["pvalue"][fam_rows]).all()
    assert len(set(got["pvalue"][fam_rows].tolist())) == 6
    if pret < 1.0:
        assert ((got["flags"] >> 16) & 1).sum() > rare.shape[0]        # some rows in the AF window fail the prefilter as well
