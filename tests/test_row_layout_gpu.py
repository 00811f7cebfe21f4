"""include/seerhip.h promises two things about presence rows (V rows of row_bytes bytes): any row_bytes with row_bytes * 8 >= n_samples is
accepted, and bits at i >= n_samples are ignored.  Every other GPU test packs its rows with pack_variants: row_bytes a multiple of 8, every
row 8-byte aligned, the padding clear.  Here the same rows go in at other widths -- the narrowest (ceil(N / 8)), odd ones (rows after the
first then start at odd addresses, on the host and on the device; that is intended), wider ones, and widths on both sides of the 1024 bytes
at which the repack changes from its LDS form (k_repack_bits) to the gather form (k_repack_bits_gather, k_row_flip) -- and with random bits
in everything from bit N on, the spare bits of the last used byte included.

For each entry point the reference is twofold: a plain high-precision reference computed from the dense 0/1 matrix (the CPU oracle), which
the canonical layout's result is held to once, and that canonical result itself, which every other layout must reproduce bit for bit --
everything behind the repack reads only the repacked words, so the layout cannot legitimately change a bit."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lineage_ref as R

pytestmark = pytest.mark.gpu

NS = (65, 127, 128, 129, 200)
WIDTHS = ("min", "canon", "+3", "+8", 1016, 1024, 1027, 1032)
# every width at N = 129 and 200 (similarity, continuous fixed effects); the other entry points: the narrowest, an odd one and the two sides of
# the LDS form's limit; every N at its narrowest width
ALL = [(N, "min") for N in (65, 127, 128)] + [(N, w) for N in (129, 200) for w in WIDTHS]
FEW = [(N, "min") for N in (65, 127, 128)] + [(N, w) for N in (129, 200) for w in ("min", "+3", 1024, 1027)]
COMPACT = [(N, w) for N in (129, 200) for w in ("min", "+3", 1024, 1027)]
V = 300                                                                # four blocks of 64 rows and a last one of 44
V_COMPACT = 1100
GLM_FIELDS = ("prep", "pvalue", "kbeta", "bse", "intercept", "betas", "flags")
LMM_FIELDS = ("prep", "pvalue", "beta", "bse", "frac_h2", "flags")
H2 = 0.6


def width(N, w):
    from pyseer_amd.packing import row_bytes_for
    if w == "min":
        return (N + 7) // 8
    if w == "canon":
        return row_bytes_for(N)
    if isinstance(w, str):
        return row_bytes_for(N) + int(w)
    return int(w)


def relayout(bits, N, row_bytes, dirty, rng):
    """The first ceil(N / 8) bytes of every row of `bits` in rows of row_bytes bytes, C-contiguous; dirty: every bit from N on random."""
    nb = (N + 7) // 8
    assert row_bytes >= nb
    out = np.zeros((bits.shape[0], row_bytes), dtype=np.uint8)
    out[:, :nb] = bits[:, :nb]
    if dirty:
        keep = np.zeros(row_bytes, dtype=np.uint8)
        keep[:N // 8] = 0xFF
        if N % 8:
            keep[N // 8] = (1 << (N % 8)) - 1
        noise = rng.integers(0, 256, size=out.shape, dtype=np.uint8)
        out = (out & keep) | (noise & ~keep)
    return np.ascontiguousarray(out)


def layouts(K, N, w, seed):
    """the layouts one case runs: (name, rows), clean and dirty"""
    from pyseer_amd.engine import pack_variants
    rng = np.random.default_rng(seed)
    bits = pack_variants(K)
    rb = width(N, w)
    out = [("%s=%d clean" % (w, rb), relayout(bits, N, rb, False, rng)), ("%s=%d dirty" % (w, rb), relayout(bits, N, rb, True, rng))]
    for name, b in out:
        assert b.shape == (K.shape[0], rb) and b.flags.c_contiguous
        assert np.array_equal(np.unpackbits(b, axis=1, bitorder="little")[:, :N], K)
    if rb * 8 > N:
        assert not np.array_equal(out[0][1], out[1][1])
    return out


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


def rows_across_af(rng, N, n_rows, lo=0.0, hi=1.0):
    K = (rng.random((n_rows, N)) < rng.uniform(lo, hi, (n_rows, 1))).astype(np.uint8)
    K[0] = 0; K[1] = 1
    return K


# ---- similarity ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sim_case(N):
    from oracle import oracle as orc
    K = rows_across_af(np.random.default_rng(10 + N), N, V)
    return K, orc.similarity(K), orc.similarity(K, 0.05, 0.9)


@pytest.mark.parametrize("N,w", ALL)
def test_similarity(N, w):
    from pyseer_amd.engine import Engine
    K, want, want_af = sim_case(N)
    e = Engine(N)
    try:
        for name, bits in layouts(K, N, w, 1):
            e.set_af_filter(0.0, 1.0)
            e.sim_begin(); e.sim_accumulate(bits[:100]); e.sim_accumulate(bits[100:])
            assert np.array_equal(e.sim_finish(), want), name
            e.set_af_filter(0.05, 0.9)
            e.sim_begin(); e.sim_accumulate(bits)
            assert np.array_equal(e.sim_finish(), want_af), name + " (AF filter)"
    finally:
        e.close()


# ---- fixed effects ---------------------------------------------------------------------------------------------------------------------

class Glm(object):
    def __init__(self, N, q=3):
        from pyseer_amd.model import fit_null
        rng = np.random.default_rng(20 + N)
        self.N = N
        W = rng.standard_normal((N, q)); self.W = W / np.abs(W).max(axis=0)
        eta = -0.2 + self.W[:, 0]
        self.yv = {True: eta + rng.standard_normal(N), False: (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(float)}
        e0 = np.zeros((0, 0))
        self.null = {True: (fit_null(self.yv[True], self.W, e0, True).llf, np.nan),
                     False: (fit_null(self.yv[False], self.W, e0, False).llf, fit_null(self.yv[False], self.W, e0, False, firth=True))}

    def engine(self, cont, pret=1.0, dedup=False):
        from pyseer_amd.engine import Engine
        e = Engine(self.N)
        e.set_af_filter(0.01, 0.99); e.set_dedup(dedup)
        e.glm_setup(self.yv[cont], self.W, cont, self.null[cont][0], self.null[cont][1], pret, 1.0)
        return e

    def run(self, bits, cont, pret=1.0, dedup=False):
        e = self.engine(cont, pret, dedup)
        try:
            r = e.glm_batch(bits)
            return r, e.dedup_info()
        finally:
            e.close()

    def check_oracle(self, r, K, cont, pret=1.0):
        """as tests/test_glm_gpu.py test_af_compaction_changes_nothing: the rows outside the AF window carry the filter's note and NaN; the rest
        agree with the oracle in their notes, and in their values where the oracle did not route the row to Firth"""
        from oracle import oracle as orc
        af = K.mean(axis=1); kept = (af >= 0.01) & (af <= 0.99)
        assert ((r["flags"][~kept] & 0x101FF) == 0x10001).all() and np.isnan(r["pvalue"][~kept]).all() and np.isnan(r["prep"][~kept]).all()
        want = orc.fixed_effects_batch(self.yv[cont], K[kept].astype(float), self.W, cont, pret, 1.0, self.null[cont][0], self.null[cont][1])
        firth = (want["notes"] & 0x7C) != 0
        for f in ("prep", "pvalue", "kbeta", "bse", "intercept"):
            close(r[f][kept][~firth], want[f][~firth], rtol=1e-6, atol=1e-12, what=f)
        assert ((r["flags"][kept] & 0x1FF) == want["notes"]).all()
        assert (((r["flags"][kept] >> 16) & 1) == want["prefilter"]).all()
        return kept, want


@functools.lru_cache(maxsize=None)
def glm_problem(N):
    return Glm(N)


@functools.lru_cache(maxsize=None)
def glm_case(N, cont):
    """the canonical layout's result, held to the oracle"""
    from pyseer_amd.engine import pack_variants
    g = glm_problem(N)
    K = rows_across_af(np.random.default_rng(30 + N), N, V, 0.03, 0.97)
    r, _ = g.run(pack_variants(K), cont)
    g.check_oracle(r, K, cont)
    return K, r


@pytest.mark.parametrize("N,w", ALL)
def test_glm_continuous(N, w):
    K, want = glm_case(N, True)
    for name, bits in layouts(K, N, w, 2):
        same(glm_problem(N).run(bits, True)[0], want, GLM_FIELDS, name)


@pytest.mark.parametrize("N,w", FEW)
def test_glm_binary(N, w):
    K, want = glm_case(N, False)
    for name, bits in layouts(K, N, w, 3):
        same(glm_problem(N).run(bits, False)[0], want, GLM_FIELDS, name)


_compact = {}


def compact_case(N, mode):
    """1100 rows with the compaction forced (the caller has set SEERHIP_ROUTE).  mode "af": continuous phenotype, 40 % of the rows rare
    (k_af_rows classifies them); mode "pf": binary phenotype and --filter-pvalue 0.05 (k_pf_rows), some rare rows as well."""
    from pyseer_amd.engine import pack_variants
    if (N, mode) not in _compact:
        g = glm_problem(N)
        rng = np.random.default_rng(40 + N)
        K = rows_across_af(rng, N, V_COMPACT, 0.03, 0.97)
        rare = rng.random(V_COMPACT) < (0.4 if mode == "af" else 0.05)
        K[rare] = (rng.random((int(rare.sum()), N)) < 0.004).astype(np.uint8)
        if mode == "pf":                                               # rows that pass the prefilter: carried by the cases more often
            causal = rng.random(V_COMPACT) < 0.1
            y = g.yv[False]
            K[causal] = ((rng.random((int(causal.sum()), N)) < 0.25) | ((y == 1) & (rng.random((int(causal.sum()), N)) < 0.4))).astype(np.uint8)
        cont, pret = (True, 1.0) if mode == "af" else (False, 0.05)
        r, _ = g.run(pack_variants(K), cont, pret)
        kept, want = g.check_oracle(r, K, cont, pret)
        if mode == "af":
            assert (~kept).sum() > 0.3 * V_COMPACT
        else:
            assert want["prefilter"].mean() > 0.5 and (want["prefilter"] == 0).sum() > 30 and (~kept).sum() > 10
        _compact[(N, mode)] = (K, r, cont, pret)
    return _compact[(N, mode)]


@pytest.mark.parametrize("mode", ["af", "pf"])
@pytest.mark.parametrize("N,w", COMPACT)
def test_glm_compactions_read_the_rows_as_given(N, w, mode, monkeypatch):
    """The AF and the prefilter compaction classify the rows as submitted, before any repack: k_af_rows and k_pf_rows count carriers (and the
    2x2 table) byte by byte when the row width is no multiple of 8, and k_dd_gather_rows copies the kept rows at that width."""
    from pyseer_amd import _route
    monkeypatch.setenv("SEERHIP_ROUTE", _route.with_route(os.environ.get("SEERHIP_ROUTE"), afcompact=2))
    K, want, cont, pret = compact_case(N, mode)
    for name, bits in layouts(K, N, w, 4):
        same(glm_problem(N).run(bits, cont, pret)[0], want, GLM_FIELDS, name)


@pytest.mark.parametrize("w,offset", [("canon", 1), ("+3", 1), ("+3", 8), (1024, 1), (1024, 4), (1027, 1), (1032, 2)])
def test_glm_device_rows_at_an_unaligned_address(w, offset):
    """sh_glm_batch_dev takes the rows where they are: a base address that is no multiple of 16 sends k_repack_bits through its byte copy, one
    that is no multiple of 8 keeps the gather form and the row kernels off their 64-bit loads."""
    import torch
    N = 129
    K, want = glm_case(N, True)
    g = glm_problem(N)
    e = g.engine(True)
    try:
        e.use_torch_stream()
        for name, bits in layouts(K, N, w, 5):
            buf = torch.zeros(bits.size + 64, dtype=torch.uint8, device="cuda")
            base = (-buf.data_ptr()) % 16 + offset                     # the rows start `offset` bytes past a 16-byte boundary
            rows = buf[base:base + bits.size].view(bits.shape)
            rows.copy_(torch.from_numpy(bits))
            assert rows.data_ptr() % 16 == offset and rows.is_contiguous()
            out, fl = e.glm_batch_dev(rows)
            torch.cuda.synchronize()
            out = out.cpu().numpy(); fl = fl.cpu().numpy().astype(np.uint32)
            got = dict(prep=out[0], pvalue=out[1], kbeta=out[2], bse=out[3], intercept=out[4], betas=np.ascontiguousarray(out[5:].T), flags=fl)
            same(got, want, GLM_FIELDS, name + " at +%d" % offset)
    finally:
        e.close()


# ---- LMM -------------------------------------------------------------------------------------------------------------------------------

class Lmm(object):
    def __init__(self, N, D):
        rng = np.random.default_rng(50 + 7 * N + D)
        k = N - D
        self.N, self.D = N, D
        self.U = rng.standard_normal((N, k)) / np.sqrt(N)
        self.S = np.sort(rng.gamma(0.5, 2.0, k))[::-1].copy()
        self.covar = np.ones((N, 1)) if D == 1 else np.c_[rng.standard_normal((N, D - 1)), np.ones((N, 1))]
        self.y = (rng.random(N) < 0.4).astype(float)
        K = (rng.random((V, N)) < rng.uniform(0.05, 0.95, (V, 1))).astype(np.uint8)
        K[::4] = (rng.random((len(K[::4]), N)) < 0.9).astype(np.uint8)  # a quarter of the rows is stored complemented
        self.K = K

    def run(self, bits, dedup=False):
        from pyseer_amd.engine import Engine
        e = Engine(self.N)
        try:
            e.set_dedup(dedup)
            e.lmm_setup(self.U, self.S, self.y, self.covar, H2)
            r = e.lmm_batch(bits)
            return r, e.dedup_info()
        finally:
            e.close()


@functools.lru_cache(maxsize=None)
def lmm_case(N, D):
    """the canonical layout's result, held to the oracle as tests/test_lmm_gpu.py test_lmm_many_covariates_and_continuous_vs_oracle holds it"""
    from oracle import oracle as orc
    from pyseer_amd.engine import pack_variants
    p = Lmm(N, D)
    assert (2 * p.K.sum(axis=1) > N).sum() > V // 4
    r, _ = p.run(pack_variants(p.K))
    wb, ws, wf, wp = orc.LmmOracle(p.U, p.S, p.y, p.covar).block(H2, p.K.astype(float))
    close(r["beta"], wb, atol=1e-12, what="beta"); close(r["bse"], ws, what="bse")
    close(r["frac_h2"], wf, atol=1e-9, what="frac_h2"); close(r["pvalue"], wp, atol=1e-300, what="pvalue")
    for v in range(0, V, 7):
        pr, bad = orc.pre_filtering(p.y, p.K[v].astype(float), False)
        close(r["prep"][v], pr, what="prep"); assert bool(r["flags"][v] & 4) == bad
    return p, r


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("N,w", FEW)
def test_lmm(N, w, D):
    p, want = lmm_case(N, D)
    for name, bits in layouts(p.K, N, w, 6):
        same(p.run(bits)[0], want, LMM_FIELDS, name)


# ---- lineage ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lineage_case(N):
    """the canonical layout's answers, held to the reference's arithmetic as tests/test_lineage_counts_gpu.py holds them"""
    from pyseer_amd.engine import pack_variants
    l = 5
    cluster_of, K = R.oracle_case(N, l, V, 60 + N)
    lin = R.design(cluster_of, l)
    got = lineage_run(N, lin, pack_variants(K))
    cnt = [R.counts(cluster_of, l, k) for k in K]
    cond, dense = [R.well_conditioned(*c) for c in cnt], R.dense_rows(lin, K)
    R.check_rows(got, dense, cond, l, cnt=cnt, loose_max=R.loose_bound(cnt, cond, dense))
    assert (got >= 0).sum() > V // 2
    return lin, K, got


def lineage_run(N, lin, bits):
    from pyseer_amd.engine import Engine
    e = Engine(N)
    try:
        e.lineage_setup(lin)
        return e.lineage_batch(bits)
    finally:
        e.close()


@pytest.mark.parametrize("N,w", FEW)
def test_lineage(N, w):
    lin, K, want = lineage_case(N)
    for name, bits in layouts(K, N, w, 7):
        assert np.array_equal(lineage_run(N, lin, bits), want), name


# ---- the run-wide pattern set, and the per-batch de-duplication --------------------------------------------------------------------------

def rows_with_duplicates(N, seed, n_patterns=120):
    rng = np.random.default_rng(seed)
    pool = rows_across_af(rng, N, n_patterns, 0.05, 0.95)
    return pool[np.concatenate([np.arange(n_patterns), rng.integers(0, n_patterns, V - n_patterns)])][rng.permutation(V)]


@pytest.mark.parametrize("N,w", FEW)
def test_pattern_set(N, w):
    """PatternSet.add_rows hashes the rows as submitted (k_ps_insert_rows, ps_row_word): the keys are those of the canonical rows"""
    from pyseer_amd.engine import Engine, PatternSet, hash_rows, pack_variants
    K = rows_with_duplicates(N, 70 + N)
    n = len(np.unique(K, axis=0))
    assert n == 120
    keys = hash_rows(pack_variants(K), N)
    assert len(np.unique(keys, axis=0)) == n
    e = Engine(N)
    try:
        for name, bits in layouts(K, N, w, 8):
            assert np.array_equal(hash_rows(bits, N), keys), name
            ps = PatternSet(e, 1024)
            ps.add_rows(bits)
            assert ps.count() == n, name
            ps.add_keys(keys)                                          # the device's keys of these rows are the host's of the canonical rows:
            assert ps.count() == n, name                               # nothing is new
            ps.close()
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["glm", "lmm"])
@pytest.mark.parametrize("N,w", [(N, w) for N in (129, 200) for w in ("min", 1027)])
def test_dedup_sees_only_the_sample_bits(N, w, kind):
    """De-duplication on at the narrowest width and past the LDS form's limit: the outputs are those of the plain path at the canonical
    width, and dirty padding creates no new patterns."""
    from pyseer_amd.engine import pack_variants
    K = rows_with_duplicates(N, 80 + N)
    p = glm_problem(N) if kind == "glm" else lmm_case(N, 1)[0]
    run = (lambda b, d: p.run(b, True, 1.0, d)) if kind == "glm" else (lambda b, d: p.run(b, d))
    want, _ = run(pack_variants(K), False)
    for name, bits in layouts(K, N, w, 9):
        got, count = run(bits, True)
        same(got, want, GLM_FIELDS if kind == "glm" else LMM_FIELDS, name)
        assert count == len(np.unique(K, axis=0)), name
