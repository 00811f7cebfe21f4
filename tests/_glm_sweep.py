"""The volume sweep of the fixed-effects engine against the oracle (tests/test_glm_sweep_gpu.py, tests/test_glm_shapes_sweep_gpu.py): the row
generator and the per-chunk comparison.  Test infrastructure.

Rows of one chunk: half at uniform allele frequencies, half from a U-shaped distribution, 15 % with real / near-separating effects, and the
TAIL rows -- carriers exactly the last k samples (k from the 1 % frequency floor up 48 more, across the last 16-sample group of the f16 MFMA
operands and the last 64-bit word), the last sample alone plus a minimum-frequency set elsewhere, and every sample but the last few: the
rows whose carriers sit in the packed records' odd last sample and in the zero-padded tail behind sample N.

What one chunk asserts:
  * notes bit-exact, except rows the ORACLE calls firth-fail (its rounding-noise failures, DESIGN.md section 6: the HIP path fits them) --
    every one of those must carry SH_FLAG_FIRTH_SENSITIVE (bit 18); prefilter and filter bits (16, 17) bit-exact, under the same exception;
  * p-value within 1e-6 relative, where a likelihood-ratio statistic below the noise of its two log-likelihoods (32 ulp of |llf|) is compared
    as a statistic, not as its tail (p = 1 - 2e-6 against p = 1 is lr = 1e-11 against lr <= 0);
  * Firth-routed rows (bad-chisq / high-bse / separation): 1e-6 relative + the 3e-7 halving-tie slack on the rows the tie detector names
    (tests/_firth_tol.py).
and it accumulates, over the Newton-fitted (or OLS) rows, the maximum relative deviation of each field, which the tests hold to ceilings."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# |d| / max(|want|, floor): one row in a million has an intercept that cancels to ~1e-4; kbeta against a five-hundredth of the smallest bse
FLOOR = {"kbeta": 1e-4, "intercept": 1e-2, "bse": 0.0, "betas": 1e-3}
RANDOM, STRONG, TAIL = 0, 1, 2                 # row kinds of the generator
CHUNK = 32768


def rows(rng, v, N, y):
    """v random + strong-effect rows and the tail rows, those inside the 1 % .. 99 % frequency window.  -> (K (rows, N) uint8, kind (rows,))"""
    af = np.concatenate([rng.uniform(0.02, 0.98, v // 2), rng.beta(0.3, 0.3, v - v // 2)]).astype(np.float32)
    K = rng.random((v, N), dtype=np.float32) < af[:, None]
    eff = np.flatnonzero(rng.random(v) < 0.15)
    hi = (0.05 + 0.8 * (y > np.median(y))).astype(np.float32)
    K[eff] = rng.random((eff.size, N), dtype=np.float32) < hi[None, :] * rng.uniform(0.1, 1.0, eff.size).astype(np.float32)[:, None]
    kind = np.full(v, RANDOM, np.int8); kind[eff] = STRONG
    kmin = -(-N // 100)                                                 # the fewest carriers inside the frequency window
    T = []
    for k in range(kmin, kmin + 49):                                    # exactly the last k samples
        t = np.zeros(N, bool); t[N - k:] = True; T.append(t)
    for _ in range(16):                                                 # the last sample alone + a minimum-frequency set elsewhere
        t = np.zeros(N, bool); t[N - 1] = True; t[rng.choice(N - 1, kmin - 1, replace=False)] = True; T.append(t)
    for _ in range(16):                                                 # random carriers among the last 64 + kmin, the last one always
        t = np.zeros(N, bool); t[N - 1] = True
        t[N - 1 - rng.choice(np.arange(1, min(N, 64 + kmin)), kmin + int(rng.integers(0, 24)), replace=False)] = True; T.append(t)
    for j in range(kmin, kmin + 8):                                     # every sample but the last j
        t = np.ones(N, bool); t[N - j:] = False; T.append(t)
    K = np.concatenate([K, np.array(T)]); kind = np.concatenate([kind, np.full(len(T), TAIL, np.int8)])
    m = K.mean(axis=1)
    keep = (m >= 0.01) & (m <= 0.99)
    return K[keep].astype(np.uint8), kind[keep]


NOTE_PRE_FILTER, NOTE_LRT_FILTER = 1 << 1, 1 << 8        # (include/seerhip.h: the notes bits)
# the reference against the oracle: a prep below 1e-250 decides nothing (it is only ever compared with pret), and down there the two
# t tails round differently (1e-310 is subnormal)
REF_FLOOR = {"pvalue": 1e-300, "prep": 1e-250}
NEAR = 1e-9                                              # a statistic this close (relative) to its threshold: the oracle decides the row


def ols_reference(y, K, W, pret=1.0, lrtt=1.0, block=4096):
    """The whole fixed-effects row of y on [1, k, W] for every row of K, continuous phenotype (model.py:202-394 without lineage), in fp64:
      * prep: Welch's t-test of y between carriers and non-carriers (model.py:53-55), two-sided; prefilter = prep > pret or not finite
        (model.py:266), the row's fit then NaN and its notes NOTE_PRE_FILTER;
      * the fit through a QR of the null design [1, W]: k is projected off it twice (classical Gram-Schmidt with one
        re-orthogonalisation), kbeta = k'y / k'k on the projections, the null coefficients corrected by kbeta R^-1 Q'k; bse and the
        two-sided t p-value at n - q - 2 degrees of freedom (statsmodels OLS, model.py:300-312);
      * filter = p-value > lrtt or not finite (model.py:384), notes NOTE_LRT_FILTER.
    Rank-deficient rows (a projection below 1e-8 of |k|^2: the oracle's pinv decides those) and rows whose prep or p-value lies within NEAR
    of its threshold come back in `oracle_only`: the caller must hold them to the oracle."""
    from scipy import stats
    N = y.shape[0]; V = K.shape[0]
    X0 = np.ones((N, 1)) if W is None else np.concatenate([np.ones((N, 1)), np.asarray(W, float).reshape(N, -1)], axis=1)
    Q, R = np.linalg.qr(X0)
    yq = Q.T @ y; yp = y - Q @ yq; yp -= Q @ (Q.T @ yp)
    bnull = np.linalg.solve(R, yq); syy = float(yp @ yp); df = N - X0.shape[1] - 1
    yc = y - y.mean(); yc2 = yc * yc
    out = {f: np.empty(V) for f in ("prep", "kbeta", "intercept", "bse", "pvalue")}
    out["betas"] = np.empty((V, X0.shape[1] - 1)); rankdef = np.empty(V, bool)
    for i in range(0, V, block):
        k = K[i:i + block].astype(float)
        # prefilter: Welch (model.py:53-55; seer_oracle.c orc_pre_filtering), on y centred to keep the sums of squares exact
        n1 = k.sum(axis=1); n0 = N - n1
        s1 = k @ yc; m1 = s1 / n1; m0 = -s1 / n0
        q1 = k @ yc2 - n1 * m1 * m1; q0 = (float(yc2.sum()) - k @ yc2) - n0 * m0 * m0
        vn1 = q1 / (n1 - 1) / n1; vn0 = q0 / (n0 - 1) / n0
        wdf = (vn1 + vn0) ** 2 / (vn1 * vn1 / (n1 - 1) + vn0 * vn0 / (n0 - 1))
        wdf = np.where(np.isnan(wdf), 1.0, wdf)
        out["prep"][i:i + block] = 2 * stats.t.sf(np.abs((m1 - m0) / np.sqrt(vn1 + vn0)), wdf)
        a = k @ Q; kp = k - a @ Q.T
        a2 = kp @ Q; kp -= a2 @ Q.T; a += a2
        s = np.einsum("ij,ij->i", kp, kp); ky = kp @ yp
        kb = ky / s
        ssr = syy - ky * kb
        bse = np.sqrt(ssr / df / s)
        b0 = bnull[None, :] - kb[:, None] * np.linalg.solve(R, a.T).T
        bad = s < 1e-8 * np.einsum("ij,ij->i", k, k)
        kb[bad] = np.nan; bse[bad] = np.nan; b0[bad] = np.nan; rankdef[i:i + block] = bad
        out["kbeta"][i:i + block] = kb; out["bse"][i:i + block] = bse
        out["pvalue"][i:i + block] = 2 * stats.t.sf(np.abs(kb / bse), df)
        out["intercept"][i:i + block] = b0[:, 0]; out["betas"][i:i + block] = b0[:, 1:]
    prep, pv = out["prep"], out["pvalue"]
    pre = ~(prep <= pret)
    for f in ("kbeta", "intercept", "bse", "pvalue", "betas"):
        out[f][pre] = np.nan
    filt = ~pre & ~((pv <= lrtt) & np.isfinite(out["kbeta"]))
    out["prefilter"] = pre.astype(np.int32); out["filter"] = filt.astype(np.int32)
    out["notes"] = np.where(pre, NOTE_PRE_FILTER, 0).astype(np.uint32) | np.where(filt, NOTE_LRT_FILTER, 0).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        out["oracle_only"] = rankdef | (np.abs(prep - pret) <= NEAR * pret) | (~pre & (np.abs(pv - lrtt) <= NEAR * lrtt))
    return out


class Sweep(object):
    """Runs chunks through the engine and the oracle and holds what they agree on; the maxima, counts and timings accumulate."""

    def __init__(self, e, y, W, continuous, null_llf, null_firth, pret=1.0, lrtt=1.0, oracle_every=1):
        """oracle_every > 1 (OLS only): every row is held to ols_reference -- notes, prefilter and filter bits and values --, and the oracle
        runs on the tail rows, every oracle_every-th other row and the rows the reference leaves to it; on the rows both see the reference
        must give the oracle's notes and bits and its values to 1e-10."""
        self.e, self.y, self.W, self.cont = e, y, (W if np.size(W) else None), continuous
        assert oracle_every == 1 or continuous
        self.every = oracle_every
        self.nl, self.nf, self.pret, self.lrtt = null_llf, null_firth, pret, lrtt
        self.lr_noise = 32 * 2.2e-16 * abs(null_llf)
        self.mx = {k: 0.0 for k in ("kbeta", "intercept", "bse", "pvalue", "betas", "firth_kbeta", "firth_bse")}
        self.rows = self.newton = self.firth_rows = self.oracle_fail = self.strong = self.tie_rows = 0
        self.tail = self.tail_newton = self.effect_rows = self.prefiltered = self.oracle_rows = 0
        self.ref_vs_oracle = 0.0
        self.t_or = self.t_gpu = 0.0

    def run(self, rng, V, chunk=CHUNK):
        N = self.y.shape[0]
        while self.rows < V:
            K, kind = rows(rng, min(chunk, V), N, self.y)
            self.chunk(K, kind)
        return self

    def chunk(self, K, kind):
        from scipy.special import erfcinv
        from oracle import oracle as orc
        from pyseer_amd.engine import pack_variants
        from _firth_tol import firth_rows_close
        y, W, nl, nf = self.y, self.W, self.nl, self.nf
        sub = (kind == TAIL) | (np.arange(K.shape[0]) % self.every == 0)
        if self.every > 1:
            ref = ols_reference(y, K, W, self.pret, self.lrtt)
            sub |= ref["oracle_only"]
        t0 = time.time(); want = orc.fixed_effects_batch(y, K[sub].astype(float), W, self.cont, self.pret, self.lrtt, nl, nf); self.t_or += time.time() - t0
        t0 = time.time(); r = self.e.glm_batch(pack_variants(K)); self.t_gpu += time.time() - t0
        self.oracle_rows += int(sub.sum())
        if self.every > 1:
            # every row held to ols_reference -- notes, prefilter and filter bits, values --, the oracle's own answer on the rows it saw, and
            # the reference held to the oracle there: the same notes and bits, the same values to 1e-10
            both = ~ref["oracle_only"][sub]
            for f in ("notes", "prefilter", "filter"):
                assert (ref[f][sub][both] == want[f][both]).all(), ("the OLS reference and the oracle disagree", f)
            for f in ("prep", "kbeta", "intercept", "bse", "pvalue", "betas"):
                a, b = ref[f][sub][both], want[f][both]
                assert (np.isnan(a) == np.isnan(b)).all(), ("the OLS reference and the oracle disagree", f, "NaN")
                ok = ~np.isnan(b)
                if ok.any():
                    self.ref_vs_oracle = max(self.ref_vs_oracle, float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), REF_FLOOR.get(f) or FLOOR[f]))))
            assert self.ref_vs_oracle <= 1e-10, ("the OLS reference and the oracle disagree", self.ref_vs_oracle)
            full = {f: ref[f].copy() for f in ("prep", "kbeta", "intercept", "bse", "pvalue", "betas", "notes", "prefilter", "filter")}
            for f in full:
                full[f][sub] = want[f]
            want = full
        notes = want["notes"]; fl = r["flags"]
        ofail = (notes & 0x40) != 0                                     # the oracle's firth-fail (rounding-noise failures: fitted here)
        diff = (fl & 0x1FF) != notes
        assert not (diff & ~ofail).any(), ("notes differ", np.flatnonzero(diff & ~ofail)[:5], fl[diff & ~ofail][:5] & 0x1FF, notes[diff & ~ofail][:5])
        assert (((fl >> 18) & 1)[ofail & diff] == 1).all(), "a row the oracle fails and this library fits does not carry SH_FLAG_FIRTH_SENSITIVE"
        assert (((fl >> 16) & 1) == want["prefilter"]).all(), ("prefilter bits differ", np.flatnonzero(((fl >> 16) & 1) != want["prefilter"])[:5])
        fdiff = (((fl >> 17) & 1) != want["filter"]) & ~(ofail & diff)       # the oracle's firth-fail sets its filter bit too (model.py:357-362)
        assert not fdiff.any(), ("filter bits differ", np.flatnonzero(fdiff)[:5])
        self.oracle_fail += int((ofail & diff).sum())
        fr = ((notes & 0x7C) != 0) & ~ofail
        nw = ~fr & ~ofail & np.isfinite(want["kbeta"])
        self.rows += K.shape[0]; self.newton += int(nw.sum()); self.firth_rows += int(fr.sum())
        self.strong += int((np.abs(want["kbeta"][nw]) >= 2).sum())
        self.tail += int((kind == TAIL).sum()); self.tail_newton += int((nw & (kind == TAIL)).sum())
        self.effect_rows += int(((nw | fr) & (kind == STRONG)).sum()); self.prefiltered += int((want["prefilter"] != 0).sum())
        for f in ("kbeta", "intercept", "bse"):
            a, b = r[f][nw], want[f][nw]
            assert np.isfinite(a).all(), f
            if a.size:
                self.mx[f] = max(self.mx[f], float(np.max(np.abs(a - b) / np.maximum(np.abs(b), FLOOR[f]))))
        if W is not None and nw.any():
            self.mx["betas"] = max(self.mx["betas"], float(np.max(np.abs(r["betas"][nw] - want["betas"][nw]) / np.maximum(np.abs(want["betas"][nw]), FLOOR["betas"]))))
        # p: relative, or -- for statistics inside the noise of the two log-likelihoods -- through the statistic
        pg, pw = r["pvalue"][nw], want["pvalue"][nw]
        lrw = 2 * erfcinv(np.clip(pw, 1e-300, 1.0)) ** 2
        allow = 1e-6 * pw + self.lr_noise / np.sqrt(2 * np.pi * np.maximum(lrw, self.lr_noise))
        bad = np.abs(pg - pw) > allow
        assert not bad.any(), ("pvalue", pg[bad][:5], pw[bad][:5])
        big = lrw > 1e-6
        if big.any():
            self.mx["pvalue"] = max(self.mx["pvalue"], float(np.max(np.abs(pg[big] - pw[big]) / np.maximum(pw[big], 1e-300))))
        if fr.any():
            # (tests/_firth_tol.py: 1e-6 relative, the 3e-7 slack only where the tie detector fires on the row)
            Kf = K[fr].astype(float)
            vs = orc.firth_noise_variants(lambda: orc.fixed_effects_batch(y, Kf, W, self.cont, self.pret, self.lrtt, nl, nf))
            allr = np.ones(int(fr.sum()), bool)
            for f in ("kbeta", "bse", "intercept"):
                good, nt = firth_rows_close(r[f][fr], vs, f, allr); self.tie_rows += nt
                assert good.all(), ("firth " + f, r[f][fr][~good][:5], vs[0][f][~good][:5])
            self.mx["firth_kbeta"] = max(self.mx["firth_kbeta"], float(np.max(np.abs(r["kbeta"][fr] - want["kbeta"][fr]))))
            self.mx["firth_bse"] = max(self.mx["firth_bse"], float(np.max(np.abs(r["bse"][fr] - want["bse"][fr]) / want["bse"][fr])))

    def summary(self, label):
        if self.cont:
            what = "%d OLS-fitted" % self.newton
            if self.every > 1:
                what += "; oracle on %d rows, every row against the OLS reference, which is within %.2g of the oracle" % (self.oracle_rows, self.ref_vs_oracle)
            mx = {k: v for k, v in self.mx.items() if not k.startswith("firth")}
        else:
            what = ("%d Newton-fitted, %d of them |kbeta| >= 2; %d Firth-routed, %d values of those on a halving tie; %d oracle firth-fails fitted here"
                    % (self.newton, self.strong, self.firth_rows, self.tie_rows, self.oracle_fail))
            mx = self.mx
        if self.pret < 1.0 or self.lrtt < 1.0:
            what += "; %d prefiltered" % self.prefiltered
        return ("%s: %d rows (%s; %d tail rows, %d of them fitted; %d strong-effect rows fitted), oracle %.0f s, engine calls %.1f s; max relative deviation %s"
                % (label, self.rows, what, self.tail, self.tail_newton, self.effect_rows, self.t_or, self.t_gpu, {k: float("%.3g" % v) for k, v in mx.items()}))
