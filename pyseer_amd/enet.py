"""Whole-genome elastic net (pyseer/enet.py) on the device: a resident bit matrix, its phenotype correlations, and the
cross-validated elastic-net path (sh_enet_*, include/seerhip.h).  The host parts that carry no weight -- fold assignment,
sample weights, the quantile cut -- are here in numpy."""
import ctypes as C

import numpy as np

from . import _abi
from .packing import row_bytes_for

GAUSSIAN, BINOMIAL = 0, 1


def assign_folds(n_samples, n_folds, seed=1):
    """Balanced random folds as cvglmnet draws them (sample i of a random order goes to fold i mod F), from a seeded
    generator (--enet-seed): glmnet_python's own draw is unseeded and cannot be reproduced."""
    if n_folds < 2 or n_folds > n_samples:
        raise ValueError("n_folds must lie in [2, n_samples]")
    perm = np.random.default_rng(seed).permutation(n_samples)
    fold = np.empty(n_samples, dtype=np.int32)
    fold[perm] = np.arange(n_samples, dtype=np.int32) % n_folds
    return fold


def sequence_weights(cluster_ids):
    """pyseer/__main__.py:650-654: every sample weighs 1 / (size of its lineage cluster)."""
    cluster_ids = np.asarray(cluster_ids)
    _, inv, counts = np.unique(cluster_ids, return_inverse=True, return_counts=True)
    return 1.0 / counts[inv].astype(float)


def correlation_cut(abs_cor, quantile):
    """enet.py:420: indices whose |correlation| is strictly above numpy's (linear-interpolation) percentile of ALL values;
    NaN rows (no carriers) never pass and, as in the reference, one NaN makes the percentile NaN and nothing passes."""
    abs_cor = np.asarray(abs_cor, dtype=float)
    with np.errstate(invalid="ignore"):
        return np.nonzero(abs_cor > np.percentile(abs_cor, quantile * 100))[0]


class EnetFit(object):
    """Result of EnetMatrix.fit: arrays over the fitted part of the path."""

    def __init__(self, owner, out, arrays, n_cov):
        n = out.n_lambda
        self._owner = owner
        self.n_lambda, self.i_min, self.n_cov = n, out.i_min, n_cov
        self.lambdas = arrays["lambda_"][:n].copy()
        self.cvm, self.cvsd = arrays["cvm"][:n].copy(), arrays["cvsd"][:n].copy()
        self.dev_ratio, self.nzero = arrays["dev_ratio"][:n].copy(), arrays["nzero"][:n].copy()
        self.fold_dev = arrays["fold_dev"][:, :n].copy()
        self.fold_weight = arrays["fold_weight"].copy()
        self.beta0, self.beta = out.beta0, arrays["beta"]
        self.kkt_rounds, self.cd_sweeps, self.cd_steps, self.state_in_lds = out.kkt_rounds, out.cd_sweeps, out.cd_steps, bool(out.state_in_lds)

    def betas_at(self, i_lambda, problem=0):
        """(intercept, slopes[n_cov + rows]) on the original scale: problem 0 = the full fit, 1 + k = fold k held out."""
        return self._owner._betas_at(problem, i_lambda)

    def eta_at(self, i_lambda):
        return self._owner._eta_at(i_lambda)


class EnetMatrix(object):
    """The variants of a whole-genome fit, resident on the device of `engine`."""

    def __init__(self, engine, capacity):
        self._e, self._lib, self._h = engine, engine._lib, engine._h
        self.n = engine.n
        self.row_bytes = row_bytes_for(self.n)
        _abi.check(self._lib.sh_enet_begin(self._h, self.row_bytes, int(capacity)))
        self._open = True

    def close(self):
        if self._open and self._e._h:
            self._lib.sh_enet_end(self._h)
        self._open = False

    @property
    def rows(self):
        return int(self._lib.sh_enet_rows(self._h))

    def _u8(self, a, V):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != (V, self.row_bytes):
            raise ValueError("packed rows must be (V, %d) bytes" % self.row_bytes)
        return a

    def append(self, present, missing=None, flip=None):
        """Add packed rows; flip[v]: store row v by its absences (af > 0.5), a missing call being 0 (enet.py:95-106)."""
        present = np.ascontiguousarray(present, dtype=np.uint8)
        V = present.shape[0]
        present = self._u8(present, V)
        missing = None if missing is None else self._u8(missing, V)
        flip = None if flip is None else np.ascontiguousarray(flip, dtype=np.uint8)
        if flip is not None and flip.shape != (V,):
            raise ValueError("flip must have one entry per row")
        p8 = lambda a: None if a is None else a.ctypes.data_as(_abi.c_u8p)
        _abi.check(self._lib.sh_enet_append(self._h, p8(present), p8(missing), p8(flip), V))

    def ingest(self, bits, min_count, max_count):
        """A block of parsed rows without missing calls (a RawBlock's bits): the rows with min_count <= carriers <= max_count are appended in
        their order, coded by the minor allele, on the device (k_enet_ingest_*); the matrix grows as needed.  Returns (index in the block,
        carrier count) of the kept rows."""
        bits = np.asarray(bits)
        V = bits.shape[0]
        if bits.dtype != np.uint8 or bits.shape != (V, self.row_bytes) or not bits.flags.c_contiguous:
            bits = self._u8(bits, V)
        idx, cnt = np.empty(V, dtype=np.int32), np.empty(V, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        kept = self._lib.sh_enet_ingest(self._h, C.cast(bits.ctypes.data, _abi.c_u8p), V, int(min_count), int(max_count), idx.ctypes.data_as(i32),
                                        cnt.ctypes.data_as(i32))
        if kept < 0:
            _abi.check(int(kept))
        return idx[:kept], cnt[:kept]

    def ingest_calls(self, present, missing, skip, lo, hi, mm):
        """A block of parsed rows with missing calls (an input.CallBlock's present / missing rows; missing and skip may be None): the rows
        that are not skipped, with lo <= present + missing <= hi and missing <= mm (call_bounds), are appended in their order, coded by the
        minor allele, on the device (k_enet_ingest_calls_*).  Returns (index in the block, present count, missing count) of the kept rows."""
        def rows_of(a, V):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.shape != (V, self.row_bytes) or not a.flags.c_contiguous:
                a = self._u8(a, V)
            return a
        V = np.asarray(present).shape[0]
        present = rows_of(present, V)
        missing = None if missing is None else rows_of(missing, V)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.int32)
            if skip.shape != (V,):
                raise ValueError("skip must have one entry per row")
        idx, n_p, n_m = np.empty(V, dtype=np.int32), np.empty(V, dtype=np.int32), np.empty(V, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        kept = self._lib.sh_enet_ingest_calls(self._h, C.cast(present.ctypes.data, _abi.c_u8p),
                                              None if missing is None else C.cast(missing.ctypes.data, _abi.c_u8p),
                                              None if skip is None else skip.ctypes.data_as(i32), V, int(lo), int(hi), int(mm),
                                              idx.ctypes.data_as(i32), n_p.ctypes.data_as(i32), n_m.ctypes.data_as(i32))
        if kept < 0:
            _abi.check(int(kept))
        return idx[:kept], n_p[:kept], n_m[:kept]

    def correlations(self, y):
        if self.rows < 1:
            raise ValueError("No variants passed filters")
        y = np.ascontiguousarray(y, dtype=float)
        out = np.empty(self.rows)
        _abi.check(self._lib.sh_enet_correlations(self._h, y.ctypes.data_as(_abi.c_dp), out.ctypes.data_as(_abi.c_dp)))
        return out

    def carrier_sums(self, vectors):
        """(n_vectors, N) -> (n_vectors, rows): sum of each vector over the carriers of every row (k_enet_grad)."""
        v = np.ascontiguousarray(np.asarray(vectors, dtype=float).reshape(-1, self.n))
        out = np.empty((v.shape[0], self.rows))
        _abi.check(self._lib.sh_enet_carrier_sums(self._h, v.ctypes.data_as(_abi.c_dp), v.shape[0], out.ctypes.data_as(_abi.c_dp)))
        return out

    def keep(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        _abi.check(self._lib.sh_enet_keep(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size))

    def get_rows(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = np.zeros((idx.size, self.row_bytes), dtype=np.uint8)
        _abi.check(self._lib.sh_enet_get_rows(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, out.ctypes.data_as(_abi.c_u8p)))
        return out

    def fit(self, y, continuous, alpha, weights=None, covariates=None, fold_id=None, n_folds=0, thresh=1e-7, n_lambda=100,
            lambda_min_ratio=0.0, state_in_global=False, lambdas=None):
        """Cross-validated elastic-net path.  covariates: (N, n_cov) or None; fold_id: (N,) ints in [0, n_folds)."""
        if self.rows < 1:
            raise ValueError("No variants passed filters")
        if not (0.0 <= alpha <= 1.0):
            raise ValueError("alpha must lie in [0, 1]")
        N, P = self.n, self.rows
        y = np.ascontiguousarray(y, dtype=float)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=float)
        cov = None
        n_cov = 0
        if covariates is not None and np.size(covariates):
            cov = np.ascontiguousarray(np.asarray(covariates, dtype=float).reshape(N, -1).T)     # one column after the other
            n_cov = cov.shape[0]
        fid = None if fold_id is None else np.ascontiguousarray(fold_id, dtype=np.int32)
        if fid is not None and not n_folds:
            n_folds = int(fid.max()) + 1
        seq = None
        if lambdas is not None:
            seq = np.ascontiguousarray(lambdas, dtype=float)
            n_lambda = seq.size
        opts = _abi.EnetOpts(int(n_lambda), 0, int(bool(state_in_global)), 0, float(thresh), float(lambda_min_ratio),
                             None if seq is None else seq.ctypes.data_as(_abi.c_dp))
        arrays = {k: np.full(n_lambda, np.nan) for k in ("lambda_", "cvm", "cvsd", "dev_ratio")}
        arrays["fold_dev"] = np.full((max(n_folds, 1), n_lambda), np.nan)
        arrays["fold_weight"] = np.zeros(max(n_folds, 1))
        arrays["beta"] = np.zeros(n_cov + P)
        arrays["nzero"] = np.zeros(n_lambda, dtype=np.int32)
        out = _abi.EnetOut()
        for k in ("lambda_", "cvm", "cvsd", "dev_ratio", "fold_dev", "fold_weight", "beta"):
            setattr(out, k, arrays[k].ctypes.data_as(_abi.c_dp))
        out.nzero = arrays["nzero"].ctypes.data_as(C.POINTER(C.c_int32))
        dp = lambda a: None if a is None else a.ctypes.data_as(_abi.c_dp)
        _abi.check(self._lib.sh_enet_fit(self._h, dp(y), dp(w), dp(cov), n_cov, None if fid is None else fid.ctypes.data_as(C.POINTER(C.c_int32)),
                                         int(n_folds), BINOMIAL if not continuous else GAUSSIAN, float(alpha), C.byref(opts), C.byref(out)))
        self._n_coef = n_cov + P
        return EnetFit(self, out, arrays, n_cov)

    def _betas_at(self, problem, i_lambda):
        b0 = C.c_double()
        beta = np.zeros(self._n_coef)
        _abi.check(self._lib.sh_enet_betas_at(self._h, int(problem), int(i_lambda), C.byref(b0), beta.ctypes.data_as(_abi.c_dp)))
        return b0.value, beta

    def _eta_at(self, i_lambda):
        eta = np.zeros(self.n)
        _abi.check(self._lib.sh_enet_eta_at(self._h, int(i_lambda), eta.ctypes.data_as(_abi.c_dp)))
        return eta


# ---------------------------------------------------------------------------------------------------------------
# the command line's --wg enet (pyseer/__main__.py:598-712 over pyseer/enet.py)
# ---------------------------------------------------------------------------------------------------------------
TEST_BETAS = None          # test-only hook: a function (n_cov, var_indices) -> betas[1 + n_cov + P] used instead of the fit's
LAST_LOAD_ROUTE = None     # how the last run_cli loaded its variants: "calls" (native VCF reader, sh_enet_ingest_calls), "blocks" (raw k-mer
                           # blocks, sh_enet_ingest) or "lines" (read_variant): the three print the same, so a test needs this to tell them apart


def load_all_vars(engine, var_type, p, burden, burden_regions, infile, all_strains, sample_order, min_af, max_af, max_missing, uncompressed):
    """pyseer/enet.py:33-118 with the matrix on the device: (EnetMatrix, var_indices, number of variants read).  The filters are the
    reference's strict inequalities; var_indices count every variant read."""
    from .input import read_variant
    n, rb = len(p), row_bytes_for(len(p))
    pres, miss, flip, selected, var_idx = [], [], [], [], 0
    while True:
        eof, k, var_name, kstrains, nkstrains, af, missing = read_variant(infile, p, var_type, burden, burden_regions, uncompressed,
                                                                          all_strains, sample_order)
        if eof:
            break
        if k is not None and af > min_af and af < max_af and missing < max_missing:
            k = np.asarray(k, dtype=float)
            pres.append(k == 1)
            miss.append(np.isnan(k))
            flip.append(af > 0.5)                                     # enet.py:97: coded by the absences
            selected.append(var_idx)
        var_idx += 1
    if not selected:
        raise ValueError("No variants passed filters")

    def pack(rows):
        out = np.zeros((len(rows), rb), dtype=np.uint8)
        pk = np.packbits(np.array(rows, dtype=bool).reshape(len(rows), n), axis=1, bitorder="little")
        out[:, :pk.shape[1]] = pk
        return out
    M = EnetMatrix(engine, len(selected))
    for s in range(0, len(selected), 65536):
        M.append(pack(pres[s:s + 65536]), pack(miss[s:s + 65536]), np.array(flip[s:s + 65536], dtype=np.uint8))
    return M, selected, var_idx


def count_bounds(n, min_af, max_af, max_missing):
    """load_all_vars' rule for a line without missing calls as an interval of carrier counts: the reference's own expression (enet.py:95)
    evaluated at every count 0 .. n -- it is monotone in the count, so the kept counts are one interval.  (1, 0) keeps nothing."""
    af = np.array([float(c) / n for c in range(n + 1)])
    keep = np.nonzero((af > min_af) & (af < max_af) & (0.0 < max_missing))[0]
    return (int(keep[0]), int(keep[-1])) if keep.size else (1, 0)


def _take_names(blob, off, idx):
    """(blob, offsets) of the names idx[] of (blob, off), in the order of idx."""
    blob = np.frombuffer(blob, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    start, length = off[idx], off[idx + 1] - off[idx]
    new_off = np.zeros(idx.size + 1, dtype=np.int64)
    np.cumsum(length, out=new_off[1:])
    src = np.repeat(start - new_off[:-1], length) + np.arange(new_off[-1], dtype=np.int64)
    return blob[src], new_off


def load_all_vars_blocks(engine, p, blocks, min_af, max_af, max_missing, capacity=1 << 16):
    """load_all_vars for k-mers over the raw block stream of the native reader or the packed cache (input.RawBlock: every parsed line, in
    order): each block goes to the device as parsed and sh_enet_ingest keeps, codes and appends its rows there.
    Returns (EnetMatrix, var_indices, number of lines read, names blob, name offsets, carrier counts), the last four per row of the matrix."""
    n = len(p)
    lo, hi = count_bounds(n, min_af, max_af, max_missing)
    M = EnetMatrix(engine, capacity)                                  # (the initial capacity: the matrix grows with the stream)
    var_idx, blobs, lens, counts, loaded = [], [], [], [], 0
    try:
        for blk in blocks:
            idx, cnt = M.ingest(blk.bits, lo, hi)
            if idx.size:
                b, o = _take_names(blk.blob, blk.off, idx)
                var_idx.append(idx.astype(np.int64) + loaded); blobs.append(b); lens.append(np.diff(o)); counts.append(cnt)
            loaded += len(blk)
            if blk.release is not None:
                blk.release()
    except BaseException:
        M.close()
        raise
    if not var_idx:
        M.close()
        raise ValueError("No variants passed filters")
    off = np.zeros(sum(x.size for x in lens) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(lens), out=off[1:])
    return M, np.concatenate(var_idx), loaded, np.concatenate(blobs), off, np.concatenate(counts)


def call_bounds(n, min_af, max_af, max_missing):
    """load_all_vars' rule for a line with missing calls as bounds on counts: (lo, hi, mm) with the line kept iff lo <= t <= hi and m <= mm,
    t = present + missing calls (read_variant counts a missing call as a carrier in af), m = missing calls.  The reference's own expressions
    (enet.py:95: `af > min_af and af < max_af and missing < max_missing`, af = float(t) / n, missing = float(m) / n) are evaluated at every
    count 0 .. n; both are monotone in the count.  (1, 0) for the interval, -1 for mm, when nothing passes."""
    af = np.array([float(t) / n for t in range(n + 1)])
    keep = np.nonzero((af > min_af) & (af < max_af))[0]
    miss = np.nonzero(np.array([float(m) / n for m in range(n + 1)]) < max_missing)[0]
    lo, hi = (int(keep[0]), int(keep[-1])) if keep.size else (1, 0)
    return lo, hi, (int(miss[-1]) if miss.size else -1)


class KeptCalls(object):
    """What load_all_vars_calls keeps on the host per row of the matrix: the name (blob / off), t = present + missing calls, the packed
    missing row of a row that has a missing call (row_bytes each: a row stored by its absences cannot be complemented back without it) and
    the text read_variant writes while it parses the variant.  take(idx) cuts all of them together."""

    def __init__(self, blob, off, counts, has_missing, missing_rows, messages):
        self.blob, self.off, self.counts, self.has_missing, self.missing_rows, self.messages = blob, off, counts, has_missing, missing_rows, messages

    def take(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        blob, off = _take_names(self.blob, self.off, idx)
        at = np.cumsum(self.has_missing) - 1                          # row of missing_rows of every row that has one
        has = self.has_missing[idx]
        return KeptCalls(blob, off, self.counts[idx], has, self.missing_rows[at[idx][has]], self.messages[idx])

    def missing_list(self):
        """per row its packed missing row, None where it has no missing call"""
        at = np.cumsum(self.has_missing) - 1
        return [self.missing_rows[at[i]] if self.has_missing[i] else None for i in range(self.has_missing.size)]


def load_all_vars_calls(engine, p, call_blocks, min_af, max_af, max_missing, err, capacity=1 << 16):
    """load_all_vars for VCF input over the call-block stream of the native reader (input.CallBlock: every variant, in order, with its
    missing calls): per block the variants' messages go to `err` in order, as read_variant writes them on the first pass ("No observations
    of X in selected samples" for every parsed variant nobody carries), and sh_enet_ingest_calls keeps, codes and appends the rows.
    Returns (EnetMatrix, var_indices, number of variants read, KeptCalls); var_indices count every variant read, skipped records included."""
    n = len(p)
    lo, hi, mm = call_bounds(n, min_af, max_af, max_missing)
    M = EnetMatrix(engine, capacity)
    var_idx, blobs, lens, counts, has, mrows, msgs, loaded = [], [], [], [], [], [], [], 0
    try:
        for blk in call_blocks:
            empty = (np.asarray(blk.skip) == 0) & (np.asarray(blk.n_present) + np.asarray(blk.n_missing) == 0)
            messages = blk.messages
            said = set(np.nonzero(empty)[0].tolist())
            said.update(i for i, t in enumerate(messages) if t)
            for i in sorted(said):
                err.write(messages[i])
                if empty[i]:
                    err.write("No observations of " + bytes(blk.blob[blk.off[i]:blk.off[i + 1]]).decode() + " in selected samples\n")
            idx, n_p, n_m = M.ingest_calls(blk.present, blk.missing, blk.skip, lo, hi, mm)
            if idx.size:
                b, o = _take_names(blk.blob, blk.off, idx)
                var_idx.append(idx.astype(np.int64) + loaded); blobs.append(b); lens.append(np.diff(o)); counts.append(n_p + n_m)
                has.append(n_m > 0); mrows.append(np.asarray(blk.missing)[idx[n_m > 0]])
                msgs.append(np.array([messages[i] for i in idx], dtype=object))
            loaded += len(blk)
    except BaseException:
        M.close()
        raise
    if not var_idx:
        M.close()
        raise ValueError("No variants passed filters")
    off = np.zeros(sum(x.size for x in lens) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(lens), out=off[1:])
    kept = KeptCalls(np.concatenate(blobs), off, np.concatenate(counts), np.concatenate(has), np.concatenate(mrows), np.concatenate(msgs))
    return M, np.concatenate(var_idx), loaded, kept


def _r2(y_true, y_pred):
    """sklearn.metrics.r2_score for one output."""
    ss_res, ss_tot = np.sum((y_true - y_pred) ** 2), np.sum((y_true - np.mean(y_true)) ** 2)
    return 1.0 - ss_res / ss_tot


def write_lineage_predictions(true_values, predictions, fold_ids, lineage_dict, continuous, out):
    """pyseer/enet.py:309-376: R2 (and TP / TN / FP / FN for a binary phenotype) within each lineage."""
    out.write("\t".join(['Lineage', 'Size', 'R2']) + ("" if continuous else "\t" + "\t".join(['TP', 'TN', 'FP', 'FN'])) + "\n")
    for fold in range(int(max(fold_ids)) + 1):
        idx = np.where(fold_ids == fold)[0]
        if idx.size == 0:                                             # (enet_predict --true-values: a lineage none of whose samples has a true value)
            continue
        y_true, y_pred = true_values[idx], predictions[idx].reshape(-1)
        fold_r2 = np.nan if np.all(y_true == y_true[0]) else _r2(y_true, y_pred)
        line = [lineage_dict[fold], str(idx.shape[0]), '%.3f' % fold_r2]
        if not continuous:
            tp, tn = int(np.sum((y_true == 1) & (y_pred == 1))), int(np.sum((y_true == 0) & (y_pred == 0)))
            fp, fn = int(np.sum((y_true == 0) & (y_pred == 1))), int(np.sum((y_true == 1) & (y_pred == 0)))
            line += [str(x) for x in (tp, tn, fp, fn)]
        out.write("\t".join(line) + "\n")


def write_predictions(samples, true_values, predictions, fold_ids, lineage_dict, fname):
    """pyseer/enet.py:258-306."""
    with open(fname, 'w') as fout:
        lin = lineage_dict is not None and fold_ids is not None
        fout.write("\t".join(["sample"] + (["lineage", "fold_id"] if lin else []) + ["true_value", "predicted_value"]) + "\n")
        for i, sample in enumerate(samples):
            mid = [lineage_dict[fold_ids[i]], str(fold_ids[i])] if lin else []
            fout.write("\t".join([sample] + mid + [str(true_values[i]), str(predictions[i])]) + "\n")


def find_enet_selected(enet_betas, var_indices, p, c, var_type, fit_seer, burden, burden_regions, infile, all_strains, sample_order,
                       continuous, find_lineage, lin, uncompressed):
    """pyseer/enet.py:424-516: the variants with a non-zero slope, in file order, as Enet tuples."""
    from .classes import Enet
    from .input import read_variant
    from .model import fixed_effects_regression, pre_filtering, fit_lineage_effect
    enet_betas = enet_betas[c.shape[1] + 1:]
    current_var = 0
    for beta, var_idx in zip(enet_betas, var_indices):
        if beta == 0:
            continue
        while current_var < var_idx:
            read_variant(infile, p, var_type, burden, burden_regions, uncompressed, all_strains, sample_order, noparse=True)
            current_var += 1
        eof, k, var_name, kstrains, nkstrains, af, missing = read_variant(infile, p, var_type, burden, burden_regions, uncompressed,
                                                                          all_strains, sample_order)
        current_var += 1
        yield _enet_row(var_name, k, af, kstrains, nkstrains, beta, p, c, fit_seer, continuous, find_lineage, lin)


def _enet_row(var_name, k, af, kstrains, nkstrains, beta, p, c, fit_seer, continuous, find_lineage, lin):
    """the tail of find_enet_selected's loop (pyseer/enet.py:424-516): the Enet tuple of one selected variant."""
    from .classes import Enet
    from .model import fixed_effects_regression, pre_filtering, fit_lineage_effect
    notes = []
    if fit_seer is not None:
        m, null_res, null_firth = fit_seer
        s = fixed_effects_regression(var_name, p.values, k, m, c, af, None, find_lineage, lin, 1, 1, null_res, null_firth,
                                     kstrains, nkstrains, continuous)
        pval, adj_pval, max_lineage, notes = s.prep, s.pvalue, s.max_lineage, s.notes
    else:
        pval, bad = pre_filtering(p.values, k, continuous)
        adj_pval = np.nan
        if bad:
            notes.append("bad-chisq")
        max_lineage = fit_lineage_effect(lin, c, k) if find_lineage else None
    return Enet(var_name, af, pval, adj_pval, beta, max_lineage, kstrains, nkstrains, notes)


def selected_from_rows(enet_betas, rows, names, counts, p, c, fit_seer, continuous, find_lineage, lin, err, missing_rows=None, messages=None):
    """find_enet_selected without a second pass over the input: `rows` are the matrix's rows of the columns with a non-zero slope
    (EnetMatrix.get_rows, fetched before the matrix was closed), in stream order; names = (blob, offsets) and counts are theirs.  A row
    stored by its absences (2 * count > n) is complemented back over the n samples.
    VCF input (load_all_vars_calls): counts are present + missing calls; missing_rows[i] is the packed missing row of row i, or None where
    it has no missing call -- a missing call is 0 in either stored coding, so present = ~stored & ~missing when flipped --, and messages[i]
    the text the reference's second pass writes again when it parses the selected line (a burden line's "Multiple alleles" and "Could not
    parse region").  A missing call is a carrier in the sample lists and in af, and NaN in k, as read_variant has it."""
    from .input import strains_from_bits
    n = len(p)
    samples = [str(x) for x in p.index]
    order = sorted(range(n), key=lambda i: samples[i])
    blob, off = names
    tail = np.zeros(rows.shape[1] * 8, dtype=np.uint8)
    tail[:n] = 1
    valid = np.packbits(tail, bitorder="little")
    for i, beta in enumerate(enet_betas):
        row = rows[i]
        miss = None if missing_rows is None else missing_rows[i]
        if messages is not None:
            err.write(messages[i])
        if 2 * int(counts[i]) > n:
            row = ~row & valid
            if miss is not None:
                row = row & ~miss
        var_name = bytes(blob[off[i]:off[i + 1]]).decode()
        kstrains, nkstrains = strains_from_bits(row if miss is None else (row | (miss & valid)), order, samples)
        if len(kstrains) == 0:                                        # (read_variant says so whenever it parses such a line)
            err.write("No observations of " + var_name + " in selected samples\n")
        k = np.unpackbits(row, bitorder="little")[:n].astype(np.int64)
        if miss is not None:
            k = k.astype(float)
            k[np.unpackbits(miss, bitorder="little")[:n].astype(bool)] = np.nan
        yield _enet_row(var_name, k, float(int(counts[i])) / n, kstrains, nkstrains, beta, p, c, fit_seer, continuous, find_lineage, lin)


def run_cli(options, p, cov, m, null_fit, firth_null, lineage_clusters, lineage_dict, clusters_full, dict_full, enet_seer, out, err):
    """The --wg enet branch of the command line; returns the closing counters (prefilter, tested, printed)."""
    import collections
    from decimal import Decimal
    from .engine import Engine
    from .input import open_variant_file
    from .utils import format_output
    kmers = list(options.kmers) if options.kmers else []
    var_type, var_file = ("kmers", kmers[0]) if kmers else (("vcf", options.vcf) if options.vcf else ("Rtab", options.pres))
    all_strains = set(p.index)
    # k-mers come as raw blocks from the native reader or the packed cache (load_all_vars_blocks), --vcf (with or without --burden) as call
    # blocks from the native VCF reader (load_all_vars_calls): both are filtered, coded and stored on the device and read once;
    # --python-reader and --pres go line by line through read_variant (load_all_vars)
    global LAST_LOAD_ROUTE
    native = bool(options.load_packed) or (var_type == "kmers" and not options.python_reader)
    calls = var_type == "vcf" and not options.python_reader and not options.load_packed
    LAST_LOAD_ROUTE = "blocks" if native else ("calls" if calls else "lines")

    def reopen():
        regions = collections.deque([]) if options.burden else None
        infile, sample_order = open_variant_file(var_type, var_file, options.burden, regions, options.uncompressed)
        return infile, sample_order, regions
    names = counts = kept = None
    engine = Engine(len(p), device=options.gpu)
    if native:
        from .input import open_kmer_block_stream
        blocks, cache_out = open_kmer_block_stream(options, p, kmers, max(options.block_size, 1 << 18), select=engine)
    err.write("Reading all variants\n")
    if native:
        try:
            M, var_indices, loaded, blob, off, counts = load_all_vars_blocks(engine, p, blocks, options.min_af, options.max_af, options.max_missing)
        except ValueError:                                            # (no line passed: the input was read to its end all the same)
            if cache_out is not None:
                cache_out.close()
            raise
        names = (blob, off)
        if cache_out is not None:
            cache_out.close()                                         # (the whole input has been read: the cache is complete)
    elif calls:
        from .input import iter_call_blocks_vcf_native, load_burden
        regions = None
        if options.burden:
            regions = []
            load_burden(options.burden, regions)
        # (2^14 records a block: 2 x 10 MB of rows at N = 5000, and the reader's launches and the three of the ingest are spread over many records)
        blocks = iter_call_blocks_vcf_native(p, var_file, engine, max(options.block_size, 1 << 14), burden_regions=regions)
        M, var_indices, loaded, kept = load_all_vars_calls(engine, p, blocks, options.min_af, options.max_af, options.max_missing, err)
    else:
        infile, sample_order, regions = reopen()
        M, var_indices, loaded = load_all_vars(engine, var_type, p, bool(options.burden), regions, infile, all_strains, sample_order,
                                               options.min_af, options.max_af, options.max_missing, options.uncompressed)
    var_indices = np.array(var_indices)
    pv = p.values.astype(float)
    if options.cor_filter > 0:
        err.write("Applying correlation filtering\n")
        keep = correlation_cut(M.correlations(pv), options.cor_filter)
        if keep.size == 0:
            raise ValueError("No variants passed filters")
        M.keep(keep)
        var_indices = var_indices[keep]
        if native:
            names, counts = _take_names(names[0], names[1], keep), counts[keep]
        if calls:
            kept = kept.take(keep)
    tested = len(var_indices)
    prefilter = loaded - tested
    weights, fold_ids = np.ones(len(p)), None
    if options.sequence_reweighting:                                  # __main__.py:650-654
        weights = np.matmul(clusters_full, 1 / np.sum(clusters_full, axis=0)).reshape(-1)
    if options.lineage_clusters:
        fold_ids = np.where(clusters_full == 1)[1]
        assert fold_ids.shape[0] == weights.shape[0]
    err.write("Fitting elastic net to top " + str(tested) + " variants\n")
    folds = fold_ids if fold_ids is not None else assign_folds(len(p), options.n_folds, options.enet_seed)
    n_folds = int(folds.max()) + 1
    cv = cov.values.astype(float) if cov.shape[1] > 0 else None
    fit = M.fit(pv, options.continuous, options.alpha, weights=weights, covariates=cv, fold_id=folds, n_folds=n_folds,
                thresh=options.enet_thresh)
    betas = np.concatenate([[fit.beta0], fit.beta])
    if TEST_BETAS is not None:
        betas = np.asarray(TEST_BETAS(cov.shape[1], var_indices), dtype=float)
    eta = fit.eta_at(fit.i_min)
    preds = eta if options.continuous else (eta > 0).astype(float)   # cvglmnetPredict: 'link' / 'class'
    sstot = np.sum(np.square(pv - np.mean(pv)))
    r2 = (1 - np.sum(np.square(pv - preds)) / sstot) if sstot != 0 else None
    err.write("Best penalty (lambda) from cross-validation: " + '%.2E' % Decimal(fit.lambdas[fit.i_min]) + "\n")
    if not options.continuous:
        err.write("Best model deviance from cross-validation: " + '%.3f' % Decimal(fit.cvm[fit.i_min]) + " ± " +
                  '%.2E' % Decimal(fit.cvsd[fit.i_min]) + "\n")
    err.write("Best R^2 from cross-validation: " + ('%.3f' % Decimal(float(r2)) if r2 is not None else "nan") + "\n")
    if fold_ids is not None:
        err.write("Predictions within each lineage\n")
        write_lineage_predictions(pv, preds, fold_ids, dict_full, options.continuous, err)
    if options.save_predictions is not None:
        err.write("Writing predictions to " + options.save_predictions + "\n")
        write_predictions(list(p.index), p.values, preds, fold_ids, dict_full if fold_ids is not None else None, options.save_predictions)
    err.write("Finding and printing selected variants\n")
    for beta, covariate in zip(betas[1:cov.shape[1] + 1], cov.columns):
        if beta != 0:
            err.write("Kept covariate '" + str(covariate) + "', slope: " + '%.2E' % Decimal(float(beta)) + "\n")
    header = ['variant', 'af', 'filter-pvalue', 'lrt-pvalue', 'beta']
    lineage_col = bool(options.lineage or (options.sequence_reweighting and options.lineage_clusters))
    if lineage_col:
        header.append('lineage')
    if options.print_samples:
        header += ['k-samples', 'nk-samples']
    header.append('notes')
    out.write('\t'.join(header) + "\n")
    fit_seer = (m, null_fit, firth_null) if enet_seer else None
    if native:
        # the selected variants are resident: their rows come back from the matrix, no input is read a second time
        sel = np.nonzero(betas[cov.shape[1] + 1:])[0]
        sel_rows = M.get_rows(sel)
        selected = selected_from_rows(betas[cov.shape[1] + 1:][sel], sel_rows, _take_names(names[0], names[1], sel), counts[sel], p, cov, fit_seer,
                                      options.continuous, bool(options.lineage), lineage_clusters, err)
    if calls:
        sel = np.nonzero(betas[cov.shape[1] + 1:])[0]
        sel_rows = M.get_rows(sel)
        kept = kept.take(sel)
        selected = selected_from_rows(betas[cov.shape[1] + 1:][sel], sel_rows, (kept.blob, kept.off), kept.counts, p, cov, fit_seer,
                                      options.continuous, bool(options.lineage), lineage_clusters, err,
                                      missing_rows=kept.missing_list(), messages=kept.messages)
    M.close()
    engine.close()
    if not (native or calls):
        infile, sample_order, regions = reopen()
        selected = find_enet_selected(betas, var_indices, p, cov, var_type, fit_seer, bool(options.burden), regions, infile, all_strains,
                                      sample_order, options.continuous, bool(options.lineage), lineage_clusters, options.uncompressed)
    printed = 0
    label = (lineage_dict if lineage_dict is not None else []) if lineage_col else None
    # the model of --save-enet-model (__main__.py:677-711): the intercept, the covariates with a slope (at the mean of their column over the
    # training samples, from the same positions of `betas` as the lines above), the printed variants with the af and beta of their rows
    pred_model = collections.OrderedDict([('intercept', (1, betas[0]))])
    for beta, covariate in zip(betas[1:cov.shape[1] + 1], cov.columns):
        if beta != 0:
            pred_model[str(covariate)] = (float(np.mean(cov[covariate])), beta)
    for x in selected:
        printed += 1
        out.write(format_output(x, label, 'enet', options.print_samples) + "\n")
        pred_model[x.kmer] = (x.af, x.kbeta)
    if getattr(options, "save_enet_model", None):
        write_model(options.save_enet_model, pred_model, options.continuous)
        err.write("Saved enet model as " + options.save_enet_model + "\n")
    return prefilter, tested, printed


# ---------------------------------------------------------------------------------------------------------------
# the saved model and its predictor (python -m pyseer_amd.enet_predict; pyseer/enet_predict.py)
# ---------------------------------------------------------------------------------------------------------------
MODEL_MAGIC = "#pyseer_amd-enet-model"
MODEL_VERSION = 1


def write_model(fname, model, continuous):
    """The model as text: a header line, then name<TAB>af<TAB>beta per entry of `model` (a mapping name -> (af, beta)) in its order.  Floats
    are written with repr, so read_model returns the same bits.  A name may hold spaces (Rtab gene names), not a tab or a line break."""
    with open(fname, "w", newline="\n") as fout:
        fout.write("%s\tversion=%d\tcontinuous=%d\n" % (MODEL_MAGIC, MODEL_VERSION, 1 if continuous else 0))
        for name, (af, beta) in model.items():
            name = str(name)
            if name == "" or "\t" in name or "\n" in name or "\r" in name:
                raise ValueError("a model entry's name may not be empty or hold a tab or a line break: %r" % name)
            fout.write("%s\t%s\t%s\n" % (name, repr(float(af)), repr(float(beta))))


class _ModelUnpickler(object):
    """pickle.Unpickler that admits what the reference's model needs -- a list of a dict of tuples of Python and numpy scalars and a bool --
    and no other global: loading a model runs nobody's code."""
    ALLOWED = {("collections", "OrderedDict"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"), ("numpy", "dtype"),
               ("_codecs", "encode")}                                 # (protocol 2 writes the bytes of a numpy scalar as an encoded str)

    @classmethod
    def load(cls, fh):
        import pickle

        class Restricted(pickle.Unpickler):
            def find_class(self, module, name):
                if (module, name) in cls.ALLOWED:
                    return pickle.Unpickler.find_class(self, module, name)
                raise pickle.UnpicklingError("the model names the global %s.%s: refused (a model holds names and numbers only)" % (module, name))
        return Restricted(fh).load()


def read_model(fname):
    """(OrderedDict name -> (af, beta), continuous) from the text form of write_model, or from the reference's pickle
    ([{name: (af, beta), 'intercept': (1, b0)}, continuous], pyseer/__main__.py:705-711) through an unpickler that refuses every other global.
    Raises ValueError for anything else."""
    import collections
    import pickle
    with open(fname, "rb") as fh:
        head = fh.read(2)
        fh.seek(0)
        if head[:1] == b"\x80":                                       # a pickle of protocol 2 and later begins with PROTO
            try:
                obj = _ModelUnpickler.load(fh)
                model_dict, continuous = obj
                model = collections.OrderedDict((str(k), (float(v[0]), float(v[1]))) for k, v in model_dict.items())
            except pickle.UnpicklingError as e:
                raise ValueError(str(e))
            except Exception as e:
                raise ValueError("%s is not a model pickle of [dict of (af, beta), continuous]: %s" % (fname, e))
            return model, bool(continuous)
        text = fh.read()
    try:
        lines = text.decode("utf-8").split("\n")
    except UnicodeDecodeError:
        raise ValueError("%s is neither a text model nor a pickle" % fname)
    header = lines[0].split("\t")
    if header[0] != MODEL_MAGIC or len(header) != 3 or header[1] != "version=%d" % MODEL_VERSION or header[2] not in ("continuous=0", "continuous=1"):
        raise ValueError("%s does not begin with the header of a version %d model (%s)" % (fname, MODEL_VERSION, MODEL_MAGIC))
    model = collections.OrderedDict()
    for i, line in enumerate(lines[1:]):
        if line == "":
            continue
        f = line.split("\t")
        try:
            if len(f) != 3 or f[0] == "":
                raise ValueError
            model[f[0]] = (float(f[1]), float(f[2]))                  # (a name given twice: the last stands, as in a dict)
        except ValueError:
            raise ValueError("%s line %d is not name<TAB>af<TAB>beta" % (fname, i + 2))
    return model, header[2] == "continuous=1"


class NameSet(object):
    """The model's names as the library's hash set (sh_nameset_*): match() returns the rows of a block's name blob that are in the model and
    were not met before, with the index of the name; a name is retired at its first hit."""

    def __init__(self, names):
        self._lib = _abi.load()
        enc = [str(x).encode() for x in names]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in enc], out=off[1:])
        h = self._lib.sh_nameset_new(b"".join(enc), off.ctypes.data_as(C.POINTER(C.c_int64)), len(enc))
        if not h:
            raise MemoryError("sh_nameset_new failed")
        self._h = C.c_void_p(h)

    def match(self, blob, off):
        """blob: bytes or a uint8 array; off: V + 1 int64 offsets -> (row indices int64, model indices int32), in block order."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        V = off.size - 1
        if V < 1:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
        rows, which = np.empty(V, dtype=np.int64), np.empty(V, dtype=np.int32)
        if isinstance(blob, np.ndarray):
            keep = np.ascontiguousarray(blob, dtype=np.uint8)
            ptr = C.c_void_p(keep.ctypes.data)
        else:
            keep = bytes(blob)
            ptr = C.cast(C.c_char_p(keep), C.c_void_p)
        n = self._lib.sh_nameset_match(self._h, ptr, off.ctypes.data_as(C.POINTER(C.c_int64)), V, rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                       which.ctypes.data_as(C.POINTER(C.c_int32)))
        if n < 0:
            raise ValueError("sh_nameset_match: bad arguments")
        return rows[:n], which[:n]

    @property
    def left(self):
        return int(self._lib.sh_nameset_left(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sh_nameset_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EnetPredictor(object):
    """The sum of pyseer/enet_predict.py:174-179 on the device of `engine` (sh_predict_*): an fp64 accumulator per sample that starts at
    `start` and takes `k * beta` of every row added, in the order added."""

    def __init__(self, engine, start):
        self._e, self._lib, self._h = engine, engine._lib, engine._h
        self.n = engine.n
        self.row_bytes = row_bytes_for(self.n)
        start = np.ascontiguousarray(start, dtype=float).reshape(-1)
        if start.shape != (self.n,):
            raise ValueError("start must hold one value per sample")
        _abi.check(self._lib.sh_predict_begin(self._h, start.ctypes.data_as(_abi.c_dp)))
        self._open = True

    def add(self, block_bits, idx, beta, flip, missing=None):
        """Rows idx[] of the packed block (V, row_bytes) with slopes beta[] and flips flip[], in this order; missing: the block's missing-call
        rows (same shape) or None."""
        bits = np.asarray(block_bits)
        if bits.dtype != np.uint8 or bits.ndim != 2 or bits.shape[1] != self.row_bytes or not bits.flags.c_contiguous:
            bits = np.ascontiguousarray(bits, dtype=np.uint8)
            if bits.ndim != 2 or bits.shape[1] != self.row_bytes:
                raise ValueError("packed rows must be (V, %d) bytes" % self.row_bytes)
        V = bits.shape[0]
        miss = None
        if missing is not None:
            miss = np.ascontiguousarray(missing, dtype=np.uint8)
            if miss.shape != bits.shape:
                raise ValueError("the missing rows must have the shape of the block")
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        beta = np.ascontiguousarray(beta, dtype=float).reshape(-1)
        flip = np.ascontiguousarray(np.asarray(flip).reshape(-1) != 0, dtype=np.uint8)
        if beta.shape != idx.shape or flip.shape != idx.shape:
            raise ValueError("idx, beta and flip must have one entry per selected row")
        if idx.size == 0:
            return
        if idx.min() < 0 or idx.max() >= V:
            raise ValueError("row index outside the block")
        _abi.check(self._lib.sh_predict_add(self._h, C.cast(bits.ctypes.data, _abi.c_u8p), None if miss is None else C.cast(miss.ctypes.data, _abi.c_u8p),
                                            self.row_bytes, idx.ctypes.data_as(C.POINTER(C.c_int64)), beta.ctypes.data_as(_abi.c_dp),
                                            flip.ctypes.data_as(_abi.c_u8p), idx.size))

    def finish(self):
        """The accumulator, (n,) float64; the predictor is closed."""
        out = np.empty(self.n)
        self._open = False
        _abi.check(self._lib.sh_predict_end(self._h, out.ctypes.data_as(_abi.c_dp)))
        return out

    def close(self):
        if self._open and self._e._h:
            self._lib.sh_predict_end(self._h, None)
        self._open = False
