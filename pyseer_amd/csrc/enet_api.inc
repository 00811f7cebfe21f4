// enet_api.inc -- sh_enet_*: the whole-genome elastic net of pyseer/enet.py on one resident bit matrix (included by api.hip).
// The device does every pass over samples or rows (enet_kernels.hip); this file sequences lambda values, strong sets and the KKT loop.

extern "C++" {
struct EnetPoint { double b0 = 0.0; std::vector<int> idx; std::vector<double> val; };     // one solution, standardised scale, non-zeros only
struct EnetState {
    int64_t NW = 0, cap = 0, P = 0;
    uint64_t *d_B = nullptr;
    // sh_enet_ingest: the block as it came from the host, and per row its count and destination, the kept rows' indices and counts, the total
    uint64_t *d_stage = nullptr; int32_t *d_meta = nullptr; int64_t stage_rows = 0;
    // sh_enet_ingest_calls: the present and the missing block, and per row its two counts, skip flag and destination, the kept rows' figures
    uint64_t *d_cstage_p = nullptr, *d_cstage_m = nullptr; int32_t *d_cmeta = nullptr; int64_t cstage_rows = 0;
    // the last fit
    int F1 = 0, n_cov = 0, n_lam = 0, N = 0;
    std::vector<std::vector<EnetPoint>> path;                        // [problem][lambda]
    std::vector<std::vector<double>> m, sinv, cmean, csinv;          // [problem][P], [problem][n_cov]
    std::vector<double> eta;                                         // [lambda][N] of the full fit
};
struct DevBuf {                                                      // a device allocation that ends with its scope
    void *p = nullptr;
    ~DevBuf() { hipFree(p); }
    hipError_t alloc(size_t bytes) { hipFree(p); p = nullptr; return hipMalloc(&p, bytes ? bytes : 8); }
    template <typename T> T *as() { return static_cast<T *>(p); }
};
}

// the solutions of the last fit belong to the matrix they were fitted on: a changed matrix, or a fit that fails, leaves none
static void enet_forget_fit(EnetState *e) { e->n_lam = 0; e->F1 = 0; e->path.clear(); e->eta.clear(); }

// (the staging of the last ingested block is of no use to a fit or a cut: up to 166 MB at N = 5000 go back to the device)
static void enet_free_cstage(EnetState *e)
{
    hipFree(e->d_cstage_p); hipFree(e->d_cstage_m); hipFree(e->d_cmeta);
    e->d_cstage_p = e->d_cstage_m = nullptr; e->d_cmeta = nullptr; e->cstage_rows = 0;
}
static void enet_free_stage(EnetState *e)
{
    hipFree(e->d_stage); hipFree(e->d_meta); e->d_stage = nullptr; e->d_meta = nullptr; e->stage_rows = 0;
    enet_free_cstage(e);
}

static void enet_free(sh_ctx *c)
{
    if (!c->enet) return;
    enet_free_stage(c->enet);
    hipFree(c->enet->d_B);
    delete c->enet; c->enet = nullptr;
}

int sh_enet_begin(sh_ctx *c, int64_t row_bytes, int64_t capacity)
{
    if (!c) return fail(SH_EINVAL, "null ctx");
    if (row_bytes % 8 || row_bytes * 8 < c->N || capacity < 1) return fail(SH_ESHAPE, "sh_enet_begin: row_bytes must be a multiple of 8 covering n_samples, capacity >= 1");
    HIPCHK(hipSetDevice(c->device));
    enet_free(c);
    c->enet = new EnetState();
    c->enet->NW = row_bytes / 8; c->enet->cap = capacity;
    if (hipMalloc((void **)&c->enet->d_B, (size_t)capacity * row_bytes) != hipSuccess) { enet_free(c); return fail(SH_ENOMEM, "sh_enet_begin: the bit matrix does not fit the device"); }
    return SH_OK;
}

int sh_enet_end(sh_ctx *c) { if (!c) return fail(SH_EINVAL, "null ctx"); hipSetDevice(c->device); enet_free(c); return SH_OK; }

int64_t sh_enet_rows(sh_ctx *c) { return c && c->enet ? c->enet->P : -1; }

#define ENET_UP(buf, vec) do { HIPCHK((buf).alloc((vec).size() * sizeof((vec)[0]))); HIPCHK(hipMemcpy((buf).p, (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice)); } while (0)

int sh_enet_append(sh_ctx *c, const uint8_t *present, const uint8_t *missing, const uint8_t *flip, int64_t V)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_append before sh_enet_begin");
    EnetState *e = c->enet;
    if (V < 0 || e->P + V > e->cap) return fail(SH_ESHAPE, "sh_enet_append: more rows than sh_enet_begin reserved");
    enet_forget_fit(e);
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = (size_t)V * e->NW * 8;
    DevBuf dp, dm, df;
    HIPCHK(dp.alloc(bytes)); HIPCHK(hipMemcpy(dp.p, present, bytes, hipMemcpyHostToDevice));
    if (missing) { HIPCHK(dm.alloc(bytes)); HIPCHK(hipMemcpy(dm.p, missing, bytes, hipMemcpyHostToDevice)); }
    if (flip) { HIPCHK(df.alloc(V)); HIPCHK(hipMemcpy(df.p, flip, V, hipMemcpyHostToDevice)); }
    HIPCHK(shk_enet_store(c->stream, dp.as<uint8_t>(), dm.as<uint8_t>(), df.as<uint8_t>(), V, (int)e->NW, c->N, e->d_B + e->P * e->NW));
    HIPCHK(hipStreamSynchronize(c->stream));
    e->P += V;
    return SH_OK;
}

// room for `rows` rows: a new allocation of at least twice the capacity, the stored rows copied device to device; a failure leaves the matrix as it was
static int enet_reserve(sh_ctx *c, int64_t rows)
{
    EnetState *e = c->enet;
    if (rows <= e->cap) return SH_OK;
    uint64_t *nb = nullptr;
    int64_t cap = std::max<int64_t>(rows, 2 * e->cap);
    if (hipMalloc((void **)&nb, (size_t)cap * e->NW * 8) != hipSuccess) {
        (void)hipGetLastError();
        cap = rows; nb = nullptr;                                     // (twice does not fit: what is needed now may)
        if (hipMalloc((void **)&nb, (size_t)cap * e->NW * 8) != hipSuccess) { (void)hipGetLastError(); return fail(SH_ENOMEM, "sh_enet_ingest: the bit matrix does not fit the device"); }
    }
    if (e->P > 0) {
        const hipError_t rc = hipMemcpy(nb, e->d_B, (size_t)e->P * e->NW * 8, hipMemcpyDeviceToDevice);
        if (rc != hipSuccess) { hipFree(nb); return fail(SH_EHIP, std::string("sh_enet_ingest: copy of the stored rows: ") + hipGetErrorString(rc)); }
    }
    hipFree(e->d_B); e->d_B = nb; e->cap = cap;
    return SH_OK;
}

int64_t sh_enet_ingest(sh_ctx *c, const uint8_t *bits, int64_t V, int32_t min_count, int32_t max_count, int32_t *kept_idx, int32_t *kept_count)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_ingest before sh_enet_begin");
    EnetState *e = c->enet;
    if (V < 0 || V > INT32_MAX) return fail(SH_ESHAPE, "sh_enet_ingest: a block holds 0 .. 2^31 - 1 rows");
    if (V > 0 && (!bits || !kept_idx || !kept_count)) return fail(SH_EINVAL, "sh_enet_ingest: null argument");
    enet_forget_fit(e);
    if (V == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    if (V > e->stage_rows) {
        enet_free_stage(e);
        if (hipMalloc((void **)&e->d_stage, (size_t)V * e->NW * 8) != hipSuccess || hipMalloc((void **)&e->d_meta, ((size_t)4 * V + 1) * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError(); enet_free_stage(e);
            return fail(SH_ENOMEM, "sh_enet_ingest: the block does not fit the device");
        }
        e->stage_rows = V;
    }
    int32_t *d_cnt = e->d_meta, *d_dest = d_cnt + V, *d_kidx = d_dest + V, *d_kcnt = d_kidx + V, *d_n = d_kcnt + V;
    HIPCHK(hipMemcpyAsync(e->d_stage, bits, (size_t)V * e->NW * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(shk_enet_ingest_count(c->stream, e->d_stage, V, (int)e->NW, c->N, min_count, max_count, d_cnt, d_dest, d_kidx, d_kcnt, d_n));
    int32_t kept = 0;
    HIPCHK(hipMemcpyAsync(&kept, d_n, sizeof(kept), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kept < 0 || kept > V) return fail(SH_EHIP, "sh_enet_ingest: the scan returned an impossible count");
    if (kept == 0) return 0;
    const int rc = enet_reserve(c, e->P + kept); if (rc) return rc;
    HIPCHK(shk_enet_ingest_scatter(c->stream, e->d_stage, V, (int)e->NW, c->N, d_cnt, d_dest, e->d_B + e->P * e->NW));
    HIPCHK(hipMemcpyAsync(kept_idx, d_kidx, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(kept_count, d_kcnt, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    e->P += kept;
    return kept;
}

int64_t sh_enet_ingest_calls(sh_ctx *c, const uint8_t *present, const uint8_t *missing, const int32_t *skip, int64_t V, int32_t min_count, int32_t max_count,
                             int32_t max_missing_count, int32_t *kept_idx, int32_t *kept_present, int32_t *kept_missing)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_ingest_calls before sh_enet_begin");
    EnetState *e = c->enet;
    if (V < 0 || V > INT32_MAX) return fail(SH_ESHAPE, "sh_enet_ingest_calls: a block holds 0 .. 2^31 - 1 rows");
    if (V > 0 && (!present || !kept_idx || !kept_present || !kept_missing)) return fail(SH_EINVAL, "sh_enet_ingest_calls: null argument");
    enet_forget_fit(e);
    if (V == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    if (V > e->cstage_rows) {
        enet_free_cstage(e);
        if (hipMalloc((void **)&e->d_cstage_p, (size_t)V * e->NW * 8) != hipSuccess || hipMalloc((void **)&e->d_cstage_m, (size_t)V * e->NW * 8) != hipSuccess ||
            hipMalloc((void **)&e->d_cmeta, ((size_t)7 * V + 1) * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError(); enet_free_cstage(e);
            return fail(SH_ENOMEM, "sh_enet_ingest_calls: the block does not fit the device");
        }
        e->cstage_rows = V;
    }
    int32_t *d_cp = e->d_cmeta, *d_cm = d_cp + V, *d_skip = d_cm + V, *d_dest = d_skip + V, *d_kidx = d_dest + V, *d_kp = d_kidx + V, *d_km = d_kp + V, *d_n = d_km + V;
    const size_t bytes = (size_t)V * e->NW * 8;
    HIPCHK(hipMemcpyAsync(e->d_cstage_p, present, bytes, hipMemcpyHostToDevice, c->stream));
    if (missing) HIPCHK(hipMemcpyAsync(e->d_cstage_m, missing, bytes, hipMemcpyHostToDevice, c->stream));
    if (skip) HIPCHK(hipMemcpyAsync(d_skip, skip, (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const uint64_t *d_miss = missing ? e->d_cstage_m : nullptr;
    HIPCHK(shk_enet_ingest_calls_count(c->stream, e->d_cstage_p, d_miss, skip ? d_skip : nullptr, V, (int)e->NW, c->N, min_count, max_count, max_missing_count,
                                       d_cp, d_cm, d_dest, d_kidx, d_kp, d_km, d_n));
    int32_t kept = 0;
    HIPCHK(hipMemcpyAsync(&kept, d_n, sizeof(kept), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kept < 0 || kept > V) return fail(SH_EHIP, "sh_enet_ingest_calls: the scan returned an impossible count");
    if (kept == 0) return 0;
    const int rc = enet_reserve(c, e->P + kept); if (rc) return rc;
    HIPCHK(shk_enet_ingest_calls_scatter(c->stream, e->d_cstage_p, d_miss, V, (int)e->NW, c->N, d_cp, d_cm, d_dest, e->d_B + e->P * e->NW));
    HIPCHK(hipMemcpyAsync(kept_idx, d_kidx, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(kept_present, d_kp, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(kept_missing, d_km, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    e->P += kept;
    return kept;
}

int sh_enet_correlations(sh_ctx *c, const double *y, double *out_abs_cor)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_correlations before sh_enet_begin");
    EnetState *e = c->enet; const int N = c->N; const int64_t Np = e->NW * 64;
    HIPCHK(hipSetDevice(c->device));
    double mean = 0.0; for (int i = 0; i < N; ++i) mean += y[i]; mean /= N;
    std::vector<double> yc(Np, 0.0); double sb2 = 0.0;
    for (int i = 0; i < N; ++i) { yc[i] = y[i] - mean; sb2 += yc[i] * yc[i]; }
    DevBuf dy, dout; ENET_UP(dy, yc); HIPCHK(dout.alloc(e->P * sizeof(double)));
    HIPCHK(shk_enet_moments(c->stream, e->d_B, e->P, (int)e->NW, N, dy.as<double>(), sb2, dout.as<double>()));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out_abs_cor, dout.p, e->P * sizeof(double), hipMemcpyDeviceToHost));
    return SH_OK;
}

static int enet_gather(sh_ctx *c, const int64_t *idx, int64_t n, uint64_t *d_dst)
{
    EnetState *e = c->enet;
    for (int64_t k = 0; k < n; ++k) if (idx[k] < 0 || idx[k] >= e->P) return fail(SH_ESHAPE, "row index out of range");
    DevBuf di; HIPCHK(di.alloc(n * sizeof(int64_t))); HIPCHK(hipMemcpy(di.p, idx, n * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(shk_enet_gather(c->stream, e->d_B, di.as<int64_t>(), n, (int)e->NW, d_dst));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SH_OK;
}

int sh_enet_keep(sh_ctx *c, const int64_t *idx, int64_t n_keep)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_keep before sh_enet_begin");
    EnetState *e = c->enet;
    if (n_keep < 0 || n_keep > e->P) return fail(SH_ESHAPE, "sh_enet_keep: bad count");
    HIPCHK(hipSetDevice(c->device));
    enet_free_stage(e);
    uint64_t *nb = nullptr;
    HIPCHK(hipMalloc((void **)&nb, (size_t)std::max<int64_t>(n_keep, 1) * e->NW * 8));
    const int rc = enet_gather(c, idx, n_keep, nb);
    if (rc) { hipFree(nb); return rc; }
    enet_forget_fit(e);
    hipFree(e->d_B); e->d_B = nb; e->P = n_keep; e->cap = std::max<int64_t>(n_keep, 1);
    return SH_OK;
}

int sh_enet_get_rows(sh_ctx *c, const int64_t *idx, int64_t n, uint8_t *rows)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_get_rows before sh_enet_begin");
    EnetState *e = c->enet;
    if (n <= 0) return SH_OK;
    HIPCHK(hipSetDevice(c->device));
    DevBuf d; HIPCHK(d.alloc((size_t)n * e->NW * 8));
    const int rc = enet_gather(c, idx, n, d.as<uint64_t>()); if (rc) return rc;
    HIPCHK(hipMemcpy(rows, d.p, (size_t)n * e->NW * 8, hipMemcpyDeviceToHost));
    return SH_OK;
}

// carrier sums of nv vectors (host, [nv][Np]) over every row -> out[nv][P], 16 vectors a pass
static int enet_carrier_sums(sh_ctx *c, const double *d_V, int nv, double *d_G, std::vector<double> *out)
{
    EnetState *e = c->enet; const int64_t Np = e->NW * 64;
    for (int f0 = 0; f0 < nv; f0 += 16) {
        const int nf = std::min(16, nv - f0);
        HIPCHK(shk_enet_grad(c->stream, e->d_B, e->P, (int)e->NW, d_V + f0 * Np, Np, nf, d_G + f0 * e->P, e->P));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out) { out->resize((size_t)nv * e->P); HIPCHK(hipMemcpy(out->data(), d_G, out->size() * sizeof(double), hipMemcpyDeviceToHost)); }
    return SH_OK;
}

int sh_enet_carrier_sums(sh_ctx *c, const double *vectors, int n_vectors, double *out)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_carrier_sums before sh_enet_begin");
    EnetState *e = c->enet; const int N = c->N; const int64_t Np = e->NW * 64;
    if (n_vectors < 1 || !vectors || !out) return fail(SH_EINVAL, "sh_enet_carrier_sums: vectors");
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> v((size_t)n_vectors * Np, 0.0), g;
    for (int f = 0; f < n_vectors; ++f) std::copy(vectors + (size_t)f * N, vectors + (size_t)(f + 1) * N, v.begin() + (size_t)f * Np);
    DevBuf dv, dg; ENET_UP(dv, v); HIPCHK(dg.alloc((size_t)n_vectors * e->P * sizeof(double)));
    const int rc = enet_carrier_sums(c, dv.as<double>(), n_vectors, dg.as<double>(), nullptr); if (rc) return rc;
    HIPCHK(hipMemcpy(out, dg.p, (size_t)n_vectors * e->P * sizeof(double), hipMemcpyDeviceToHost));
    return SH_OK;
}

int sh_enet_fit(sh_ctx *c, const double *y, const double *weights, const double *covariates, int n_cov, const int32_t *fold_id, int n_folds,
                int family, double alpha, const sh_enet_opts *opts, sh_enet_out *out)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_fit before sh_enet_begin");
    if (!y || !opts || !out) return fail(SH_EINVAL, "sh_enet_fit: null argument");
    EnetState *e = c->enet; const int N = c->N; const int64_t P = e->P, NW = e->NW, Np = NW * 64, PT = P + n_cov;
    enet_forget_fit(e);
    if (P < 1) return fail(SH_ESHAPE, "No variants passed filters");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(SH_EINVAL, "sh_enet_fit: alpha must lie in [0, 1]");
    if (family != 0 && family != 1) return fail(SH_EINVAL, "sh_enet_fit: family is 0 (gaussian) or 1 (binomial)");
    if (n_folds < 0 || n_folds == 1 || (n_folds > 0 && !fold_id) || n_cov < 0 || (n_cov > 0 && !covariates)) return fail(SH_EINVAL, "sh_enet_fit: folds / covariates");
    if (PT > INT32_MAX) return fail(SH_ESHAPE, "sh_enet_fit: too many coordinates");
    const int nlam = opts->n_lambda > 0 ? opts->n_lambda : 100;
    const double thresh = opts->thresh > 0.0 ? opts->thresh : 1e-7;
    const int max_sweeps = opts->max_sweeps > 0 ? opts->max_sweeps : 100000;
    const int F1 = n_folds + 1;
    HIPCHK(hipSetDevice(c->device));
    enet_free_stage(e);
    if (family == 1) for (int i = 0; i < N; ++i) if (y[i] != 0.0 && y[i] != 1.0) return fail(SH_EINVAL, "sh_enet_fit: a binomial response is 0 or 1");
    for (int i = 0; i < N && n_folds; ++i) if (fold_id[i] < 0 || fold_id[i] >= n_folds) return fail(SH_EINVAL, "sh_enet_fit: fold_id outside [0, n_folds)");

    // ---- weights of the F1 problems: problem 0 is the full fit, problem 1 + k leaves fold k out; each normalised to sum 1
    std::vector<double> wfull(N), w((size_t)F1 * Np, 0.0), hw((size_t)F1 * Np, 0.0), ind((size_t)F1 * Np, 0.0), yp(Np, 0.0), hwsum(F1, 0.0);
    { double s = 0.0; for (int i = 0; i < N; ++i) { wfull[i] = weights ? weights[i] : 1.0; if (!(wfull[i] >= 0.0)) return fail(SH_EINVAL, "sh_enet_fit: negative weight"); s += wfull[i]; }
      if (!(s > 0.0)) return fail(SH_EINVAL, "sh_enet_fit: weights sum to 0");
      for (int i = 0; i < N; ++i) { wfull[i] /= s; yp[i] = y[i]; } }
    for (int f = 0; f < F1; ++f) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) { const bool held = f > 0 && fold_id[i] == f - 1; if (!held) s += wfull[i]; else { hw[f * Np + i] = wfull[i]; hwsum[f] += wfull[i]; } }
        if (!(s > 0.0)) return fail(SH_EINVAL, "sh_enet_fit: a fold holds every weighted sample");
        for (int i = 0; i < N; ++i) { const bool held = f > 0 && fold_id[i] == f - 1; if (!held) { w[f * Np + i] = wfull[i] / s; ind[f * Np + i] = wfull[i] > 0.0 ? 1.0 : 0.0; } }
    }
    // ---- standardisation per problem: weighted mean of every row (a carrier sum of w) and the count of its carriers among the trained samples
    DevBuf d_w, d_hw, d_ind, d_y, d_G; ENET_UP(d_w, w); ENET_UP(d_hw, hw); ENET_UP(d_ind, ind); ENET_UP(d_y, yp);
    HIPCHK(d_G.alloc((size_t)F1 * P * sizeof(double)));
    std::vector<double> mv, cntv, sinv((size_t)F1 * P);
    int rc = enet_carrier_sums(c, d_w.as<double>(), F1, d_G.as<double>(), &mv); if (rc) return rc;
    rc = enet_carrier_sums(c, d_ind.as<double>(), F1, d_G.as<double>(), &cntv); if (rc) return rc;
    for (int f = 0; f < F1; ++f) {
        double ntrain = 0.0; for (int i = 0; i < N; ++i) ntrain += ind[f * Np + i];
        for (int64_t j = 0; j < P; ++j) {
            const double m = mv[f * P + j], cn = cntv[f * P + j], v = m - m * m;        // x^2 = x
            sinv[f * P + j] = (cn == 0.0 || cn == ntrain || !(v > 0.0)) ? 0.0 : 1.0 / sqrt(v);
        }
    }
    std::vector<double> Xc((size_t)F1 * std::max(n_cov, 1) * Np, 0.0), cmean((size_t)F1 * std::max(n_cov, 1), 0.0), csinv(cmean.size(), 0.0);
    for (int f = 0; f < F1; ++f) for (int k = 0; k < n_cov; ++k) {
        const double *x = covariates + (size_t)k * N, *wf = &w[f * Np];
        double m = 0.0, v = 0.0;
        for (int i = 0; i < N; ++i) m += wf[i] * x[i];
        for (int i = 0; i < N; ++i) v += wf[i] * (x[i] - m) * (x[i] - m);
        const double si = v > 0.0 ? 1.0 / sqrt(v) : 0.0;
        cmean[f * n_cov + k] = m; csinv[f * n_cov + k] = si;
        for (int i = 0; i < N; ++i) Xc[((size_t)f * n_cov + k) * Np + i] = (x[i] - m) * si;
    }
    // ---- null models
    std::vector<double> b0n(F1), nulldev(F1), thr(F1), vr0((size_t)F1 * Np, 0.0);
    for (int f = 0; f < F1; ++f) {
        const double *wf = &w[f * Np];
        double mu = 0.0; for (int i = 0; i < N; ++i) mu += wf[i] * y[i];
        double nd = 0.0;
        if (family == 0) { for (int i = 0; i < N; ++i) nd += wf[i] * (y[i] - mu) * (y[i] - mu); b0n[f] = mu; thr[f] = thresh * nd; }
        else {
            if (!(mu > 0.0 && mu < 1.0)) return fail(SH_EINVAL, "sh_enet_fit: a binomial response is constant over the trained samples of one problem");
            nd = -2.0 * (mu * log(mu) + (1.0 - mu) * log(1.0 - mu)); b0n[f] = log(mu / (1.0 - mu)); thr[f] = thresh * 0.5 * nd;
        }
        nulldev[f] = nd;
        for (int i = 0; i < N; ++i) vr0[f * Np + i] = wf[i] * (y[i] - mu);
    }
    // ---- buffers of the descent
    std::vector<double> zeroPT((size_t)F1 * PT, 0.0);
    DevBuf d_m, d_sinv, d_Xc, d_thr, d_b0n, d_act, d_nact, d_skip, d_beta, d_bold, d_xv, d_state, d_scal, d_vr, d_eta, d_res;
    ENET_UP(d_m, mv); ENET_UP(d_sinv, sinv); ENET_UP(d_Xc, Xc); ENET_UP(d_thr, thr); ENET_UP(d_b0n, b0n); ENET_UP(d_beta, zeroPT); ENET_UP(d_vr, vr0);
    HIPCHK(d_act.alloc((size_t)F1 * PT * sizeof(int))); HIPCHK(d_nact.alloc(F1 * sizeof(int))); HIPCHK(d_skip.alloc(F1 * sizeof(int)));
    HIPCHK(d_bold.alloc((size_t)F1 * PT * sizeof(double))); HIPCHK(d_xv.alloc((size_t)F1 * PT * sizeof(double)));
    HIPCHK(d_state.alloc((size_t)F1 * 3 * Np * sizeof(double))); HIPCHK(d_scal.alloc(F1 * 4 * sizeof(double)));
    HIPCHK(d_eta.alloc((size_t)F1 * Np * sizeof(double))); HIPCHK(d_res.alloc(F1 * 8 * sizeof(double)));
    HIPCHK(hipMemset(d_state.p, 0, (size_t)F1 * 3 * Np * sizeof(double))); HIPCHK(hipMemset(d_scal.p, 0, F1 * 4 * sizeof(double)));
    HIPCHK(hipMemset(d_xv.p, 0, (size_t)F1 * PT * sizeof(double))); HIPCHK(hipMemset(d_bold.p, 0, (size_t)F1 * PT * sizeof(double)));
    // the per-sample state stays in the LDS of the problem's CU while it fits what one workgroup may declare there
    int lds_max = 0; HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    if (lds_max < 160 * 1024) { int optin = 0; if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, c->device) == hipSuccess) lds_max = std::max(lds_max, optin); }
    const bool use_lds = !opts->state_in_global && shk_enet_cd_lds_bytes((int)NW, family) <= (size_t)lds_max;

    EnetCdArgs a{};
    a.B = e->d_B; a.P = P; a.N = N; a.NW = (int)NW; a.n_cov = n_cov; a.family = family; a.use_lds = use_lds ? 1 : 0; a.max_sweeps = max_sweeps; a.max_outer = 25;
    a.alpha = alpha; a.y = d_y.as<double>(); a.w = d_w.as<double>(); a.hw = d_hw.as<double>(); a.m = d_m.as<double>(); a.sinv = d_sinv.as<double>();
    a.Xc = d_Xc.as<double>(); a.thr = d_thr.as<double>(); a.b0_null = d_b0n.as<double>(); a.act = d_act.as<int>(); a.nact = d_nact.as<int>();
    a.skip = d_skip.as<int>(); a.beta = d_beta.as<double>(); a.bold = d_bold.as<double>(); a.xv = d_xv.as<double>(); a.state = d_state.as<double>();
    a.scal = d_scal.as<double>(); a.vr = d_vr.as<double>(); a.eta = d_eta.as<double>(); a.res = d_res.as<double>();

    // the gradient of the penalised coordinates of problem f from the carrier sums G of its v r: g_j = sinv_j (G_j - m_j sum(v r))
    std::vector<double> G, svr(F1, 0.0);
    auto grad_abs = [&](int f, int64_t j) { return fabs(sinv[f * P + j] * (G[f * P + j] - mv[f * P + j] * svr[f])); };
    rc = enet_carrier_sums(c, d_vr.as<double>(), F1, d_G.as<double>(), &G); if (rc) return rc;
    // ---- lambda sequence from the full problem at its null model (glmnet: lambda_max = max |x~_j . w (y - mu0)| / max(alpha, 1e-3))
    double gmax = 0.0;
    for (int64_t j = 0; j < P; ++j) gmax = std::max(gmax, grad_abs(0, j));
    for (int k = 0; k < n_cov; ++k) { double g = 0.0; for (int i = 0; i < N; ++i) g += Xc[(size_t)k * Np + i] * vr0[i]; gmax = std::max(gmax, fabs(g)); }
    if (!(gmax > 0.0)) return fail(SH_EINVAL, "sh_enet_fit: no column varies with the response");
    const double lmax = gmax / std::max(alpha, 1e-3);
    const double ratio = opts->lambda_min_ratio > 0.0 ? opts->lambda_min_ratio : (N < PT ? 1e-2 : 1e-4);
    std::vector<double> lam(nlam);
    for (int l = 0; l < nlam; ++l) lam[l] = opts->lambda_seq ? opts->lambda_seq[l] : nlam > 1 ? exp(log(lmax) + (log(lmax * ratio) - log(lmax)) * l / (nlam - 1)) : lmax;
    for (int l = 0; l < nlam; ++l) if (!(lam[l] > 0.0) || (l && !(lam[l] < lam[l - 1]))) return fail(SH_EINVAL, "sh_enet_fit: lambda_seq must be positive and decreasing");

    // ---- the path
    std::vector<std::vector<int>> act(F1); std::vector<std::vector<uint8_t>> in_act(F1, std::vector<uint8_t>(P, 0));
    for (int f = 0; f < F1; ++f) for (int k = 0; k < n_cov; ++k) if (csinv[f * n_cov + k] > 0.0) act[f].push_back(k);       // dense columns are always swept
    e->path.assign(F1, std::vector<EnetPoint>()); e->eta.clear(); e->F1 = F1; e->n_cov = n_cov; e->N = N;
    e->m.assign(F1, {}); e->sinv.assign(F1, {}); e->cmean.assign(F1, {}); e->csinv.assign(F1, {});
    for (int f = 0; f < F1; ++f) { e->m[f].assign(mv.begin() + f * P, mv.begin() + (f + 1) * P); e->sinv[f].assign(sinv.begin() + f * P, sinv.begin() + (f + 1) * P);
                                   e->cmean[f].assign(cmean.begin() + f * n_cov, cmean.begin() + (f + 1) * n_cov); e->csinv[f].assign(csinv.begin() + f * n_cov, csinv.begin() + (f + 1) * n_cov); }
    std::vector<double> res(F1 * 8), beta_h((size_t)F1 * PT), cvraw((size_t)F1 * nlam, 0.0), devratio(nlam, 0.0), eta_h(Np);
    std::vector<int> skip(F1), nact(F1), nz(nlam, 0);
    int64_t total_sweeps = 0, total_steps = 0; int kkt_rounds = 0, fitted = 0; bool first = true, failed = false;
    const int64_t maxit = 100000;                                    // glmnet's maxit: sweeps one problem may spend at one lambda
    for (int l = 0; l < nlam && !failed; ++l) {
        std::vector<int64_t> spent(F1, 0);
        const double lambda = lam[l], strong = alpha * (2.0 * lambda - lam[l ? l - 1 : 0]);
        for (int f = 0; f < F1; ++f) {
            bool grown = false;
            for (int64_t j = 0; j < P; ++j) if (!in_act[f][j] && sinv[f * P + j] > 0.0 && grad_abs(f, j) > strong) { in_act[f][j] = 1; act[f].push_back((int)(n_cov + j)); grown = true; }
            if (grown) std::sort(act[f].begin(), act[f].end());
            skip[f] = 0;
        }
        for (int round = 0; !failed; ++round) {
            for (int f = 0; f < F1; ++f) {                           // (only the problems that will run, only their nact entries)
                nact[f] = (int)act[f].size();
                if (!skip[f] && nact[f]) HIPCHK(hipMemcpy(d_act.as<int>() + (size_t)f * PT, act[f].data(), nact[f] * sizeof(int), hipMemcpyHostToDevice));
            }
            HIPCHK(hipMemcpy(d_nact.p, nact.data(), F1 * sizeof(int), hipMemcpyHostToDevice));
            for (int budget = 0;; ++budget) {                        // a launch ends at convergence or when its sweep budget is spent
                HIPCHK(hipMemcpy(d_skip.p, skip.data(), F1 * sizeof(int), hipMemcpyHostToDevice));
                a.lambda = lambda; a.init = first ? 1 : 0;
                HIPCHK(shk_enet_cd(c->stream, &a, F1));
                HIPCHK(hipStreamSynchronize(c->stream));
                first = false;
                std::vector<double> r2(F1 * 8);
                HIPCHK(hipMemcpy(r2.data(), d_res.p, r2.size() * sizeof(double), hipMemcpyDeviceToHost));
                bool again = false;
                for (int f = 0; f < F1; ++f) if (!skip[f]) { std::copy(r2.begin() + f * 8, r2.begin() + f * 8 + 8, res.begin() + f * 8); total_sweeps += (int64_t)res[f * 8 + 2];
                                                               spent[f] += (int64_t)res[f * 8 + 2]; total_steps += (int64_t)res[f * 8 + 7];
                                                               if (res[f * 8 + 3] == 2.0 || (res[f * 8 + 3] == 0.0 && spent[f] >= maxit)) failed = true;
                                                               else if (res[f * 8 + 3] == 0.0) again = true; else skip[f] = 1; }
                if (!again || failed) break;
            }
            if (failed) break;
            // KKT over ALL rows at the converged active-set solution: a row outside the list whose gradient exceeds alpha lambda enters it
            rc = enet_carrier_sums(c, d_vr.as<double>(), F1, d_G.as<double>(), &G); if (rc) return rc;
            ++kkt_rounds;
            bool any = false;
            for (int f = 0; f < F1; ++f) {
                svr[f] = res[f * 8 + 6];
                bool grown = false;
                for (int64_t j = 0; j < P; ++j) if (!in_act[f][j] && sinv[f * P + j] > 0.0 && grad_abs(f, j) > alpha * lambda) { in_act[f][j] = 1; act[f].push_back((int)(n_cov + j)); grown = true; }
                if (grown) std::sort(act[f].begin(), act[f].end());
                skip[f] = grown ? 0 : 1; any |= grown;
            }
            if (!any) break;
            if (round > 1000) return fail(SH_EINVAL, "sh_enet_fit: the KKT loop did not end");
        }
        // one problem did not converge at this lambda (glmnet: "convergence for k-th lambda value not reached ... solutions for larger lambdas
        // returned"; cv.glmnet keeps the lambdas every fold reached): the path ends at the previous value for all of them
        if (failed) { if (l == 0) return fail(SH_EINVAL, "sh_enet_fit: no convergence at the first lambda"); break; }
        // ---- this lambda's solutions
        HIPCHK(hipMemcpy(beta_h.data(), d_beta.p, beta_h.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<double> scal(F1 * 4); HIPCHK(hipMemcpy(scal.data(), d_scal.p, scal.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int f = 0; f < F1; ++f) {
            EnetPoint pt; pt.b0 = scal[f * 4 + 1];
            for (int j : act[f]) if (beta_h[(size_t)f * PT + j] != 0.0) { pt.idx.push_back(j); pt.val.push_back(beta_h[(size_t)f * PT + j]); }
            if (f == 0) { int n = 0; for (int j : pt.idx) n += j >= n_cov; nz[l] = n; }
            e->path[f].push_back(std::move(pt));
            cvraw[(size_t)f * nlam + l] = res[f * 8 + 1];
        }
        HIPCHK(hipMemcpy(eta_h.data(), d_eta.p, Np * sizeof(double), hipMemcpyDeviceToHost));
        e->eta.insert(e->eta.end(), eta_h.begin(), eta_h.begin() + N);
        devratio[l] = 1.0 - res[0] / nulldev[0];
        fitted = l + 1;
        // glmnet's early end of the path (full fit): deviance ratio above 0.999, or a relative gain below 1e-5 once min(5, n_lambda) values are in
        if (l > 0 && (devratio[l] > 0.999 || (l + 1 >= std::min(5, nlam) && devratio[l] - devratio[l - 1] < 1e-5 * devratio[l]))) break;
    }
    e->n_lam = fitted;
    // ---- cross-validation figures (cv.glmnet, grouped): per-fold weighted mean of the held-out deviance, their weighted mean and standard error
    out->n_lambda = fitted; out->i_min = -1; out->kkt_rounds = kkt_rounds; out->state_in_lds = use_lds ? 1 : 0; out->cd_sweeps = total_sweeps; out->cd_steps = total_steps;
    for (int l = 0; l < fitted; ++l) {
        if (out->lambda) out->lambda[l] = lam[l];
        if (out->dev_ratio) out->dev_ratio[l] = devratio[l];
        if (out->nzero) out->nzero[l] = nz[l];
        double cvm = NAN, cvsd = NAN;
        if (n_folds) {
            double sw = 0.0, sm = 0.0, sv = 0.0; int nf = 0;
            for (int f = 1; f < F1; ++f) if (hwsum[f] > 0.0) { sw += hwsum[f]; sm += cvraw[(size_t)f * nlam + l]; ++nf; }
            cvm = sm / sw;
            for (int f = 1; f < F1; ++f) if (hwsum[f] > 0.0) { const double d = cvraw[(size_t)f * nlam + l] / hwsum[f] - cvm; sv += hwsum[f] * d * d; }
            cvsd = nf > 1 ? sqrt(sv / sw / (nf - 1)) : NAN;
            if (out->fold_dev) for (int f = 1; f < F1; ++f) out->fold_dev[(size_t)(f - 1) * nlam + l] = hwsum[f] > 0.0 ? cvraw[(size_t)f * nlam + l] / hwsum[f] : NAN;
        }
        if (out->cvm) out->cvm[l] = cvm;
        if (out->cvsd) out->cvsd[l] = cvsd;
        if (n_folds && (out->i_min < 0 || cvm < out->cvm_min)) { out->i_min = l; out->cvm_min = cvm; }
    }
    if (out->fold_weight) for (int f = 1; f < F1; ++f) out->fold_weight[f - 1] = hwsum[f];
    const int at = out->i_min >= 0 ? out->i_min : fitted - 1;
    if (out->beta) return sh_enet_betas_at(c, 0, at, &out->beta0, out->beta);
    return SH_OK;
}

int sh_enet_betas_at(sh_ctx *c, int problem, int i_lambda, double *beta0, double *beta)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_betas_at before sh_enet_fit");
    EnetState *e = c->enet;
    if (problem < 0 || problem >= e->F1 || i_lambda < 0 || i_lambda >= e->n_lam) return fail(SH_ESHAPE, "sh_enet_betas_at: no such problem / lambda");
    const EnetPoint &pt = e->path[problem][i_lambda];
    const int64_t PT = e->P + e->n_cov;
    std::fill(beta, beta + PT, 0.0);
    double b0 = pt.b0;                                                // original scale: b_j / s_j, the centring goes to the intercept
    for (size_t k = 0; k < pt.idx.size(); ++k) {
        const int j = pt.idx[k];
        const double si = j < e->n_cov ? e->csinv[problem][j] : e->sinv[problem][j - e->n_cov];
        const double mj = j < e->n_cov ? e->cmean[problem][j] : e->m[problem][j - e->n_cov];
        beta[j] = pt.val[k] * si; b0 -= beta[j] * mj;
    }
    if (beta0) *beta0 = b0;
    return SH_OK;
}

int sh_enet_eta_at(sh_ctx *c, int i_lambda, double *eta)
{
    if (!c || !c->enet) return fail(SH_EINVAL, "sh_enet_eta_at before sh_enet_fit");
    EnetState *e = c->enet;
    if (i_lambda < 0 || i_lambda >= e->n_lam) return fail(SH_ESHAPE, "sh_enet_eta_at: no such lambda");
    std::copy(e->eta.begin() + (size_t)i_lambda * e->N, e->eta.begin() + (size_t)(i_lambda + 1) * e->N, eta);
    return SH_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// sh_predict_*: a saved model applied to new samples (pyseer/enet_predict.py:159-185).  One fp64 accumulator of n_samples stays on the device
// between sh_predict_begin and sh_predict_end; sh_predict_add adds the selected rows of a host block to it, in the order given.
extern "C++" {
struct PredictState {
    double *d_acc = nullptr;
    uint8_t *h_stage = nullptr, *d_stage = nullptr; size_t stage_bytes = 0;     // pinned host staging and its device twin
};
}
#define PREDICT_STAGE_BYTES ((size_t)32 << 20)                       // rows of one upload: what fits 32 MB (one row at least)

static void predict_free(sh_ctx *c)
{
    if (!c->predict) return;
    hipFree(c->predict->d_acc); hipFree(c->predict->d_stage);
    if (c->predict->h_stage) hipHostFree(c->predict->h_stage);
    delete c->predict; c->predict = nullptr;
}

int sh_predict_begin(sh_ctx *c, const double *start)
{
    if (!c || !start) return fail(SH_EINVAL, "sh_predict_begin: null argument");
    HIPCHK(hipSetDevice(c->device));
    predict_free(c);
    c->predict = new PredictState();
    if (hipMalloc((void **)&c->predict->d_acc, (size_t)c->N * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); predict_free(c); return fail(SH_ENOMEM, "sh_predict_begin: no room for the accumulator"); }
    const hipError_t rc = hipMemcpy(c->predict->d_acc, start, (size_t)c->N * sizeof(double), hipMemcpyHostToDevice);
    if (rc != hipSuccess) { predict_free(c); return fail(SH_EHIP, std::string("sh_predict_begin: ") + hipGetErrorString(rc)); }
    return SH_OK;
}

int sh_predict_add(sh_ctx *c, const uint8_t *present, const uint8_t *missing, int64_t row_bytes, const int64_t *row_idx, const double *beta, const uint8_t *flip,
                   int64_t n_sel)
{
    if (!c || !c->predict) return fail(SH_EINVAL, "sh_predict_add before sh_predict_begin");
    if (n_sel < 0 || row_bytes <= 0 || row_bytes % 8 || row_bytes * 8 < c->N) return fail(SH_ESHAPE, "sh_predict_add: row_bytes must be a multiple of 8 covering n_samples");
    if (n_sel == 0) return SH_OK;
    if (!present || !row_idx || !beta || !flip) return fail(SH_EINVAL, "sh_predict_add: null argument");
    for (int64_t k = 0; k < n_sel; ++k) if (row_idx[k] < 0) return fail(SH_ESHAPE, "sh_predict_add: negative row index");
    PredictState *p = c->predict;
    HIPCHK(hipSetDevice(c->device));
    // one staged row: its present words, its missing words (if any), its slope and its flip, each kind contiguous over the chunk
    const size_t per_row = (size_t)row_bytes * (missing ? 2 : 1) + sizeof(double) + 1;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_sel, (int64_t)(PREDICT_STAGE_BYTES / per_row)));
    const size_t need = (size_t)chunk * per_row + 16;
    if (need > p->stage_bytes) {
        hipFree(p->d_stage); p->d_stage = nullptr; if (p->h_stage) hipHostFree(p->h_stage); p->h_stage = nullptr; p->stage_bytes = 0;
        if (hipHostMalloc((void **)&p->h_stage, need, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&p->d_stage, need) != hipSuccess) {
            (void)hipGetLastError();
            if (p->h_stage) hipHostFree(p->h_stage); p->h_stage = nullptr; hipFree(p->d_stage); p->d_stage = nullptr;
            return fail(SH_ENOMEM, "sh_predict_add: no room for the staging buffers");
        }
        p->stage_bytes = need;
    }
    const int NW = (int)(row_bytes / 8);
    for (int64_t s = 0; s < n_sel; s += chunk) {
        const int64_t n = std::min(chunk, n_sel - s);
        const size_t o_miss = (size_t)n * row_bytes, o_beta = o_miss + (missing ? (size_t)n * row_bytes : 0), o_flip = o_beta + (size_t)n * sizeof(double);
        for (int64_t k = 0; k < n; ++k) {
            memcpy(p->h_stage + (size_t)k * row_bytes, present + (size_t)row_idx[s + k] * row_bytes, (size_t)row_bytes);
            if (missing) memcpy(p->h_stage + o_miss + (size_t)k * row_bytes, missing + (size_t)row_idx[s + k] * row_bytes, (size_t)row_bytes);
        }
        memcpy(p->h_stage + o_beta, beta + s, (size_t)n * sizeof(double));
        memcpy(p->h_stage + o_flip, flip + s, (size_t)n);
        HIPCHK(hipMemcpyAsync(p->d_stage, p->h_stage, o_flip + (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(shk_enet_predict(c->stream, reinterpret_cast<const uint64_t *>(p->d_stage), missing ? reinterpret_cast<const uint64_t *>(p->d_stage + o_miss) : nullptr,
                                reinterpret_cast<const double *>(p->d_stage + o_beta), p->d_stage + o_flip, n, NW, c->N, p->d_acc));
        HIPCHK(hipStreamSynchronize(c->stream));                      // (the staging buffer is free again; the sums of this chunk precede the next one's)
    }
    return SH_OK;
}

int sh_predict_end(sh_ctx *c, double *link)
{
    if (!c || !c->predict) return fail(SH_EINVAL, "sh_predict_end before sh_predict_begin");
    hipSetDevice(c->device);
    hipError_t rc = hipStreamSynchronize(c->stream);
    if (rc == hipSuccess && link) rc = hipMemcpy(link, c->predict->d_acc, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost);
    predict_free(c);
    if (rc != hipSuccess) return fail(SH_EHIP, std::string("sh_predict_end: ") + hipGetErrorString(rc));
    return SH_OK;
}
