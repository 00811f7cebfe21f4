// glm_api_impl.inc -- fixed-effects entry points (included inside extern "C" of api.hip)

int sh_glm_setup(sh_ctx *c, const double *y, const double *W, int q, int continuous, double null_llf, double null_firth,
                 double pret, double lrtt, int force_firth)
{
    if (!c || !y || (q > 0 && !W)) return fail(SH_EINVAL, "null argument");
    if (q < 0 || q > 32) return fail(SH_EINVAL, "q (MDS components + covariates) must be 0..32 in this build");
    if (const char *ce = sh_route("bitdot")) if (std::atoi(ce) == 2) return fail(SH_EINVAL, "SEERHIP_ROUTE: bitdot=2 is not a route of this build (keys: csrc/route.h)");
    const bool wide = q > 14;                             // glm_wide.hip: run-time width on scratch arrays
    HIPCHK(hipSetDevice(c->device));
    { const int rc0 = drain_pending(c); if (rc0) return rc0; }        // a batch still in flight belongs to the model being replaced
    if (c->lanes) { const int rl = lanes_wait(c); lanes_destroy(c); if (rl) return rl; }     // (so do the lanes: they are set up again from the new model at their next use)
    forget_announced(c);
    GlmState &g = c->glm;
    glm_free(&g);
    const int N = c->N;
    std::vector<uint64_t> y1(c->NB64p, 0), y0(c->NB64p, 0);
    int n1 = 0, n0 = 0; double ymean = 0;
    for (int i = 0; i < N; ++i) { if (y[i] == 1.0) { y1[i >> 6] |= 1ull << (i & 63); ++n1; } else if (y[i] == 0.0) { y0[i >> 6] |= 1ull << (i & 63); ++n0; } ymean += y[i]; }
    ymean /= N;
    std::vector<double> yc(N); double ycs = 0, ycq = 0;
    for (int i = 0; i < N; ++i) { yc[i] = y[i] - ymean; ycs += yc[i]; ycq += yc[i] * yc[i]; }
    // shared blocks of X^T X and X^T y for the OLS kernel: Z = [1, W]
    const int pz = q + 1;
    std::vector<double> ZtZ((size_t)pz * (pz + 1) / 2, 0.0), Zty(pz, 0.0);
    for (int i = 0; i < N; ++i) {
        double z[40]; z[0] = 1.0; for (int j = 0; j < q; ++j) z[1 + j] = W[(size_t)i * q + j];
        for (int a = 0; a < pz; ++a) { Zty[a] += z[a] * y[i]; for (int b = 0; b <= a; ++b) ZtZ[(size_t)a * (a + 1) / 2 + b] += z[a] * z[b]; }
    }
    HIPCHK(dmalloc(&g.d_y, N)); HIPCHK(dmalloc(&g.d_yc, N)); HIPCHK(dmalloc(&g.d_W, (size_t)N * (q > 0 ? q : 1)));
    HIPCHK(dmalloc(&g.d_Wf, (size_t)N * (q > 0 ? q : 1)));
    // the fast Newton phase iterates on per-column standardised covariates (k_glm_fast); everything else sees W as given
    std::vector<double> Ws((size_t)N * (q > 0 ? q : 1), 0.0), wstd((size_t)2 * (q > 0 ? q : 1), 0.0);
    for (int j = 0; j < q; ++j) {
        double mu = 0, ss = 0;
        for (int i = 0; i < N; ++i) mu += W[(size_t)i * q + j];
        mu /= N;
        for (int i = 0; i < N; ++i) { const double d = W[(size_t)i * q + j] - mu; ss += d * d; }
        double sd = std::sqrt(ss / N);
        if (!(sd > 0.0) || !std::isfinite(sd)) { mu = 0.0; sd = 1.0; }        // a constant column: leave it (the fit is singular anyway)
        wstd[j] = mu; wstd[q + j] = sd;
        for (int i = 0; i < N; ++i) Ws[(size_t)i * q + j] = (W[(size_t)i * q + j] - mu) / sd;
    }
    std::vector<float> Wf((size_t)N * (q > 0 ? q : 1), 0.0f);
    for (size_t i = 0; i < (size_t)N * q; ++i) Wf[i] = (float)Ws[i];
    // table for fast_pass_mfma (glm_kernels.hip FastCols<Q>): per sample the products z_j z_k (k <= j), padded to 32-column blocks
    const int zz_np = q * (q + 1) / 2, zz_ncb = std::max(1, (zz_np + 31) / 32), zz_stride = zz_ncb * 32;
    std::vector<float> zz(wide ? 32 : (size_t)N * zz_stride, 0.0f);
    for (int i = 0; i < N && !wide; ++i) {
        float *r = zz.data() + (size_t)i * zz_stride;
        for (int j = 0; j < q; ++j)
            for (int k = 0; k <= j; ++k) r[j * (j + 1) / 2 + k] = (float)(Ws[(size_t)i * q + j] * Ws[(size_t)i * q + k]);
    }
    // the same products as halves in the B layout of v_mfma_f32_32x32x16_f16 (pass32_pk): per 16-sample group and 32-column block, hi and lo
    // parts, one uint4 per lane: lane (n = lane & 31, kg = lane >> 5) holds column n of samples 16 g + 8 kg .. + 7; zero behind sample N
    {
        const int ng = (N + 15) / 16;
        std::vector<uint16_t> z16(wide ? 8 : (size_t)ng * zz_ncb * 2 * 64 * 8, 0);
        for (int gq = 0; gq < ng && !wide; ++gq)
            for (int cb = 0; cb < zz_ncb; ++cb)
                for (int ln = 0; ln < 64; ++ln)
                    for (int t = 0; t < 8; ++t) {
                        const int i = gq * 16 + 8 * (ln >> 5) + t, col = cb * 32 + (ln & 31);
                        // (columns behind the products: z_j itself, as many as fit -- the intercept row of the Hessian from the same MFMAs, pass32_pk_f16)
                        if (i >= N || col >= zz_np + q) continue;
                        const float x = col < zz_np ? zz[(size_t)i * zz_stride + col] : (float)Ws[(size_t)i * q + (col - zz_np)];
                        const _Float16 hi = (_Float16)x, lo = (_Float16)(x - (float)hi);
                        uint16_t hb, lb; std::memcpy(&hb, &hi, 2); std::memcpy(&lb, &lo, 2);
                        z16[((((size_t)gq * zz_ncb + cb) * 2 + 0) * 64 + ln) * 8 + t] = hb;
                        z16[((((size_t)gq * zz_ncb + cb) * 2 + 1) * 64 + ln) * 8 + t] = lb;
                    }
        // the linear block of the steering pass: (1, z) in columns 0..q of one 32-column block (glm_params.h zl16)
        std::vector<uint16_t> zl(wide || q > 31 ? 8 : (size_t)ng * 64 * 8, 0);
        for (int gq = 0; gq < ng && !wide && q <= 31; ++gq)
            for (int ln = 0; ln < 64; ++ln)
                for (int t = 0; t < 8; ++t) {
                    const int i = gq * 16 + 8 * (ln >> 5) + t, col = ln & 31;
                    if (i >= N || col > q) continue;
                    const _Float16 hv = (_Float16)(col == 0 ? 1.0f : (float)Ws[(size_t)i * q + (col - 1)]);
                    uint16_t hb; std::memcpy(&hb, &hv, 2);
                    zl[((size_t)gq * 64 + ln) * 8 + t] = hb;
                }
        HIPCHK(dmalloc(&g.d_zl16, zl.size()));
        HIPCHK(hipMemcpyAsync(g.d_zl16, zl.data(), sizeof(uint16_t) * zl.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(dmalloc(&g.d_zz16, z16.size()));
        HIPCHK(hipMemcpyAsync(g.d_zz16, z16.data(), sizeof(uint16_t) * z16.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    HIPCHK(dmalloc(&g.d_zz, zz.size())); HIPCHK(dmalloc(&g.d_Ws, Ws.size())); HIPCHK(dmalloc(&g.d_wstd, wstd.size()));
    HIPCHK(dmalloc(&g.d_y1, c->NB64p)); HIPCHK(dmalloc(&g.d_y0, c->NB64p));
    HIPCHK(dmalloc(&g.d_ZtZ, ZtZ.size())); HIPCHK(dmalloc(&g.d_Zty, Zty.size())); HIPCHK(dmalloc(&g.d_fcount, 4));
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(g.d_y, y, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_yc, yc.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    if (q > 0) HIPCHK(hipMemcpyAsync(g.d_W, W, sizeof(double) * (size_t)N * q, hipMemcpyHostToDevice, st));
    if (q > 0) HIPCHK(hipMemcpyAsync(g.d_Wf, Wf.data(), sizeof(float) * (size_t)N * q, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_zz, zz.data(), sizeof(float) * zz.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_Ws, Ws.data(), sizeof(double) * Ws.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_wstd, wstd.data(), sizeof(double) * wstd.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_y1, y1.data(), sizeof(uint64_t) * c->NB64p, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_y0, y0.data(), sizeof(uint64_t) * c->NB64p, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_ZtZ, ZtZ.data(), sizeof(double) * ZtZ.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g.d_Zty, Zty.data(), sizeof(double) * Zty.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    g.q = q;
    GlmParams &P = g.P;
    P.N = N; P.NB64 = c->NB64; P.continuous = continuous; P.force_firth = force_firth; P.n1 = n1; P.n0 = n0;
    P.ymean_logit = std::log(ymean / (1.0 - ymean));          // model.py:323-324
    P.newton_mode = 0;
    if (const char *nm = sh_route("newton")) P.newton_mode = std::atoi(nm);
    // Step halving (model.py:467-474).  Default: the two noise rules of round 2 (an increase of F within 4 ulp is not an increase; a step whose
    // largest component is below 1e-10 is accepted).  SEERHIP_ROUTE firth_literal=1: the reference's literal `F(new) > F(old)`; its 1000-step walk at
    // the fixed point of the halving map is cut short with the same verdict (firth_rounds.hip), so it runs at 0.75 of the default's speed
    // instead of 1/16 (round 2).  Why it is not the default: the rows the literal rule decides differently are decided by the last bit of F,
    // i.e. by the order of a 5000-term sum -- measured on 24 332 C4 rows (profiles/r03/firth_modes_vs_reference_restatement.json) the CPU restatement of the
    // reference reports 26 spurious firth-fails, the literal GPU modes 2 and 29, with NO row in common, so the literal modes differ from the
    // reference on 28 / 55 rows and the default on 26.  SEERHIP_ROUTE firth_strict=1: literal rule + the reference's start vector + one log per
    // sample in the rounds (the A/B closest to the reference's own evaluation order).
    P.firth_noise = FIRTH_F_NOISE; P.firth_accept = FIRTH_ACCEPT_BELOW;
    if (const char *fs = sh_route("firth_literal")) if (std::atoi(fs) != 0) { P.firth_noise = 0.0; P.firth_accept = 0.0; }
    P.firth_last_taylor = 1;
    if (const char *fs = sh_route("firth_last")) P.firth_last_taylor = std::atoi(fs) != 0;
    const bool firth_strict = sh_route("firth_strict") && std::atoi(sh_route("firth_strict")) != 0;
    if (firth_strict) { P.firth_noise = 0.0; P.firth_accept = 0.0; }
    // Firth-routed variants of an ordinary run at large N are few (a 2x2 cell <= 5 needs a rare k-mer), so they skip the rounds: one
    // workgroup each from the first step (41 vs 55 ms for a 262 144-variant batch with 0.13 % routed at N = 5000).  Small N routes
    // whole percents of a batch, and Firth-on-everything is a throughput job: those keep the rounds and hand off after 16 steps.
    P.firth_handoff = (!force_firth && N >= 768) ? 0 : 16;      // (round 2: 2048 -> 768; at N = 1000 with 0.9 % routed a 2^20-variant batch takes 12.4 instead of 15.6 ms)
    P.firth_halv_handoff = 6;
    // null-model MLE on [1, Ws] by Newton in fp64 on the host (N x (q+1): microseconds): the warm start of k_glm_fast
    P.warm_on = 0;
    for (int a = 0; a < 16; ++a) P.warm[a] = 0.0;
    if (!continuous && !wide && !(sh_route("warm") && std::atoi(sh_route("warm")) == 0) && ymean > 0.0 && ymean < 1.0) {
        const int pz1 = q + 1;
        std::vector<double> b(pz1, 0.0), H((size_t)pz1 * pz1), gr(pz1);
        b[0] = std::log(ymean / (1.0 - ymean));
        bool ok = false;
        for (int it = 0; it < 50 && !ok; ++it) {
            std::fill(H.begin(), H.end(), 0.0); std::fill(gr.begin(), gr.end(), 0.0);
            for (int i = 0; i < N; ++i) {
                double z[16]; z[0] = 1.0; for (int j = 0; j < q; ++j) z[1 + j] = Ws[(size_t)i * q + j];
                double eta = 0; for (int a = 0; a < pz1; ++a) eta += b[a] * z[a];
                const double mu = 1.0 / (1.0 + std::exp(-eta)), w = mu * (1.0 - mu), r = y[i] - mu;
                for (int a = 0; a < pz1; ++a) { gr[a] += r * z[a]; for (int c2 = 0; c2 <= a; ++c2) H[(size_t)a * pz1 + c2] += w * z[a] * z[c2]; }
            }
            // Cholesky solve H d = gr
            bool pd = true;
            for (int a = 0; a < pz1 && pd; ++a) {
                for (int c2 = 0; c2 <= a; ++c2) {
                    double sv = H[(size_t)a * pz1 + c2];
                    for (int k2 = 0; k2 < c2; ++k2) sv -= H[(size_t)a * pz1 + k2] * H[(size_t)c2 * pz1 + k2];
                    if (a == c2) { if (!(sv > 0.0)) { pd = false; break; } H[(size_t)a * pz1 + a] = std::sqrt(sv); }
                    else H[(size_t)a * pz1 + c2] = sv / H[(size_t)c2 * pz1 + c2];
                }
            }
            if (!pd) break;
            for (int a = 0; a < pz1; ++a) { double sv = gr[a]; for (int k2 = 0; k2 < a; ++k2) sv -= H[(size_t)a * pz1 + k2] * gr[k2]; gr[a] = sv / H[(size_t)a * pz1 + a]; }
            for (int a = pz1 - 1; a >= 0; --a) { double sv = gr[a]; for (int k2 = a + 1; k2 < pz1; ++k2) sv -= H[(size_t)k2 * pz1 + a] * gr[k2]; gr[a] = sv / H[(size_t)a * pz1 + a]; }
            double mx = 0; bool fin = true;
            for (int a = 0; a < pz1; ++a) { b[a] += gr[a]; mx = std::max(mx, std::fabs(gr[a])); fin = fin && std::isfinite(b[a]); }
            if (!fin) break;
            if (mx < 1e-10) ok = true;
        }
        if (ok) { P.warm_on = 1; for (int a = 0; a < pz1; ++a) P.warm[a] = b[a]; }
        // the null model's weights and its z x z information block, for the final pass (k_glm_final<Q, true>)
        if (ok && q > 0) {
            std::vector<double> w0(N), a0((size_t)q * (q + 1) / 2, 0.0);
            for (int i = 0; i < N; ++i) {
                double eta = b[0]; for (int j = 0; j < q; ++j) eta += b[1 + j] * Ws[(size_t)i * q + j];
                const double mu = 1.0 / (1.0 + std::exp(-eta)); w0[i] = mu * (1.0 - mu);
                for (int j = 0; j < q; ++j) for (int k2 = 0; k2 <= j; ++k2) a0[(size_t)j * (j + 1) / 2 + k2] += w0[i] * Ws[(size_t)i * q + j] * Ws[(size_t)i * q + k2];
            }
            // the kernel adds float(w - w0) x float(z_j z_k) to a0: use the same rounded products here, so that the two parts belong together
            std::fill(a0.begin(), a0.end(), 0.0);
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < q; ++j) for (int k2 = 0; k2 <= j; ++k2)
                    a0[(size_t)j * (j + 1) / 2 + k2] += w0[i] * (double)(float)(Ws[(size_t)i * q + j] * Ws[(size_t)i * q + k2]);
            HIPCHK(dmalloc(&g.d_w0, N)); HIPCHK(dmalloc(&g.d_a0, a0.size()));
            HIPCHK(hipMemcpy(g.d_w0, w0.data(), sizeof(double) * N, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(g.d_a0, a0.data(), sizeof(double) * a0.size(), hipMemcpyHostToDevice));
            // per-sample (w0, w0 z, r0) for the carrier sums (bitdot_i8.hip), the rest of the null model's information matrix and its score
            const int NE = q + 2;
            std::vector<double> vals((size_t)N * NE);
            for (int a = 0; a < 16; ++a) { P.null_h[a] = 0.0; P.null_g[a] = 0.0; }
            for (int i = 0; i < N; ++i) {
                double eta = b[0]; for (int j = 0; j < q; ++j) eta += b[1 + j] * Ws[(size_t)i * q + j];
                const double mu = 1.0 / (1.0 + std::exp(-eta)), r0 = y[i] - mu;
                vals[(size_t)i * NE] = w0[i]; vals[(size_t)i * NE + q + 1] = r0;
                P.null_h[0] += w0[i]; P.null_g[0] += r0;
                for (int j = 0; j < q; ++j) {
                    const double z = Ws[(size_t)i * q + j];
                    vals[(size_t)i * NE + 1 + j] = w0[i] * z; P.null_h[1 + j] += w0[i] * z; P.null_g[1 + j] += r0 * z;
                }
            }
            {                                                     // records of the packed-fp32 passes and of the fp64 score / ll kernels
                const size_t np = (size_t)(N / 2), nq = (size_t)q, rs = nq + 2;
                std::vector<float> pk(np * rs * 2 + 2 * (size_t)N + 4, 0.0f);
                for (size_t p2 = 0; p2 < np; ++p2) {
                    float *r = pk.data() + p2 * rs * 2;
                    for (int j = 0; j < q; ++j) { r[2 * j] = (float)Ws[(2 * p2) * nq + j]; r[2 * j + 1] = (float)Ws[(2 * p2 + 1) * nq + j]; }
                    r[2 * nq] = (float)y[2 * p2]; r[2 * nq + 1] = (float)y[2 * p2 + 1];
                    r[2 * nq + 2] = (float)w0[2 * p2]; r[2 * nq + 3] = (float)w0[2 * p2 + 1];
                }
                float *yf = pk.data() + np * rs * 2, *w0f = yf + N + (N & 1);
                for (int i = 0; i < N; ++i) { yf[i] = (float)y[i]; w0f[i] = (float)w0[i]; }
                HIPCHK(dmalloc(&g.d_pk, pk.size()));
                HIPCHK(hipMemcpy(g.d_pk, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice));
                std::vector<double> rec((size_t)N * (nq + 1));
                for (int i = 0; i < N; ++i) { for (int j = 0; j < q; ++j) rec[(size_t)i * (nq + 1) + j] = Ws[(size_t)i * nq + j]; rec[(size_t)i * (nq + 1) + nq] = y[i]; }
                HIPCHK(dmalloc(&g.d_rec, rec.size()));
                HIPCHK(hipMemcpy(g.d_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice));
            }
            {   // constants of the bordered first step (GlmParams.b1): order (intercept, covariates | variant); the same scaling and ridge as
                // k_glm_solve32<Q, true> (A / n, diagonal - 1e-10), the same relative pivot test (1e-4) on the constant block
                const int m = q + 1;
                const double nobs = (double)N;
                auto sidx = [](int i, int j) { return i * (i + 1) / 2 + j; };   // packed lower, i >= j (glm_common.h)
                std::vector<double> Ac((size_t)m * (m + 1) / 2), gc(m);
                Ac[sidx(0, 0)] = P.null_h[0] / nobs - 1e-10; gc[0] = P.null_g[0] / nobs;
                for (int j = 0; j < q; ++j) {
                    Ac[sidx(1 + j, 0)] = P.null_h[1 + j] / nobs; gc[1 + j] = P.null_g[1 + j] / nobs;
                    for (int k2 = 0; k2 <= j; ++k2) Ac[sidx(1 + j, 1 + k2)] = a0[(size_t)j * (j + 1) / 2 + k2] / nobs - (k2 == j ? 1e-10 : 0.0);
                }
                bool okf = true;
                std::vector<double> D(m);
                for (int j = 0; j < m && okf; ++j) {                   // L D L^T in place: unit-lower L below the diagonal, D kept aside
                    const double ajj = Ac[sidx(j, j)];
                    double d = ajj;
                    for (int k2 = 0; k2 < j; ++k2) d -= Ac[sidx(j, k2)] * Ac[sidx(j, k2)] * D[k2];
                    if (d == 0.0 || std::fabs(d) <= 1e-4 * std::fabs(ajj) || !std::isfinite(d)) { okf = false; break; }
                    D[j] = d;
                    for (int i = j + 1; i < m; ++i) {
                        double sv = Ac[sidx(i, j)];
                        for (int k2 = 0; k2 < j; ++k2) sv -= Ac[sidx(i, k2)] * Ac[sidx(j, k2)] * D[k2];
                        Ac[sidx(i, j)] = sv / d;
                    }
                }
                if (okf) {
                    std::vector<double> b1((size_t)m * (m + 1) / 2 + 3 * (size_t)m), yc(gc), xc(m);
                    for (int i = 0; i < m; ++i) for (int k2 = 0; k2 < i; ++k2) yc[i] -= Ac[sidx(i, k2)] * yc[k2];
                    for (int i = 0; i < m; ++i) xc[i] = yc[i] / D[i];
                    for (int i = m - 1; i >= 0; --i) for (int k2 = i + 1; k2 < m; ++k2) xc[i] -= Ac[sidx(k2, i)] * xc[k2];
                    for (int i = 0; i < m; ++i) for (int k2 = 0; k2 <= i; ++k2) b1[sidx(i, k2)] = (k2 == i) ? 1.0 : Ac[sidx(i, k2)];
                    double *w = b1.data() + (size_t)m * (m + 1) / 2;
                    for (int i = 0; i < m; ++i) { w[i] = 1.0 / D[i]; w[m + i] = yc[i]; w[2 * m + i] = xc[i]; }
                    HIPCHK(dmalloc(&g.d_b1, b1.size()));
                    HIPCHK(hipMemcpy(g.d_b1, b1.data(), sizeof(double) * b1.size(), hipMemcpyHostToDevice));
                }
            }
            {   // the table of the carrier sums: base-256 digits for the int8 matrix cores (bitdot_i8.hip)
                std::vector<int8_t> at((size_t)shk_bitdot_i8_table_bytes(NE, c->NB64));
                std::vector<double> sc((size_t)4 * ((NE + 3) / 4));
                shk_bitdot_i8_digits(vals.data(), N, NE, c->NB64, at.data(), sc.data());
                HIPCHK(hipMalloc((void **)&g.d_bdi8, at.size())); HIPCHK(dmalloc(&g.d_bdscale, sc.size()));
                HIPCHK(hipMemcpy(g.d_bdi8, at.data(), at.size(), hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(g.d_bdscale, sc.data(), sizeof(double) * sc.size(), hipMemcpyHostToDevice));
            }
        }
    }
    // the same fit in the original covariate coordinates: start of the Firth rounds when every variant goes through them (not in strict mode,
    // which follows the reference's trajectory from its own start vector; not with the hand-off at step 0, where the routed variants are
    // the pathological ones)
    P.firth_warm = 0;
    for (int a = 0; a < 16; ++a) P.fwarm[a] = 0.0;
    // fit_firth's iteration converges LINEARLY (the penalty's curvature is not in its Hessian), with a ratio ~p/N: where it stops (one step
    // after a step below 1e-4) depends on the path by ~ratio x 1e-4.  At N >= 4096 that is below 1e-7 and a better start is safe; below, the
    // reference's own start vector is kept (measured: 5.7e-6 on a golden case at N = 100).
    // ... and only on covariates that are roughly centred: fit_firth iterates on the columns as given, and with an un-centred one (year of
    // isolation, 2000 +- 10) its contraction is slow enough for the start to show at 2e-6 (tools/gpu_firth_sweep.py), against 1e-7 otherwise
    bool centred = true;
    for (int j = 0; j < q; ++j) centred = centred && std::fabs(wstd[j]) <= 10.0 * wstd[q + j];
    if (P.warm_on && force_firth && N >= 4096 && centred && !firth_strict && P.firth_handoff >= FIRTH_WARM_LIMIT + 2) {
        P.firth_warm = 1;
        P.fwarm[0] = P.warm[0];
        for (int j = 0; j < q; ++j) { P.fwarm[1 + j] = P.warm[1 + j] / wstd[q + j]; P.fwarm[0] -= P.fwarm[1 + j] * wstd[j]; }
    }
    P.dbg = nullptr;
    // Single-precision passes (eta, exp, score, Hessian all fp32) cost 2.5 ms against 8.6 ms for a pass with the fp64 score (N = 5000,
    // q = 10, 262 144 variants).  Iterated to their own fixed point they stop ~1e-6 from the exact one (the fp32 ACCUMULATION of the score:
    // partial sums of ~100 round at 6e-6), which the final pass cannot absorb without a second pass; so they only open the iteration
    // (f32_steps), and a lane is never declared converged by one (f32_tol = 0).
    P.f32_steps = P.warm_on ? 2 : 3;
    P.f32_tol = 0.0;                                          // measured: their floor is ~1e-6 (fp32 accumulation of the score), not enough: see DESIGN.md
    // The fast phase stops at the first fp64-score step of at most fast_tol (the error left is ~1e-5 of that step: the fp32 Hessian); the
    // final pass then takes one exact fp64 Newton step from there (k_glm_final), which lands on the fixed point the reference's own
    // stopping rule (|step| <= 1e-8, SM optimizer.py:407-446) reaches.  (fast_tol = 1e-8 would be the reference's rule in the fast phase.)
    P.fast_tol = 1e-4;
    P.zz = wide ? nullptr : g.d_zz;
    P.zz16 = wide ? nullptr : g.d_zz16;
    P.zl16 = (wide || q > 31) ? nullptr : g.d_zl16;
    P.w0 = g.d_w0; P.a0 = g.d_a0;
    P.ztz = g.d_ZtZ; P.zty = g.d_Zty;
    P.ws = (wide || q == 0) ? nullptr : g.d_Ws; P.wstd = g.d_wstd;
    // Chord rounds instead of fp64-score Newton passes (glm_params.h; SEERHIP_ROUTE chord=0 turns them off): need the products table and the
    // standardised covariates, i.e. the same conditions as the matrix-pipe passes.  A lane leaves them once its predicted distance from the
    // fixed point is <= chord_tol, half of what the final pass absorbs without repeating itself.
    P.chord_on = (P.warm_on && P.zz && P.ws && q > 0) ? 1 : 0;
    if (const char *ce = sh_route("chord")) P.chord_on = P.chord_on && std::atoi(ce) != 0;
    P.chord_n32 = 5; P.chord_rounds = 4;
    if (const char *ce = sh_route("chord_n32")) P.chord_n32 = std::min(8, std::max(1, std::atoi(ce)));
    P.chord_enter = 5e-3;
    if (const char *ce = sh_route("chord_enter")) P.chord_enter = std::atof(ce);
    P.chord_tol = 2.5e-7;
    // the first step from carrier sums and the finishing kernels need the null-model tables (built with w0 / a0 above)
    P.bd_i8 = (P.chord_on && g.d_bdi8 && g.d_bdscale && P.a0 && P.w0) ? g.d_bdi8 : nullptr; P.bd_scale = g.d_bdscale;
    if (const char *ce = sh_route("bitdot")) if (std::atoi(ce) == 0) P.bd_i8 = nullptr;
    P.b1 = (P.bd_i8 && g.d_b1 && P.chord_n32 > 1) ? g.d_b1 : nullptr;     // (a single Newton round has no next round to hand a small first step to)
    if (const char *ce = sh_route("first_bordered")) if (std::atoi(ce) == 0) P.b1 = nullptr;
    P.wfp = P.yf = P.w0f = nullptr;
    if (P.bd_i8 && g.d_pk && !(sh_route("pk") && std::atoi(sh_route("pk")) == 0)) {
        P.wfp = g.d_pk; P.yf = g.d_pk + (size_t)(N / 2) * (q + 2) * 2; P.w0f = P.yf + N + (N & 1);
    }
    P.rec = g.d_rec;
    P.rec_o = nullptr; P.rec_f = nullptr; P.rec_pf = nullptr; P.firth_lean = 3;
    {   // records of the Firth rounds: covariates as given + y, for a 0/1 phenotype on the register-resident designs
        bool yb = !continuous && !wide; for (int i = 0; i < N && yb; ++i) yb = (y[i] == 0.0 || y[i] == 1.0);
        // strict mode decides step halvings on the last bit of F: it keeps the plain evaluation (info_pass: one log per sample, as the reference sums them)
        if (yb && !firth_strict) {
            const size_t rs = (size_t)q + 1;
            std::vector<double> ro((size_t)N * rs);
            for (int i = 0; i < N; ++i) { for (int j = 0; j < q; ++j) ro[(size_t)i * rs + j] = W[(size_t)i * q + j]; ro[(size_t)i * rs + q] = y[i]; }
            HIPCHK(dmalloc(&g.d_rec_o, ro.size()));
            HIPCHK(hipMemcpy(g.d_rec_o, ro.data(), sizeof(double) * ro.size(), hipMemcpyHostToDevice));
            P.rec_o = g.d_rec_o;
            // round 3 (firth_rounds.hip): the same record with s = 1 - 2y in place of y, and per PAIR of samples the standardised covariates
            // as float2 = (even, odd) for the single-precision hat diagonal of k_firth_step2..
            if (q >= 1) {
                for (int i = 0; i < N; ++i) ro[(size_t)i * rs + q] = 1.0 - 2.0 * y[i];
                HIPCHK(dmalloc(&g.d_rec_f, ro.size()));
                HIPCHK(hipMemcpy(g.d_rec_f, ro.data(), sizeof(double) * ro.size(), hipMemcpyHostToDevice));
                const size_t np = (size_t)(N / 2);
                std::vector<float> pf(std::max<size_t>(np, 1) * q * 2, 0.0f);
                for (size_t p2 = 0; p2 < np; ++p2)
                    for (int j = 0; j < q; ++j) { pf[(p2 * q + j) * 2] = (float)Ws[(2 * p2) * q + j]; pf[(p2 * q + j) * 2 + 1] = (float)Ws[(2 * p2 + 1) * q + j]; }
                HIPCHK(dmalloc(&g.d_rec_pf, pf.size()));
                HIPCHK(hipMemcpy(g.d_rec_pf, pf.data(), sizeof(float) * pf.size(), hipMemcpyHostToDevice));
                P.rec_f = g.d_rec_f; P.rec_pf = g.d_rec_pf;
            }
        }
    }
    if (!P.rec) P.chord_on = 0;
    // Firth rounds one Newton step ahead of the null-model fit (k_firth_init2): needs the carrier sums of the logistic rounds (shk_bitdot_i8 runs
    // whenever chord_on and bd_i8 are set) and the round-3 kernels.
    if (P.firth_warm == 1 && P.chord_on && P.bd_i8 && P.a0 && P.rec_f)
        P.firth_warm = 2;
    // The one-pass iteration (firth_fast.hip) where the rounds start warm (every variant through fit_firth at N >= 4096, centred covariates,
    // default noise rules) and the third-moment tensor fits the accumulators (Q <= 10).  SEERHIP_ROUTE firth_fast=0: the two-pass rounds only.
    P.ff_tab = nullptr; P.ff_rec = nullptr; P.ff_inull = nullptr;
    if (P.firth_warm == 2 && P.firth_noise > 0.0 && shk_firth_fast_supported(q) &&
        !(sh_route("firth_fast") && std::atoi(sh_route("firth_fast")) == 0)) {
        int t2 = 0, t3 = 0, rs = 0;
        shk_firth_fast_tiles(q, &t2, &t3, &rs);
        const int z1 = q + 1, n2 = z1 * (z1 + 1) / 2, n3 = z1 * (z1 + 1) * (z1 + 2) / 6, nta = t2 + t3;
        const int NG = (N + 15) / 16;
        auto f2h = [](float f) -> uint16_t {                       // float -> IEEE half, round to nearest even (the tables' hi and lo parts)
            uint32_t x; std::memcpy(&x, &f, 4);
            const uint32_t sign = (x >> 16) & 0x8000u;
            x &= 0x7fffffffu;
            if (x >= 0x47800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));       // overflow -> inf, nan stays nan
            if (x < 0x38800000u) {                                  // subnormal half (or zero): shift the significand with its hidden bit
                if (x < 0x33000000u) return (uint16_t)sign;
                const int sh = 126 - (int)(x >> 23);
                uint32_t m = (x & 0x7fffffu) | 0x800000u;
                const uint32_t half = 1u << (sh - 1), rest = m & ((1u << sh) - 1u);
                m >>= sh;
                if (rest > half || (rest == half && (m & 1u))) ++m;
                return (uint16_t)(sign | m);
            }
            uint32_t m = x - 0x38000000u;                           // rebias 127 -> 15
            const uint32_t rest = m & 0x1fffu;
            m >>= 13;
            if (rest > 0x1000u || (rest == 0x1000u && (m & 1u))) ++m;
            return (uint16_t)(sign | m);
        };
        auto h2f = [](uint16_t hh) -> float {
            const uint32_t sign = (uint32_t)(hh & 0x8000u) << 16; uint32_t e = (hh >> 10) & 0x1fu, m = hh & 0x3ffu, x;
            if (e == 0) { if (m == 0) x = sign; else { int sh = 0; while (!(m & 0x400u)) { m <<= 1; ++sh; } x = sign | ((uint32_t)(113 - sh) << 23) | ((m & 0x3ffu) << 13); } }
            else if (e == 31) x = sign | 0x7f800000u | (m << 13);
            else x = sign | ((e + 112u) << 23) | (m << 13);
            float f; std::memcpy(&f, &x, 4); return f;
        };
        // the null model's weights in the standardised coordinates (P.warm = its fit [b0, bz...]), and its covariate block of I summed over the
        // table's own values, so that the table's rounding is in neither part of I = I(null) + sum (w - w0) m2
        std::vector<double> w0n((size_t)N), inull((size_t)n2, 0.0);
        for (int i = 0; i < N; ++i) {
            double eta = P.warm[0]; for (int j = 0; j < q; ++j) eta += P.warm[1 + j] * Ws[(size_t)i * q + j];
            const double mu = 1.0 / (1.0 + std::exp(-eta)); w0n[i] = mu * (1.0 - mu);
        }
        std::vector<uint16_t> tab((size_t)NG * nta * 2 * 64 * 8, 0);
        std::vector<double> rec((size_t)NG * 16 * rs + 640, 0.0);       // (+ 5 KB: a group's records are fetched as 1 KB pieces, the last ones padding)
        std::vector<double> zv((size_t)z1);
        for (int i = 0; i < N; ++i) {
            double *r = rec.data() + (size_t)i * rs;
            for (int j = 0; j < q; ++j) r[j] = Ws[(size_t)i * q + j];
            r[q] = 1.0 - 2.0 * y[i]; r[q + 1] = 1.0; r[q + 2] = -4096.0 * w0n[i];     // (-FF_SCALE w0: the kernels form 2^12 (w - w0) by one fma)
            zv[0] = 1.0; for (int j = 0; j < q; ++j) zv[1 + j] = Ws[(size_t)i * q + j];
            const int gq = i >> 4, hh = (i >> 3) & 1, jj = i & 7;
            auto put = [&](int ta, int m, double val) -> double {
                const float f = (float)val;
                const uint16_t hi = f2h(f), lo = f2h(f - h2f(hi));
                const size_t at = ((((size_t)gq * nta + ta) * 2) * 64 + (size_t)(hh * 32 + m)) * 8 + jj;
                tab[at] = hi; tab[at + 64 * 8] = lo;
                return (double)h2f(hi) + (double)h2f(lo);
            };
            for (int a2 = 0; a2 < z1; ++a2) for (int b2 = 0; b2 <= a2; ++b2) {
                const int row2 = shk_firth_fast_row2(q, a2, b2);               // (the monomials with the constant first: firth_fast.hip)
                inull[row2] += w0n[i] * put(row2 >> 5, row2 & 31, zv[a2] * zv[b2]);
            }
            int row = 0;
            for (int a2 = 0; a2 < z1; ++a2) for (int b2 = 0; b2 <= a2; ++b2) for (int c2 = 0; c2 <= b2; ++c2, ++row) put(t2 + (row >> 5), row & 31, zv[a2] * zv[b2] * zv[c2]);
        }
        (void)n2; (void)n3;
        HIPCHK(dmalloc(&g.d_ff_tab, tab.size())); HIPCHK(dmalloc(&g.d_ff_rec, rec.size()));
        HIPCHK(hipMemcpy(g.d_ff_tab, tab.data(), sizeof(uint16_t) * tab.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.d_ff_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice));
        {
            // firth_fast_w.hip: the same monomials as 16-row tiles of 32-sample groups (hi halves only: the single-precision pass takes one
            // product per tile), lane (m = lane & 15, kq = lane >> 4) = row m, samples 32 g + 8 kq .. + 7; records (z_s, s, -2^12 w0) as floats
            int t2h = 0, t3h = 0, rsw = 0, rows = 0;
            shk_firth_fastw_layout(q, &t2h, &t3h, &rsw, &rows);
            const int ntw = t2h + t3h, NG32 = (N + 31) / 32;
            std::vector<uint16_t> tw((size_t)NG32 * ntw * 64 * 8, 0);
            std::vector<float> rw((size_t)NG32 * 32 * rsw + 1024, 0.0f);      // (+ 4 KB: a group's records are fetched as whole 1 KB pieces)
            for (int i = 0; i < N; ++i) {
                float *r = rw.data() + (size_t)i * rsw;
                for (int j = 0; j < q; ++j) r[j] = (float)Ws[(size_t)i * q + j];
                r[q] = (float)(1.0 - 2.0 * y[i]); r[q + 1] = (float)(-4096.0 * w0n[i]);
                zv[0] = 1.0; for (int j = 0; j < q; ++j) zv[1 + j] = Ws[(size_t)i * q + j];
                const int gq = i >> 5, kq = (i >> 3) & 3, jj = i & 7;
                auto putw = [&](int ta, int m, double val) { tw[(((size_t)gq * ntw + ta) * 64 + (size_t)(kq * 16 + m)) * 8 + jj] = f2h((float)val); };
                for (int a2 = 0; a2 < z1; ++a2) for (int b2 = 0; b2 <= a2; ++b2) { const int row2 = shk_firth_fast_row2(q, a2, b2); putw(row2 >> 4, row2 & 15, zv[a2] * zv[b2]); }
                int row = 0;
                for (int a2 = 0; a2 < z1; ++a2) for (int b2 = 0; b2 <= a2; ++b2) for (int c2 = 0; c2 <= b2; ++c2, ++row) putw(t2h + (row >> 4), row & 15, zv[a2] * zv[b2] * zv[c2]);
            }
            HIPCHK(dmalloc(&g.d_ffw_tab, tw.size())); HIPCHK(dmalloc(&g.d_ffw_rec, rw.size()));
            HIPCHK(hipMemcpy(g.d_ffw_tab, tw.data(), sizeof(uint16_t) * tw.size(), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(g.d_ffw_rec, rw.data(), sizeof(float) * rw.size(), hipMemcpyHostToDevice));
            g.ffw_rows = rows;
        }
        HIPCHK(dmalloc(&g.d_ff_inull, inull.size()));
        HIPCHK(hipMemcpy(g.d_ff_inull, inull.data(), sizeof(double) * inull.size(), hipMemcpyHostToDevice));
        P.ff_tab = g.d_ff_tab; P.ff_rec = g.d_ff_rec; P.ff_inull = g.d_ff_inull;
    }
    // the finishing kernels take y in {0, 1} (k_glm_ll); anything else keeps k_glm_final, which mirrors statsmodels' general formula
    bool ybin = true; for (int i = 0; i < N; ++i) ybin = ybin && (y[i] == 0.0 || y[i] == 1.0);
    P.fin_rounds = (P.bd_i8 != nullptr && ybin) ? 1 : 0;
    if (const char *ce = sh_route("fin_rounds")) P.fin_rounds = P.fin_rounds && std::atoi(ce) != 0;
    P.ll_first = P.fin_rounds;                                       // SEERHIP_ROUTE ll_first=0: score pass first, likelihood pass last (rounds 2 - 3a)
    if (const char *ce = sh_route("ll_first")) P.ll_first = P.ll_first && std::atoi(ce) != 0;
    P.ch_bs = P.ch_fac = P.ch_g = P.ch_md = P.ch_bd = P.ch_ll = P.ch_b0 = nullptr; P.ch_hf = P.ch_rho = nullptr; P.ch_cnt = nullptr;
    for (int i = 0; i < 5; ++i) P.ch_list[i] = nullptr;
    P.yc_sum = ycs; P.yc_sq = ycq; P.null_llf = null_llf; P.null_firth = null_firth; P.pret = pret; P.lrtt = lrtt;
    g.ymean = ymean; g.yty = 0; for (int i = 0; i < N; ++i) g.yty += y[i] * y[i];
    if (continuous && !wide) {                            // nibble tables for k_glm_ols_tab
        HIPCHK(dmalloc(&g.d_olstab, (size_t)c->NB64 * 256 * (q + 2)));
        HIPCHK(shk_glm_ols_tab(st, q, 0, nullptr, 0, 0, g.d_y, g.d_yc, g.d_W, g.d_olstab, g.d_ZtZ, g.d_Zty, P, g.ymean, g.yty, nullptr, nullptr, nullptr, nullptr));
        HIPCHK(hipStreamSynchronize(st));
    }
    g.ff_first32 = sh_route("firth_first32") ? std::max(0, std::min(3, std::atoi(sh_route("firth_first32")))) : 2;    // how many of the first passes run in single precision
    g.ready = true;
    if (!c->is_lane) {                                    // what the lanes of this context will be set up with (lanes_api.inc)
        GlmSetupArgs &a = c->glm_args;
        a.y.assign(y, y + N); a.W.assign(W ? W : y, W ? W + (size_t)N * q : y);
        { const char *rs = sh_route_string(); a.route = rs ? rs : ""; }
        a.q = q; a.continuous = continuous; a.force_firth = force_firth; a.null_llf = null_llf; a.null_firth = null_firth; a.pret = pret; a.lrtt = lrtt;
    }
    return SH_OK;
}

int sh_glm_batch_dev(sh_ctx *c, const void *d_bits, int64_t row_bytes, int64_t V, void *d_out, void *d_flags)
{
    if (!c || !c->glm.ready) return fail(SH_EINVAL, "sh_glm_setup has not run");
    if (V <= 0) return SH_OK;
    if (V > 2147483647ll) return fail(SH_EINVAL, "V too large for one call");
    if (row_bytes * 8 < c->N) return fail(SH_ESHAPE, "row_bytes*8 < n_samples");
    auto body = [&](const void *b, int64_t n, void *o, void *f) -> int {
        if (c->dedup)
            return dedup_wrap(c, b, row_bytes, n, o, f, 5 + c->glm.q,
                              [&](const void *b2, int64_t n2, void *o2, void *f2) { return glm_batch_dev_inner(c, b2, row_bytes, n2, o2, f2); });
        return glm_batch_dev_inner(c, b, row_bytes, n, o, f);
    };
    PrefilterRows pf;
    if (!c->glm.P.continuous) { pf.y1 = c->glm.d_y1; pf.y0 = c->glm.d_y0; pf.n1 = c->glm.P.n1; pf.n0 = c->glm.P.n0; pf.pret = c->glm.P.pret; }
    return af_wrap(c, d_bits, row_bytes, V, d_out, d_flags, 5 + c->glm.q, body, pf);
}

// doubles per padded variant of the round workspaces (GlmParams.ch_*): bs, g, bd [PC], fac [NH], md, ll, hf (NH floats), rho (floats), 5 int lists
static size_t glm_round_ws_doubles(int q) { const int PC = q + 2, NH = PC * (PC + 1) / 2; return (size_t)(4 * PC + NH + 2 + (NH + 1) / 2 + 1 + 3); }

// Firth as rounds of (likelihood-at-candidate, score-and-step) kernels over re-listed live variants (glm_kernels.hip).
// The list lengths come back to the host once per round: they size the next launches and end the loop.
static int firth_rounds(sh_ctx *c, int64_t Vpad, int64_t V, const GlmParams &P, double *d_out, uint32_t *d_flags)
{
    GlmState &g = c->glm;
    hipStream_t st = c->stream;
    // (list lengths come back through host-mapped memory written by a one-thread kernel, not through the copy engine: readback_sync, api.hip)
    int nf = 0;
    { const int rcb = readback_sync(c, st, g.d_fcount, nullptr, nullptr, nullptr, &nf); if (rcb) return rcb; }
    if (nf <= 0) return SH_OK;
    if (nf > g.fcap) {
        hipFree(g.d_fst); hipFree(g.d_fmeta); for (int i = 0; i < 5; ++i) { hipFree(g.d_fl[i]); g.d_fl[i] = nullptr; }
        g.d_fst = nullptr; g.d_fmeta = nullptr;
        const int64_t cap = ((int64_t)nf + 1023) / 1024 * 1024;
        HIPCHK(dmalloc(&g.d_fst, (size_t)cap * shk_firth_state_doubles(g.q))); HIPCHK(dmalloc(&g.d_fmeta, (size_t)cap * 3));
        for (int i = 0; i < 5; ++i) HIPCHK(dmalloc(&g.d_fl[i], (size_t)cap));
        if (!g.d_fcnt) HIPCHK(dmalloc(&g.d_fcnt, 8));
        g.fcap = cap;
    }
    int *it = g.d_fmeta, *hv = g.d_fmeta + g.fcap, *vr = g.d_fmeta + 2 * g.fcap;
    int *E = g.d_fl[0], *En = g.d_fl[1], *S = g.d_fl[2], *B = g.d_fl[3], *S64 = g.d_fl[4];
    int *cE = g.d_fcnt, *cEn = g.d_fcnt + 1, *cS = g.d_fcnt + 2, *cB = g.d_fcnt + 3, *cS64 = g.d_fcnt + 4;
    const bool v2 = P.rec_f && P.rec_pf && P.ws && P.wstd;             // round-3 kernels (firth_rounds.hip)
    const bool dbg = sh_debug("firth");
    HIPCHK(hipMemsetAsync(cB, 0, sizeof(int), st));
    if (v2)
        HIPCHK(shk_firth2_launch(st, g.q, 0, nf, c->d_T, Vpad, V, P, g.d_fst, it, hv, vr, g.fcap, g.d_flist, g.d_fcount, E, cE,
                                 nullptr, nullptr, d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB, S64, cS64));
    else
        HIPCHK(shk_firth_launch(st, g.q, 0, nf, c->d_T, Vpad, V, g.d_y, g.d_W, P, g.d_fst, it, hv, vr, g.fcap, g.d_flist, g.d_fcount, E, cE,
                                nullptr, nullptr, d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB));
    int nE = nf, round = 0, nS64 = 0, nB_seen = -1;
    if (v2 && P.ff_tab && P.firth_warm == 2) {
        // One-pass iterations first (firth_fast.hip): every pass re-lists the fits that go on (ping-pong E / En) and appends to X the slots the
        // exact kernels take over -- the candidate that meets the stop rule (k_firth_eval2 evaluates F and I11 there and writes the outputs), or
        // a fit that is not an ordinary one.  The exact rounds below then start from X.
        int *Fa = E, *Fb = En, *X = S, *cFa = cE, *cFb = cEn, *cX = cS;
        HIPCHK(hipMemsetAsync(cX, 0, sizeof(int), st));
        int nF = nf, passes = 0;
        // Round 6: TWO single-precision passes at two wavefronts per SIMD (2 x 2.8 ms), then ONE fp64 pass that finds a last step of ~1e-8
        // and finishes the fit (6 ms) -- instead of one + two (the second fp64 pass only took the fit from 1e-5 to 1e-8 of its fixed point).
        // What made the second single-precision pass land within 1e-7: its sums in double precision across groups, and the next candidate
        // formed from the point the pass really evaluated (firth_fast_w.hip).
        while (nF > 0) {
            HIPCHK(hipMemsetAsync(cFb, 0, sizeof(int), st));
            // (the first pass, at the start vector, in single precision: its step is 1e-5 from the fit at best)
            if (passes < g.ff_first32) {
                // (the first pass at two wavefronts per SIMD: firth_fast_w.hip; its sums cross to the per-fit kernel through the workspace)
                if (nF > g.ffw_cap) {
                    hipFree(g.d_ffw_ws); g.d_ffw_ws = nullptr; g.ffw_cap = 0;
                    // (rows are fits-long: a row stride that is a multiple of 1 MB would put the ~480 rows a fit's lane walks on one HBM channel --
                    // measured 3.4 ms for the per-fit kernel of 2^18 fits; + 4 KB + 256 B spreads consecutive rows over the channels)
                    const int64_t capw = ((int64_t)nF + 1023) / 1024 * 1024 + 1088;
                    HIPCHK(dmalloc(&g.d_ffw_ws, (size_t)capw * g.ffw_rows)); g.ffw_cap = capw;
                }
                HIPCHK(shk_firth_fastw_launch(st, g.q, nF, c->d_T, Vpad, P, g.d_fst, it, hv, vr, g.fcap, Fa, cFa, Fb, cFb, X, cX, g.d_ffw_tab, g.d_ffw_rec,
                                              g.d_ffw_ws, g.ffw_cap));
            } else
                HIPCHK(shk_firth_fast_launch(st, g.q, nF, c->d_T, Vpad, P, g.d_fst, it, hv, vr, g.fcap, Fa, cFa, Fb, cFb, X, cX, V, d_out, d_flags));
            { int two[2] = {0, 0}; const int rcb = readback_sync(c, st, cFb, cX, nullptr, nullptr, two); if (rcb) return rcb; nF = two[0]; nE = two[1]; }
            if (dbg) fprintf(stderr, "[firth debug] one-pass round %d: %d go on\n", passes, nF);
            ++passes;
            std::swap(Fa, Fb); std::swap(cFa, cFb);
        }
        E = X; cE = cX; En = Fa; cEn = cFa; S = Fb; cS = cFb;
        if (dbg) fprintf(stderr, "[firth debug] %d one-pass rounds; %d slots to the exact kernels\n", passes, nE);
    }
    while (nE > 0 || nS64 > 0) {
        if (dbg) fprintf(stderr, "[firth debug] round %d: %d to evaluate, %d all-fp64 score passes\n", round, nE, nS64);
        ++round;
        HIPCHK(hipMemsetAsync(cEn, 0, sizeof(int), st));
        HIPCHK(hipMemsetAsync(cS, 0, sizeof(int), st));
        if (v2) {
            // slots the pivot guard of the previous round kept away from the single-precision hat diagonal: their all-fp64 score pass runs
            // first and appends to THIS round's evaluation list (their number came back with the previous round's count; launching the pass
            // for a list known to be empty cost 0.4 ms per round: 4055 blocks that only read the count)
            if (nS64 > 0) {
                HIPCHK(shk_firth_launch(st, g.q, 2, nS64, c->d_T, Vpad, V, g.d_y, g.d_W, P, g.d_fst, it, hv, vr, g.fcap, S64, cS64, E, cE, nullptr, nullptr,
                                        d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB));
                nE += nS64;
            }
            HIPCHK(hipMemsetAsync(cS64, 0, sizeof(int), st));
            HIPCHK(shk_firth2_launch(st, g.q, 1, nE, c->d_T, Vpad, V, P, g.d_fst, it, hv, vr, g.fcap, E, cE, En, cEn, S, cS,
                                     d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB, S64, cS64));
            HIPCHK(shk_firth2_launch(st, g.q, 2, nE, c->d_T, Vpad, V, P, g.d_fst, it, hv, vr, g.fcap, S, cS, En, cEn, nullptr, nullptr,
                                     d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB, S64, cS64));
        } else {
            HIPCHK(shk_firth_launch(st, g.q, 1, nE, c->d_T, Vpad, V, g.d_y, g.d_W, P, g.d_fst, it, hv, vr, g.fcap, E, cE, En, cEn, S, cS,
                                    d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB));
            HIPCHK(shk_firth_launch(st, g.q, 2, nE, c->d_T, Vpad, V, g.d_y, g.d_W, P, g.d_fst, it, hv, vr, g.fcap, S, cS, En, cEn, nullptr, nullptr,
                                    d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB));
        }
        int back[3] = {0, 0, 0};
        { const int rcb = readback_sync(c, st, cEn, v2 ? cS64 : nullptr, cB, nullptr, back); if (rcb) return rcb; }
        nE = back[0]; nS64 = back[1]; nB_seen = back[2];
        std::swap(E, En); std::swap(cE, cEn);
    }
    // variants still iterating after P.firth_handoff accepted steps are finished one per workgroup
    // (the hand-off count came back with the last round's; a run that had no exact round reads it now)
    int nB = nB_seen;
    if (nB < 0) { const int rcb = readback_sync(c, st, cB, nullptr, nullptr, nullptr, &nB); if (rcb) return rcb; }
    if (dbg) fprintf(stderr, "[firth debug] %d rounds; %d handed to one workgroup each\n", round, nB);
    if (nB > 0)
        HIPCHK(shk_firth_launch(st, g.q, 3, nB, c->d_T, Vpad, V, g.d_y, g.d_W, P, g.d_fst, it, hv, vr, g.fcap, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, d_out, d_flags, g.d_plist, g.d_fcount + 1, B, cB));
    return SH_OK;
}

static int glm_batch_dev_inner(sh_ctx *c, const void *d_bits, int64_t row_bytes, int64_t V, void *d_out, void *d_flags)
{
    if (V <= 0) return SH_OK;
    HIPCHK(hipSetDevice(c->device));
    GlmState &g = c->glm;
    const int64_t Vpad = (V + 255) / 256 * 256;
    int rc = ensure_ws(c, Vpad); if (rc) return rc;
    if (Vpad > g.cap_list) { hipFree(g.d_flist); hipFree(g.d_plist); g.d_flist = g.d_plist = nullptr; HIPCHK(dmalloc(&g.d_flist, Vpad)); HIPCHK(dmalloc(&g.d_plist, Vpad));
        hipFree(g.d_bw); hipFree(g.d_state); hipFree(g.d_slist); g.d_bw = nullptr; g.d_state = g.d_slist = nullptr;
        HIPCHK(dmalloc(&g.d_bw, (size_t)Vpad * (g.q + 2))); HIPCHK(dmalloc(&g.d_state, Vpad)); HIPCHK(dmalloc(&g.d_slist, Vpad));
        hipFree(g.d_tile_list); g.d_tile_list = nullptr; HIPCHK(dmalloc(&g.d_tile_list, Vpad));
        hipFree(g.d_chord); g.d_chord = nullptr;
        if (g.P.chord_on) HIPCHK(dmalloc(&g.d_chord, (size_t)Vpad * glm_round_ws_doubles(g.q) + 16));      // + 32 int counters
        g.cap_list = Vpad; }
    hipStream_t st = c->stream;
    GlmParams P = g.P; P.min_af = c->min_af; P.max_af = c->max_af; P.af_on = c->af_on;
    if (P.chord_on) {                                     // carve the round workspaces for THIS batch's Vpad (SoA strides are Vpad)
        const int PC = g.q + 2, NH = PC * (PC + 1) / 2;
        double *w = g.d_chord;
        P.ch_bs = w; w += (size_t)Vpad * PC; P.ch_g = w; w += (size_t)Vpad * PC; P.ch_fac = w; w += (size_t)Vpad * NH; P.ch_md = w; w += Vpad;
        P.ch_bd = w; w += (size_t)Vpad * PC; P.ch_ll = w; w += Vpad; P.ch_b0 = w; w += (size_t)Vpad * PC;
        P.ch_hf = (float *)w; w += (size_t)Vpad * ((NH + 1) / 2); P.ch_rho = (float *)w; w += Vpad;      // Vpad floats used of Vpad doubles
        int *l = (int *)w; for (int i = 0; i < 6; ++i) P.ch_list[i] = l + (size_t)i * Vpad; w += 3 * Vpad;
        P.ch_cnt = (int *)w;
        HIPCHK(hipMemsetAsync(P.ch_cnt, 0, 32 * sizeof(int), c->stream));
    }
    HIPCHK(shk_repack_bits(st, (const uint8_t *)d_bits, row_bytes, V, Vpad, c->N, c->NB64p, c->d_T, nullptr));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipMemsetAsync(g.d_fcount, 0, 4 * sizeof(int), st));
    if (g.q > 14) {                                       // wide designs: glm_wide.hip (prefilter + Newton, then Firth / OLS lists)
        if (c->timing) { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventRecord(e0, st)); }
        // 0 = prefilter + routing (binary: lists the variants to fit), 3 = Newton, one workgroup per variant, 1 = Firth, 2 = OLS
        const int blk_newton = 1;
        int *nl = (blk_newton && !P.continuous) ? g.d_slist : nullptr, *nc = g.d_fcount + 2;
        // binary + workgroup kernels: 0, 3 (Newton), 4 (Firth; singular ones go to the plist), 5 (kernel 2 on the plist)
        const int order[6] = {0, 3, 1, 4, 5, 2};
        for (int k = 0; k < 6; ++k) {
            const int which = order[k];
            if ((which == 1 || which == 4 || which == 5) && P.continuous) continue;
            if (which == 2 && !P.continuous) continue;
            if (which == 3 && !nl) continue;
            if (which == 1 && nl) continue;
            if ((which == 4 || which == 5) && !nl) continue;
            HIPCHK(shk_glm_wide(st, which, g.q, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_y1, g.d_y0, g.d_yc, P, (double *)d_out,
                                (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, nl, nc));
        }
        if (c->timing) { HIPCHK(hipEventRecord(e1, st)); c->tev.emplace_back(e0, e1); }
        return SH_OK;
    }
    if (P.continuous) {
        if (c->timing) { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventRecord(e0, st)); }
        if (g.ols_tab && g.d_olstab)
            HIPCHK(shk_glm_ols_tab(st, g.q, 1, c->d_T, Vpad, V, g.d_y, g.d_yc, g.d_W, g.d_olstab, g.d_ZtZ, g.d_Zty, P, g.ymean, g.yty,
                                   (double *)d_out, (uint32_t *)d_flags, g.d_plist, g.d_fcount + 1));
        else
            HIPCHK(shk_glm_launch(st, g.q, 2, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_Wf, g.d_y1, g.d_y0, g.d_yc, g.d_ZtZ, g.d_Zty, P,
                                  (double *)d_out, (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, g.d_bw, g.d_state, g.d_slist, g.d_fcount + 2, g.d_tile_list, g.d_fcount + 3));
        if (c->timing) { HIPCHK(hipEventRecord(e1, st)); c->tev.emplace_back(e0, e1); }
        HIPCHK(shk_glm_launch(st, g.q, 6, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_Wf, g.d_y1, g.d_y0, g.d_yc, g.d_ZtZ, g.d_Zty, P,
                              (double *)d_out, (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, g.d_bw, g.d_state, g.d_slist, g.d_fcount + 2, g.d_tile_list, g.d_fcount + 3));
        return SH_OK;
    }
    // timing: one event pair around every kernel of the fit (Newton, Firth rounds with their list-length round trips, final pass)
    if (c->timing) { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventRecord(e0, st)); }
    HIPCHK(shk_glm_launch(st, g.q, 0, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_Wf, g.d_y1, g.d_y0, g.d_yc, g.d_ZtZ, g.d_Zty, P,
                          (double *)d_out, (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, g.d_bw, g.d_state, g.d_slist, g.d_fcount + 2, g.d_tile_list, g.d_fcount + 3));
    HIPCHK(shk_glm_launch(st, g.q, 4, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_Wf, g.d_y1, g.d_y0, g.d_yc, g.d_ZtZ, g.d_Zty, P,
                          (double *)d_out, (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, g.d_bw, g.d_state, g.d_slist, g.d_fcount + 2, g.d_tile_list, g.d_fcount + 3));
    HIPCHK(shk_glm_launch(st, g.q, 5, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_Wf, g.d_y1, g.d_y0, g.d_yc, g.d_ZtZ, g.d_Zty, P,
                          (double *)d_out, (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, g.d_bw, g.d_state, g.d_slist, g.d_fcount + 2, g.d_tile_list, g.d_fcount + 3));
    rc = firth_rounds(c, Vpad, V, P, (double *)d_out, (uint32_t *)d_flags); if (rc) return rc;
    HIPCHK(shk_glm_launch(st, g.q, 3, c->d_T, Vpad, V, g.d_y, g.d_W, g.d_Wf, g.d_y1, g.d_y0, g.d_yc, g.d_ZtZ, g.d_Zty, P,
                          (double *)d_out, (uint32_t *)d_flags, g.d_flist, g.d_fcount, g.d_plist, g.d_fcount + 1, g.d_bw, g.d_state, g.d_slist, g.d_fcount + 2, g.d_tile_list, g.d_fcount + 3));
    if (c->timing) { HIPCHK(hipEventRecord(e1, st)); c->tev.emplace_back(e0, e1); }
    return SH_OK;
}

static int glm_batch_host(sh_ctx *c, const uint8_t *bits, int64_t row_bytes, int64_t V, double *prep, double *pvalue, double *kbeta,
                          double *bse, double *intercept, double *betas, uint32_t *flags, bool async)
{
    if (!c || !c->glm.ready) return fail(SH_EINVAL, "sh_glm_setup has not run");
    if (!bits || !prep || !pvalue || !kbeta || !bse || !intercept || !flags) return fail(SH_EINVAL, "null argument");
    const int q = c->glm.q;
    if (q > 0 && !betas) return fail(SH_EINVAL, "null betas");
    if (V <= 0) { HIPCHK(hipSetDevice(c->device)); return drain_pending(c); }      // (an empty batch still completes the one before it)
    double *outs[5] = {prep, pvalue, kbeta, bse, intercept};
    return host_batch(c, bits, row_bytes, V, 5 + q, outs, betas, q, flags, async,
                      [&](const void *b, int64_t n, void *o, void *f) { return sh_glm_batch_dev(c, b, row_bytes, n, o, f); });
}

int sh_glm_batch(sh_ctx *c, const uint8_t *bits, int64_t row_bytes, int64_t V, double *prep, double *pvalue, double *kbeta,
                 double *bse, double *intercept, double *betas, uint32_t *flags)
{
    return glm_batch_host(c, bits, row_bytes, V, prep, pvalue, kbeta, bse, intercept, betas, flags, false);
}

int sh_glm_batch_async(sh_ctx *c, const uint8_t *bits, int64_t row_bytes, int64_t V, double *prep, double *pvalue, double *kbeta,
                       double *bse, double *intercept, double *betas, uint32_t *flags)
{
    return glm_batch_host(c, bits, row_bytes, V, prep, pvalue, kbeta, bse, intercept, betas, flags, true);
}

int sh_glm_info(sh_ctx *c, int64_t *firth_routed, int64_t *pinv_routed)
{
    if (!c || !c->glm.ready) return fail(SH_EINVAL, "sh_glm_setup has not run");
    HIPCHK(hipSetDevice(c->device));
    int cnt[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(cnt, c->glm.d_fcount, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->glm.P.dbg) {
        int d[8]; HIPCHK(hipMemcpy(d, c->glm.P.dbg, sizeof(d), hipMemcpyDeviceToHost));
        fprintf(stderr, "[glm debug] wave passes %d over %d waves (%.2f per wave); lane steps %d over %d fitted lanes (%.2f per lane); final-pass repeats %d\n",
                d[0], d[1], d[1] ? (double)d[0] / d[1] : 0.0, d[2], d[3], d[3] ? (double)d[2] / d[3] : 0.0, d[4]);
        if (c->glm.P.chord_on && c->glm.d_chord && c->glm.cap_list) {
            const int64_t Vp = c->glm.cap_list;
            const int *cp = (const int *)(c->glm.d_chord + (size_t)Vp * glm_round_ws_doubles(c->glm.q));
            int rc[32]; HIPCHK(hipMemcpy(rc, cp, sizeof(rc), hipMemcpyDeviceToHost));
            fprintf(stderr, "[glm debug] last batch (if it had the workspace's capacity): Newton-round lists");
            for (int r = 0; r <= c->glm.P.chord_n32; ++r) fprintf(stderr, " %d", rc[r]);
            fprintf(stderr, "; chord-round lists");
            for (int r = 0; r <= c->glm.P.chord_rounds; ++r) fprintf(stderr, " %d", rc[c->glm.P.chord_n32 + 1 + r]);
            fprintf(stderr, "; finishing list %d, finished from the first chord round's likelihood pass %d; fp64 restarts %d\n", rc[30], rc[29], cnt[2]);
        }
        HIPCHK(hipMemset(c->glm.P.dbg, 0, 8 * sizeof(int)));
    }
    if (firth_routed) *firth_routed = cnt[0];
    if (pinv_routed) *pinv_routed = cnt[1];
    return SH_OK;
}

// a6 fit_lineage_effect (model.py:151-199).  lin: n x l row-major (MDS components or cluster indicators), cov: n x j or NULL.
int sh_lineage_setup(sh_ctx *c, const double *lin, int l, const double *cov, int j)
{
    if (!c || !lin || l < 1 || j < 0 || (j > 0 && !cov)) return fail(SH_EINVAL, "bad argument");
    const int PC = 1 + l + j, N = c->N;
    // The count route (k_glm_lineage_counts): a design of disjoint cluster indicators and nothing else -- every entry exactly 0 or 1, at most
    // one 1 per row, no covariates, somebody in no column (the reference cluster, whose column the command line dropped).  An empty column
    // is legal (every variant answers None, as the reference does).
    const std::string head = "1 + lineages + covariates must be <= 50 in this build unless the design is cluster indicators without covariates: ";
    if (PC > 50) {
        if (j > 0) return fail(SH_EINVAL, head + "this one has covariates");
        if (l > LIN_COUNTS_MAX) return fail(SH_EINVAL, head + "more than LIN_COUNTS_MAX = " + std::to_string(LIN_COUNTS_MAX) + " clusters");
        if (c->lin_counts == 0) return fail(SH_EINVAL, head + "and SEERHIP_ROUTE lin_counts=0 keeps it off the count kernel");
    }
    // (the design is only looked through where the count route can be taken at all)
    bool by_counts = j == 0 && l <= LIN_COUNTS_MAX && c->lin_counts != 0 && (c->lin_counts == 1 || PC > 50);
    std::vector<uint16_t> cof;
    std::vector<int> nc;
    if (by_counts) {
        cof.assign((size_t)N, 0); nc.assign((size_t)l + 1, 0);
        bool indicators = true;
        for (int i = 0; i < N && indicators; ++i)
            for (int a = 0; a < l; ++a) {
                const double z = lin[(size_t)i * l + a];
                if (z == 0.0) continue;
                if (z != 1.0 || cof[i] != 0) { indicators = false; break; }
                cof[i] = (uint16_t)(a + 1);                      // (l <= LIN_COUNTS_MAX < 65536)
            }
        if (indicators) for (int i = 0; i < N; ++i) ++nc[cof[i]];
        by_counts = indicators && nc[0] > 0;
        if (PC > 50 && !indicators) return fail(SH_EINVAL, head + "its lineage columns are not the indicators of disjoint clusters");
        if (PC > 50 && !by_counts) return fail(SH_EINVAL, head + "no sample is left for the reference cluster (every row has a 1)");
    }
    HIPCHK(hipSetDevice(c->device));
    GlmState &g = c->glm;
    hipFree(g.d_lin_cof); g.d_lin_cof = nullptr; hipFree(g.d_lin_nc); g.d_lin_nc = nullptr; g.lin_by_counts = false;
    hipFree(g.d_Xlin); g.d_Xlin = nullptr; g.lin_n = 0; g.lin_pc = 0;
    if (by_counts) {
        HIPCHK(dmalloc(&g.d_lin_cof, cof.size())); HIPCHK(dmalloc(&g.d_lin_nc, nc.size()));
        HIPCHK(hipMemcpyAsync(g.d_lin_cof, cof.data(), sizeof(uint16_t) * cof.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(g.d_lin_nc, nc.data(), sizeof(int) * nc.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        g.lin_by_counts = true;
        if (PC > 50) { g.lin_pc = PC; g.lin_n = l; return SH_OK; }     // (narrower designs keep the dense design as well)
    }
    std::vector<double> X((size_t)N * PC);
    for (int i = 0; i < N; ++i) {                    // [1, lin, c] as model.py:172-179
        X[(size_t)i * PC] = 1.0;
        for (int a = 0; a < l; ++a) X[(size_t)i * PC + 1 + a] = lin[(size_t)i * l + a];
        for (int a = 0; a < j; ++a) X[(size_t)i * PC + 1 + l + a] = cov[(size_t)i * j + a];
    }
    HIPCHK(dmalloc(&g.d_Xlin, X.size()));
    HIPCHK(hipMemcpyAsync(g.d_Xlin, X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    g.lin_pc = PC; g.lin_n = l;
    return SH_OK;
}

// max_lineage[v] = index of the most significant lineage for variant v, or -1 (None)
int sh_lineage_batch(sh_ctx *c, const uint8_t *bits, int64_t row_bytes, int64_t V, int32_t *max_lineage)
{
    if (!c || !c->glm.lin_n) return fail(SH_EINVAL, "sh_lineage_setup has not run");
    if (V <= 0) return SH_OK;
    if (!bits || !max_lineage) return fail(SH_EINVAL, "null argument");
    if (row_bytes * 8 < c->N) return fail(SH_ESHAPE, "row_bytes*8 < n_samples");
    HIPCHK(hipSetDevice(c->device));
    GlmState &g = c->glm;
    const int64_t CH = 1 << 20;
    for (int64_t s = 0; s < V; s += CH) {
        const int64_t n = std::min(CH, V - s);
        const int64_t Vpad = (n + 255) / 256 * 256;
        int rc = ensure_ws(c, Vpad); if (rc) return rc;
        rc = ensure_staging(c, n * row_bytes, 1, 1); if (rc) return rc;
        if (Vpad > g.cap_lin) { hipFree(g.d_lin_out); g.d_lin_out = nullptr; HIPCHK(dmalloc(&g.d_lin_out, Vpad)); g.cap_lin = Vpad; }
        HIPCHK(hipMemcpyAsync(c->d_bits, bits + s * row_bytes, n * row_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(shk_repack_bits(c->stream, c->d_bits, row_bytes, n, Vpad, c->N, c->NB64p, c->d_T, nullptr));
        HIPCHK(glm_lineage_launch(g, c->stream, c->d_T, Vpad, n, c->N, c->NB64, g.d_lin_out, LinList{nullptr, nullptr, nullptr, 0}));
        HIPCHK(hipMemcpyAsync(max_lineage + s, g.d_lin_out, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SH_OK;
}
