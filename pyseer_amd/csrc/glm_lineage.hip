// glm_lineage.hip -- fit_lineage_effect (model.py:151-199; split off glm_kernels.hip in round 5)
#include "glm_passes.h"

// =====================================================================================================================
// a6 fit_lineage_effect (model.py:151-199): logistic regression of the VARIANT on [1, lineages, covariates] (statsmodels
// Newton, default zero start), returns argmax_j |beta_j| / bse_j over the lineage columns, or -1 (None) on
// PerfectSeparationError / LinAlgError.  Here the whole design row is wave-uniform and the response is the per-lane bit.
// X: N x PC row-major with the intercept in column 0.
// =====================================================================================================================
// LinList (the job stream, job_api.inc): fit only the rows a compacted list names -- the PRINTED rows of a block, list[p] = the row's index in
// the block, *cnt of them -- and of those only the ones the reference reaches fit_lineage_effect with (mode 1, fixed effects: not
// pre-filtered, no firth-fail, model.py:355-382; mode 2, LMM per variant: not pre-filtered, not lrt-filtered, lmm.py:200-213); out[p] in list
// order, -1 for the others.  list == nullptr: rows 0 .. V-1, out[v] (sh_lineage_batch).
template <int PC>
__global__ __launch_bounds__(256) void k_glm_lineage(const uint64_t *__restrict__ T, int64_t Vpad, int64_t V, int N, int NB64,
                                                    const double *__restrict__ X, int nlin, int *__restrict__ out, LinList L)
{
    const XWave xw = xwave();                                        // up to four wavefronts share the 64 variants of a block
    int64_t v = (int64_t)blockIdx.x * 64 + xw.lane;
    bool live = v < V;
    const int64_t slot = v;                                          // where the answer goes
    bool wanted = true;
    if (L.list) {
        const long long n = *L.cnt;
        if ((int64_t)blockIdx.x * 64 >= n) return;                   // (the whole block: the launch is sized for every row of the block)
        live = slot < n;
        v = live ? (int64_t)L.list[slot] : 0;
        wanted = live && lin_wanted(L.flags[v], L.mode);
    }
    const int64_t vr = live ? v : 0;
    double beta[PC];
#pragma unroll
    for (int a = 0; a < PC; ++a) beta[a] = 0.0;
    int it = 0, status = 0, best = -1;
    bool fin = false, active = live && wanted;
    const double nobs = (double)N;
    while (__any(active)) {                                          // `active` is kept identical in all the waves of a block
        double H[PC * (PC + 1) / 2], g[PC], maxdev = 0.0, unused = 0.0;
#pragma unroll
        for (int a = 0; a < PC * (PC + 1) / 2; ++a) H[a] = 0.0;
#pragma unroll
        for (int a = 0; a < PC; ++a) g[a] = 0.0;
        if (active) {
            for (int sb = xw.w; sb < NB64; sb += xw.S) {
                const uint64_t w64 = T[(int64_t)sb * Vpad + vr];
                const int nb = min(64, N - sb * 64);
                for (int b = 0; b < nb; ++b) {
                    const int i = sb * 64 + b;
                    double x[PC];
#pragma unroll
                    for (int a = 0; a < PC; ++a) x[a] = X[(int64_t)i * PC + a];
                    double eta = 0.0;
#pragma unroll
                    for (int a = 0; a < PC; ++a) eta = fma(beta[a], x[a], eta);
                    const double mu = logit_cdf(eta), wgt = mu * (1.0 - mu);
                    const double r = (double)(unsigned)((w64 >> b) & 1ull) - mu;
                    maxdev = fmax(maxdev, fabs(r));
#pragma unroll
                    for (int a = 0; a < PC; ++a) {
                        g[a] = fma(r, x[a], g[a]);
                        const double wa = wgt * x[a];
#pragma unroll
                        for (int c = 0; c <= a; ++c) H[sidx(a, c)] = fma(wa, x[c], H[sidx(a, c)]);
                    }
                }
            }
        }
        xw_sum(xw, H); xw_sum(xw, g); xw_sum_max(xw, unused, maxdev);
        if (active && xw.w == 0) {
#pragma unroll
            for (int a = 0; a < PC * (PC + 1) / 2; ++a) H[a] = H[a] / nobs;
            double det;
            if (it > 0 && maxdev <= 1e-8) { status = 1; active = false; }
            else if (fin) {
                // numpy.linalg.inv only fails on an EXACT zero pivot; a numerically rank-deficient Hessian (quasi-separation after
                // 35 iterations) yields huge/NaN standard errors and the argmax simply moves on (np.argmax: first NaN wins).
                if (!ldl_factor<PC>(H, 0.0, &det)) status = 2;
                else {
                    double bestw = -1.0; int first_nan = -1;
#pragma unroll
                    for (int a = 1; a < PC; ++a) {
                        double e[PC];
#pragma unroll
                        for (int c = 0; c < PC; ++c) e[c] = (c == a) ? 1.0 : 0.0;
                        ldl_solve<PC>(H, e);
                        const double wald = fabs(beta[a]) / sqrt(e[a] / nobs);
                        if (a <= nlin) {
                            if (isnan(wald)) { if (first_nan < 0) first_nan = a - 1; }
                            else if (wald > bestw) { bestw = wald; best = a - 1; }
                        }
                    }
                    if (first_nan >= 0) best = first_nan;
                }
                active = false;
            } else {
#pragma unroll
                for (int a = 0; a < PC; ++a) { H[sidx(a, a)] -= 1e-10; g[a] = g[a] / nobs; }
                if (!ldl_factor<PC>(H, 0.0, &det)) { status = 2; active = false; }
                else {
                    ldl_solve<PC>(H, g);
                    bool moving = false;
#pragma unroll
                    for (int a = 0; a < PC; ++a) { beta[a] += g[a]; moving = moving || (fabs(g[a]) > 1e-8); }
                    ++it;
                    if (!moving || it >= 35) fin = true;
                }
            }
        }
        xw_bcast(xw, beta, active);
    }
    if (live && xw.w == 0) out[slot] = (status == 0 && wanted) ? best : -1;
}

extern "C" hipError_t shk_glm_lineage(hipStream_t st, int PC, const uint64_t *T, int64_t Vpad, int64_t V, int N, int NB64,
                                      const double *X, int nlin, int *out, LinList L)
{
    const int S = std::min(4, glm_split_waves(NB64));
    const dim3 grid((unsigned)((V + 63) / 64)), blk(64 * S);
#define LIN_CASE(p) case p: hipLaunchKernelGGL(k_glm_lineage<p>, grid, blk, glm_split_lds(S), st, T, Vpad, V, N, NB64, X, nlin, out, L); break;
    switch (PC) {
        LIN_CASE(2) LIN_CASE(3) LIN_CASE(4) LIN_CASE(5) LIN_CASE(6) LIN_CASE(7) LIN_CASE(8) LIN_CASE(9) LIN_CASE(10)
        LIN_CASE(11) LIN_CASE(12) LIN_CASE(13) LIN_CASE(14) LIN_CASE(15) LIN_CASE(16)
    default: return hipErrorInvalidValue;
    }
#undef LIN_CASE
    return hipGetLastError();
}


// =====================================================================================================================
// The count route: fit_lineage_effect for a design X = [1, indicators of l disjoint clusters] and nothing else (--lineage-clusters without
// covariates).  Samples in none of the l columns are the reference cluster (entry 0 below, coefficient fixed at 0); with n_c the size of
// cluster c and s_c its carriers, every sample of a cluster has the same mu_c = logit_cdf(b0 + b_c), and
//     h_c = n_c mu_c (1 - mu_c) / n,   g_c = (s_c - n_c mu_c) / n
// are the whole Hessian (an arrow: diagonal h_c, border h_c, corner sum_c h_c) and score.  statsmodels' ridge is +1e-10 on the diagonal of
// hessian/nobs, which is negative definite: h_c - 1e-10 on this side (k_glm_lineage: H[a][a] -= 1e-10).  With R = -1e-10 the Newton step is
//     d0 = (g_r + sum_c g_c R / (h_c + R)) / (h_r + R + sum_c h_c R / (h_c + R)),   d_c = (g_c - h_c d0) / (h_c + R)       (c = 1 .. l)
// (the corner's Schur complement h_00 - sum h_c^2 / (h_c + R) written without its cancellation), and at the last iterate, without the ridge,
// the inverse's diagonal is 1/h_c + 1/h_r.  Control flow as k_glm_lineage: PerfectSeparationError when, after an update, every sample's
// |y - mu| <= 1e-8 (every cluster pure and its mu at its side); stop when no |d| > 1e-8 or after 35 iterations; an exact zero pivot is
// LinAlgError; np.argmax over the Wald values, the first NaN winning.
// One wavefront per variant, four adjacent variants per block.  Phase 1: lanes stride over the row's 64-bit words and add each carrier into
// its cluster's LDS counter (integer atomics: any order gives the same counts).  Phase 2: lane t owns entries t, t + 64, ... (b_c in LDS,
// read and written by its owner alone); the two sums are per-lane partial sums in entry order, then a butterfly over the lanes: a fixed order.
// LDS: double b[4][l + 1], int n[l + 1], int s[4][l + 1].
// =====================================================================================================================
#define LINC_RIDGE (-1e-10)
__device__ __forceinline__ double linc_wave_sum(double t)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m);
    return t;
}

__global__ __launch_bounds__(256) void k_glm_lineage_counts(const uint64_t *__restrict__ T, int64_t Vpad, int64_t V, int N, int NB64,
                                                           const uint16_t *__restrict__ cluster_of, const int *__restrict__ n_c, int l,
                                                           int *__restrict__ out, LinList L)
{
    extern __shared__ double linc_lds[];
    const int E = l + 1, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *b = linc_lds + (size_t)w * E;
    int *nn = (int *)(linc_lds + (size_t)4 * E);
    int *s = nn + E + (size_t)w * E;
    const int64_t slot = (int64_t)blockIdx.x * 4 + w;                // where the answer goes
    int64_t v = slot;
    bool live = slot < V, wanted = true;
    if (L.list) {
        const long long n = *L.cnt;
        if ((int64_t)blockIdx.x * 4 >= n) return;                    // (the whole block: the launch is sized for every row of the block)
        live = slot < n;
        v = live ? (int64_t)L.list[slot] : 0;
        wanted = live && lin_wanted(L.flags[v], L.mode);
    }
    const bool active = live && wanted;                              // wave-uniform
    for (int c = threadIdx.x; c < E; c += 256) nn[c] = n_c[c];
    for (int c = lane; c < E; c += 64) { b[c] = 0.0; s[c] = 0; }
    __syncthreads();
    if (active) {
        for (int sb = lane; sb < NB64; sb += 64) {
            uint64_t w64 = T[(int64_t)sb * Vpad + v];
            const int nb = N - sb * 64;                              // (bits behind sample N - 1 are padding, whatever they hold)
            if (nb < 64) w64 &= (1ull << nb) - 1ull;
            while (w64) {
                const int bit = __builtin_ctzll(w64);
                w64 &= w64 - 1ull;
                atomicAdd(&s[cluster_of[sb * 64 + bit]], 1);
            }
        }
    }
    __syncthreads();                                                 // (the last barrier: from here on every wavefront runs alone)
    if (!live) return;
    if (!active) { if (lane == 0) out[slot] = -1; return; }
    const double nobs = (double)N, R = LINC_RIDGE;
    double b0 = 0.0;
    int it = 0, status = 0, best = -1;
    bool fin = false;
    for (;;) {
        // this pass's h, g at the current iterate; the separation test of the update that led here
        double sa = 0.0, sh = 0.0, gr = 0.0, hr = 0.0;
        bool sep = true, zero = false, zden = false;
        for (int c = lane; c < E; c += 64) {
            const int nc = nn[c], sc = s[c];
            const double mu = logit_cdf(b0 + b[c]);
            const double h = (double)nc * mu * (1.0 - mu) / nobs, g = ((double)sc - (double)nc * mu) / nobs;
            if (nc > 0 && !((sc == 0 || sc == nc) && fabs(mu - (sc > 0 ? 1.0 : 0.0)) <= 1e-8)) sep = false;
            if (h == 0.0) zero = true;
            if (c == 0) { gr = g; hr = h; }
            else {
                const double den = h + R;
                if (den == 0.0) zden = true;
                sa += g * R / den; sh += h * R / den;
            }
        }
        if (it > 0 && __all(sep)) { status = 1; break; }             // PerfectSeparationError -> None
        if (fin) {
            if (__any(zero)) { status = 2; break; }                  // numpy.linalg.inv fails on an exact zero pivot only
            hr = __shfl(hr, 0);
            double bestw = -1.0; int bi = 0x7fffffff, nan_i = 0x7fffffff;
            for (int c = lane; c < E; c += 64) {
                if (c == 0) continue;
                const double mu = logit_cdf(b0 + b[c]);
                const double h = (double)nn[c] * mu * (1.0 - mu) / nobs;
                const double wald = fabs(b[c]) / sqrt((1.0 / h + 1.0 / hr) / nobs);
                if (isnan(wald)) { if (nan_i == 0x7fffffff) nan_i = c - 1; }
                else if (wald > bestw) { bestw = wald; bi = c - 1; }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {                      // np.argmax: the largest value, its first index; a NaN before all
                const double ow = __shfl_xor(bestw, m); const int oi = __shfl_xor(bi, m), on = __shfl_xor(nan_i, m);
                if (ow > bestw || (ow == bestw && oi < bi)) { bestw = ow; bi = oi; }
                nan_i = min(nan_i, on);
            }
            best = nan_i != 0x7fffffff ? nan_i : (bi != 0x7fffffff ? bi : 0);
            break;
        }
        sa = linc_wave_sum(sa); sh = linc_wave_sum(sh);
        gr = __shfl(gr, 0); hr = __shfl(hr, 0);
        const double d0den = hr + R + sh;
        if (__any(zden) || d0den == 0.0) { status = 2; break; }      // LinAlgError -> None
        const double d0 = (gr + sa) / d0den;
        bool moving = fabs(d0) > 1e-8;
        for (int c = lane; c < E; c += 64) {
            if (c == 0) continue;
            const int nc = nn[c], sc = s[c];
            const double mu = logit_cdf(b0 + b[c]);
            const double h = (double)nc * mu * (1.0 - mu) / nobs, g = ((double)sc - (double)nc * mu) / nobs;
            const double d = (g - h * d0) / (h + R);
            b[c] += d;
            moving = moving || (fabs(d) > 1e-8);
        }
        b0 += d0;
        ++it;
        if (!__any(moving) || it >= 35) fin = true;
    }
    if (lane == 0) out[slot] = (status == 0) ? best : -1;
}

extern "C" size_t shk_glm_lineage_counts_lds(int l) { return (size_t)(l + 1) * (4 * sizeof(double) + 5 * sizeof(int)); }
extern "C" hipError_t shk_glm_lineage_counts(hipStream_t st, const uint64_t *T, int64_t Vpad, int64_t V, int N, int NB64,
                                             const uint16_t *cluster_of, const int *n_c, int l, int *out, LinList L)
{
    if (l < 1 || l > LIN_COUNTS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_glm_lineage_counts, dim3((unsigned)((V + 3) / 4)), dim3(256), shk_glm_lineage_counts_lds(l), st, T, Vpad, V, N, NB64,
                       cluster_of, n_c, l, out, L);
    return hipGetLastError();
}
