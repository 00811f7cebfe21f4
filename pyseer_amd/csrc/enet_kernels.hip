// enet_kernels.hip -- the whole-genome elastic net (pyseer/enet.py: load_all_vars, correlation_filter, fit_enet) on packed presence bits.
//
// One bit matrix B (P rows of row_bytes, LSB first, bits at and above N are 0) stays on the device; the full fit and every cross-validation
// fold are the SAME problem with different sample weights (a held-out sample has weight 0), so they share B and differ in N-vectors only.
//   k_enet_store        minor-allele coding of load_all_vars (enet.py:95-106) while the rows are put in place
//   k_enet_ingest_*     the same rule and coding applied ON the device to a block of parsed k-mer rows: count, ordered scan, compacted store
//   k_enet_ingest_calls_*  the same for rows with missing calls (VCF records, burden regions): a present and a missing row, a skip flag
//   k_enet_moments      |correlation| of every row with the phenotype (enet.py:379-421)
//   k_enet_grad         G[f][j] = sum over the carriers i of row j of V[f][i], up to 16 vectors per pass, fp64: weighted means, training
//                       counts, lambda_max, the strong rule and the KKT check over ALL rows
//   k_enet_cd           cyclic coordinate descent over a problem's active list, one persistent workgroup per problem, per-sample state in LDS
//                       (or in a global buffer of the same layout when N is too large); binomial by IRLS inside the same workgroup
//   k_enet_gather       rows idx[] of B, compacted (sh_enet_keep, and the rows of the selected variants for the per-variant engine)
//   k_enet_predict      a saved model applied to new samples (pyseer/enet_predict.py:159-179): acc[sample] += bit * beta, row after row
// State kept per sample: v (working weight), Rr (working residual r = Rr - o; the centring of the standardised columns is carried in the scalar
// o, so a coordinate step touches the carriers only, as glmnet does for sparse input), and for binomial the working response z.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "enet_params.h"

#define ENET_TPB 256
#define ENET_WAVES (ENET_TPB / 64)

__device__ __forceinline__ double enet_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;                                                         // lane 0 holds the sum
}

// The words of one row for a whole wavefront: 64 words per coalesced load (lane l holds word base + l), then every NON-EMPTY word, in
// ascending order, is handed to all lanes by a shuffle.  No load waits for the value of the one before it, and an empty word (most words of
// a minor-allele row) costs a bit of a ballot instead of a trip to memory.
template <typename F>
__device__ __forceinline__ void enet_for_words(const uint64_t *__restrict__ row, int NW, int lane, F f)
{
    for (int base = 0; base < NW; base += 64) {
        const uint64_t mine = base + lane < NW ? row[base + lane] : 0ull;
        unsigned long long any = __ballot(mine != 0ull);
        while (any) {
            const int k = __ffsll((long long)any) - 1;
            any &= any - 1ull;
            f(base + k, (uint64_t)__shfl((long long)mine, k, 64));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void k_enet_store(const uint8_t *__restrict__ present, const uint8_t *__restrict__ missing, const uint8_t *__restrict__ flip,
                             int64_t V, int NW, int N, uint64_t *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= V * NW) return;
    const int64_t v = t / NW; const int wd = (int)(t % NW);
    uint64_t b = reinterpret_cast<const uint64_t *>(present)[t];
    const int left = N - wd * 64;
    const uint64_t valid = left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);   // (a row may carry whole spare words)
    if (flip && flip[v]) {                                            // af > 0.5: coded by the absences; a missing call is 0 in either coding
        b = ~b;
        if (missing) b &= ~reinterpret_cast<const uint64_t *>(missing)[t];
    }
    dst[t] = b & valid;
}

__global__ void k_enet_gather(const uint64_t *__restrict__ src, const int64_t *__restrict__ idx, int64_t n, int NW, uint64_t *__restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * NW) return;
    dst[t] = src[idx[t / NW] * NW + (t % NW)];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// k_enet_ingest_*: a block of V parsed rows (no missing calls: k-mers) goes into B by load_all_vars' rule (enet.py:33-118) without the host
// looking at a row: count the carriers, keep the rows whose count lies in [lo, hi], give every kept row the number of kept rows before it
// (the order of the stream is the order of the matrix: no atomics), store it by its minor allele (enet.py:95-106).
__device__ __forceinline__ uint64_t enet_valid_bits(int wd, int N)
{
    const int left = N - wd * 64;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
}

// one wavefront per row: carriers over the first N bits (whatever the reader left in the padding is not counted)
__global__ void k_enet_ingest_count(const uint64_t *__restrict__ rows, int64_t V, int NW, int N, int32_t *__restrict__ cnt)
{
    const int64_t v = (int64_t)blockIdx.x * ENET_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= V) return;
    const uint64_t *row = rows + v * NW;
    int c = 0;
    for (int wd = lane; wd < NW; wd += 64) c += __popcll(row[wd] & enet_valid_bits(wd, N));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if (lane == 0) cnt[v] = c;
}

// ONE workgroup walks the V counts, ENET_SCAN_TPB at a time: a ballot orders the rows of a wavefront, the LDS the wavefronts of a step, a
// running total the steps.  dest[v] = position among the kept rows or -1; kept_idx / kept_cnt = block index and carriers of every kept row.
#define ENET_SCAN_TPB 1024
__global__ __launch_bounds__(ENET_SCAN_TPB) void k_enet_ingest_scan(const int32_t *__restrict__ cnt, int64_t V, int lo, int hi, int32_t *__restrict__ dest,
                                                                    int32_t *__restrict__ kept_idx, int32_t *__restrict__ kept_cnt, int32_t *__restrict__ n_kept)
{
    __shared__ int wsum[ENET_SCAN_TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0;
    for (int64_t base = 0; base < V; base += ENET_SCAN_TPB) {
        const int64_t v = base + tid;
        const int c = v < V ? cnt[v] : 0;
        const bool keep = v < V && c >= lo && c <= hi;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < ENET_SCAN_TPB / 64; ++w) { const int s = wsum[w]; if (w < wv) before += s; total += s; }
        if (v < V) {
            dest[v] = keep ? carry + before : -1;
            if (keep) { kept_idx[carry + before] = (int32_t)v; kept_cnt[carry + before] = c; }
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) *n_kept = carry;
}

// one wavefront per row: a kept row goes to dst + dest[v] * NW, complemented over the first N bits when more than half the samples carry it
// (af > 0.5 is 2c > N; exactly N / 2 carriers is not flipped), padding bits 0: the words k_enet_store writes for (present, NULL, flip)
__global__ void k_enet_ingest_scatter(const uint64_t *__restrict__ rows, int64_t V, int NW, int N, const int32_t *__restrict__ cnt,
                                      const int32_t *__restrict__ dest, uint64_t *__restrict__ dst)
{
    const int64_t v = (int64_t)blockIdx.x * ENET_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= V) return;
    const int d = dest[v];
    if (d < 0) return;
    const bool flip = 2 * (int64_t)cnt[v] > (int64_t)N;
    const uint64_t *row = rows + v * NW;
    uint64_t *out = dst + (int64_t)d * NW;
    for (int wd = lane; wd < NW; wd += 64) { const uint64_t b = row[wd]; out[wd] = (flip ? ~b : b) & enet_valid_bits(wd, N); }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// k_enet_ingest_calls_*: the same for rows WITH missing calls (VCF records, burden regions): a present and a missing row per variant, and
// the reader's skip flag.  c = present, m = missing and not present (a sample set in both rows is present, as in k_enet_store), both over
// the first N bits; the reference counts a missing call as a carrier in af (input.py:439-446), so the AF interval is on t = c + m and the
// missing rule on m alone.
// one wavefront per row, two popcounts per word; miss == NULL: no missing calls
__global__ void k_enet_ingest_calls_count(const uint64_t *__restrict__ pres, const uint64_t *__restrict__ miss, int64_t V, int NW, int N,
                                          int32_t *__restrict__ cnt_p, int32_t *__restrict__ cnt_m)
{
    const int64_t v = (int64_t)blockIdx.x * ENET_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= V) return;
    const uint64_t *rp = pres + v * NW, *rm = miss ? miss + v * NW : nullptr;
    int c = 0, m = 0;
    for (int wd = lane; wd < NW; wd += 64) {
        const uint64_t valid = enet_valid_bits(wd, N), b = rp[wd];
        c += __popcll(b & valid);
        if (rm) m += __popcll(rm[wd] & ~b & valid);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_down(c, o, 64); m += __shfl_down(m, o, 64); }
    if (lane == 0) { cnt_p[v] = c; cnt_m[v] = m; }
}

// the ordered scan of k_enet_ingest_scan with the three-part predicate: not skipped, lo <= c + m <= hi, m <= mm (mm < 0 keeps nothing)
__global__ __launch_bounds__(ENET_SCAN_TPB) void k_enet_ingest_calls_scan(const int32_t *__restrict__ cnt_p, const int32_t *__restrict__ cnt_m,
                                                                          const int32_t *__restrict__ skip, int64_t V, int lo, int hi, int mm,
                                                                          int32_t *__restrict__ dest, int32_t *__restrict__ kept_idx,
                                                                          int32_t *__restrict__ kept_p, int32_t *__restrict__ kept_m, int32_t *__restrict__ n_kept)
{
    __shared__ int wsum[ENET_SCAN_TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0;
    for (int64_t base = 0; base < V; base += ENET_SCAN_TPB) {
        const int64_t v = base + tid;
        const int c = v < V ? cnt_p[v] : 0, m = v < V ? cnt_m[v] : 0;
        const int t = c + m;
        const bool keep = v < V && !(skip && skip[v] != 0) && t >= lo && t <= hi && m <= mm;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < ENET_SCAN_TPB / 64; ++w) { const int s = wsum[w]; if (w < wv) before += s; total += s; }
        if (v < V) {
            dest[v] = keep ? carry + before : -1;
            if (keep) { kept_idx[carry + before] = (int32_t)v; kept_p[carry + before] = c; kept_m[carry + before] = m; }
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) *n_kept = carry;
}

// one wavefront per row: both rows of a kept row are read; 2 (c + m) > N stores the absences, a missing call being 0 in either coding
// (~present & ~missing), padding bits 0: the words k_enet_store writes for (present, missing, flip)
__global__ void k_enet_ingest_calls_scatter(const uint64_t *__restrict__ pres, const uint64_t *__restrict__ miss, int64_t V, int NW, int N,
                                            const int32_t *__restrict__ cnt_p, const int32_t *__restrict__ cnt_m, const int32_t *__restrict__ dest,
                                            uint64_t *__restrict__ dst)
{
    const int64_t v = (int64_t)blockIdx.x * ENET_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= V) return;
    const int d = dest[v];
    if (d < 0) return;
    const bool flip = 2 * ((int64_t)cnt_p[v] + (int64_t)cnt_m[v]) > (int64_t)N;
    const uint64_t *rp = pres + v * NW, *rm = miss ? miss + v * NW : nullptr;
    uint64_t *out = dst + (int64_t)d * NW;
    for (int wd = lane; wd < NW; wd += 64) {
        uint64_t b = rp[wd];
        if (flip) { b = ~b; if (rm) b &= ~rm[wd]; }
        out[wd] = b & enet_valid_bits(wd, N);
    }
}

// one wavefront per row: carrier count and carrier sum of yc = y - mean(y);  cor = |ab / sqrt(sum a^2 sum b^2)| with a = k - mean(k)
__global__ void k_enet_moments(const uint64_t *__restrict__ B, int64_t P, int NW, int N, const double *__restrict__ yc, double sum_b2,
                               double *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * ENET_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= P) return;
    const uint64_t *row = B + j * NW;
    double s = 0.0; int cnt = 0;
    enet_for_words(row, NW, lane, [&](int wd, uint64_t b) { if ((b >> lane) & 1ull) { s += yc[wd * 64 + lane]; ++cnt; } });
    s = enet_wave_sum(s);
    double c = enet_wave_sum((double)cnt);
    if (lane == 0) {
        if (c == 0.0) { out[j] = NAN; return; }                       // enet.py:411: an empty row
        const double km = c / (double)N;
        // sum_i b_i = 0, so ab = k.b; sum a^2 = k.k - 2 km sum(k) + km^2 N
        const double sa2 = c - 2.0 * km * c + km * km * (double)N;
        out[j] = fabs(s / sqrt(sa2 * sum_b2));
    }
}

// one wavefront per row, NF <= 16 vectors V[f][i] (stride ldv): G[f][j] = carrier sum
template <int NF>
__global__ void k_enet_grad(const uint64_t *__restrict__ B, int64_t P, int NW, const double *__restrict__ V, int64_t ldv, int nf,
                            double *__restrict__ G, int64_t ldg)
{
    const int64_t j = (int64_t)blockIdx.x * ENET_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= P) return;
    const uint64_t *row = B + j * NW;
    double acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = 0.0;
    enet_for_words(row, NW, lane, [&](int wd, uint64_t b) {
        if ((b >> lane) & 1ull) {
            const double *vp = V + wd * 64 + lane;
#pragma unroll
            for (int f = 0; f < NF; ++f) if (f < nf) acc[f] += vp[f * ldv];
        }
    });
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (f < nf) { const double s = enet_wave_sum(acc[f]); if (lane == 0) G[f * ldg + j] = s; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// block-wide sum of K values; every thread returns the same figures (fixed order: lanes by shuffle, then the four wavefronts in order)
template <int K>
__device__ __forceinline__ void enet_block_sum(double (&x)[K], double *red /* [ENET_WAVES * K] */)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = enet_wave_sum(x[k]); if (lane == 0) red[wv * K + k] = x[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) { double s = 0.0; for (int w = 0; w < ENET_WAVES; ++w) s += red[w * K + k]; x[k] = s; }
}

__device__ __forceinline__ double enet_soft(double u, double t) { const double a = fabs(u) - t; return a > 0.0 ? copysign(a, u) : 0.0; }

__global__ __launch_bounds__(ENET_TPB) void k_enet_cd(EnetCdArgs a)
{
    extern __shared__ double lds[];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.skip[f]) return;
    const int N = a.N, NW = a.NW, Np = NW * 64, ncov = a.n_cov;
    const int64_t PT = a.P + ncov;
    double *red = lds;                                                // 2 x ENET_WAVES x 4 doubles (double-buffered)
    double *gst = a.state + (int64_t)f * 3 * Np;                      // the state between launches (and during them when it does not fit the LDS)
    double *sv, *sR, *sz;
    if (a.use_lds) { sv = lds + 64; sR = sv + Np; sz = sR + Np; } else { sv = gst; sR = gst + Np; sz = gst + 2 * Np; }
    const double *w = a.w + (int64_t)f * Np, *hw = a.hw + (int64_t)f * Np, *y = a.y;
    const double *mj = a.m + (int64_t)f * a.P, *sinv = a.sinv + (int64_t)f * a.P;
    const double *Xc = a.Xc + (int64_t)f * ncov * Np;
    double *beta = a.beta + f * PT, *bold = a.bold + f * PT, *xvs = a.xv + f * PT;
    const int *act = a.act + f * PT; const int nact = a.nact[f];
    const bool binom = a.family == 1, init = a.init != 0;
    const double lam = a.lambda, al = a.alpha, thr = a.thr[f];
    const double l1 = al * lam, l2 = (1.0 - al) * lam;
    double o, b0;
    // ---- state in
    if (init) {
        b0 = a.b0_null[f]; o = 0.0;
        for (int i = tid; i < Np; i += ENET_TPB) {
            if (!binom) { sv[i] = i < N ? w[i] : 0.0; sR[i] = i < N ? y[i] - b0 : 0.0; }
            else { sz[i] = b0; sR[i] = 0.0; sv[i] = 0.0; }            // eta = z - (Rr - o) = b0: the first IRLS step below builds the rest
        }
    } else {
        o = a.scal[f * 4 + 0]; b0 = a.scal[f * 4 + 1];
        if (a.use_lds) for (int i = tid; i < (binom ? 3 : 2) * Np; i += ENET_TPB) sv[i] = gst[i];
    }
    __syncthreads();
    int sweeps = 0, outer = 0, conv = 0; double dlx = 0.0, SV = 0.0, SVR = 0.0; int par = 0;
    for (;;) {
        // ---- IRLS step: p, working weights and working response from eta (binomial); the exact sums of v and v r in either family
        double b0s = b0;
        {
            double s[2] = {0.0, 0.0};
            for (int i = tid; i < N; i += ENET_TPB) {
                if (binom) {
                    const double eta = sz[i] - (sR[i] - o);
                    double p = 1.0 / (1.0 + exp(-eta));
                    p = fmin(fmax(p, 1e-9), 1.0 - 1e-9);
                    const double pq = p * (1.0 - p), r = (y[i] - p) / pq;
                    sv[i] = w[i] * pq; sz[i] = eta + r; sR[i] = r;
                    s[0] += sv[i]; s[1] += sv[i] * r;
                } else { s[0] += sv[i]; s[1] += sv[i] * (sR[i] - o); }
            }
            __syncthreads();
            enet_block_sum<2>(s, red + par * 16); par ^= 1;
            SV = s[0]; SVR = s[1];
            if (binom) o = 0.0;
            if (binom) for (int k = tid; k < nact; k += ENET_TPB) bold[act[k]] = beta[act[k]];
            __syncthreads();
        }
        // ---- sweeps at fixed working weights
        for (;;) {
            dlx = 0.0;
            for (int k = 0; k < nact; ++k) {
                const int j = act[k];
                double g, xv, dsvr_unit, bj = beta[j];
                double c[3] = {0.0, 0.0, 0.0};
                const uint64_t *row = nullptr; const double *x = nullptr; double si = 0.0, m = 0.0;
                if (j < ncov) {
                    x = Xc + (int64_t)j * Np;
                    for (int i = tid; i < N; i += ENET_TPB) { const double vx = sv[i] * x[i]; c[0] += vx * (sR[i] - o); c[1] += vx * x[i]; c[2] += vx; }
                    enet_block_sum<3>(c, red + par * 16); par ^= 1;
                    g = c[0]; xv = c[1]; dsvr_unit = c[2];
                } else {
                    const int64_t jj = j - ncov;
                    si = sinv[jj]; m = mj[jj];
                    row = a.B + jj * NW;
                    for (int wd = wv; wd < NW; wd += ENET_WAVES) {
                        const uint64_t b = row[wd];
                        if (!b) continue;
                        if ((b >> lane) & 1ull) { const int i = wd * 64 + lane; const double vi = sv[i]; c[0] += vi * sR[i]; c[1] += vi; }
                    }
                    enet_block_sum<3>(c, red + par * 16); par ^= 1;
                    g = si * ((c[0] - o * c[1]) - m * SVR);
                    xv = si * si * (c[1] * (1.0 - 2.0 * m) + m * m * SV);
                    dsvr_unit = si * (c[1] - m * SV);
                }
                if (!(xv > 0.0)) continue;                            // (uniform: every thread holds the same sums)
                const double bn = enet_soft(g + xv * bj, l1) / (xv + l2);
                const double d = bn - bj;
                if (tid == 0) xvs[j] = xv;
                if (d == 0.0) continue;
                if (tid == 0) beta[j] = bn;
                dlx = fmax(dlx, xv * d * d);
                SVR -= d * dsvr_unit;
                if (x) { for (int i = tid; i < N; i += ENET_TPB) sR[i] -= d * x[i]; }
                else {
                    const double ds = d * si;
                    o -= ds * m;
                    for (int wd = wv; wd < NW; wd += ENET_WAVES) {
                        const uint64_t b = row[wd];
                        if ((b >> lane) & 1ull) sR[wd * 64 + lane] -= ds;
                    }
                }
                __syncthreads();
            }
            {   // the intercept
                const double d = SVR / SV;
                b0 += d; o += d; SVR = 0.0;
                dlx = fmax(dlx, SV * d * d);
            }
            ++sweeps;
            if (dlx < thr) { conv = 1; break; }
            if (!isfinite(dlx)) { conv = 2; break; }                  // the IRLS step ran away (no step halving, as in glmnet): the path ends here
            if (sweeps >= a.max_sweeps) { conv = 0; break; }
        }
        if (!binom || conv != 1) break;
        // ---- outer convergence (binomial): the change of every coefficient over this IRLS step
        ++outer;
        double ch = SV * (b0 - b0s) * (b0 - b0s);
        __syncthreads();
        for (int k = tid; k < nact; k += ENET_TPB) { const int j = act[k]; const double d = beta[j] - bold[j]; ch = fmax(ch, xvs[j] * d * d); }
        {
            // block-wide maximum through the same scratch
            for (int off = 32; off > 0; off >>= 1) ch = fmax(ch, __shfl_down(ch, off, 64));
            double *rb = red + par * 16; par ^= 1;
            if (lane == 0) rb[wv] = ch;
            __syncthreads();
            ch = fmax(fmax(rb[0], rb[1]), fmax(rb[2], rb[3]));
        }
        if (ch < thr) break;
        if (outer >= a.max_outer) { conv = 2; break; }
    }
    __syncthreads();
    // ---- figures of this solution: training deviance, held-out deviance, eta, v r for the gradient pass; state out
    double s[3] = {0.0, 0.0, 0.0};
    double *eta_out = a.eta + (int64_t)f * Np, *vr = a.vr + (int64_t)f * Np;
    for (int i = tid; i < Np; i += ENET_TPB) {
        if (i >= N) { vr[i] = 0.0; continue; }
        const double r = sR[i] - o;
        const double eta = binom ? sz[i] - r : y[i] - r;
        eta_out[i] = eta;
        if (binom) {
            // the next IRLS step would start from this eta: its w (y - p) is the gradient's vector at the solution
            double p = 1.0 / (1.0 + exp(-eta));
            p = fmin(fmax(p, 1e-9), 1.0 - 1e-9);
            vr[i] = w[i] * (y[i] - p); s[2] += vr[i];
            const double lse = eta > 0.0 ? eta + log1p(exp(-eta)) : log1p(exp(eta));
            s[0] += w[i] * -2.0 * (y[i] * eta - lse);
            if (hw[i] != 0.0) {
                double pc = 1.0 / (1.0 + exp(-eta));
                pc = fmin(fmax(pc, 1e-5), 1.0 - 1e-5);
                s[1] += hw[i] * -2.0 * (y[i] * log(pc) + (1.0 - y[i]) * log(1.0 - pc));
            }
        } else {
            vr[i] = sv[i] * r; s[2] += vr[i];
            s[0] += w[i] * r * r;
            s[1] += hw[i] * r * r;
        }
    }
    __syncthreads();
    enet_block_sum<3>(s, red + par * 16);
    if (a.use_lds) for (int i = tid; i < (binom ? 3 : 2) * Np; i += ENET_TPB) gst[i] = sv[i];
    if (tid == 0) {
        a.scal[f * 4 + 0] = o; a.scal[f * 4 + 1] = b0; a.scal[f * 4 + 2] = SVR; a.scal[f * 4 + 3] = SV;
        a.res[f * 8 + 0] = s[0]; a.res[f * 8 + 1] = s[1]; a.res[f * 8 + 2] = (double)sweeps; a.res[f * 8 + 3] = (double)conv;
        a.res[f * 8 + 4] = dlx; a.res[f * 8 + 5] = (double)outer; a.res[f * 8 + 6] = s[2]; a.res[f * 8 + 7] = (double)sweeps * (double)nact;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// k_enet_predict: the sum of pyseer/enet_predict.py:174-179 for the rows of one call, `predictions += k * pred_beta` row after row.
// One lane owns one sample and keeps its sum in a register; a wavefront owns word blockIdx.x of every row, so the word, the slope and the
// flip of a row are the same for all 64 lanes (scalar loads, one per 64 samples).  The order of the additions is the order of the rows and
// nothing else: no atomics, no split of the row loop, so every sample's sum is the reference's sequential fp64 sum.  The addend is the
// PRODUCT (double)k * beta, as in the reference, not a conditional add: 0 * beta keeps the sign of the zero that numpy adds.  A missing call
// is NaN where the row is taken as it is and 0 where it is flipped (af > 0.5: ~np.array(k, dtype=bool) of a NaN is False).
// Rows come eight at a time so that the loads of a group are in flight together; the adds stay in row order.
template <bool HAS_MISSING>
__global__ void __launch_bounds__(64) k_enet_predict(const uint64_t *__restrict__ rows, const uint64_t *__restrict__ miss, const double *__restrict__ beta,
                                                    const uint8_t *__restrict__ flip, int64_t n_rows, int NW, int N, double *__restrict__ acc)
{
    const int wd = blockIdx.x, lane = threadIdx.x;
    const int sample = wd * 64 + lane;                                // (bits at and above N belong to nobody: their lanes store nothing)
    double a = sample < N ? acc[sample] : 0.0;
    auto step = [&](uint64_t w, uint64_t m, double b, uint32_t f) {
        const uint32_t bit = ((uint32_t)(w >> lane) & 1u) ^ f;
        double k = (double)bit;
        if (HAS_MISSING && ((m >> lane) & 1ull)) k = f ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);
        a = a + k * b;
    };
    int64_t r = 0;
    for (; r + 8 <= n_rows; r += 8) {
        uint64_t w[8], m[8]; double b[8]; uint32_t f[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            w[u] = rows[(r + u) * NW + wd]; m[u] = HAS_MISSING ? miss[(r + u) * NW + wd] : 0ull;
            b[u] = beta[r + u]; f[u] = flip[r + u] ? 1u : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) step(w[u], m[u], b[u], f[u]);
    }
    for (; r < n_rows; ++r) step(rows[r * NW + wd], HAS_MISSING ? miss[r * NW + wd] : 0ull, beta[r], flip[r] ? 1u : 0u);
    if (sample < N) acc[sample] = a;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
extern "C" {
// n_rows rows of NW words (and their missing rows, or NULL), slopes and flips on the device -> acc[0 .. N); NW * 64 >= N is the caller's check
hipError_t shk_enet_predict(hipStream_t st, const uint64_t *rows, const uint64_t *miss, const double *beta, const uint8_t *flip, int64_t n_rows, int NW, int N,
                            double *acc)
{
    if (n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + 63) / 64)), block(64);
    if (miss) hipLaunchKernelGGL(k_enet_predict<true>, grid, block, 0, st, rows, miss, beta, flip, n_rows, NW, N, acc);
    else hipLaunchKernelGGL(k_enet_predict<false>, grid, block, 0, st, rows, miss, beta, flip, n_rows, NW, N, acc);
    return hipGetLastError();
}
hipError_t shk_enet_store(hipStream_t st, const uint8_t *present, const uint8_t *missing, const uint8_t *flip, int64_t V, int NW, int N, uint64_t *dst)
{
    if (V <= 0) return hipSuccess;
    const int64_t n = V * NW;
    hipLaunchKernelGGL(k_enet_store, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, present, missing, flip, V, NW, N, dst);
    return hipGetLastError();
}
hipError_t shk_enet_gather(hipStream_t st, const uint64_t *src, const int64_t *idx, int64_t n, int NW, uint64_t *dst)
{
    if (n <= 0) return hipSuccess;
    const int64_t t = n * NW;
    hipLaunchKernelGGL(k_enet_gather, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, src, idx, n, NW, dst);
    return hipGetLastError();
}
// count + scan of a block (n_kept is on the device: the caller reads it before it makes room and calls shk_enet_ingest_scatter)
hipError_t shk_enet_ingest_count(hipStream_t st, const uint64_t *rows, int64_t V, int NW, int N, int lo, int hi, int32_t *cnt, int32_t *dest,
                                 int32_t *kept_idx, int32_t *kept_cnt, int32_t *n_kept)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_enet_ingest_count, dim3((unsigned)((V + ENET_WAVES - 1) / ENET_WAVES)), dim3(ENET_TPB), 0, st, rows, V, NW, N, cnt);
    hipLaunchKernelGGL(k_enet_ingest_scan, dim3(1), dim3(ENET_SCAN_TPB), 0, st, cnt, V, lo, hi, dest, kept_idx, kept_cnt, n_kept);
    return hipGetLastError();
}
hipError_t shk_enet_ingest_scatter(hipStream_t st, const uint64_t *rows, int64_t V, int NW, int N, const int32_t *cnt, const int32_t *dest, uint64_t *dst)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_enet_ingest_scatter, dim3((unsigned)((V + ENET_WAVES - 1) / ENET_WAVES)), dim3(ENET_TPB), 0, st, rows, V, NW, N, cnt, dest, dst);
    return hipGetLastError();
}
// the same two steps for rows with missing calls (miss and skip may be NULL)
hipError_t shk_enet_ingest_calls_count(hipStream_t st, const uint64_t *pres, const uint64_t *miss, const int32_t *skip, int64_t V, int NW, int N, int lo, int hi,
                                       int mm, int32_t *cnt_p, int32_t *cnt_m, int32_t *dest, int32_t *kept_idx, int32_t *kept_p, int32_t *kept_m, int32_t *n_kept)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_enet_ingest_calls_count, dim3((unsigned)((V + ENET_WAVES - 1) / ENET_WAVES)), dim3(ENET_TPB), 0, st, pres, miss, V, NW, N, cnt_p, cnt_m);
    hipLaunchKernelGGL(k_enet_ingest_calls_scan, dim3(1), dim3(ENET_SCAN_TPB), 0, st, cnt_p, cnt_m, skip, V, lo, hi, mm, dest, kept_idx, kept_p, kept_m, n_kept);
    return hipGetLastError();
}
hipError_t shk_enet_ingest_calls_scatter(hipStream_t st, const uint64_t *pres, const uint64_t *miss, int64_t V, int NW, int N, const int32_t *cnt_p,
                                         const int32_t *cnt_m, const int32_t *dest, uint64_t *dst)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_enet_ingest_calls_scatter, dim3((unsigned)((V + ENET_WAVES - 1) / ENET_WAVES)), dim3(ENET_TPB), 0, st, pres, miss, V, NW, N, cnt_p, cnt_m,
                       dest, dst);
    return hipGetLastError();
}
hipError_t shk_enet_moments(hipStream_t st, const uint64_t *B, int64_t P, int NW, int N, const double *yc, double sum_b2, double *out)
{
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_enet_moments, dim3((unsigned)((P + ENET_WAVES - 1) / ENET_WAVES)), dim3(ENET_TPB), 0, st, B, P, NW, N, yc, sum_b2, out);
    return hipGetLastError();
}
hipError_t shk_enet_grad(hipStream_t st, const uint64_t *B, int64_t P, int NW, const double *V, int64_t ldv, int nf, double *G, int64_t ldg)
{
    if (P <= 0 || nf <= 0) return hipSuccess;
    if (nf > 16) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((P + ENET_WAVES - 1) / ENET_WAVES)), block(ENET_TPB);
    if (nf <= 4) hipLaunchKernelGGL(k_enet_grad<4>, grid, block, 0, st, B, P, NW, V, ldv, nf, G, ldg);
    else hipLaunchKernelGGL(k_enet_grad<16>, grid, block, 0, st, B, P, NW, V, ldv, nf, G, ldg);
    return hipGetLastError();
}
// bytes of LDS k_enet_cd needs to keep the state of one problem on the CU; the caller compares it with the device's limit
size_t shk_enet_cd_lds_bytes(int NW, int family) { return (size_t)(64 + (family == 1 ? 3 : 2) * NW * 64) * sizeof(double); }
hipError_t shk_enet_cd(hipStream_t st, const EnetCdArgs *a, int n_problems)
{
    size_t lds = 64 * sizeof(double);
    if (a->use_lds) {
        lds = shk_enet_cd_lds_bytes(a->NW, a->family);
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_enet_cd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_enet_cd, dim3(n_problems), dim3(ENET_TPB), lds, st, *a);
    return hipGetLastError();
}
}
