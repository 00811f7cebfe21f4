// glm_api.inc -- GLM state held in sh_ctx (included by api.hip before sh_ctx is defined)
#include "glm_params.h"
extern "C" hipError_t shk_glm_launch(hipStream_t, int, int, const uint64_t *, int64_t, int64_t, const double *, const double *, const float *,
                                     const uint64_t *, const uint64_t *, const double *, const double *, const double *, GlmParams,
                                     double *, uint32_t *, int *, int *, int *, int *, double *, int *, int *, int *, int *, int *);
extern "C" int64_t shk_bitdot_i8_table_bytes(int NE, int NB64);
extern "C" void shk_bitdot_i8_digits(const double *vals, int N, int NE, int NB64, int8_t *atab, double *scale);
extern "C" hipError_t shk_glm_ols_tab(hipStream_t, int, int, const uint64_t *, int64_t, int64_t, const double *, const double *, const double *,
                                      double *, const double *, const double *, GlmParams, double, double, double *, uint32_t *, int *, int *);
extern "C" hipError_t shk_glm_wide(hipStream_t, int, int, const uint64_t *, int64_t, int64_t, const double *, const double *, const uint64_t *,
                                   const uint64_t *, const double *, GlmParams, double *, uint32_t *, int *, int *, int *, int *, int *, int *);
extern "C" hipError_t shk_glm_wide_lineage(hipStream_t, const uint64_t *, int64_t, int64_t, int, int, const double *, int, int, int *, LinList);
extern "C" int shk_firth_state_doubles(int Q);
extern "C" hipError_t shk_firth_launch(hipStream_t, int, int, int64_t, const uint64_t *, int64_t, int64_t, const double *, const double *, GlmParams,
                                       double *, int *, int *, int *, int64_t, const int *, const int *, int *, int *, int *, int *, double *,
                                       uint32_t *, int *, int *, int *, int *);
extern "C" hipError_t shk_firth2_launch(hipStream_t, int, int, int64_t, const uint64_t *, int64_t, int64_t, GlmParams, double *, int *, int *, int *, int64_t,
                                        const int *, const int *, int *, int *, int *, int *, double *, uint32_t *, int *, int *, int *, int *, int *, int *);
extern "C" int shk_firth_fast_supported(int Q);
extern "C" int shk_firth_fast_tiles(int Q, int *t2, int *t3, int *rs);
extern "C" int shk_firth_fast_row2(int Q, int a, int b);
extern "C" hipError_t shk_firth_fast_launch(hipStream_t, int, int64_t, const uint64_t *, int64_t, GlmParams, double *, int *, int *, int *, int64_t,
                                            const int *, const int *, int *, int *, int *, int *, int64_t, double *, uint32_t *);
extern "C" int shk_firth_fastw_layout(int Q, int *t2h, int *t3h, int *rs, int *rows);
extern "C" hipError_t shk_firth_fastw_launch(hipStream_t, int, int64_t, const uint64_t *, int64_t, GlmParams, double *, int *, int *, int *, int64_t,
                                             const int *, const int *, int *, int *, int *, int *, const uint16_t *, const float *, float *, int64_t);
extern "C" hipError_t shk_glm_lineage(hipStream_t, int, const uint64_t *, int64_t, int64_t, int, int, const double *, int, int *, LinList);
extern "C" hipError_t shk_glm_lineage_counts(hipStream_t, const uint64_t *, int64_t, int64_t, int, int, const uint16_t *, const int *, int, int *, LinList);
struct GlmState {
    bool ready = false;
    int q = 0;
    GlmParams P{};
    double *d_Ws = nullptr, *d_wstd = nullptr; float *d_Wf = nullptr, *d_zz = nullptr; uint16_t *d_zz16 = nullptr, *d_zl16 = nullptr; double *d_olstab = nullptr; double ymean = 0, yty = 0; int ols_tab = 1;
    double *d_y = nullptr, *d_W = nullptr, *d_yc = nullptr, *d_ZtZ = nullptr, *d_Zty = nullptr;
    uint64_t *d_y1 = nullptr, *d_y0 = nullptr;
    double *d_Xlin = nullptr; int lin_pc = 0, lin_n = 0; int *d_lin_out = nullptr; int64_t cap_lin = 0;
    // the count route (k_glm_lineage_counts): every sample's cluster (0: the reference cluster, in no column) and the clusters' sizes [lin_n + 1]
    uint16_t *d_lin_cof = nullptr; int *d_lin_nc = nullptr; bool lin_by_counts = false;
    double *d_bw = nullptr; int *d_state = nullptr, *d_slist = nullptr; int bw_q = -1;
    int *d_flist = nullptr, *d_fcount = nullptr, *d_plist = nullptr; int64_t cap_list = 0;   // d_fcount[0] firth, [1] pinv, [2] slow-Newton
    // Firth state machine (k_firth_init/eval/step): per-slot state, the work lists (eval, next eval, step, hand-off, fp64 step), their counters [0..4]
    double *d_fst = nullptr; int *d_fmeta = nullptr, *d_fl[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *d_fcnt = nullptr; int64_t fcap = 0;
    int *d_dbg = nullptr;
    double *d_rec = nullptr;            // per-sample records of k_glm_score / k_glm_ll
    double *d_rec_o = nullptr;          // per-sample records of the Firth rounds (covariates as given)
    double *d_rec_f = nullptr; float *d_rec_pf = nullptr;   // firth_rounds.hip: (covariates as given, 1 - 2y) per sample; standardised covariates per pair of samples
    uint16_t *d_ff_tab = nullptr; double *d_ff_rec = nullptr, *d_ff_inull = nullptr;   // firth_fast.hip: monomial tables (halves, hi / lo) and per-sample records
    float *d_pk = nullptr;              // pass32_pk tables: wfp [N/2][q][2], yf [N], w0f [N]
    int8_t *d_bdi8 = nullptr; double *d_bdscale = nullptr;   // bitdot_i8.hip: digit table and column scales
    double *d_b1 = nullptr;             // constants of the bordered first step (GlmParams.b1)
    double *d_chord = nullptr;          // chord-round workspaces (GlmParams.ch_*), sized with the lists
    double *d_w0 = nullptr, *d_a0 = nullptr;
    // firth_fast_w.hip (the single-precision first pass at two wavefronts per SIMD): its tables (16-row tiles, hi halves; compact fp32
    // records) and the hand-over workspace [rows][ffw_cap] between its sample pass and its per-fit kernel
    uint16_t *d_ffw_tab = nullptr; float *d_ffw_rec = nullptr, *d_ffw_ws = nullptr; int64_t ffw_cap = 0; int ffw_rows = 0;
    int ff_first32 = 2;                // one-pass Firth: the first passes in single precision (SEERHIP_ROUTE firth_first32, read at set-up)
    int *d_tile_list = nullptr;        // (a list argument of shk_glm_launch that no kernel uses any more)
};
// fit_lineage_effect of the rows in T on the route sh_lineage_setup chose
static hipError_t glm_lineage_launch(const GlmState &g, hipStream_t st, const uint64_t *T, int64_t Vpad, int64_t V, int N, int NB64, int *out, LinList L)
{
    if (g.lin_by_counts) return shk_glm_lineage_counts(st, T, Vpad, V, N, NB64, g.d_lin_cof, g.d_lin_nc, g.lin_n, out, L);
    if (g.lin_pc > 16) return shk_glm_wide_lineage(st, T, Vpad, V, N, NB64, g.d_Xlin, g.lin_pc, g.lin_n, out, L);
    return shk_glm_lineage(st, g.lin_pc, T, Vpad, V, N, NB64, g.d_Xlin, g.lin_n, out, L);
}
static void glm_free(GlmState *g)
{
    hipFree(g->d_Ws); hipFree(g->d_wstd); hipFree(g->d_Wf); hipFree(g->d_zz); hipFree(g->d_zz16); hipFree(g->d_zl16); hipFree(g->d_olstab); hipFree(g->d_y); hipFree(g->d_W); hipFree(g->d_yc); hipFree(g->d_ZtZ); hipFree(g->d_Zty); hipFree(g->d_y1); hipFree(g->d_y0);
    hipFree(g->d_bw); hipFree(g->d_state); hipFree(g->d_slist); hipFree(g->d_Xlin); hipFree(g->d_lin_out); hipFree(g->d_lin_cof); hipFree(g->d_lin_nc); hipFree(g->d_flist); hipFree(g->d_fcount); hipFree(g->d_plist);
    hipFree(g->d_fst); hipFree(g->d_fmeta); hipFree(g->d_fl[0]); hipFree(g->d_fl[1]); hipFree(g->d_fl[2]); hipFree(g->d_fl[3]); hipFree(g->d_fl[4]); hipFree(g->d_fcnt); hipFree(g->d_dbg); hipFree(g->d_tile_list); hipFree(g->d_w0); hipFree(g->d_a0); hipFree(g->d_bdi8); hipFree(g->d_bdscale); hipFree(g->d_chord); hipFree(g->d_b1); hipFree(g->d_pk); hipFree(g->d_rec); hipFree(g->d_rec_o); hipFree(g->d_rec_f); hipFree(g->d_rec_pf); hipFree(g->d_ff_tab); hipFree(g->d_ff_rec); hipFree(g->d_ff_inull); hipFree(g->d_ffw_tab); hipFree(g->d_ffw_rec); hipFree(g->d_ffw_ws);
    *g = GlmState();
}
