// lmm_params.h -- structures passed by value between the host side (api.hip) and the LMM kernel launchers (lmm_kernels.hip)
#pragma once

struct LmmLinOut {              // per-variant outputs of the linear-terms kernel, Vpad each (of the row AS STORED, i.e. complemented when flip[v])
    int *t11, *t01, *m;
    double *xky, *dg, *rss, *s1, *q1;
    const unsigned char *flip;  // 1 = the row was stored complemented (k_repack_bits), or null
};

struct LmmFinParams {
    int N, D, continuous;
    int n1, n0;                 // #(y == 1), #(y == 0)   (binary prefilter margins)
    double yc_sum, yc_sq;       // sum / sum of squares of the centred phenotype (Welch, group 0 by subtraction)
    double yKy, inv_scale;
    double pret, lrtt;
    double min_af, max_af; int af_on;
    double sumv;                // sum_i v_i (= 0 up to rounding when the intercept is in the covariate span): x.v of a complemented row
    // a-posteriori bound of the fixed-point contraction: |x^T (G - Gq/s) x| <= err_norm * m', m' = carriers of the row as stored
    double err_norm;            // spectral norm of the symmetrised quantisation error of the main-pass limbs, in units of G
    double tol;                 // relative bound on xKx above which a variant is re-contracted with the extra limbs (0 = never)
    double inv_scale_low;       // 1 / scale of the extra (low) limbs
};

struct LmmRefine {              // device-side work list of the variants whose bound exceeds tol
    int *list, *count;          // variant indices, number of entries
    unsigned long long *bound_max;   // max over the batch of the final relative bound (bit pattern of a non-negative double)
};

// The ragged row tile.  N = 128 nf + r: when 1 <= r <= LMM_RAGGED_MAX (and nf >= 3, so that k_lmm_quadform_i8w still walks the
// three segments its DMA cursor needs), the r rows behind the last full 128-row tile are contracted by k_lmm_ragged_i8 from a compact image of
// their limbs -- limb l, row s at stacked row l * rp + s, rp = r rounded up to 8 -- in `mt` MFMA row tiles of 32 (even when more than one: the
// kernel takes them two at a time) against the nsb = 2 nf + 1 sample blocks of 64 that hold a column j < i.
#ifndef LMM_RAGGED_MAX
#define LMM_RAGGED_MAX 8              // the case sized in DESIGN.md 5.1; the threshold itself is still to be measured (profiles/README.md, r07)
#endif
struct LmmRagged { int nf, r, rp, mt, nsb; };
static inline bool lmm_ragged_shape(int N, int L, LmmRagged *g)
{
    g->nf = N / 128; g->r = N % 128; g->rp = (g->r + 7) & ~7; g->nsb = 2 * g->nf + 1;
    g->mt = (L * g->rp + 31) / 32; if (g->mt > 1) g->mt = (g->mt + 1) & ~1;
    return g->r >= 1 && g->r <= LMM_RAGGED_MAX && g->nf >= 3;
}
static inline size_t lmm_ragged_bytes(const LmmRagged &g) { return (size_t)g.mt * g.nsb * 2048; }
