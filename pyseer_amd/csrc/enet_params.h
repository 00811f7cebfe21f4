// enet_params.h -- the argument block of k_enet_cd (enet_kernels.hip), shared with its caller (enet_api.inc).
#pragma once
#include <stdint.h>

struct EnetCdArgs {
    const uint64_t *B;            // P x NW words
    int64_t P; int N, NW, n_cov, family /* 0 gaussian, 1 binomial */, init, use_lds, max_sweeps, max_outer;
    double lambda, alpha;
    // per problem f (a stride of Np = 64 NW for per-sample vectors, P for per-row vectors, PT = n_cov + P for per-coordinate vectors)
    const double *y;              // [Np]
    const double *w, *hw;         // [F1][Np] training weights (sum 1); the full fit's weight of the samples this problem holds out
    const double *m, *sinv;       // [F1][P] weighted mean and 1 / sd of every row (sinv = 0: the row is constant in this problem and left out)
    const double *Xc;             // [F1][n_cov][Np] standardised dense columns
    const double *thr, *b0_null;  // [F1]
    const int *act, *nact;        // [F1][PT] ascending coordinates; [F1]
    const int *skip;              // [F1]
    double *beta, *bold, *xv;     // [F1][PT] slopes on the standardised scale; scratch
    double *state;                // [F1][3][Np]
    double *scal;                 // [F1][4]  o, b0, sum v r, sum v
    double *vr, *eta;             // [F1][Np]
    double *res;                  // [F1][8]  deviance, held-out deviance sum, sweeps, converged, last dlx, IRLS steps, sum vr, coordinate steps
};
