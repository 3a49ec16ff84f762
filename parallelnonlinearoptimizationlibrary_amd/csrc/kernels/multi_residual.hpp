// multi_residual.hpp -- the residual of the small curve-fit objectives (ExpCurve, Cubic), the
// one definition every kernel that evaluates them compiles (fd.hip: one thread per (point,
// residual); lm_batch.hip: one lane per problem).  Plain + and * in the objective's own order;
// the build has -ffp-contract=off, so the same X and data give the same bits in every kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "pnol_amd.h"

namespace pnol {

// Residual of one data row (xv, yv).  aux: exp(X[1] * xv) for ExpCurve -- the caller forms it, so
// points that share X[1] share it -- and the host-tabulated pow(xv, 3.0) for Cubic.
template <int KIND>
__device__ __forceinline__ double multi_residual_row(const double* X, double xv, double yv, double aux) {
    if (KIND == PNOL_OBJ_EXPCURVE) {
        double func = X[0] * aux + X[2];                        // ExampleObjectives.hpp:128
        return yv - func;
    } else {
        double func = X[0] * aux + X[1] * (xv * xv) + X[2] * xv + X[3];   // :175, pow(x,3) tabulated
        return yv - func;
    }
}

template <int KIND>
__device__ __forceinline__ double multi_residual(const double* X, int k, const double* xd, const double* yd,
                                                 const double* p3) {
    if (KIND == PNOL_OBJ_EXPCURVE) return multi_residual_row<KIND>(X, xd[k], yd[k], exp(X[1] * xd[k]));
    return multi_residual_row<KIND>(X, xd[k], yd[k], p3[k]);
}

}  // namespace pnol
