// scalar_terms.hpp -- term k of the built-in scalar objectives (Rosenbrock, Power, the synthetic
// quadratic), the one definition every kernel that evaluates them compiles (fd.hip: the FD
// gradient's term form; simplex_batch.hip and bfgs_batch.hip: one lane per search, through
// lane_batch.hpp's lane_eval).  f = sum_k t_k accumulated in k
// order is the objective's own sequential sum; plain + and * in the objective's operation order
// and -ffp-contract=off, so the same point gives the same bits in every kernel and on the host
// (host/scalar_host.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "pnol_amd.h"

namespace pnol {

template <int KIND>
__device__ __forceinline__ int scalar_nterms(int n) { return KIND == PNOL_OBJ_ROSENBROCK ? max(n - 1, 0) : n; }

// term k at the point whose coordinates k, k + 1 are xk, xk1 (the objective's own expression)
template <int KIND>
__device__ __forceinline__ double scalar_term(int k, int n, double xk, double xk1, const double* __restrict__ p0,
                                              const double* __restrict__ p1, double power) {
    if (KIND == PNOL_OBJ_ROSENBROCK) {
        const double t = xk1 - xk * xk, u = 1.0 - xk;   // ExampleObjectives.hpp:93-96
        return 100.0 * (t * t) + u * u;
    } else if (KIND == PNOL_OBJ_QUADRATIC) {
        double t = (0.5 * p0[k] * xk) * xk - p1[k] * xk;
        if (k + 1 < n) t = t + (0.25 * xk) * xk1;
        return t;
    } else {
        return power == 2.0 ? xk * xk : pow(xk, power);
    }
}

}  // namespace pnol
