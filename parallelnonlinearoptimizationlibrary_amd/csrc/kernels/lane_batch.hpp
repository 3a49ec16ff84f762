// lane_batch.hpp -- what the "one lane per problem, whole algorithm in one launch" kernels share
// (lm_batch.hip, simplex_batch.hip, bfgs_batch.hip): the lane count, the LDS budget their sizes
// are bounded by, the launch tail, and for the two scalar-objective solvers the objective's
// sequential sum over a lane-minor LDS point, the objective check and the kind dispatch.  The
// kernels' state machines and LDS layouts are their own.
#pragma once

#include <type_traits>

#include "../pnol_internal.hpp"
#include "scalar_terms.hpp"

namespace pnol {

constexpr int kLaneBatchLanes = 64;                // problems per workgroup: one wave
constexpr size_t kLaneBatchLdsMax = 160 * 1024;    // LDS of one CU

// f at the point in the n slots from xs on (stride kLaneBatchLanes): the objective's sequential sum
template <int KIND>
__device__ __forceinline__ double lane_eval(const double* xs, int n, const double* __restrict__ p0,
                                            const double* __restrict__ p1, double power) {
    const int nt = scalar_nterms<KIND>(n);
    double f = 0.0;
    double xk = xs[0];
    for (int k = 0; k < nt; ++k) {
        const double xk1 = k + 1 < n ? xs[(k + 1) * kLaneBatchLanes] : 0.0;
        f = f + scalar_term<KIND>(k, n, xk, xk1, p0, p1, power);
        xk = xk1;
    }
    return f;
}

// The launch tail: `count` items on 64-lane workgroups with `lds` bytes of dynamic LDS (the limit
// is raised only above the 64 KB every kernel has) on the context stream, timed under `timer`
template <typename Kernel, typename... Args>
int lane_batch_launch(pnol_ctx* ctx, const char* timer, Kernel kern, size_t count, size_t lds, Args... args) {
    const size_t blocks = (count + kLaneBatchLanes - 1) / kLaneBatchLanes;
    if (blocks > 0x7fffffffull) return PNOL_ERR_ARG;
    if (lds > 64 * 1024)
        PNOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    ScopedTimer tm(ctx, timer);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kLaneBatchLanes), lds, ctx->stream, args...);
    return launch_check();
}

// the objective of a scalar-objective batch: there, 1 <= n <= nmax, a quadratic's data n long
inline int scalar_batch_check(const pnol_dobj* o, int nmax) {
    if (!o || o->n < 1) return PNOL_ERR_ARG;
    if (o->n > nmax) return PNOL_ERR_UNSUPPORTED;
    if (o->kind == PNOL_OBJ_QUADRATIC && (o->len0 < (size_t)o->n || o->len1 < (size_t)o->n)) return PNOL_ERR_ARG;
    return PNOL_OK;
}

// f(std::integral_constant<int, KIND>) for the scalar kind `kind`
template <typename F>
int scalar_batch_dispatch(int kind, F&& f) {
    switch (kind) {
        case PNOL_OBJ_ROSENBROCK: return f(std::integral_constant<int, PNOL_OBJ_ROSENBROCK>{});
        case PNOL_OBJ_POWER: return f(std::integral_constant<int, PNOL_OBJ_POWER>{});
        case PNOL_OBJ_QUADRATIC: return f(std::integral_constant<int, PNOL_OBJ_QUADRATIC>{});
        default: return PNOL_ERR_UNSUPPORTED;
    }
}

}  // namespace pnol
