// lane_batch.hpp -- what the "one lane per problem, whole algorithm in one launch" kernels share
// (lm_batch.hip, simplex_batch.hip, bfgs_batch.hip, bfgs_bnd_batch.hip): the lane count, the LDS
// budget their sizes are bounded by, the launch tail, for the scalar-objective solvers the
// objective's sequential sum over a lane-minor LDS point, the objective check and the kind
// dispatch, and for the two BFGS solvers the exact inverse-Hessian update and the direction.  The
// kernels' state machines and LDS layouts are their own.
// ga_batch.hip (one wave per run, not one lane per problem) uses lane_eval, the objective check, the
// kind dispatch and the workgroup-count form of the launch tail.
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

// updateHessianInv (BFGS_with_linesearch.cpp:389-432) of one lane, exact and in place:
// D <- M1 D M2 + M3 with M1 = I - rho s y^T, M2 = I - rho y s^T, M3 = rho s s^T, rho = 1 / (y . s).
// D is n x n row-major, s, y and tmp n slots each, all lane-minor (stride kLaneBatchLanes).  Column
// j of M1 D needs only column j of D, and row i of (M1 D) M2 only row i of M1 D, so both products
// go through the n-slot temporary with the per-entry sums of the two GEMMs (l ascending from 0.0,
// then + M3); the entries of M1, M2, M3 are recomputed where used.
__device__ __forceinline__ void lane_bfgs_update(double* D, const double* s, const double* y, double* tmp, int n) {
    double ys = 0.0;
    for (int i = 0; i < n; ++i) ys = ys + y[i * kLaneBatchLanes] * s[i * kLaneBatchLanes];
    const double rho = 1 / ys;
    for (int j = 0; j < n; ++j) {          // column j of M1 D
        for (int i = 0; i < n; ++i) {
            const double rs = rho * s[i * kLaneBatchLanes];
            double acc = 0.0;
            for (int l = 0; l < n; ++l) {
                const double e = i == l ? 1.0 : 0.0;
                acc = acc + (e - rs * y[l * kLaneBatchLanes]) * D[(l * n + j) * kLaneBatchLanes];
            }
            tmp[i * kLaneBatchLanes] = acc;
        }
        for (int i = 0; i < n; ++i) D[(i * n + j) * kLaneBatchLanes] = tmp[i * kLaneBatchLanes];
    }
    for (int i = 0; i < n; ++i) {          // row i of (M1 D) M2, + M3
        for (int j = 0; j < n; ++j) {
            const double sj = s[j * kLaneBatchLanes];
            double acc = 0.0;
            for (int l = 0; l < n; ++l) {
                const double e = l == j ? 1.0 : 0.0;
                acc = acc + D[(i * n + l) * kLaneBatchLanes] * (e - rho * y[l * kLaneBatchLanes] * sj);
            }
            tmp[j * kLaneBatchLanes] = acc;
        }
        const double rs = rho * s[i * kLaneBatchLanes];
        for (int j = 0; j < n; ++j)
            D[(i * n + j) * kLaneBatchLanes] = tmp[j * kLaneBatchLanes] + rs * s[j * kLaneBatchLanes];
    }
}

// p = -D g of one lane (BFGS_with_linesearch.cpp:52-56): row sums over j ascending from 0.0
__device__ __forceinline__ void lane_bfgs_direction(const double* D, const double* g, double* p, int n) {
    for (int i = 0; i < n; ++i) {
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc = acc + D[(i * n + j) * kLaneBatchLanes] * g[j * kLaneBatchLanes];
        p[i * kLaneBatchLanes] = -acc;
    }
}

// The launch tail: `blocks` 64-lane workgroups with `lds` bytes of dynamic LDS (the limit is
// raised only above the 64 KB every kernel has) on the context stream, timed under `timer`
template <typename Kernel, typename... Args>
int wave_batch_launch(pnol_ctx* ctx, const char* timer, Kernel kern, size_t blocks, size_t lds, Args... args) {
    if (blocks > 0x7fffffffull) return PNOL_ERR_ARG;
    if (lds > 64 * 1024)
        PNOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    ScopedTimer tm(ctx, timer);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kLaneBatchLanes), lds, ctx->stream, args...);
    return launch_check();
}
// the one-lane-per-problem form: `count` problems, 64 to a workgroup
template <typename Kernel, typename... Args>
int lane_batch_launch(pnol_ctx* ctx, const char* timer, Kernel kern, size_t count, size_t lds, Args... args) {
    return wave_batch_launch(ctx, timer, kern, (count + kLaneBatchLanes - 1) / kLaneBatchLanes, lds, args...);
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
