// lm_batch.hip -- batched Levenberg-Marquardt for the small curve-fit objectives (gfx950).
//
// Many independent ExpCurve (n = 3) / Cubic (n = 4) fits in one launch: one lane owns one problem
// and runs that problem's whole LevMarq::findMin (LevenbergMarquardt.cpp:11-167), every
// statement in the reference's operation order, so a problem's result does not depend on the
// batch it is solved in and (no transcendental: Cubic) equals the CPU path bit for bit.
//
// No Jacobian is stored.  Per loop trip:
//   pass A  rows l ascending: r0 = F_l(X), r_j = F_l(X + h e_j), J_l[j] = (r_j - r0) / h,
//           S[i][j] += J_l[i] J_l[j] (i <= j: the product commutes, so the upper triangle is
//           bitwise the reference's full J^T J), g[i] += J_l[i] r0
//   solve   A = S, A_ii = (1 + lambda) S_ii, rhs = -g, luSolve's partial-pivot elimination and
//           back substitution fully unrolled (pivot swap by selects: nothing is indexed at run
//           time, so everything stays in registers)
//   pass B  chi^2 of X + sigma, rows ascending; accept / reject, lambda update, stop test
// F(X) is never kept: the same X gives the same bits when it is needed again.
//
// yData is [nprob][m]: a lane walking its own row is a strided access across the wave, so the
// 64-lane workgroup stages a 64-problem x R-row block through LDS (128-byte segments per problem
// on the global side, an odd row stride on the LDS side) and each lane reads its own row there;
// per-problem x grids and their cube tables are staged the same way, a shared grid is read at a
// wave-uniform address.  Small problems are staged once and stay resident for the whole solve
// (kLmbResident); larger ones are re-staged in kLmbRows-row chunks, twice per trip, from L2.
#include "../pnol_env.hpp"
#include "lane_batch.hpp"
#include "multi_residual.hpp"

#include <cstdlib>

namespace pnol {
namespace {

constexpr int kLmbRows = 32;   // data rows staged per chunk
// Rows stay resident in LDS for the whole solve when that takes at most this much of it: the
// footprint of the measured case (m = 100 on a shared grid: 64 x 101 doubles, three waves per
// CU), which took 12-18% less time than re-staging 32-row chunks twice per trip
// (profiles/lm_batch_probe.json).  Larger footprints, not measured, are staged in chunks.
constexpr size_t kLmbResident = 52 * 1024;

template <int KIND>
struct LmbDim {
    static constexpr int n = KIND == PNOL_OBJ_EXPCURVE ? 3 : 4;
};

// rows [c0, c0 + len) of the 64 problems from p0 on: dst[q * stride + r] = src[(p0 + q) * m + c0 + r]
// (zero for problems past the batch).  16 lanes cover 128 contiguous bytes of one problem.
__device__ __forceinline__ void lmb_stage(double* __restrict__ dst, const double* __restrict__ src, size_t p0,
                                          size_t nprob, int m, int c0, int len, int stride) {
    const int sub = threadIdx.x & 15, qq = threadIdx.x >> 4;
    for (int q = qq; q < kLaneBatchLanes; q += 4) {
        const size_t p = p0 + q;
        const bool in = p < nprob;
        const double* s = src + (in ? p * (size_t)m + c0 : 0);
        for (int r = sub; r < len; r += 16) dst[q * stride + r] = in ? s[r] : 0.0;
    }
}

// PERX: per-problem x grids (xg / p3g hold nprob * m values), else one shared grid of m.
template <int KIND, bool PERX>
__global__ __launch_bounds__(kLaneBatchLanes) void k_lm_batch(
    const double* __restrict__ xg, const double* __restrict__ p3g, const double* __restrict__ yg, int m, size_t nprob,
    int R, int stride, double lambda0, double factor, double h, int maxIter, double xMinDiff,
    double* __restrict__ Xio, double* __restrict__ chi0, double* __restrict__ chi, int* __restrict__ iters,
    long long* __restrict__ evals, double* __restrict__ F0, double* __restrict__ FOpt) {
    constexpr int N = LmbDim<KIND>::n;
    constexpr bool kCubic = KIND == PNOL_OBJ_CUBIC;
    if (R < 1) return;   // the row loops step by R (the launcher never passes less; uniform)
    extern __shared__ double lmb_lds[];
    double* ys = lmb_lds;
    double* xs = ys + kLaneBatchLanes * stride;    // PERX only
    double* ps = xs + kLaneBatchLanes * stride;    // PERX && Cubic only
    const int lane = threadIdx.x;
    const size_t p0 = (size_t)blockIdx.x * kLaneBatchLanes, p = p0 + lane;
    const bool valid = p < nprob;
    const bool resident = R >= m;   // one chunk: staged once, kept for the whole solve

    auto stage = [&](int c0, int len) {
        lmb_stage(ys, yg, p0, nprob, m, c0, len, stride);
        if (PERX) {
            lmb_stage(xs, xg, p0, nprob, m, c0, len, stride);
            if (kCubic) lmb_stage(ps, p3g, p0, nprob, m, c0, len, stride);
        }
    };
    // fn(row, x, y, aux3) for every data row ascending on the lanes with act set; the staging
    // and its barriers are outside the lane predicate (the loop bounds are wave-uniform)
    auto for_rows = [&](bool act, auto&& fn) {
        for (int c0 = 0; c0 < m; c0 += R) {
            const int len = min(R, m - c0);
            if (!resident) {
                __syncthreads();
                stage(c0, len);
                __syncthreads();
            }
            if (act) {
                const double* yl = ys + lane * stride;
                const double* xl = xs + lane * stride;
                const double* pl = ps + lane * stride;
                for (int r = 0; r < len; ++r) {
                    const double xv = PERX ? xl[r] : xg[c0 + r];
                    const double a3 = kCubic ? (PERX ? pl[r] : p3g[c0 + r]) : 0.0;
                    fn(c0 + r, xv, yl[r], a3);
                }
            }
        }
    };
    if (resident) {
        stage(0, m);
        __syncthreads();
    }

    double X[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < N; ++i) X[i] = valid ? Xio[p * N + i] : 0.0;

    // F0 = F(x0), chiSq = pow(vector2Norm(F0), 2)  (LevenbergMarquardt.cpp:33-41)
    double s0 = 0.0;
    for_rows(valid, [&](int row, double xv, double yv, double a3) {
        const double aux = kCubic ? a3 : exp(X[1] * xv);
        const double r = multi_residual_row<KIND>(X, xv, yv, aux);
        if (F0) F0[p * (size_t)m + row] = r;
        s0 = s0 + r * r;
    });
    double nrm = sqrt(s0);
    double chiSq = nrm * nrm;
    const double chiStart = chiSq;
    double lambda = lambda0;
    int iter = 0;
    long long trips = 0;
    bool active = valid && iter < maxIter;

    while (__any(active)) {
        // ---- pass A: J^T J (upper triangle) and J^T F, row by row
        double S[N][N], g[N], Xp[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            g[i] = 0.0;
            Xp[i] = X[i] + h;   // XdX[j] = X[j] + dX[j]
#pragma unroll
            for (int j = 0; j < N; ++j) S[i][j] = 0.0;
        }
        for_rows(active, [&](int, double xv, double yv, double a3) {
            double r0, J[N];
            if (kCubic) {
                r0 = multi_residual_row<KIND>(X, xv, yv, a3);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double Xj[4] = {X[0], X[1], X[2], X[3]};
                    Xj[j] = Xp[j];
                    J[j] = (multi_residual_row<KIND>(Xj, xv, yv, a3) - r0) / h;
                }
            } else {
                // exp(X[1] x) serves the base point and the X[0], X[2] columns (the same bits)
                const double E = exp(X[1] * xv), E1 = exp(Xp[1] * xv);
                r0 = multi_residual_row<KIND>(X, xv, yv, E);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double Xj[4] = {X[0], X[1], X[2], X[3]};
                    Xj[j] = Xp[j];
                    J[j] = (multi_residual_row<KIND>(Xj, xv, yv, j == 1 ? E1 : E) - r0) / h;
                }
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
#pragma unroll
                for (int j = i; j < N; ++j) S[i][j] = S[i][j] + J[i] * J[j];
                g[i] = g[i] + J[i] * r0;
            }
        });

        // ---- sigma = luSolve(A, -J^T F)  (LevenbergMarquardt.cpp:63-83, luSolve's operation order)
        double A[N][N], b[N], sigma[N], Xt[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j < N; ++j) A[i][j] = i <= j ? S[i][j] : S[j][i];
            A[i][i] = (1 + lambda) * S[i][i];
            b[i] = -g[i];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            // the first strictly greater |A_ik|, i > k
            int piv = k;
            double best = fabs(A[k][k]);
#pragma unroll
            for (int i = k + 1; i < N; ++i) {
                const double v = fabs(A[i][k]);
                const bool gt = v > best;
                best = gt ? v : best;
                piv = gt ? i : piv;
            }
            // rows k and piv change places (columns < k are never read again)
#pragma unroll
            for (int i = k + 1; i < N; ++i) {
                const bool sw = piv == i;
#pragma unroll
                for (int j = k; j < N; ++j) {
                    const double t = A[k][j];
                    A[k][j] = sw ? A[i][j] : t;
                    A[i][j] = sw ? t : A[i][j];
                }
                const double t = b[k];
                b[k] = sw ? b[i] : t;
                b[i] = sw ? t : b[i];
            }
            const double akk = A[k][k];
#pragma unroll
            for (int i = k + 1; i < N; ++i) {
                const double f = A[i][k] / akk;
#pragma unroll
                for (int j = k + 1; j < N; ++j) A[i][j] = A[i][j] - f * A[k][j];
                b[i] = b[i] - f * b[k];
            }
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            double s = b[i];
#pragma unroll
            for (int j = i + 1; j < N; ++j) s = s - A[i][j] * sigma[j];
            sigma[i] = s / A[i][i];
        }
        double XtF[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < N; ++i) {
            Xt[i] = X[i] + sigma[i];
            XtF[i] = Xt[i];
        }

        // ---- pass B: chi^2 of the trial point
        double s1 = 0.0;
        for_rows(active, [&](int, double xv, double yv, double a3) {
            const double aux = kCubic ? a3 : exp(XtF[1] * xv);
            const double r = multi_residual_row<KIND>(XtF, xv, yv, aux);
            s1 = s1 + r * r;
        });

        if (active) {
            ++trips;
            nrm = sqrt(s1);
            const double c = nrm * nrm;
            bool stop = false;
            if (c >= chiSq || c != c) {
                lambda = lambda * factor;   // X, F and chiSq stand
            } else {
                chiSq = c;
#pragma unroll
                for (int i = 0; i < N; ++i) X[i] = Xt[i];
                lambda = lambda / factor;
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i) d = d + sigma[i] * sigma[i];
                stop = sqrt(d) < xMinDiff;
            }
            if (!stop) ++iter;
            active = !stop && iter < maxIter;
        }
    }

    // FOpt = F(X): recomputed, the same bits the loop saw
    if (FOpt)
        for_rows(valid, [&](int row, double xv, double yv, double a3) {
            const double aux = kCubic ? a3 : exp(X[1] * xv);
            FOpt[p * (size_t)m + row] = multi_residual_row<KIND>(X, xv, yv, aux);
        });
    if (valid) {
#pragma unroll
        for (int i = 0; i < N; ++i) Xio[p * N + i] = X[i];
        chi0[p] = chiStart;
        chi[p] = chiSq;
        iters[p] = iter;
        evals[p] = 1 + trips * (N + 2);   // F0, then per trip the Jacobian's n + 1 points and the trial point
    }
}

// PNOL_LMB_ROWS (tuning): a positive value fixes the rows per staged chunk (>= m: all resident)
bool lmb_rows_set() { return env_atoi("PNOL_LMB_ROWS", 0) > 0; }
int lmb_rows_env() { return lmb_rows_set() ? env_atoi("PNOL_LMB_ROWS", 0) : kLmbRows; }

template <int KIND, bool PERX>
int lmb_launch(pnol_ctx* ctx, const pnol_lm_batch* b, const double* y, const double* prm, double* X, double* chi0,
               double* chi, int* iters, long long* evals, double* F0, double* FOpt) {
    const int narr = 1 + (PERX ? (KIND == PNOL_OBJ_CUBIC ? 2 : 1) : 0);
    auto lds_bytes = [&](int rows) { return sizeof(double) * (size_t)narr * kLaneBatchLanes * (size_t)(rows | 1); };
    // all m rows resident when they fit kLmbResident of LDS, else kLmbRows-row chunks; a
    // PNOL_LMB_ROWS chunk that would not fit the CU's LDS is not taken
    const int want = lmb_rows_env();   // >= 1: the environment's chunk or kLmbRows
    int R = lmb_rows_set() ? want : (lds_bytes(b->m) <= kLmbResident ? b->m : kLmbRows);
    R = std::min(R, b->m);
    if (lds_bytes(R) > kLaneBatchLdsMax) R = std::min(kLmbRows, b->m);
    if (R < 1 || b->m < 1) return PNOL_ERR_ARG;   // the kernel's row loops step by R
    return lane_batch_launch(ctx, "lm_batch", &k_lm_batch<KIND, PERX>, b->nprob, lds_bytes(R), (const double*)b->x,
                             (const double*)b->p3, y, b->m, b->nprob, R, R | 1, prm[0], prm[1], prm[2], (int)prm[3],
                             prm[4], X, chi0, chi, iters, evals, F0, FOpt);
}

}  // namespace

int launch_lm_batch(pnol_ctx* ctx, const pnol_lm_batch* b, const double* y, const double* params, double* X,
                    double* chi0, double* chi, int* iters, long long* evals, double* F0, double* FOpt) {
    if (!ctx || !b || !y || !params || !X || !chi0 || !chi || !iters || !evals) return PNOL_ERR_ARG;
    if (b->nprob == 0) return PNOL_ERR_ARG;
    const bool px = b->per_problem_x;
    if (b->kind == PNOL_OBJ_EXPCURVE)
        return px ? lmb_launch<PNOL_OBJ_EXPCURVE, true>(ctx, b, y, params, X, chi0, chi, iters, evals, F0, FOpt)
                  : lmb_launch<PNOL_OBJ_EXPCURVE, false>(ctx, b, y, params, X, chi0, chi, iters, evals, F0, FOpt);
    if (b->kind == PNOL_OBJ_CUBIC)
        return px ? lmb_launch<PNOL_OBJ_CUBIC, true>(ctx, b, y, params, X, chi0, chi, iters, evals, F0, FOpt)
                  : lmb_launch<PNOL_OBJ_CUBIC, false>(ctx, b, y, params, X, chi0, chi, iters, evals, F0, FOpt);
    return PNOL_ERR_UNSUPPORTED;
}

}  // namespace pnol
