// bfgs_batch.hip -- batched BFGS: many independent Wolfe-line-search solves in one launch (gfx950).
//
// One lane owns one start and runs that start's whole BFGS::findMin (BFGS_with_linesearch.cpp:
// 12-432, host form: host/bfgs.cpp) with the exact update D <- M1 D M2 + M3, every statement in
// that order, so a start's result does not depend on the batch it is in and -- the built-in
// objectives being the sequential sum of scalar_term (scalar_terms.hpp) -- equals the one-problem
// class from the same X and parameters bit for bit (Power with power != 2 calls the device pow
// and is not bitwise against the host).  initHessFD is not offered: D starts as the identity.
//
// State.  D, the vectors and the trial point are indexed at run time, so they live in LDS,
// lane-minor: slot q of lane l is lds[q * 64 + l], an 8-byte access whose bank depends on the lane
// alone -- conflict-free whatever slot each lane picks -- and nothing goes to scratch.  Slots per
// lane:
//     [0, n n)     D, row-major
//     + n each     X, g, gprev (y = g - gprev during the update), p (s = alpha p during the
//                  update), the trial point, the n-slot temporary of the in-place products
// n^2 + 6 n doubles per lane: n = 12 -> 216 x 512 B = 108 KB, one workgroup per CU; n = 10 ->
// 80 KB; n <= 5 -> <= 28 KB.
//
// Update in place and direction: lane_bfgs_update and lane_bfgs_direction (lane_batch.hpp), shared
// with bfgs_bnd_batch.hip.
//
// Divergence.  Lanes sit in different phases (FD coordinate i, line-search trip, zoom trip).  A
// lane is a small state machine and the wave one loop with ONE objective call site: each lane
// that needs a value has its next point in its trial slots (the FD base, FD coordinate i, alpha,
// alpha + dalpha), all evaluate together, then each consumes the value by its state.  The other
// expensive part, update + direction (n^3), is one block too: a lane that has its gradient waits
// for it while any lane of the wave is still inside an FD gradient (lanes in a line search are
// not waited for), so lanes a few trips apart share one pass.  Each lane waited for arrives within
// n + 1 trips of entering its gradient, but other lanes may leave their line searches and enter
// one meanwhile; each of the 63 can do so once before it waits itself, so a wait ends within
// about 63 (n + 1) trips and cannot deadlock.  Waiting changes no lane's arithmetic, only when it
// runs (measured against a -DPNOL_BFGS_BATCH_NO_WAIT build: 1.2x at n = 2 to 3.2x at n = 10 on
// Rosenbrock, no difference on the quadratic; profiles/bfgs_batch_wait_ab.txt).  No cross-lane data, no
// cross-workgroup waiting; a lane's work is bounded by maxIter * (4 maxIterLineSearch + n + 2)
// evaluations.
#include "lane_batch.hpp"

namespace pnol {
namespace {

// doubles of LDS per lane
constexpr int bb_slots(int n) { return n * n + 6 * n; }
static_assert(sizeof(double) * bb_slots(PNOL_BFGS_BATCH_NMAX) * kLaneBatchLanes <= kLaneBatchLdsMax,
              "the largest problem's state must fit one CU's LDS");

// what a lane does with the next objective value (states before BB_STEP evaluate)
enum : int {
    BB_GBASE,    // FD gradient: the base value F(X)
    BB_GCOORD,   // FD gradient: F(X + dX e_i)
    BB_F0,       // the separate objEval(X) before the loop
    BB_LS_A,     // line search (outer or zoom): phi(alpha)
    BB_LS_B,     // line search: phi(alpha + dalpha), then the trip's decisions
    BB_STEP,     // has its gradient: update D, loop test, next direction
    BB_DONE
};

// cubicInterpMin (BFGS_with_linesearch.cpp:359-385); a zero bracket width and the NaN that
// follows are what IEEE gives, as on the host
__device__ __forceinline__ double bb_cubic(double alo, double ahi, double plo, double phi, double dlo, double dhi) {
    const double w = ahi - alo;
    const double sg = w > 0 ? 1.0 : (w < 0 ? -1.0 : 0.0);
    const double d1 = dlo + dhi - 3 * (plo - phi) / (alo - ahi);
    const double d2 = sg * sqrt(d1 * d1 - dlo * dhi);
    double an = ahi - (ahi - alo) * (dhi + d2 - d1) / (dhi - dlo + 2 * d2);
    if (alo < ahi) {
        if (an < alo) an = (ahi + alo) / 2;
    } else {
        if (an < ahi) an = (ahi + alo) / 2;
    }
    return an;
}

template <int KIND>
__global__ __launch_bounds__(kLaneBatchLanes) void k_bfgs_batch(
    int n, size_t nstart, const double* __restrict__ p0, const double* __restrict__ p1, double power, double c1,
    double c2, double dalpha, double alphaGuess, int maxIterLS, double dXGrad, int maxIter, double xMinDiff,
    double minGrad2Norm, double* __restrict__ Xio, double* __restrict__ f0out, double* __restrict__ fopt,
    double* __restrict__ gnout, int* __restrict__ iters, long long* __restrict__ evals) {
    extern __shared__ __attribute__((aligned(16))) double bb_lds[];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * kLaneBatchLanes + lane;
    const bool valid = s < nstart;
    double* const D = bb_lds + lane;               // D_ij at (i * n + j)
    double* const X = D + n * n * kLaneBatchLanes;
    double* const g = X + n * kLaneBatchLanes;
    double* const gp = g + n * kLaneBatchLanes;           // gprev; y inside the update
    double* const p = gp + n * kLaneBatchLanes;           // p; s inside the update
    double* const xt = p + n * kLaneBatchLanes;           // the point the next value is taken at
    double* const tmp = xt + n * kLaneBatchLanes;

    for (int j = 0; j < n; ++j) {
        const double x = valid ? Xio[s * (size_t)n + j] : 0.0;
        X[j * kLaneBatchLanes] = x;
        xt[j * kLaneBatchLanes] = x;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) D[(i * n + j) * kLaneBatchLanes] = i == j ? 1.0 : 0.0;

    int state = valid ? BB_GBASE : BB_DONE;
    bool first = true;    // the gradient in flight is the one before the loop (:40-45)
    bool zoom = false;    // the line search is inside lineSearchZoom
    int iter = 0, it = 0, ci = 0;
    long long ev = 0;
    double F = 0.0, f0 = 0.0, Fb = 0.0;
    double xdiff = xMinDiff * 2, gnorm = 2 * minGrad2Norm;
    double alpha = 0.0, Fopt = 0.0, phi0 = 0.0, dphi0 = 0.0;
    double ac = 0.0, pc = 0.0;                     // the trial step and phi there
    // the bracket of the zoom; in the outer search (alo, plo, dlo) are (aim1, pim1, dim1)
    double alo = 0.0, ahi = 0.0, plo = 0.0, phi = 0.0, dlo = 0.0, dhi = 0.0;

    while (__any(state != BB_DONE)) {
        double v = 0.0;
        if (state < BB_STEP) {
            v = lane_eval<KIND>(xt, n, p0, p1, power);
            ++ev;
        }
        bool lsDone = false;
        if (state == BB_GBASE) {
            // Objective::gradientApproximation (PNOL_Objective.cpp:12-34): the base value first
            Fb = v;
            ci = 0;
            xt[0] = X[0] + dXGrad;
            state = BB_GCOORD;
        } else if (state == BB_GCOORD) {
            g[ci * kLaneBatchLanes] = (v - Fb) / dXGrad;
            xt[ci * kLaneBatchLanes] = X[ci * kLaneBatchLanes];
            ++ci;
            if (ci < n) xt[ci * kLaneBatchLanes] = X[ci * kLaneBatchLanes] + dXGrad;
            else state = first ? BB_F0 : BB_STEP;
        } else if (state == BB_F0) {
            F = v;
            f0 = v;
            state = BB_STEP;
        } else if (state == BB_LS_A) {
            // lineSearchObj gave phi(ac); lineSearchFDDerivative's point (:160-174)
            pc = v;
            const double a2 = ac + dalpha;
            for (int i = 0; i < n; ++i) xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes] + a2 * p[i * kLaneBatchLanes];
            state = BB_LS_B;
        } else if (state == BB_LS_B) {
            const double dc = (v - pc) / dalpha;
            if (!zoom) {
                // cubicInterpolationLineSearch (:177-291), trip `it` at ai = ac
                if ((pc > phi0 + c1 * ac * dphi0) || (pc >= plo && it > 1)) {
                    ahi = ac; phi = pc; dhi = dc;                      // zoom(aim1, ai, ...)
                    zoom = true;
                    it = 0;
                } else if (fabs(dc) <= fabs(c2 * dphi0)) {
                    alpha = ac; Fopt = pc;
                    lsDone = true;
                } else if (dc >= 0) {
                    ahi = alo; phi = plo; dhi = dlo;                   // zoom(ai, aim1, ...)
                    alo = ac; plo = pc; dlo = dc;
                    zoom = true;
                    it = 0;
                } else {
                    alo = ac; plo = pc; dlo = dc;
                    ac = 2 * ac;
                    ++it;
                    if (it >= maxIterLS) lsDone = true;                // exhausted: alphaOpt = 0, Fopt = FX
                }
            } else {
                // lineSearchZoom (:296-356), trip `it` at aj = ac
                if (pc > phi0 + c1 * ac * dphi0 || pc >= plo) {
                    ahi = ac; phi = pc; dhi = dc;
                } else if (fabs(dc) <= fabs(c2 * dphi0)) {
                    alpha = ac; Fopt = pc;
                    lsDone = true;
                } else {
                    if (dc * (ahi - alo) >= 0) { ahi = alo; phi = plo; dhi = dlo; }
                    alo = ac; plo = pc; dlo = dc;
                }
                if (!lsDone) {
                    ++it;
                    if (it >= maxIterLS) lsDone = true;                // exhausted: alphaOpt = 0, Fopt = FX
                }
            }
            if (!lsDone) {
                if (zoom) ac = bb_cubic(alo, ahi, plo, phi, dlo, dhi);
                for (int i = 0; i < n; ++i)
                    xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes] + ac * p[i * kLaneBatchLanes];
                state = BB_LS_A;
            }
        }

        // update + loop test + direction, shared by the lanes that have their gradient (see top)
#ifdef PNOL_BFGS_BATCH_NO_WAIT   // A/B arm: a lane runs the block on the trip it gets its gradient
        const bool gradBusy = false;
#else
        const bool gradBusy = __any(state == BB_GBASE || state == BB_GCOORD);   // asked by the whole wave
#endif
        if (state == BB_STEP && !gradBusy) {
            if (!first) {
                // s = alpha p and y = g - gprev (:113-114); updateHessianInv (:389-432)
                for (int i = 0; i < n; ++i) {
                    p[i * kLaneBatchLanes] = alpha * p[i * kLaneBatchLanes];
                    gp[i * kLaneBatchLanes] = g[i * kLaneBatchLanes] - gp[i * kLaneBatchLanes];
                }
                lane_bfgs_update(D, p, gp, tmp, n);
                double gg = 0.0;
                for (int i = 0; i < n; ++i) gg = gg + g[i * kLaneBatchLanes] * g[i * kLaneBatchLanes];
                gnorm = sqrt(gg);
                ++iter;
            }
            first = false;
            if (iter < maxIter && xdiff > xMinDiff && gnorm > minGrad2Norm) {
                // p = -D g (:52-56), then the line search's start (:177-190)
                for (int i = 0; i < n; ++i) gp[i * kLaneBatchLanes] = g[i * kLaneBatchLanes];
                lane_bfgs_direction(D, g, p, n);
                double gd = 0.0;
                for (int i = 0; i < n; ++i) gd = gd + g[i * kLaneBatchLanes] * p[i * kLaneBatchLanes];
                alpha = 0.0; Fopt = F;
                phi0 = F; dphi0 = gd;
                alo = 0.0; plo = phi0; dlo = dphi0;
                ac = alphaGuess;
                it = 0;
                zoom = false;
                if (it < maxIterLS) {
                    for (int i = 0; i < n; ++i)
                        xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes] + ac * p[i * kLaneBatchLanes];
                    state = BB_LS_A;
                } else {
                    lsDone = true;
                }
            } else {
                state = BB_DONE;
            }
        }

        if (lsDone) {
            // X <- X + alpha p, xdiff = sum |X - Xprev| (:100-125), then the gradient at the new X
            double xd = 0.0;
            for (int i = 0; i < n; ++i) {
                const double xo = X[i * kLaneBatchLanes];
                const double xn = xo + alpha * p[i * kLaneBatchLanes];
                X[i * kLaneBatchLanes] = xn;
                xt[i * kLaneBatchLanes] = xn;
                xd += fabs(xn - xo);
            }
            xdiff = xd;
            F = Fopt;
            state = BB_GBASE;
        }
    }

    if (valid) {
        for (int j = 0; j < n; ++j) Xio[s * (size_t)n + j] = X[j * kLaneBatchLanes];
        f0out[s] = f0;
        fopt[s] = F;
        gnout[s] = gnorm;
        iters[s] = iter;
        evals[s] = ev;
    }
}

}  // namespace

int launch_bfgs_batch(pnol_ctx* ctx, const pnol_dobj* o, const double* params, long long nstart, double* X,
                      double* f0, double* fopt, double* gnorm, int* iters, long long* evals) {
    if (!ctx || !params || !X || !f0 || !fopt || !gnorm || !iters || !evals || nstart <= 0) return PNOL_ERR_ARG;
    PNOL_CHECK(scalar_batch_check(o, PNOL_BFGS_BATCH_NMAX));
    const double* p = params;
    const size_t ns = (size_t)nstart, lds = sizeof(double) * (size_t)bb_slots(o->n) * kLaneBatchLanes;
    return scalar_batch_dispatch(o->kind, [&](auto kind) {
        return lane_batch_launch(ctx, "bfgs_batch", &k_bfgs_batch<decltype(kind)::value>, ns, lds, o->n, ns,
                                 (const double*)o->p0, (const double*)o->p1, o->power, p[0], p[1], p[2], p[3],
                                 (int)p[4], p[5], (int)p[7], p[8], p[9], X, f0, fopt, gnorm, iters, evals);
    });
}

}  // namespace pnol
