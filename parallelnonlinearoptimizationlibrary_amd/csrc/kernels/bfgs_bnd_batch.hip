// bfgs_bnd_batch.hip -- batched box-bounded BFGS: many independent BFGS_Bnd::findMinBnd runs in
// one launch (gfx950).
//
// One lane owns one start and runs that start's whole BFGS_Bnd::findMinBnd
// (BFGS_bnd_linesearch.cpp:15-750; host form: host/bfgs_common.hpp ActiveSetRecursion and
// host/bfgs_bnd.cpp) with the exact update, every statement in that order: checkBoxBounds
// (silent), the Recur FD gradient over the free coordinates, cubicInterpolationLineSearchBnd with
// the step capped at computeAlphaBnd's alphaMax, lineSearchZoomBnd with its alphaTol test, its
// iter_ls counter shared with the outer search and its fall-back results, cubicInterpMinSimple
// with the midpoint for a NaN, and the active-set recursion of boundaryAssessment.  All starts
// share one box.  A start's result does not depend on the batch it is in and equals the
// one-problem class from the same X, box and parameters bit for bit (Power with power != 2 calls
// the device pow).  initHessFD, dXGradVec and initialScalingVec are not offered; alphaMult is
// accepted and unused, as in the class.
//
// Recursion as a stack.  The device has no call recursion; a lane keeps an explicit stack.  A
// level's coordinates are always exactly the coordinates that are not frozen, in ascending order
// (see the corner end below), so X, g, gprev, p, the trial point and the temporary stay in full
// space (n slots each), every reduced-order sum runs over the free indices ascending, and the
// frozen set is a bit mask in a register: a frozen coordinate of X keeps the value it was frozen
// at, which is what the evaluation point reads there.  One compact nr x nr D serves every level,
// because a parent's D is reset to I when its reduced problem returns; the update and the
// direction (lane_batch.hpp, shared with bfgs_batch.hip) run on the level's s, y and g gathered
// into the trial-point and temporary slots.  F is one register: a reduced problem starts from its
// parent's F and the parent takes the reduced problem's F back.  The stack holds per level the
// step's Xprev (compact: level d has at most n - d coordinates), the mask of what the level's
// assessment froze and the level's iter.  optimFlag and totalIter are per start, shared by all of
// its levels.
//
// State, lane-minor LDS as in bfgs_batch.hip (slot q of lane l at lds[q * 64 + l]), nothing in
// scratch.  Slots per lane:
//     [0, n n)          D, row-major, compact for the level (nr x nr, row stride nr)
//     + n each          X, g, gprev (y compact during the update), p, the trial point (s compact
//                       during the update, the new direction compact before it is scattered), the
//                       temporary (g compact for the direction)
//     + n (n + 1) / 2   the stack's Xprev, level d at d n - d (d - 1) / 2
//     + n each          the stack's frozen masks and iters
// n^2 + n (n + 1) / 2 + 8 n doubles per lane: n = 12 -> 318 x 512 B = 159 KB of the CU's 160 KB;
// n = 8 -> 82 KB; n <= 5 -> <= 40 KB.
//
// The corner end -- the one place the batch departs from the reference.  An assessment at depth
// >= 1 that leaves no free coordinate makes the reference clear optimFlag but keep those
// coordinates marked constant; the levels above clear only their own marks, so from then on the
// constant indicator disagrees with the level vectors and the reference reads past them
// (undefined behaviour).  The batch ends such a start at that assessment: X is the full-space
// point (every coordinate at a bound with an outward direction or gradient, a KKT corner), fOpt
// the level's F, iterations and evaluations as counted up to there (the trip that ends is not
// counted) and bit 8 of info is set.  Everything before is the reference's arithmetic.  No free
// coordinate left at depth 0 is not a corner end: the reference is consistent there and is
// followed exactly.
//
// Divergence: as bfgs_batch.hip.  A lane is a state machine and the wave one loop with ONE
// objective call site; update + assessment + loop test + direction is one block, which a lane
// that has its gradient enters once no lane of the wave is inside an FD gradient (lanes in a line
// search are not waited for).  Waiting changes no lane's arithmetic, only when it runs (measured
// against a -DPNOL_BFGS_BND_BATCH_NO_WAIT build: 1.7x at n = 2 to 6.0x at n = 8 on Rosenbrock, 1.8x
// on the quadratic; profiles/bfgs_bnd_batch_wait_ab.txt), and ends as in bfgs_batch.hip: each lane
// waited for arrives within n + 1 trips of entering its gradient.
//
// Termination.  Every trip of a level's loop raises totalIter, and a level's loop runs only while
// totalIter < maxIter; every assessment that recurses freezes at least one more coordinate, so
// the depth is at most n - 1; a level that cannot run pops.  A trip costs at most
// 2 maxIterLineSearch evaluations in its line search, n + 1 in its gradient and n + 1 in the
// gradient after a recursion returns, so a lane's work is bounded by about
// maxIter (2 maxIterLineSearch + 2 (n + 1)) + n + 2 evaluations.  No cross-lane data, no
// cross-workgroup waiting.
#include "lane_batch.hpp"

namespace pnol {
namespace {

// doubles of LDS per lane
constexpr int bnb_slots(int n) { return n * n + n * (n + 1) / 2 + 8 * n; }
static_assert(sizeof(double) * bnb_slots(PNOL_BFGS_BND_BATCH_NMAX) * kLaneBatchLanes <= kLaneBatchLdsMax,
              "the largest problem's state must fit one CU's LDS");
static_assert(PNOL_BFGS_BND_BATCH_NMAX >= 8 && PNOL_BFGS_BND_BATCH_NMAX <= 31, "the frozen set is a 32-bit mask");

// what a lane does with the next objective value (states before BNB_STEP evaluate)
enum : int {
    BNB_GBASE,    // FD gradient: the base value at the level's point
    BNB_GCOORD,   // FD gradient: the value at X + dX e_ci, ci a free coordinate
    BNB_F0,       // objEvalRecur(X) before the loop
    BNB_LS_A,     // line search (outer or zoom): phi(alpha)
    BNB_LS_B,     // line search: phi(alpha + dalpha), then the trip's decisions
    BNB_STEP,     // has its gradient: update, assessment, loop test, next direction
    BNB_DONE
};
// which gradient a lane in BNB_STEP has just finished
enum : int { BNB_FIRST, BNB_TRIP, BNB_RETURNED };

struct BndBatchParams {
    double c1, c2, dalpha, alphaGuess, alphaTol, bndTol, dXGrad, xMinDiff, minGrad2Norm;
    int maxIterLS, maxIter;
};

// cubicInterpMinSimple (BFGS_bnd_linesearch.cpp:736-750)
__device__ __forceinline__ double bnb_cubic(double aa, double ab, double pa, double pb, double da, double db) {
    const double w = ab - aa;
    const double sg = w > 0 ? 1.0 : (w < 0 ? -1.0 : 0.0);
    const double d1 = da + db - 3 * (pa - pb) / (aa - ab);
    const double d2 = sg * sqrt(d1 * d1 - da * db);
    double an = ab - (ab - aa) * (db + d2 - d1) / (db - da + 2 * d2);
    if (an < aa || an > ab || an != an) an = (aa + ab) / 2;
    return an;
}

__device__ __forceinline__ bool bnb_free(unsigned mask, int i) { return ((mask >> i) & 1u) == 0; }

// D = I for a level of nl coordinates
__device__ __forceinline__ void bnb_identity(double* D, int nl) {
    for (int i = 0; i < nl; ++i)
        for (int j = 0; j < nl; ++j) D[(i * nl + j) * kLaneBatchLanes] = i == j ? 1.0 : 0.0;
}

template <int KIND>
__global__ __launch_bounds__(kLaneBatchLanes) void k_bfgs_bnd_batch(
    int n, size_t nstart, const double* __restrict__ p0, const double* __restrict__ p1, double power,
    BndBatchParams q, const double* __restrict__ Xlb, const double* __restrict__ Xub, double* __restrict__ Xio,
    double* __restrict__ f0out, double* __restrict__ fopt, int* __restrict__ iters, long long* __restrict__ evals,
    int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double bnb_lds[];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * kLaneBatchLanes + lane;
    const bool valid = s < nstart;
    double* const D = bnb_lds + lane;
    double* const X = D + n * n * kLaneBatchLanes;
    double* const g = X + n * kLaneBatchLanes;
    double* const gp = g + n * kLaneBatchLanes;           // gprev; y (compact) inside the update
    double* const p = gp + n * kLaneBatchLanes;
    double* const xt = p + n * kLaneBatchLanes;           // the point the next value is taken at
    double* const tmp = xt + n * kLaneBatchLanes;
    double* const sXprev = tmp + n * kLaneBatchLanes;     // level d at d n - d (d - 1) / 2
    double* const sMask = sXprev + (n * (n + 1) / 2) * kLaneBatchLanes;
    double* const sIter = sMask + n * kLaneBatchLanes;

    for (int j = 0; j < n; ++j) {
        double x = valid ? Xio[s * (size_t)n + j] : 0.0;
        const double lb = Xlb[j], ub = Xub[j];
        // checkBoxBounds (Box_boundary_functions.cpp:11-40), silent
        if (x - lb < -fabs(lb) / 1000 || x - ub > fabs(ub) / 1000) x = (lb + ub) / 2.0;
        X[j * kLaneBatchLanes] = x;
        xt[j * kLaneBatchLanes] = x;
    }
    bnb_identity(D, n);

    int state = valid ? BNB_GBASE : BNB_DONE;
    int phase = BNB_FIRST;
    unsigned mask = 0, rel = 0;   // the frozen set; what the level that just returned had frozen
    int depth = 0, maxDepth = 0;
    bool optim = true, corner = false;
    bool zoom = false;            // the line search is inside lineSearchZoomBnd
    int iter = 0, totalIter = 0, it = 0, ci = 0;
    long long ev = 0;
    double F = 0.0, f0 = 0.0, Fb = 0.0;
    double xdiff = q.xMinDiff * 2, gnorm = 2 * q.minGrad2Norm;
    double alpha = 0.0, Fopt = 0.0, phi0 = 0.0, dphi0 = 0.0, amax = 0.0;
    double ac = 0.0, pc = 0.0;    // the trial step and phi there
    // the zoom's bracket; in the outer search (aa, pa, da) are (aim1, pim1, dim1)
    double aa = 0.0, ab = 0.0, pa = 0.0, pb = 0.0, da = 0.0, db = 0.0;

    while (__any(state != BNB_DONE)) {
        double v = 0.0;
        if (state < BNB_STEP) {
            v = lane_eval<KIND>(xt, n, p0, p1, power);
            ++ev;
        }
        bool lsDone = false;
        if (state == BNB_GBASE) {
            // gradientApproximationRecur (PNOL_Objective.cpp:337-360): the base value first, then
            // the free coordinates in order (a level has at least one)
            Fb = v;
            ci = 0;
            while (ci < n - 1 && !bnb_free(mask, ci)) ++ci;   // (ci stays inside the n slots)
            xt[ci * kLaneBatchLanes] = X[ci * kLaneBatchLanes] + q.dXGrad;
            state = BNB_GCOORD;
        } else if (state == BNB_GCOORD) {
            g[ci * kLaneBatchLanes] = (v - Fb) / q.dXGrad;
            xt[ci * kLaneBatchLanes] = X[ci * kLaneBatchLanes];
            ++ci;
            while (ci < n && !bnb_free(mask, ci)) ++ci;
            if (ci < n) xt[ci * kLaneBatchLanes] = X[ci * kLaneBatchLanes] + q.dXGrad;
            else state = phase == BNB_FIRST ? BNB_F0 : BNB_STEP;
        } else if (state == BNB_F0) {
            F = v;
            f0 = v;
            state = BNB_STEP;
        } else if (state == BNB_LS_A) {
            // lineSearchObj gave phi(ac); lineSearchFDDerivative's point (:465-496)
            pc = v;
            const double a2 = ac + q.dalpha;
            for (int i = 0; i < n; ++i)
                if (bnb_free(mask, i)) xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes] + a2 * p[i * kLaneBatchLanes];
            state = BNB_LS_B;
        } else if (state == BNB_LS_B) {
            const double dc = (v - pc) / q.dalpha;
            if (!zoom) {
                // cubicInterpolationLineSearchBnd (:203-353), trip iter_ls = it at ai = ac
                if ((pc > phi0 + q.c1 * ac * dphi0) || (pc >= pa && it > 1)) {
                    ab = ac; pb = pc; db = dc;                         // zoom(aim1, ai, ...)
                    zoom = true;
                } else if (fabs(dc) <= fabs(q.c2 * dphi0)) {
                    alpha = ac; Fopt = pc;
                    lsDone = true;
                } else if (dc >= 0) {
                    ab = ac; pb = pc; db = dc;                         // zoom(aim1, ai, ...) here too
                    zoom = true;
                } else if (ac == amax) {
                    alpha = ac; Fopt = pc;                             // the search ends on the box
                    lsDone = true;
                } else {
                    aa = ac; pa = pc; da = dc;
                    ac = 2 * ac;
                    if (ac > amax) ac = amax;
                    ++it;
                    if (it >= q.maxIterLS) {
                        // exhausted: pim1 is phii by now, so the first result is never taken
                        if (pa < pc) { alpha = aa; Fopt = pa; }
                        else if (phi0 < pc) { alpha = 0; Fopt = phi0; }
                        else { alpha = ac; Fopt = pc; }
                        lsDone = true;
                    }
                }
            } else {
                // lineSearchZoomBnd (:358-457), a trip at alpha_c = ac
                double pmin = pa;
                if (pb < pa) pmin = pb;
                if (pc > phi0 + q.c1 * ac * dphi0 || pc >= pmin) {
                    if (pa < pb) { ab = ac; pb = pc; db = dc; }
                    else { aa = ac; pa = pc; da = dc; }
                } else {
                    if (fabs(dc) <= fabs(q.c2 * dphi0)) {
                        alpha = ac; Fopt = pc;
                        lsDone = true;
                    } else if (dc < 0) {
                        aa = ac; pa = pc; da = dc;
                    } else {
                        ab = ac; pb = pc; db = dc;
                    }
                }
                if (!lsDone) ++it;
            }
            if (!lsDone && zoom) {
                // the zoom's loop test, also on entry; without success its best end is the result
                if (it < q.maxIterLS && (ab - aa > q.alphaTol)) {
                    ac = bnb_cubic(aa, ab, pa, pb, da, db);
                } else {
                    if (pa < pb) { alpha = aa; Fopt = pa; }
                    else { alpha = ab; Fopt = pb; }
                    lsDone = true;
                }
            }
            if (!lsDone) {
                for (int i = 0; i < n; ++i)
                    if (bnb_free(mask, i))
                        xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes] + ac * p[i * kLaneBatchLanes];
                state = BNB_LS_A;
            }
        }

        // update + assessment + loop test + direction, shared by the lanes that have their gradient
#ifdef PNOL_BFGS_BND_BATCH_NO_WAIT   // A/B arm: a lane runs the block on the trip it gets its gradient
        const bool gradBusy = false;
#else
        const bool gradBusy = __any(state == BNB_GBASE || state == BNB_GCOORD);   // asked by the whole wave
#endif
        if (state == BNB_STEP && !gradBusy) {
            const int nl = n - __popc(mask);   // the level's coordinates
            bool post = false;                 // the trip's tail: xdiff, gnorm, iter, totalIter
            if (phase == BNB_TRIP) {
                // s = alpha p and y = g - gprev over the level's coordinates (mainBFGSLoop :116-201),
                // gathered for updateHessianInv
                for (int i = 0, k = 0; i < n; ++i)
                    if (bnb_free(mask, i)) {
                        const double si = alpha * p[i * kLaneBatchLanes];
                        const double yi = g[i * kLaneBatchLanes] - gp[i * kLaneBatchLanes];
                        xt[k * kLaneBatchLanes] = si;
                        gp[k * kLaneBatchLanes] = yi;
                        ++k;
                    }
                lane_bfgs_update(D, xt, gp, tmp, nl);
                for (int i = 0; i < n; ++i) xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes];
                // boundaryAssessment (:503-728): freeze the free coordinates that sit on a bound
                // with an outward direction or gradient
                unsigned fm = 0;
                for (int i = 0; i < n; ++i)
                    if (bnb_free(mask, i)) {
                        const double x = X[i * kLaneBatchLanes], pi = p[i * kLaneBatchLanes],
                                     gi = g[i * kLaneBatchLanes];
                        if ((fabs(x - Xlb[i]) < q.bndTol) && ((pi < 0) || (gi > 0))) fm |= 1u << i;
                        else if ((fabs(x - Xub[i]) < q.bndTol) && ((pi > 0) || (gi < 0))) fm |= 1u << i;
                    }
                const int nr = nl - __popc(fm);
                if (fm != 0 && nr > 0) {
                    // one level down: the reduced problem from D = I with its own iter, xdiff, gnorm
                    // (Xprev of this level's step is already in the stack)
                    sMask[depth * kLaneBatchLanes] = (double)fm;
                    sIter[depth * kLaneBatchLanes] = (double)iter;
                    mask |= fm;
                    ++depth;
                    if (depth > maxDepth) maxDepth = depth;
                    bnb_identity(D, nr);
                    iter = 0;
                    xdiff = q.xMinDiff * 2;
                    gnorm = 2 * q.minGrad2Norm;
                } else if (nr == 0) {
                    if (depth >= 1) {
                        corner = true;   // the corner end (see top)
                        state = BNB_DONE;
                    } else {
                        optim = false;
                        post = true;
                    }
                } else {
                    post = true;
                }
            } else if (phase == BNB_RETURNED) {
                // the reduced problem returned and its coordinates were released: go on only if a
                // released coordinate's gradient points back inside
                bool cont = false;
                for (int i = 0; i < n; ++i)
                    if ((rel >> i) & 1u) {
                        const double x = X[i * kLaneBatchLanes], gi = g[i * kLaneBatchLanes];
                        if ((fabs(x - Xlb[i]) < q.bndTol) && (gi < 0)) cont = true;
                        else if ((fabs(x - Xub[i]) < q.bndTol) && (gi > 0)) cont = true;
                    }
                optim = cont;
                post = true;
            }
            if (post) {
                const double* xp = sXprev + (depth * n - depth * (depth - 1) / 2) * kLaneBatchLanes;
                double xd = 0.0, gg = 0.0;
                for (int i = 0, k = 0; i < n; ++i)
                    if (bnb_free(mask, i)) {
                        xd += fabs(X[i * kLaneBatchLanes] - xp[k * kLaneBatchLanes]);
                        gg = gg + g[i * kLaneBatchLanes] * g[i * kLaneBatchLanes];
                        ++k;
                    }
                xdiff = xd;
                gnorm = sqrt(gg);
                ++iter;
                ++totalIter;
            }
            if (state != BNB_DONE) {
                if (optim && iter < q.maxIter && xdiff > q.xMinDiff && gnorm > q.minGrad2Norm &&
                    totalIter < q.maxIter) {
                    // p = -D g over the level's coordinates, then the line search's start (:203-230)
                    const int nc = n - __popc(mask);
                    for (int i = 0, k = 0; i < n; ++i)
                        if (bnb_free(mask, i)) {
                            const double gi = g[i * kLaneBatchLanes];
                            gp[i * kLaneBatchLanes] = gi;
                            tmp[k * kLaneBatchLanes] = gi;
                            ++k;
                        }
                    lane_bfgs_direction(D, tmp, xt, nc);
                    for (int i = 0, k = 0; i < n; ++i)
                        if (bnb_free(mask, i)) {
                            p[i * kLaneBatchLanes] = xt[k * kLaneBatchLanes];
                            ++k;
                        }
                    for (int i = 0; i < n; ++i) xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes];
                    double gd = 0.0;
                    // computeAlphaBnd (Box_boundary_functions.cpp:11-40) in its plain-loop form
                    double bnd = 0.0;
                    bool head = true;
                    for (int i = 0; i < n; ++i)
                        if (bnb_free(mask, i)) {
                            const double x = X[i * kLaneBatchLanes], pi = p[i * kLaneBatchLanes];
                            gd = gd + g[i * kLaneBatchLanes] * pi;
                            const double a1 = (Xub[i] - x) / pi;
                            const double a2 = (Xlb[i] - x) / pi;
                            double ai;
                            if (a1 > 0) ai = a1;
                            else if (a2 > 0) ai = a2;
                            else ai = 0;
                            if (head) bnd = ai;
                            head = false;
                            if (bnd > ai) bnd = ai;
                        }
                    amax = bnd;
                    alpha = 0.0; Fopt = F;
                    phi0 = F; dphi0 = gd;
                    aa = 0.0; pa = phi0; da = dphi0;
                    ac = q.alphaGuess;
                    if (ac > amax) ac = amax;
                    it = 0;
                    zoom = false;
                    if (it < q.maxIterLS) {
                        for (int i = 0; i < n; ++i)
                            if (bnb_free(mask, i))
                                xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes] + ac * p[i * kLaneBatchLanes];
                        state = BNB_LS_A;
                    } else {
                        // no trip at all: the exhausted results with phii = 0
                        if (pa < 0.0) { alpha = aa; Fopt = pa; }
                        else if (phi0 < 0.0) { alpha = 0; Fopt = phi0; }
                        else { alpha = ac; Fopt = 0.0; }
                        lsDone = true;
                    }
                } else if (depth == 0) {
                    state = BNB_DONE;
                } else {
                    // the level's loop is over: back to the parent, whose D is reset and whose
                    // gradient is recomputed with the level's coordinates released
                    --depth;
                    rel = (unsigned)sMask[depth * kLaneBatchLanes];
                    iter = (int)sIter[depth * kLaneBatchLanes];
                    mask &= ~rel;
                    bnb_identity(D, n - __popc(mask));
                    phase = BNB_RETURNED;
                    state = BNB_GBASE;
                }
            }
        }

        if (lsDone) {
            // Xprev = X, X <- X + alpha p over the level's coordinates (:150-160), then the
            // gradient at the new X
            double* xp = sXprev + (depth * n - depth * (depth - 1) / 2) * kLaneBatchLanes;
            for (int i = 0, k = 0; i < n; ++i)
                if (bnb_free(mask, i)) {
                    const double xo = X[i * kLaneBatchLanes];
                    const double xn = xo + alpha * p[i * kLaneBatchLanes];
                    xp[k * kLaneBatchLanes] = xo;
                    X[i * kLaneBatchLanes] = xn;
                    ++k;
                }
            for (int i = 0; i < n; ++i) xt[i * kLaneBatchLanes] = X[i * kLaneBatchLanes];
            F = Fopt;
            phase = BNB_TRIP;
            state = BNB_GBASE;
        }
    }

    if (valid) {
        for (int j = 0; j < n; ++j) Xio[s * (size_t)n + j] = X[j * kLaneBatchLanes];
        f0out[s] = f0;
        fopt[s] = F;
        iters[s] = totalIter;
        evals[s] = ev;
        info[s] = maxDepth | (corner ? PNOL_BFGS_BND_BATCH_CORNER : 0);
    }
}

}  // namespace

int launch_bfgs_bnd_batch(pnol_ctx* ctx, const pnol_dobj* o, const double* params, const double* Xlb,
                          const double* Xub, long long nstart, double* X, double* f0, double* fopt, int* iters,
                          long long* evals, int* info) {
    if (!ctx || !params || !Xlb || !Xub || !X || !f0 || !fopt || !iters || !evals || !info || nstart <= 0)
        return PNOL_ERR_ARG;
    PNOL_CHECK(scalar_batch_check(o, PNOL_BFGS_BND_BATCH_NMAX));
    const double* p = params;
    // BFGS_Bnd::setParams order; alphaMult (5), dXHess (9) and verbose (14) are unused
    const BndBatchParams q{p[0], p[1], p[2], p[3], p[4], p[7], p[8], p[11], p[12], (int)p[6], (int)p[10]};
    const size_t ns = (size_t)nstart, lds = sizeof(double) * (size_t)bnb_slots(o->n) * kLaneBatchLanes;
    return scalar_batch_dispatch(o->kind, [&](auto kind) {
        return lane_batch_launch(ctx, "bfgs_bnd_batch", &k_bfgs_bnd_batch<decltype(kind)::value>, ns, lds, o->n, ns,
                                 (const double*)o->p0, (const double*)o->p1, o->power, q, Xlb, Xub, X, f0, fopt, iters,
                                 evals, info);
    });
}

}  // namespace pnol
