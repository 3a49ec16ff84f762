// bfgs_common.hpp -- what the five host BFGS drop-ins (bfgs*.cpp) share: the exchange of a
// pooled line search's entries, the pooled secant search (BFGS_MPI, BFGSBnd_MPI), the unbounded
// quasi-Newton loop (BFGS, BFGS_MPI) and the bounded active-set recursion (BFGS_Bnd,
// BFGS_Bnd_MPI_SW).  Each is the reference's control flow restated once; what a class does
// differently -- its gradient call, its line search, its text -- comes in as a template
// argument, so every call is resolved at compile time (no std::function, no virtual on the
// cfg-5 hot path).  The pure helpers are in bfgs_helpers.hpp.
#pragma once

#include <cmath>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../pnol_comm.hpp"
#include "Box_boundary_functions.hpp"   // checkBoxBounds, computeAlphaBnd
#include "PNOL_Objective.hpp"
#include "bfgs_helpers.hpp"
#include "dense_hessian.hpp"
#include "line_points.hpp"
#include "recur_simd.hpp"

// the pooled secant search's free functions (bfgs_mpi.cpp, bfgs_bnd_mpi.cpp; also in their drop-in headers)
void findPoolBounds(std::vector<double>& alphaPool, std::vector<double>& phiPool, double alpha0, double phi0,
                    double& alpha1, double& alpha2, double& phi1, double& phi2);
void checkAlphaPoolBnd(bool& bndIndicator, std::vector<double>& alphaPool, std::vector<double>& X,
                       std::vector<double>& Xlb, std::vector<double>& Xub, std::vector<double>& p,
                       std::vector<double>& constantX, std::vector<bool>& constantIndicator);

namespace pnol {

// ---- pool exchange --------------------------------------------------------------------------
// Every rank has evaluated its own entries of the pool (PoolSlots: entry k on rank k mod P);
// `mine` holds them slot-major, `width` values per entry (1: phi; 2: phi and dphi), zero-padded
// to ps.per slots.  One allgather; pool[k width + w] is value w of entry k.
inline void pool_exchange(const PoolSlots& ps, int width, const std::vector<double>& mine, double* pool) {
    const size_t cnt = (size_t)width * ps.per;
    std::vector<double> all(cnt * ps.P, 0.0);
    check(comm_allgather_host(nullptr, mine.data(), all.data(), cnt), "allgather(alpha pool)");
    for (int k = 0; k < ps.N; ++k)
        for (int w = 0; w < width; ++w) pool[(size_t)k * width + w] = all[width * ps.at(k) + w];
}

// ---- pooled secant line search --------------------------------------------------------------
// BFGS_with_linesearch_MPI.cpp:226-492 and BFGS_with_bnd_linsearch_MPI.cpp:358-660: a geometric
// pool of Npool steps is extended until one of them brackets a minimum, then Npool interior
// points of the bracket are evaluated per zoom round.
struct SecantSearch {
    double c1, c2, maxAlphaMult, alphaGuess;
    int maxIterLineSearch, Npool;
    // the box (BFGSBnd_MPI; null: unbounded): every pool is clipped to it (checkAlphaPoolBnd) and
    // a clipped pool ends the bracketing; verbose announces that
    std::vector<double>*Xlb, *Xub;
    bool verbose;
    // stop zooming once the whole zoom pool is below alphaMin
    bool alphaMinStop;
    double alphaMin;
    // the result is the minimum of the zoom pool, bracket ends included (BFGS_MPI), or of the
    // last evaluated pool (BFGSBnd_MPI).  Without a zoom the zoom pool is all zeros -- alpha 0,
    // F 0, the reference's zero-pool defect -- unless fixZeroPool reports the best point seen.
    bool resultFromZoomPool;
    bool fixZeroPool;
};

// evalPool(alphaPool, phiPool): phiPool[k] = phi(alphaPool[k]), gathered over the ranks
template <class EvalPool>
void secant_pool_search(const SecantSearch& o, EvalPool&& evalPool, std::vector<double>& X, double FX,
                        std::vector<double>& dFdX, std::vector<double>& p, double& alphaOpt, double& Fopt) {
    const int Np = o.Npool;
    std::vector<double> ap(Np, 0.0), pp(Np, 0.0), apPrev(Np, -1.0), ppPrev(Np, 0.0), slope(Np, 0.0);
    alphaOpt = 0;
    Fopt = FX;
    const double a0 = 0, phi0 = FX, dphi0 = seq_dot(dFdX, p);
    const bool bounded = o.Xlb != nullptr;
    bool clipped = false;
    std::vector<double> nocX;   // checkAlphaPoolBnd's unused arguments
    std::vector<bool> nocI;

    const int idxMin = -(int)std::ceil((Np - 1.0) / 2.0);
    const int idxMax = (int)std::floor((Np - 1.0) / 2.0);
    double r = std::pow(o.maxAlphaMult, 1.0 / (double)idxMax);
    for (int k = 0, idx = idxMin; k < Np; ++k, ++idx) ap[k] = o.alphaGuess * std::pow(r, idx);

    bool first = true, zoom = false;
    double bestA = 0, bestP = phi0;   // best point seen, for fixZeroPool
    for (int it = 0; it < o.maxIterLineSearch && first; ++it) {
        if (bounded) checkAlphaPoolBnd(clipped, ap, X, *o.Xlb, *o.Xub, p, nocX, nocI);
        evalPool(ap, pp);
        for (int i = 0; o.fixZeroPool && i < Np; ++i) if (pp[i] < bestP) { bestP = pp[i]; bestA = ap[i]; }
        // 1. sufficient decrease
        for (int i = 0; i < Np; ++i)
            if (pp[i] > phi0 + o.c1 * ap[i] * dphi0) { zoom = true; first = false; }
        // 2. curvature against the secant slopes
        slope[0] = (pp[0] - phi0) / (ap[0] - a0);
        for (int i = 1; i < Np; ++i) slope[i] = (pp[i] - pp[i - 1]) / (ap[i] - ap[i - 1]);
        if (first)
            for (int i = 0; i < Np; ++i)
                if (std::fabs(slope[i]) <= std::fabs(o.c2 * dphi0)) { zoom = false; first = false; }
        // 3. a non-negative secant slope brackets a minimum
        if (first)
            for (int i = 0; i < Np; ++i)
                if (slope[i] >= 0) { zoom = true; first = false; }
        // 4. extend the pool, unless it was clipped to the box
        if (first && !clipped) {
            double amax; int imax;
            vector_max(ap, amax, imax);
            r = std::pow(o.maxAlphaMult, 1.0 / (double)Np);
            for (int i = 0; i < Np; ++i) {
                apPrev[i] = ap[i];
                ppPrev[i] = pp[i];
                const double power = i + 1;
                ap[i] = amax * std::pow(r, power);
            }
        } else if (clipped) {
            first = false;
            if (o.verbose && comm_rank() == ROOT_ID) {
                std::cout << std::endl << "Line search reached boundary. Attempting to find an acceptable point in "
                          << "the domain interior." << std::endl << "alpha = ";
                print_vec(ap);
                std::cout << "phi = ";
                print_vec(pp);
            }
        }
    }

    double alo, ahi, plo, phi;
    if (apPrev[0] < 0) {
        findPoolBounds(ap, pp, a0, phi0, alo, ahi, plo, phi);
    } else {
        std::vector<double> ae(2 * Np), pe(2 * Np);
        for (int i = 0; i < Np; ++i) { ae[i] = apPrev[i]; ae[i + Np] = ap[i]; pe[i] = ppPrev[i]; pe[i + Np] = pp[i]; }
        findPoolBounds(ae, pe, a0, phi0, alo, ahi, plo, phi);
    }

    // zoom: Npool interior points of [alpha_lo, alpha_hi] per round
    std::vector<double> ap2(Np + 2, 0.0), pp2(Np + 2, 0.0);
    const bool zoomed = zoom;
    for (int it = 0; it < o.maxIterLineSearch && zoom; ++it) {
        linspace(alo, ahi, Np + 2, ap2);
        pp2[0] = plo; pp2[Np + 1] = phi; ap2[0] = alo; ap2[Np + 1] = ahi;
        for (int i = 0; i < Np; ++i) { ap[i] = ap2[i + 1]; pp[i] = pp2[i + 1]; }
        evalPool(ap, pp);
        for (int i = 0; i < Np; ++i) { ap2[i + 1] = ap[i]; pp2[i + 1] = pp[i]; }
        for (int i = 0; i < Np; ++i) slope[i] = (pp2[i + 1] - pp2[i]) / (ap2[i + 1] - ap2[i]);
        for (int i = 0; i < Np; ++i)
            if (std::fabs(slope[i]) <= std::fabs(o.c2 * dphi0)) zoom = false;
        if (zoom) findPoolBounds(ap2, pp2, a0, phi0, alo, ahi, plo, phi);
        if (o.alphaMinStop) {
            double amax; int imax;
            vector_max(ap2, amax, imax);
            if (amax < o.alphaMin) zoom = false;
        }
    }
    if (!zoomed && o.fixZeroPool) {
        alphaOpt = bestA;
        Fopt = bestP;
        return;
    }
    const std::vector<double>& ar = o.resultFromZoomPool ? ap2 : ap;
    double pmin; int imin;
    vector_min(o.resultFromZoomPool ? pp2 : pp, pmin, imin);
    alphaOpt = ar[imin];
    Fopt = pmin;
}

// ---- unbounded quasi-Newton loop ------------------------------------------------------------
// BFGS_with_linesearch.cpp:12-139 and BFGS_with_linesearch_MPI.cpp:12-142.
struct QuasiNewtonParams {
    double dXGrad, dXHess, xMinDiff, minGrad2Norm;
    int maxIter, updateMode;
    bool initHessFD;
    bool shardD;       // D row-sharded over the ranks
    double* profile;   // per-phase seconds and counts, or nullptr
};

// gradient(X, dX, dFdX); lineSearch(X, F, dFdX, p, alpha, Fopt); iterText(iter, xdiff, gnorm, F)
// and finalText(f0, fOpt, X) print (or not) the class's own text
template <class Gradient, class LineSearch, class IterText, class FinalText>
void quasi_newton_loop(const QuasiNewtonParams& q, Objective* obj, std::vector<double>& X, double& f0, double& fOpt,
                       Gradient&& gradient, LineSearch&& lineSearch, IterText&& iterText, FinalText&& finalText) {
    const int n = (int)X.size();
    double* const profile = q.profile;
    DenseInverseHessian D(require_ctx(), n, q.updateMode, q.shardD);
    if (q.initHessFD) init_from_fd_hessian(obj, X, q.dXHess, D);
    else D.setIdentity();

    std::vector<double> dX(n, q.dXGrad), dFdX(n), dFdXprev(n), p(n), pnext(n), s(n), y(n), Xprev(n);
    {
        PhaseClock t(prof_slot(profile, kProfGrad));
        gradient(X, dX, dFdX);
        if (profile) profile[kProfGradCalls] += 1;
    }
    double F = obj->objEval(X);
    f0 = F;
    int iter = 0;
    double xdiff = q.xMinDiff * 2, gnorm = 2 * q.minGrad2Norm;
    bool have_next = false;
    while (iter < q.maxIter && xdiff > q.xMinDiff && gnorm > q.minGrad2Norm) {
        dFdXprev = dFdX;
        if (have_next) {
            p = pnext;
        } else {
            PhaseClock t(prof_slot(profile, kProfUpdate));
            D.direction(dFdX, p);
        }
        double alpha = 0, Fopt = 0;
        {
            PhaseClock t(prof_slot(profile, kProfLineSearch));
            lineSearch(X, F, dFdX, p, alpha, Fopt);
        }
        for (int i = 0; i < n; ++i) { Xprev[i] = X[i]; X[i] = X[i] + alpha * p[i]; }
        F = Fopt;
        {
            PhaseClock t(prof_slot(profile, kProfGrad));
            gradient(X, dX, dFdX);
            if (profile) profile[kProfGradCalls] += 1;
        }
        for (int i = 0; i < n; ++i) { s[i] = alpha * p[i]; y[i] = dFdX[i] - dFdXprev[i]; }
        {
            PhaseClock t(prof_slot(profile, kProfUpdate));
            D.update(y, s, &dFdX, &pnext);
        }
        have_next = true;
        xdiff = 0;
        for (int i = 0; i < n; ++i) xdiff += std::fabs(X[i] - Xprev[i]);
        gnorm = std::sqrt(seq_dot(dFdX, dFdX));
        iterText(iter, xdiff, gnorm, F);
        iter = iter + 1;
    }
    if (profile) profile[kProfIters] = iter;
    fOpt = F;
    finalText(f0, fOpt, X);
}

// ---- bounded active-set recursion -----------------------------------------------------------
// BFGS_bnd_linesearch.cpp:15-201, 503-728 and BFGS_bnd_linesearch_MPI_SW.cpp:12-207, 741-967: a
// coordinate that reaches a bound with an outward direction or gradient is frozen and the
// reduced problem re-optimised from D = I, one recursion level per assessment that froze
// something (about 11k levels at n = 16384, cfg 5).

// PNOL_BND_DETAIL=1: where the host time of the "other" phase goes (diagnostics, stderr)
enum BndDetail { kDetFreeze, kDetGather, kDetCopyBack, kDetIterLoops, kDetCount };
inline double* bnd_detail_all() { thread_local double slots[kDetCount]; return slots; }
inline double* bnd_detail_slot(int k) {
    static const bool on = [] {
        const char* e = std::getenv("PNOL_BND_DETAIL");
        return e && std::atoi(e) != 0;
    }();
    return on ? bnd_detail_all() + k : nullptr;
}

struct BndParams {
    double bndTol, dXGrad, dXHess, xMinDiff, minGrad2Norm;
    int maxIter, updateMode, verbose;
    bool initHessFD;
    const std::vector<double>*dXGradVec, *initialScalingVec;
    std::vector<double>* fTrace;   // F after every iteration (any level), or nullptr
    double* profile;               // per-phase seconds and counts, or nullptr
};

// Policy: what the class does its own way.
//   kShardD            D row-sharded over the ranks
//   kFusedDirection    the next direction comes out of the update's pass (D.update(y, s, &g,
//                      &pnext)); else D.update alone and D.direction at the next iteration
//   kDetailClocks      the PNOL_BND_DETAIL clocks
//   kStepTextAbove, kRecursedTextAbove   the step line / the after-recursion lines are printed
//                      when verbose exceeds these
//   gradient(X, dX, dFdX, cX, cI), lineSearch(X, Xlb, Xub, F, dFdX, p, cX, cI, alpha, Fopt)
//   startText(), announcesBoundary(verbose), boundaryText(nfrozen, X, F)
// optimFlag, recurFlag and totalIter are the caller's (the pooled class keeps them as members:
// its pool evaluation clears optimFlag).
template <class Policy>
class ActiveSetRecursion {
  public:
    ActiveSetRecursion(Policy& policy, const BndParams& params, Objective* obj, bool& optimFlag, int& recurFlag,
                       int& totalIter)
        : pol(policy), q(params), objPtr(obj), optimFlag(optimFlag), recurFlag(recurFlag), totalIter(totalIter) {}

    void findMinBody(std::vector<double>& X, std::vector<double>& Xlb, std::vector<double>& Xub, double& f0,
                     double& fOpt) {
        totalIter = 0;
        if (q.verbose >= 0 && root()) {
            std::cout << std::endl << pol.startText() << std::endl << "  X0 = ";
            print_vec(X);
        }
        const int n = (int)X.size();
        checkBoxBounds(X, Xlb, Xub);
        std::vector<double> cX(n, 0.0), X0 = X;
        std::vector<bool> cI(n, false);
        std::vector<double> dX(n, q.dXGrad);
        if (!q.dXGradVec->empty())
            for (int i = 0; i < n; ++i) dX[i] = (*q.dXGradVec)[i];
        std::vector<double> dFdX(n, 0.0);
        DenseInverseHessian D(require_ctx(), n, q.updateMode, Policy::kShardD);
        if (q.initHessFD) init_from_fd_hessian(objPtr, X, q.dXHess, D);
        else if (!q.initialScalingVec->empty()) D.setIdentity(q.initialScalingVec);
        else D.setIdentity();
        gradient(X, dX, dFdX, cX, cI);
        double F = objPtr->objEvalRecur(X, cX, cI);
        f0 = F;
        optimFlag = true;
        recurFlag = 0;
        freeIdx.resize(n);
        for (int i = 0; i < n; ++i) freeIdx[i] = i;
        freeIdxLive = true;
        mainLoop(F, X, dFdX, D, Xlb, Xub, dX, cX, cI);
        freeIdxLive = false;
        std::vector<int>().swap(freeIdx);
        fOpt = F;
        if (q.verbose >= 0 && root()) {
            std::cout << std::endl << "  Completed bounded BFGS." << std::endl << "  X0 = ";
            print_vec(X0);
            std::cout << "  Xopt = ";
            print_vec(X);
            std::cout << "  f0 = " << f0 << ", fOpt = " << fOpt << std::endl << std::endl;
        }
    }

    void mainLoop(double& F, std::vector<double>& X, std::vector<double>& dFdX, DenseInverseHessian& D,
                  std::vector<double>& Xlb, std::vector<double>& Xub, std::vector<double>& dX, std::vector<double>& cX,
                  std::vector<bool>& cI) {
        const int n = (int)X.size();
        double* const profile = q.profile;
        std::vector<double> p(n), pnext, Xprev(n);
        bool have_next = false;
        int iter = 0;
        double xdiff = q.xMinDiff * 2, gnorm = 2 * q.minGrad2Norm;
        while (optimFlag && iter < q.maxIter && xdiff > q.xMinDiff && gnorm > q.minGrad2Norm && totalIter < q.maxIter) {
            if (q.verbose > 0 && root())
                std::cout << std::endl << "Iter = " << iter << " of bounded BFGS search starting with previous F = " << F
                          << "." << std::endl;
            // p = -D g; after an iteration without recursion it came out of the update's pass
            // (the same bits: D and g are what the update left)
            if (have_next) {
                p.swap(pnext);
            } else {
                PhaseClock t(prof_slot(profile, kProfUpdate));
                D.direction(dFdX, p);
            }
            double alpha = 0, Fopt = 0;
            {
                PhaseClock t(prof_slot(profile, kProfLineSearch));
                pol.lineSearch(X, Xlb, Xub, F, dFdX, p, cX, cI, alpha, Fopt);
            }
            PhaseClock tl(det(kDetIterLoops));
            for (int i = 0; i < n; ++i) { Xprev[i] = X[i]; X[i] = X[i] + alpha * p[i]; }
            F = Fopt;
            {
                // per-iteration scratch (not live across the recursion below, so one set per thread)
                thread_local std::vector<double> gprev, s, y;
                gprev.assign(dFdX.begin(), dFdX.end());
                s.resize(n);
                y.resize(n);
                tl.stop();
                gradient(X, dX, dFdX, cX, cI);
                for (int i = 0; i < n; ++i) { s[i] = alpha * p[i]; y[i] = dFdX[i] - gprev[i]; }
                PhaseClock t(prof_slot(profile, kProfUpdate));
                if (Policy::kFusedDirection) D.update(y, s, &dFdX, &pnext);
                else D.update(y, s, nullptr, nullptr);
            }
            assessRecursed = false;
            pnextHeld = &pnext;
            assess(F, X, p, dFdX, D, Xlb, Xub, dX, cX, cI);
            pnextHeld = nullptr;
            // a recursion reset D to I and recomputed the gradient: the fused direction is stale
            have_next = Policy::kFusedDirection && !assessRecursed;
            if (!have_next) std::vector<double>().swap(pnext);
            // the step's sum |X - Xprev| and the gradient's sum of squares: two independent
            // sequential chains (each in the reference's order), one loop
            PhaseClock tl2(det(kDetIterLoops));
            xdiff = 0;
            double gg = 0.0;
            for (int i = 0; i < n; ++i) {
                xdiff += std::fabs(X[i] - Xprev[i]);
                gg = gg + dFdX[i] * dFdX[i];
            }
            gnorm = std::sqrt(gg);
            if (q.fTrace) q.fTrace->push_back(F);
            if (q.verbose > Policy::kStepTextAbove && root()) {
                std::cout << "  Step completed with F = " << F << " and mean abs xdiff is " << xdiff
                          << " and the grad2norm = " << gnorm << std::endl;
                if (q.verbose > 1) {
                    std::cout << "  X = ";
                    print_vec(X);
                }
            }
            iter = iter + 1;
            totalIter = totalIter + 1;
        }
    }

    void assess(double& F, std::vector<double>& X, std::vector<double>& p, std::vector<double>& dFdX,
                DenseInverseHessian& D, std::vector<double>& Xlb, std::vector<double>& Xub, std::vector<double>& dX,
                std::vector<double>& cX, std::vector<bool>& cI) {
        const int ncur = (int)X.size();
        const int Ndim = (int)cX.size();
        double* const profile = q.profile;
        const std::vector<double>& scaling = *q.initialScalingVec;
        PhaseClock tf(det(kDetFreeze));
        std::vector<int> fk, fi;   // positions in X frozen by this assessment (ascending), their full indices
        bool bndFlag = false;
        int Nconst = 0;            // coordinates frozen after the tests
        if (freeIdxLive && (int)freeIdx.size() == ncur) {
            // the level's coordinates are the free ones of cI in order (freeIdx): the reference's
            // walk over all Ndim indicators reduces to the tests over X's own positions
            recur::bound_hits(X.data(), Xlb.data(), Xub.data(), p.data(), dFdX.data(), (size_t)ncur, q.bndTol, fk);
            for (int k : fk) {
                const int i = freeIdx[k];
                cI[i] = true; cX[i] = X[k]; fi.push_back(i);
            }
            bndFlag = !fk.empty();
            Nconst = Ndim - ncur + (int)fk.size();
        } else {
            // any constantIndicator: the reference's walk, evaluated without short-circuit
            // branches (only a coordinate that hits a bound takes one)
            freeIdxLive = false;
            const int klast = ncur > 0 ? ncur - 1 : 0;
            int icur = 0;
            for (int i = 0; i < Ndim; ++i) {
                const bool c = cI[i];
                Nconst += c;
                if (ncur == 0) continue;
                const int k = icur < klast ? icur : klast;
                const double xk = X[k], pk = p[k], gk = dFdX[k];
                const bool lo = (std::fabs(xk - Xlb[k]) < q.bndTol) & ((pk < 0) | (gk > 0));
                const bool hi = (std::fabs(xk - Xub[k]) < q.bndTol) & ((pk > 0) | (gk < 0));
                if (!c & (lo | hi)) {
                    bndFlag = true; cI[i] = true; cX[i] = xk; fi.push_back(i);
                    if (icur < ncur) fk.push_back(icur);
                }
                icur += !c;
            }
            Nconst += (int)fi.size();   // == the count of cI after the freezes
        }
        if (bndFlag && pol.announcesBoundary(q.verbose) && root()) pol.boundaryText(fi.size(), X, F);
        const int nr = Ndim - Nconst;
        tf.stop();
        if (bndFlag && nr > 0) {
            PhaseClock tg(det(kDetGather));
            // The reduced problem runs on these same vectors: the frozen entries are set aside and
            // the others slide down in place (the reference gathers them into fresh vectors at every
            // level), so one set of n-vectors serves the whole recursion -- about 11k levels at
            // n = 16384 -- instead of five new ones per level.
            const int nf = (int)fk.size(), nk = ncur - nf;
            std::vector<double> held((size_t)nf * 5);
            for (int f = 0; f < nf; ++f) {
                const int k = fk[f];
                double* h = &held[(size_t)f * 5];
                h[0] = X[k]; h[1] = dFdX[k]; h[2] = Xlb[k]; h[3] = Xub[k]; h[4] = dX[k];
            }
            const bool idx = freeIdxLive;
            for (std::vector<double>* v : {&X, &dFdX, &Xlb, &Xub, &dX}) {
                drop_positions(*v, fk, ncur);
                v->resize(nr);
                // the fallback walk (freeIdxLive off, e.g. below a level that froze every coordinate)
                // can leave nr != nk: entries past the nk kept ones read 0.0, as the reference's
                // fresh XR(nr) would hold them (never stale values from the compaction)
                if (nr > nk) std::fill(v->begin() + nk, v->end(), 0.0);
            }
            if (idx) {
                drop_positions(freeIdx, fk, ncur);
                freeIdx.resize(nr);
            }
            const double FR = F;
            double Fr = F;
            // the outer D is discarded while the reduced problem runs (reset below), so the
            // reduced D takes over its device buffer: one n x n matrix for the whole recursion
            DenseInverseHessian DR(D, nr, q.updateMode, Policy::kShardD);
            if (!scaling.empty()) {
                std::vector<double> scaleR;
                if (idx) {
                    scaleR.resize(nr);
                    for (int k = 0; k < nr; ++k) scaleR[k] = scaling[freeIdx[k]];
                } else {
                    for (int i = 0; i < Ndim; ++i) if (!cI[i]) scaleR.push_back(scaling[i]);
                }
                DR.setIdentity(&scaleR);
            } else {
                DR.setIdentity();
            }
            recurFlag = true;
            // the caller's direction (and the next one its update prepared) are recomputed after
            // the recursion: release them while it runs
            std::vector<double>().swap(p);
            if (pnextHeld) std::vector<double>().swap(*pnextHeld);
            pnextHeld = nullptr;
            tg.stop();
            ++depth;
            if (profile && depth > profile[kProfDepth]) profile[kProfDepth] = depth;
            mainLoop(Fr, X, dFdX, DR, Xlb, Xub, dX, cX, cI);
            --depth;
            assessRecursed = true;   // after the reduced loop, which clears it for its own levels
            PhaseClock tc(det(kDetCopyBack));
            F = nk > 0 ? Fr : FR;
            for (std::vector<double>* v : {&X, &dFdX, &Xlb, &Xub, &dX}) {
                v->resize(ncur);
                reopen_positions(*v, fk, ncur);
            }
            for (int f = 0; f < nf; ++f) {
                const int k = fk[f];
                const double* h = &held[(size_t)f * 5];
                X[k] = h[0]; dFdX[k] = h[1]; Xlb[k] = h[2]; Xub[k] = h[3]; dX[k] = h[4];
            }
            if (idx && freeIdxLive) {   // (a level below may have dropped the index map)
                freeIdx.resize(ncur);
                reopen_positions(freeIdx, fk, ncur);
                for (int f = 0; f < nf; ++f) freeIdx[fk[f]] = fi[f];
            }
            for (int i : fi) cI[i] = false;
            if (!scaling.empty()) {
                std::vector<double> scale;
                if (freeIdxLive) {
                    scale.resize(ncur);
                    for (int k = 0; k < ncur; ++k) scale[k] = scaling[freeIdx[k]];
                } else {
                    for (int i = 0; i < Ndim; ++i) if (!cI[i]) scale.push_back(scaling[i]);
                    scale.resize(ncur, 1.0);
                }
                D.setIdentity(&scale);
            } else {
                D.setIdentity();
            }
            tc.stop();
            gradient(X, dX, dFdX, cX, cI);
            PhaseClock tc2(det(kDetCopyBack));
            bool cont = false;
            for (int k : fk) {
                if ((std::fabs(X[k] - Xlb[k]) < q.bndTol) && (dFdX[k] < 0)) cont = true;
                else if ((std::fabs(X[k] - Xub[k]) < q.bndTol) && (dFdX[k] > 0)) cont = true;
            }
            if (freeIdxLive) {
                Nconst = Ndim - ncur;
            } else {
                Nconst = 0;
                for (int i = 0; i < Ndim; ++i) Nconst += cI[i];
            }
            if (Nconst == 0) recurFlag = false;
            optimFlag = cont;
            if (q.verbose > Policy::kRecursedTextAbove && root())
                std::cout << (cont ? "     Optimization continuing after recursive boundary optimization."
                                   : "     Optimization exiting after recursive boundary optimization.")
                          << std::endl;
        } else if (nr == 0) {
            // the coordinates frozen here stay frozen (as in the reference): cI no longer matches
            // the levels above, so they fall back to the full walk
            freeIdxLive = false;
            optimFlag = false;
            if (q.verbose > Policy::kRecursedTextAbove && root())
                std::cout << "      NO VARIABLES LEFT TO OPTIMIZE!!!! " << std::endl;
        }
    }

  private:
    static bool root() { return comm_rank() == ROOT_ID; }
    static double* det(int k) { return Policy::kDetailClocks ? bnd_detail_slot(k) : nullptr; }
    void gradient(std::vector<double>& X, std::vector<double>& dX, std::vector<double>& dFdX, std::vector<double>& cX,
                  std::vector<bool>& cI) {
        PhaseClock t(prof_slot(q.profile, kProfGrad));
        pol.gradient(X, dX, dFdX, cX, cI);
        if (q.profile) q.profile[kProfGradCalls] += 1;
    }

    Policy& pol;
    const BndParams q;
    Objective* objPtr;
    bool& optimFlag;
    int& recurFlag;
    int& totalIter;
    // host bookkeeping of the recursion (no reference counterpart): freeIdx[k] is the full-space
    // index of the current level's coordinate k while freeIdxLive; the caller's pending next
    // direction is released while a reduced problem runs
    std::vector<int> freeIdx;
    bool freeIdxLive = false;
    std::vector<double>* pnextHeld = nullptr;
    bool assessRecursed = false;   // the last assessment re-optimised a reduced problem
    int depth = 0;
};

}  // namespace pnol
