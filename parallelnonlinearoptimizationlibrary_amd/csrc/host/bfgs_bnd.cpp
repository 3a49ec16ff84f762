// bfgs_bnd.cpp -- bounded BFGS with active-set recursion (drop-in for
// Source/BFGS_bnd_linesearch.cpp) plus the box helpers (Box_boundary_functions.cpp:11-40,
// BFGS_with_bnd_linsearch_MPI.cpp:665-708).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "BFGS_bnd_linesearch.hpp"
#include "bfgs_common.hpp"
#include "deep_stack.hpp"

using namespace pnol;

void checkBoxBounds(std::vector<double>& X, std::vector<double>& Xlb, std::vector<double>& Xub) {
    for (size_t i = 0; i < X.size(); ++i) {
        if (X[i] - Xlb[i] < -std::fabs(Xlb[i]) / 1000 || X[i] - Xub[i] > std::fabs(Xub[i]) / 1000) {
            if (comm_rank() == 0)
                std::cout << std::endl << "!!!!----------------- WARNING -----------------!!!!" << std::endl
                          << "X[" << i << "] = " << X[i] << " is outside of bounds Xlb[i] = " << Xlb[i]
                          << ", Xub[i] = " << Xub[i] << std::endl;
            X[i] = (Xlb[i] + Xub[i]) / 2.0;
            if (comm_rank() == 0)
                std::cout << " Replaced X[" << i << "] with " << X[i] << std::endl
                          << "!!!!----------------- END WARNING -----------------!!!!" << std::endl << std::endl;
        }
    }
}

double computeAlphaBnd(std::vector<double>& X, std::vector<double>& Xlb, std::vector<double>& Xub,
                       std::vector<double>& p) {
    // the same value as the reference's loop: recur::alpha_bnd (eight quotients per AVX-512 step)
    return recur::alpha_bnd(X.data(), Xlb.data(), Xub.data(), p.data(), X.size());
}

double cubicInterpMinSimple(double aa, double ab, double pa, double pb, double da, double db) {
    const double d1 = da + db - 3 * (pa - pb) / (aa - ab);
    const double d2 = sign_of(ab - aa) * std::sqrt(d1 * d1 - da * db);
    double an = ab - (ab - aa) * (db + d2 - d1) / (db - da + 2 * d2);
    if (an < aa || an > ab || an != an) an = (aa + ab) / 2;
    return an;
}

double BFGS_Bnd::lineSearchObj(double alpha, vector<double>& X, vector<double>& p, vector<double>& cX,
                               vector<bool>& cI) {
    std::vector<double> Xa;
    line_point(X, p, alpha, Xa);
    return objPtr->objEvalRecur(Xa, cX, cI);
}

double BFGS_Bnd::lineSearchFDDerivative(double alpha, double phialpha, vector<double>& X, vector<double>& p,
                                        vector<double>& cX, vector<bool>& cI) {
    std::vector<double> Xa;
    line_point(X, p, alpha + dalpha, Xa);
    const double Fa = objPtr->objEvalRecur(Xa, cX, cI);
    return (Fa - phialpha) / dalpha;
}

void BFGS_Bnd::lineSearchZoomBnd(double aa, double ab, double pa, double pb, double da, double db, double phi0,
                                 double dphi0, vector<double>& X, vector<double>& p, vector<double>& cX,
                                 vector<bool>& cI, int& iter_ls, double& aOpt, double& pOpt, double& dOpt) {
    // BFGS_bnd_linesearch.cpp:358-457
    bool success = false;
    while (iter_ls < maxIterLineSearch && (ab - aa > alphaTol)) {
        const double ac = cubicInterpMinSimple(aa, ab, pa, pb, da, db);
        const double a2[2] = {ac, ac + dalpha};   // the (phi, FD slope) pair as one batch
        double f2[2];
        eval_line_points_recur(objPtr, X, p, a2, 2, cX, cI, f2);
        if (profile) profile[kProfPoints] += 2;
        const double pc = f2[0];
        const double dc = (f2[1] - pc) / dalpha;
        double pmin = pa;
        if (pb < pa) pmin = pb;
        if (pc > phi0 + c1 * ac * dphi0 || pc >= pmin) {
            if (pa < pb) { ab = ac; pb = pc; db = dc; }
            else { aa = ac; pa = pc; da = dc; }
        } else {
            if (std::fabs(dc) <= std::fabs(c2 * dphi0)) {
                aOpt = ac; pOpt = pc; dOpt = dc; success = true;
                break;
            }
            if (dc < 0) { aa = ac; pa = pc; da = dc; }
            else { ab = ac; pb = pc; db = dc; }
        }
        iter_ls++;
    }
    if (!success) {
        if (pa < pb) { aOpt = aa; pOpt = pa; dOpt = da; }
        else { aOpt = ab; pOpt = pb; dOpt = db; }
    }
}

void BFGS_Bnd::cubicInterpolationLineSearchBnd(vector<double>& X, vector<double>& Xlb, vector<double>& Xub,
                                               double FX, vector<double>& dFdX, vector<double>& p, vector<double>& cX,
                                               vector<bool>& cI, double& aOpt, double& Fopt) {
    // BFGS_bnd_linesearch.cpp:203-353
    bool success = false, atBound = false;
    double dOpt = 0, phii = 0;
    aOpt = 0;
    Fopt = FX;
    const double phi0 = FX, dphi0 = seq_dot(dFdX, p);
    double aim1 = 0, pim1 = phi0, dim1 = dphi0;
    const double amax = computeAlphaBnd(X, Xlb, Xub, p);
    double ai = alphaGuess;
    if (ai > amax) ai = amax;
    int iter_ls = 0;
    while (iter_ls < maxIterLineSearch) {
        const double a2[2] = {ai, ai + dalpha};
        double f2[2];
        eval_line_points_recur(objPtr, X, p, a2, 2, cX, cI, f2);
        if (profile) profile[kProfPoints] += 2;
        phii = f2[0];
        const double di = (f2[1] - phii) / dalpha;
        if ((phii > phi0 + c1 * ai * dphi0) || (phii >= pim1 && iter_ls > 1)) {
            lineSearchZoomBnd(aim1, ai, pim1, phii, dim1, di, phi0, dphi0, X, p, cX, cI, iter_ls, aOpt, Fopt, dOpt);
            success = true;
            break;
        }
        if (std::fabs(di) <= std::fabs(c2 * dphi0)) { aOpt = ai; Fopt = phii; success = true; break; }
        if (di >= 0) {
            lineSearchZoomBnd(aim1, ai, pim1, phii, dim1, di, phi0, dphi0, X, p, cX, cI, iter_ls, aOpt, Fopt, dOpt);
            success = true;
            break;
        }
        if (ai == amax) { aOpt = ai; Fopt = phii; atBound = true; success = true; break; }
        aim1 = ai; pim1 = phii; dim1 = di;
        ai = 2 * ai;
        if (ai > amax) ai = amax;
        iter_ls++;
    }
    if (!success) {
        if (pim1 < phii) { aOpt = aim1; Fopt = pim1; }
        else if (phi0 < phii) { aOpt = 0; Fopt = phi0; }
        else { aOpt = ai; Fopt = phii; }
    }
    if (verbose > 0 && comm_rank() == ROOT_ID) {
        if (!atBound)
            std::cout << "  Line search completed with alpha = " << aOpt << " and F = " << Fopt << " after " << iter_ls
                      << " iterations. Note: alphaMax = " << amax << std::endl << std::endl;
        else
            std::cout << "  ! Line search terminated at boundary with alpha = " << aOpt << " and F = " << Fopt
                      << " after " << iter_ls << " iterations. Note: alphaMax = " << amax << std::endl << std::endl;
    }
}

// BFGS_Bnd's side of the shared active-set recursion (bfgs_common.hpp): the serial Recur
// gradient, the Wolfe search above, D on one GPU with the next direction out of the update's pass
struct BFGS_Bnd::Policy {
    static constexpr bool kShardD = false, kFusedDirection = true, kDetailClocks = true;
    static constexpr int kStepTextAbove = 1, kRecursedTextAbove = 0;
    BFGS_Bnd& b;
    void gradient(vector<double>& X, vector<double>& dX, vector<double>& dFdX, vector<double>& cX, vector<bool>& cI) {
        b.objPtr->gradientApproximationRecur(X, dX, dFdX, cX, cI);
    }
    void lineSearch(vector<double>& X, vector<double>& Xlb, vector<double>& Xub, double F, vector<double>& dFdX,
                    vector<double>& p, vector<double>& cX, vector<bool>& cI, double& alpha, double& Fopt) {
        b.cubicInterpolationLineSearchBnd(X, Xlb, Xub, F, dFdX, p, cX, cI, alpha, Fopt);
    }
    const char* startText() const { return "  Starting bounded BFGS with line search. "; }
    bool announcesBoundary(int verbose) const { return verbose != 0; }
    void boundaryText(size_t nfrozen, const vector<double>&, double) const {
        std::cout << std::endl << "Optimizer reached box boundary; steepest descent points outside the box at "
                  << nfrozen << " coordinate(s); recursing on the remaining ones." << std::endl;
    }
    BndParams params() const {
        return BndParams{b.bndTol, b.dXGrad, b.dXHess, b.xMinDiff, b.minGrad2Norm, b.maxIter, b.updateMode, b.verbose,
                         b.initHessFD, &b.dXGradVec, &b.initialScalingVec, b.fTrace, b.profile};
    }
};

void BFGS_Bnd::boundaryAssessment(double& F, vector<double>& X, vector<double>& p, vector<double>& dFdX,
                                  DenseInverseHessian& D, vector<double>& Xlb, vector<double>& Xub, vector<double>& dX,
                                  vector<double>& cX, vector<bool>& cI, bool& optimFlag, int& recurFlag) {
    // BFGS_bnd_linesearch.cpp:503-728
    Policy pol{*this};
    ActiveSetRecursion<Policy>(pol, pol.params(), objPtr, optimFlag, recurFlag, totalIter)
        .assess(F, X, p, dFdX, D, Xlb, Xub, dX, cX, cI);
}

void BFGS_Bnd::mainBFGSLoop(double& F, vector<double>& X, vector<double>& dFdX, DenseInverseHessian& D,
                            vector<double>& Xlb, vector<double>& Xub, vector<double>& dX, vector<double>& cX,
                            vector<bool>& cI, bool& optimFlag, int& recurFlag) {
    // BFGS_bnd_linesearch.cpp:116-201
    Policy pol{*this};
    ActiveSetRecursion<Policy>(pol, pol.params(), objPtr, optimFlag, recurFlag, totalIter)
        .mainLoop(F, X, dFdX, D, Xlb, Xub, dX, cX, cI);
}

void BFGS_Bnd::findMinBnd(vector<double>& X, vector<double>& Xlb, vector<double>& Xub, double& f0, double& fOpt) {
    // the active-set recursion goes one level deeper per frozen coordinate (about 11k levels
    // at n = 16384, SURVEY 8(d) cfg 5): run it on a thread with a stack sized for that
    PhaseClock total(prof_slot(profile, kProfTotal));
    run_deep([&] {
        double* det = bnd_detail_all();
        for (int k = 0; k < kDetCount; ++k) det[k] = 0.0;
        for (int k = 0; k < kRdCount; ++k)
            if (double* s = recur_detail(k)) *s = 0.0;
        findMinBndBody(X, Xlb, Xub, f0, fOpt);
        if (bnd_detail_slot(0)) {
            std::fprintf(stderr, "[pnol_amd] BFGS_Bnd host detail (s): freeze %.3f gather+alloc %.3f copyback %.3f iter-loops %.3f\n",
                         det[kDetFreeze], det[kDetGather], det[kDetCopyBack], det[kDetIterLoops]);
            std::fprintf(stderr, "[pnol_amd] Recur FD gradient detail (s): build %.3f check %.3f device %.3f redo %.3f gather %.3f\n",
                         *recur_detail(kRdBuild), *recur_detail(kRdCheck), *recur_detail(kRdDevice),
                         *recur_detail(kRdRedo), *recur_detail(kRdGather));
        }
    });
    if (profile) profile[kProfIters] = totalIter;
}

void BFGS_Bnd::findMinBndBody(vector<double>& X, vector<double>& Xlb, vector<double>& Xub, double& f0,
                              double& fOpt) {
    // BFGS_bnd_linesearch.cpp:15-113
    bool optimFlag = true;
    int recurFlag = 0;
    Policy pol{*this};
    ActiveSetRecursion<Policy>(pol, pol.params(), objPtr, optimFlag, recurFlag, totalIter)
        .findMinBody(X, Xlb, Xub, f0, fOpt);
}
