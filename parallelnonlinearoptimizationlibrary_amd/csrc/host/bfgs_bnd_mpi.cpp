// bfgs_bnd_mpi.cpp -- BFGSBnd_MPI: box-bounded BFGS with a pooled secant line search and
// active-set recursion (drop-in for Source/BFGS_with_bnd_linsearch_MPI.cpp).  The pool is
// evaluated round-robin over the ranks and gathered with one allgather per round (the
// reference's zero-padded MPI_Reduce + Bcast, :314-344, is exact for one owner per entry).
// The reduced problem starts from the free-free block of D, gathered on the device (:822-843).
#include <cmath>
#include <cstdio>
#include <iostream>
#include <stdexcept>

#include "BFGS_with_bnd_linesearch_MPI.hpp"
#include "bfgs_common.hpp"

using namespace pnol;

void checkAlphaPoolBnd(bool& bndIndicator, vector<double>& alphaPool, vector<double>& X, vector<double>& Xlb,
                       vector<double>& Xub, vector<double>& p, vector<double>&, vector<bool>&) {
    // BFGS_with_bnd_linsearch_MPI.cpp:711-743
    const int Npool = (int)alphaPool.size();
    bndIndicator = false;
    const double alphaBnd = computeAlphaBnd(X, Xlb, Xub, p);
    for (int i = 0; i < Npool; ++i)
        if (alphaPool[i] > alphaBnd) bndIndicator = true;
    if (bndIndicator) {
        const double deltaAlpha = alphaBnd / (Npool);
        for (int i = 0; i < Npool; ++i) alphaPool[i] = deltaAlpha * (i + 1);
    }
    for (int i = 0; i < Npool; ++i)
        if (alphaPool[i] < 0) alphaPool[i] = 0;
}

double BFGSBnd_MPI::lineSearchObj(double alpha, vector<double>& X, vector<double>& p, vector<double>& cX,
                                  vector<bool>& cI) {
    // :246-258
    std::vector<double> Xa;
    line_point(X, p, alpha, Xa);
    return objPtr->objEvalRecur(Xa, cX, cI);
}

void BFGSBnd_MPI::evalAlphaPoolMPI(vector<double>& alphaPool, vector<double>& phiPool, vector<double>& X,
                                   vector<double>& p, vector<double>& cX, vector<bool>& cI) {
    // :262-354: entry k is owned by rank k mod P; one allgather of ceil(N/P) values per rank
    const PoolSlots ps((int)phiPool.size(), comm_size());
    std::vector<double> mine(ps.per, 0.0);
    std::vector<double> mya;   // this rank's entries, one batch
    for (int k = comm_rank(); k < ps.N; k += ps.P) mya.push_back(alphaPool[k]);
    eval_line_points_recur(objPtr, X, p, mya.data(), (int)mya.size(), cX, cI, mine.data());
    pool_exchange(ps, 1, mine, phiPool.data());
    for (int k = 0; k < ps.N; ++k)
        if (phiPool[k] != phiPool[k] || std::isinf(phiPool[k]))
            throw std::runtime_error("BFGSBnd_MPI: line search produced a NaN/inf objective value");
}

void BFGSBnd_MPI::secantLineSearchBnd(vector<double>& X, vector<double>& Xlb, vector<double>& Xub, double FX,
                                      vector<double>& dFdX, vector<double>& p, double& alphaOpt, double& Fopt,
                                      vector<double>& cX, vector<bool>& cI) {
    // :358-660: pools clipped to the box, zoom stopped below alphaMin, and the result is the
    // minimum of the last evaluated pool (:651-655)
    SecantSearch o;
    o.c1 = c1; o.c2 = c2; o.maxAlphaMult = maxAlphaMult; o.alphaGuess = alphaGuess;
    o.maxIterLineSearch = maxIterLineSearch; o.Npool = poolSize > 0 ? poolSize : comm_size();
    o.Xlb = &Xlb; o.Xub = &Xub; o.verbose = verbose;
    o.alphaMinStop = true; o.alphaMin = alphaMin;
    o.resultFromZoomPool = false; o.fixZeroPool = false;
    secant_pool_search(o, [&](vector<double>& ap, vector<double>& pp) { evalAlphaPoolMPI(ap, pp, X, p, cX, cI); }, X,
                       FX, dFdX, p, alphaOpt, Fopt);
}

void BFGSBnd_MPI::boundaryAssessment(double& F, vector<double>& X, vector<double>& p, vector<double>& dFdX,
                                     DenseInverseHessian& D, vector<double>& Xlb, vector<double>& Xub,
                                     vector<double>& dX, vector<double>& cX, vector<bool>& cI, bool& optimFlag,
                                     bool& recurFlag) {
    // :748-934.  Called only at the top level (recurFlag false), where X has all Ndim entries.
    const int Ndim = (int)cX.size();
    bool bndFlag = false;
    int iRecur = 0;
    for (int i = 0; i < Ndim; ++i) {
        if (cI[i]) continue;
        if ((std::fabs(X[iRecur] - Xlb[iRecur]) < dXGrad) && (p[iRecur] < 0)) {
            bndFlag = true; cI[i] = true; cX[i] = X[iRecur];
        } else if (std::fabs(X[iRecur] - Xub[iRecur]) < dXGrad && (p[iRecur] > 0)) {
            bndFlag = true; cI[i] = true; cX[i] = X[iRecur];
        }
        iRecur++;
    }
    int Nconst = 0;
    for (int i = 0; i < Ndim; ++i) Nconst += cI[i];
    if (bndFlag && verbose && comm_rank() == ROOT_ID) {
        std::cout << std::endl << " Optimizer reached box boundary and found that the steepest descent is directed "
                  << "outside of the boundary at " << Nconst << " coordinate(s)." << std::endl << "    X = ";
        print_vec(X);
        std::cout << "    F = " << F << std::endl;
    }
    const int nr = Ndim - Nconst;
    if (!(bndFlag && nr > 0)) return;

    double FRecur = F;
    std::vector<double> XR, gR, lbR, ubR, dXR;
    std::vector<int> idx;
    for (int i = 0; i < Ndim; ++i)
        if (!cI[i]) {
            XR.push_back(X[i]); gR.push_back(dFdX[i]); lbR.push_back(Xlb[i]); ubR.push_back(Xub[i]);
            dXR.push_back(dX[i]); idx.push_back(i);
        }
    DenseInverseHessian DR(require_ctx(), nr, updateMode, true);
    DR.setSubmatrixOf(D, idx);
    recurFlag = true;
    mainBFGSLoop(FRecur, XR, gR, DR, lbR, ubR, dXR, cX, cI, optimFlag, recurFlag);

    // the reduced solution goes back into X; F keeps its pre-recursion value, as in the
    // reference (FRecur is not copied back, :845-864)
    for (int a = 0; a < nr; ++a) {
        const int i = idx[a];
        X[i] = XR[a]; dFdX[i] = gR[a]; Xlb[i] = lbR[a]; Xub[i] = ubR[a]; dX[i] = dXR[a];
    }
    D.setIdentity();
    objPtr->gradientApproximationMPI(X, dX, dFdX);

    // release everything, then re-freeze where the gradient still points out of the box
    for (int i = 0; i < Ndim; ++i) {
        cI[i] = false;
        if ((std::fabs(X[i] - Xlb[i]) < dXGrad) && (dFdX[i] > 0)) {
            bndFlag = true; cI[i] = true; cX[i] = X[i];
        } else if (std::fabs(X[i] - Xub[i]) < dXGrad && (dFdX[i] < 0)) {
            bndFlag = true; cI[i] = true; cX[i] = X[i];
        }
    }
    Nconst = 0;
    for (int i = 0; i < Ndim; ++i) Nconst += cI[i];
    optimFlag = Nconst == 0;
    recurFlag = false;
    if (verbose && comm_rank() == ROOT_ID)
        std::cout << (optimFlag ? "Optimization continuing after recursive boundary optimization, as the gradient "
                                  "through the boundary points to the domain interior."
                                : "Optimization exiting after recursive boundary optimization, as the gradient "
                                  "through the boundary still points out of the domain.")
                  << std::endl;
}

void BFGSBnd_MPI::mainBFGSLoop(double& F, vector<double>& X, vector<double>& dFdX, DenseInverseHessian& D,
                               vector<double>& Xlb, vector<double>& Xub, vector<double>& dX, vector<double>& cX,
                               vector<bool>& cI, bool& optimFlag, bool& recurFlag) {
    // :84-243
    const int n = (int)X.size();
    double Fprev = 2 * F;
    if (verbose && comm_rank() == ROOT_ID) {
        std::cout << std::endl << "Starting bounded BFGS loop with F(X) = " << F << " over " << n << " variables."
                  << std::endl << "    X = ";
        print_vec(X);
    }
    std::vector<double> Xprev(n, 0.0), dFdXprev = dFdX, p(n), s(n), g(n);
    D.direction(dFdX, p);
    int iter = 0;
    double xdiff = xMinDiff * 2, grad2Norm = 2 * minGrad2Norm, alpha = alphaMin * 2;
    while (iter < maxIter && xdiff > xMinDiff && grad2Norm > minGrad2Norm && alpha > alphaMin && optimFlag) {
        double Fopt = 0;
        secantLineSearchBnd(X, Xlb, Xub, F, dFdX, p, alpha, Fopt, cX, cI);
        // a step that misses the tolerance is retried along steepest descent (:153-166)
        if (F - Fopt < FStepTolerance) {
            // printed on the root rank whatever the verbosity (BFGS_with_bnd_linsearch_MPI.cpp:156-158)
            if (comm_rank() == ROOT_ID)
                std::cout << "Line search failed in the quasi-newton direction. Recomputing gradient and "
                          << "attempting steepest descent instead." << std::endl;
            objPtr->gradientApproximationMPIRecur(X, dX, dFdX, cX, cI);
            for (int i = 0; i < n; ++i) p[i] = -dFdX[i];
            secantLineSearchBnd(X, Xlb, Xub, F, dFdX, p, alpha, Fopt, cX, cI);
        }
        for (int i = 0; i < n; ++i) { Xprev[i] = X[i]; X[i] = X[i] + alpha * p[i]; }
        Fprev = F;
        F = Fopt;
        objPtr->gradientApproximationMPIRecur(X, dX, dFdX, cX, cI);
        for (int i = 0; i < n; ++i) { s[i] = alpha * p[i]; g[i] = dFdX[i] - dFdXprev[i]; }
        // the update is skipped on a zero curvature product (:189-192)
        if (seq_dot(g, s) != 0) D.update(g, s, &dFdX, &p);
        else D.direction(dFdX, p);
        dFdXprev = dFdX;
        if (F > Fprev) optimFlag = false;
        xdiff = 0;
        for (int i = 0; i < n; ++i) xdiff += std::fabs(X[i] - Xprev[i]);
        grad2Norm = std::sqrt(seq_dot(dFdX, dFdX));
        if (verbose && comm_rank() == ROOT_ID) {
            std::cout << std::endl << "---> At iter = " << iter << " the mean abs xdiff is " << xdiff
                      << " and the grad2norm = " << grad2Norm << std::endl << "    X = ";
            print_vec(X);
            std::cout << "    with a minimum function evaluation of " << F << std::endl;
        }
        if (!recurFlag) boundaryAssessment(F, X, p, dFdX, D, Xlb, Xub, dX, cX, cI, optimFlag, recurFlag);
        iter = iter + 1;
    }
}

void BFGSBnd_MPI::findMinBnd(vector<double>& X, vector<double>& Xlb, vector<double>& Xub, double& f0,
                             double& fOpt) {
    // :14-81
    require_comm("BFGSBnd_MPI::findMinBnd");
    const int n = (int)X.size();
    std::vector<double> cX(n, 0.0), dX(n, dXGrad), dFdX(n, 0.0);
    std::vector<bool> cI(n, false);
    checkBoxBounds(X, Xlb, Xub);
    DenseInverseHessian D(require_ctx(), n, updateMode, true);   // row-sharded over the ranks
    if (initHessFD) init_from_fd_hessian(objPtr, X, dXHess, D);
    else D.setIdentity();
    objPtr->gradientApproximationMPI(X, dX, dFdX);
    double F = objPtr->objEval(X);
    f0 = F;
    bool optimFlag = true, recurFlag = false;
    mainBFGSLoop(F, X, dFdX, D, Xlb, Xub, dX, cX, cI, optimFlag, recurFlag);
    fOpt = F;
    if (verbose && comm_rank() == ROOT_ID) {
        std::cout << std::endl << "Completed bounded bfgs." << std::endl << "f0 = " << f0 << ", fOpt = " << fOpt
                  << " with variable:" << std::endl << "X = ";
        print_vec(X);
    }
}
