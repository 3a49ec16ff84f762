// bfgs_mpi.cpp -- BFGS_MPI: sharded FD gradient + pooled secant line search (drop-in for
// Source/BFGS_with_linesearch_MPI.cpp).  The pool of trial step sizes is evaluated round-robin
// over the ranks and gathered with one allgather per round (:163-223).
#include <cmath>
#include <cstdio>
#include <iostream>

#include "BFGS_with_linesearch_MPI.hpp"
#include "bfgs_common.hpp"

using namespace pnol;

void findPoolBounds(vector<double>& ap, vector<double>& pp, double a0, double p0, double& a1, double& a2, double& p1,
                    double& p2) {
    // BFGS_with_linesearch_MPI.cpp:496-530.  The reference reads past the pool end when the
    // minimum is its last entry (undefined behaviour); the index is clamped to the pool.
    double pmin; int imin;
    vector_min(pp, pmin, imin);
    const int N = (int)pp.size();
    const int hi = imin + 1 < N ? imin + 1 : N - 1;
    if (p0 < pmin) {
        a1 = a0; a2 = ap[0]; p1 = p0; p2 = pp[0];
    } else if (p0 >= pmin && imin == 0) {
        a1 = a0; a2 = ap[hi]; p1 = p0; p2 = pp[hi];
    } else {
        a1 = ap[imin - 1]; a2 = ap[hi]; p1 = pp[imin - 1]; p2 = pp[hi];
    }
}

double BFGS_MPI::lineSearchObj(double alpha, vector<double>& X, vector<double>& p) {
    std::vector<double> Xa;
    line_point(X, p, alpha, Xa);
    return objPtr->objEval(Xa);
}

void BFGS_MPI::evalAlphaPoolMPI(vector<double>& alphaPool, vector<double>& phiPool, vector<double>& X,
                                vector<double>& p) {
    // entry k is owned by rank k mod P (:186-197); one allgather of ceil(N/P) values per rank
    const PoolSlots ps((int)phiPool.size(), comm_size());
    std::vector<double> mine(ps.per, 0.0);
    std::vector<double> mya;   // this rank's entries, one batch
    for (int k = comm_rank(); k < ps.N; k += ps.P) mya.push_back(alphaPool[k]);
    eval_line_points(objPtr, X, p, mya.data(), (int)mya.size(), mine.data());
    pool_exchange(ps, 1, mine, phiPool.data());
}

void BFGS_MPI::secantLineSearch(vector<double>& X, double FX, vector<double>& dFdX, vector<double>& p,
                                double& alphaOpt, double& Fopt) {
    // BFGS_with_linesearch_MPI.cpp:226-492: the result is read from the zoom pool, so a search
    // that never zooms reports the untouched zero pool (alpha 0, F 0, :483-488) unless fixZeroPool
    SecantSearch o;
    o.c1 = c1; o.c2 = c2; o.maxAlphaMult = maxAlphaMult; o.alphaGuess = alphaGuess;
    o.maxIterLineSearch = maxIterLineSearch; o.Npool = poolSize > 0 ? poolSize : comm_size();
    o.Xlb = o.Xub = nullptr; o.verbose = false;   // no box
    o.alphaMinStop = false; o.alphaMin = 0;
    o.resultFromZoomPool = true; o.fixZeroPool = fixZeroPool;
    secant_pool_search(o, [&](vector<double>& ap, vector<double>& pp) { evalAlphaPoolMPI(ap, pp, X, p); }, X, FX,
                       dFdX, p, alphaOpt, Fopt);
}

void BFGS_MPI::findMin(vector<double>& X, double& f0, double& fOpt) {
    // BFGS_with_linesearch_MPI.cpp:12-142
    require_comm("BFGS_MPI::findMin");   // Npool = Nprocs of MPI_COMM_WORLD (:231-235)
    const bool say = verbose && comm_rank() == 0;
    // D row-sharded over the ranks; no profile
    const QuasiNewtonParams q{dXGrad, dXHess, xMinDiff, minGrad2Norm, maxIter, updateMode, initHessFD, true, nullptr};
    quasi_newton_loop(
        q, objPtr, X, f0, fOpt,
        [&](vector<double>& x, vector<double>& dX, vector<double>& g) { objPtr->gradientApproximationMPI(x, dX, g); },
        [&](vector<double>& x, double F, vector<double>& g, vector<double>& p, double& alpha, double& Fopt) {
            secantLineSearch(x, F, g, p, alpha, Fopt);
        },
        [&](int iter, double xdiff, double gnorm, double F) {
            if (!say) return;
            std::cout << "---> At iter = " << iter << " the mean abs xdiff is " << xdiff << " and the grad2norm = "
                      << gnorm << std::endl;
            std::cout << "                 with a minimum function evaluation of " << F << std::endl;
        },
        [&](double f0v, double fOptv, const vector<double>& x) {
            if (!say) return;
            std::cout << std::endl << "-----------------------------------------------------------------------------------" << std::endl;
            std::cout << "Completed bfgs." << std::endl;
            std::cout << "f0 = " << f0v << ", fOpt = " << fOptv << " with variable:" << std::endl << "X = ";
            print_vec(x);
            std::cout << "-----------------------------------------------------------------------------------" << std::endl << std::endl;
        });
}
