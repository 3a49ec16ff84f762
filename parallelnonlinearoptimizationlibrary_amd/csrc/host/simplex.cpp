// simplex.cpp -- SimplexSearch (SimplexSearch.cpp:13-349): Nelder-Mead in the reference's control
// flow and operation order, the n + 1 vertices of the initial simplex and of a shrink evaluated
// as one batch.  kernels/simplex_batch.hip runs the same statements, one GPU lane per search.
#include "SimplexSearch.hpp"

#include <cmath>
#include <ctime>
#include <iostream>
#include <stdexcept>

#include "../pnol_internal.hpp"
#include "device_util.hpp"

using namespace pnol;

namespace {

void print_row(const double* x, int n, const char* name) {
    std::cout << name << " = ";
    for (int j = 0; j < n; j++) std::cout << x[j] << " ";
    std::cout << std::endl;
}

}  // namespace

// SimplexSearch.cpp:243-256
double SimplexSearch::evaluateVariableArray(double* x, vector<double>& X) {
    for (size_t j = 0; j < X.size(); j++) X[j] = x[j];
    return objPtr->objEval(X);
}

// SimplexSearch.cpp:258-266, the Nsimplex points as one batch: the device batch for device
// objectives (the objective's own per-point order), objEvalBatch otherwise
void SimplexSearch::evaluateVariableSet(double** xvec, int Nsimplex, vector<double>& X, double* fvec) {
    const int n = (int)X.size();
    if (Nsimplex <= 0) return;
    vector<double> pts((size_t)Nsimplex * n);
    for (int i = 0; i < Nsimplex; i++)
        for (int j = 0; j < n; j++) pts[(size_t)i * n + j] = xvec[i][j];
    for (int j = 0; j < n; j++) X[j] = xvec[Nsimplex - 1][j];   // the reference leaves the last point in X
    if (pnol_dobj* d = objPtr->deviceObjective(n)) {
        check(pnol_dobj_eval_batch(d->ctx, d, pts.data(), Nsimplex, fvec), "dobj_eval_batch(simplex)");
        objPtr->countEvals(Nsimplex);
        return;
    }
    objPtr->objEvalBatch(pts.data(), Nsimplex, n, fvec);
}

// SimplexSearch.cpp:272-327 (selection sort by f): the first minimum among the vertices not yet
// placed -- the reference's order whenever its 2*max(f) sentinel exceeds every f
void simplexSort(double* fvec, double** xvec, int Nd) {
    const int Nsimplex = Nd + 1;
    vector<vector<double>> xs(Nsimplex);
    vector<double> fs(Nsimplex);
    vector<bool> taken(Nsimplex, false);
    for (int k = 0; k < Nsimplex; k++) {
        int best = -1;
        for (int i = 0; i < Nsimplex; i++)
            if (!taken[i] && (best < 0 || fvec[i] < fvec[best])) best = i;
        taken[best] = true;
        xs[k].assign(xvec[best], xvec[best] + Nd);
        fs[k] = fvec[best];
    }
    for (int k = 0; k < Nsimplex; k++) {
        fvec[k] = fs[k];
        for (int j = 0; j < Nd; j++) xvec[k][j] = xs[k][j];
    }
}

// SimplexSearch.cpp:331-349
double simplexDiff(double** xvec, int Nd, int Nsimplex) {
    double xDiffMax = 0;
    for (int k = 1; k < Nsimplex; k++)
        for (int j = 0; j < Nd; j++) {
            const double diff = std::fabs(xvec[0][j] - xvec[k][j]);
            if (diff > xDiffMax) xDiffMax = diff;
        }
    return xDiffMax;
}

// SimplexSearch.cpp:13-240
void SimplexSearch::findMin(vector<double>& X, double& f0, double& fOpt) {
    if (!objPtr) throw std::runtime_error("SimplexSearch: no objective (setObjPtr)");
    const int Ndim = (int)X.size();
    if (Ndim < 1) throw std::runtime_error("SimplexSearch: X is empty");
    const int Nsimplex = Ndim + 1;   // n + 1 points in the simplex
    if (verbose) {
        std::cout << std::endl << "------------------------------------------------------------" << std::endl;
        std::cout << "Computing simplex search with settings " << std::endl;
        std::cout << "alpha = " << alpha << ", gamma = " << gamma << ", rho = " << rho << ", sigma = " << sigma
                  << std::endl;
        std::cout << "------------------------------------------------------------" << std::endl << std::endl;
    }
    vector<double> store((size_t)Nsimplex * Ndim);
    vector<double*> rows(Nsimplex);
    for (int k = 0; k < Nsimplex; k++) rows[k] = store.data() + (size_t)k * Ndim;
    double** xvec = rows.data();
    vector<double> xbar(Ndim), xref(Ndim), xe(Ndim), xc(Ndim), fvec(Nsimplex);

    for (int j = 0; j < Ndim; j++) xvec[0][j] = X[j];
    if (verbose) {
        std::cout << "Initial guess: " << std::endl;
        print_row(xvec[0], Ndim, "X0");
        std::cout << std::endl;
    }
    // the other vertices: X plus a uniform step in [-initRandMax, initRandMax) (:60-67)
    GARandom rng{seeded ? seed : (unsigned long long)time(0)};
    for (int i = 1; i < Nsimplex; i++)
        for (int j = 0; j < Ndim; j++) xvec[i][j] = xvec[0][j] + initRandMax * (rng.next() - 0.5) * 2.0;

    evaluateVariableSet(xvec, Nsimplex, X, fvec.data());
    f0 = fvec[0];
    simplexSort(fvec.data(), xvec, Ndim);

    int iter = 0;
    double xdiff = xMinDiff * 2;
    while (iter < maxIter && xdiff > xMinDiff) {
        // centroid of the first n vertices (:90-101)
        for (int i = 0; i < Ndim; i++) xbar[i] = 0.0;
        for (int i = 0; i < Ndim; i++)
            for (int k = 0; k < Ndim; k++) xbar[i] = xbar[i] + xvec[k][i] / ((double)Ndim);
        // reflection (:105-110)
        for (int i = 0; i < Ndim; i++) xref[i] = xbar[i] + alpha * (xbar[i] - xvec[Nsimplex - 1][i]);
        const double fref = evaluateVariableArray(xref.data(), X);

        if (fref >= fvec[0] && fref < fvec[Ndim - 1]) {
            // 1. neither the best nor among the worst: it replaces the worst (:115-122)
            for (int i = 0; i < Ndim; i++) xvec[Nsimplex - 1][i] = xref[i];
            fvec[Nsimplex - 1] = fref;
        } else if (fref < fvec[0]) {
            // 2. better than the best: expand, keep the better of the two (:124-153)
            for (int i = 0; i < Ndim; i++) xe[i] = xbar[i] + gamma * (xbar[i] - xvec[Nsimplex - 1][i]);
            const double fe = evaluateVariableArray(xe.data(), X);
            const bool useE = fe < fref;
            for (int i = 0; i < Ndim; i++) xvec[Nsimplex - 1][i] = useE ? xe[i] : xref[i];
            fvec[Nsimplex - 1] = useE ? fe : fref;
        } else {
            // 3. contract (:155-191)
            for (int i = 0; i < Ndim; i++) xc[i] = xbar[i] + rho * (xvec[Nsimplex - 1][i] - xbar[i]);
            const double fc = evaluateVariableArray(xc.data(), X);
            if (fc < fvec[Nsimplex - 1]) {
                for (int i = 0; i < Ndim; i++) xvec[Nsimplex - 1][i] = xc[i];
                fvec[Nsimplex - 1] = fc;
            } else {
                // everything failed: shrink toward the best vertex, which stays, and evaluate
                // all n + 1 again
                for (int k = 1; k < Nsimplex; k++)
                    for (int i = 0; i < Ndim; i++) xvec[k][i] = xvec[0][i] + sigma * (xvec[k][i] - xvec[0][i]);
                evaluateVariableSet(xvec, Nsimplex, X, fvec.data());
            }
        }
        simplexSort(fvec.data(), xvec, Ndim);
        xdiff = simplexDiff(xvec, Ndim, Nsimplex);
        if (verbose && iter % 10 == 0)
            std::cout << "At iter = " << iter << " the xdiff is " << xdiff
                      << " with a minimum function evaluation of " << fvec[0] << std::endl;
        iter = iter + 1;
    }
    iterations = iter;
    fOpt = fvec[0];
    for (int j = 0; j < Ndim; j++) X[j] = xvec[0][j];
    if (verbose) {
        std::cout << std::endl << "-----------------------------------------------------------------------------------"
                  << std::endl;
        std::cout << "Completed simplex search." << std::endl;
        std::cout << "f0 = " << f0 << ", fOpt = " << fOpt << " with variable:" << std::endl;
        print_row(xvec[0], Ndim, "X");
        std::cout << "-----------------------------------------------------------------------------------" << std::endl
                  << std::endl;
    }
}
