/*
 * BFGS_bnd_linesearch_Batch.hpp  (MI355X-native PNOL addition)
 *
 * Multi-start box-bounded BFGS in one GPU launch: nstart independent solves of one built-in
 * scalar objective (RosenbrockObject, PowerObject -- Source/ExampleObjectives.hpp:79-111, :206-234
 * -- or the synthetic quadratic) in one box shared by all starts, each run through the whole of
 * BFGS_Bnd::findMinBnd (Source/BFGS_bnd_linesearch.cpp:15-750: checkBoxBounds, FD gradient over
 * the free coordinates, the bounded cubic-interpolation Wolfe line search, the update
 * D <- M1 D M2 + M3, the active-set recursion of boundaryAssessment) by one GPU lane in the
 * reference's operation order.  Start s is BFGS_Bnd::findMinBnd from the same X, box and
 * parameters, bit for bit (PowerObject with power != 2 excepted: the device pow), with one
 * exception, the corner end: when an assessment at recursion depth >= 1 leaves no free
 * coordinate, the reference goes on with a constant indicator that no longer matches its reduced
 * vectors (undefined behaviour); the batch ends such a start there -- X the full-space point,
 * every coordinate at a bound with an outward direction or gradient, fOpt the level's F -- and
 * sets PNOL_BFGS_BND_BATCH_CORNER in info.  The reference has no batched class; this one stands
 * where a host loop of BFGS_Bnd::findMinBnd over starting points would.  setParams has
 * BFGS_Bnd's order and defaults; initHessFD is not offered (the library reports it as
 * unsupported), nor are setGradVec, setinitialScalingVec and setUpdateMode; alphaMult and dXHess
 * are unused and nothing is printed whatever verbose says.  n <= PNOL_BFGS_BND_BATCH_NMAX.
 *
 * Header-only over the C ABI (pnol_run_bfgs_bnd_batch, pnol_amd.h): link libpnol_amd.so.
 */
#ifndef PNOL_AMD_BFGS_BND_LINESEARCH_BATCH_HPP_
#define PNOL_AMD_BFGS_BND_LINESEARCH_BATCH_HPP_

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "pnol_amd.h"

class BFGS_BndBatch {
  private:
    double c1, c2;
    double dalpha;
    double alphaGuess;
    double alphaTol;
    double alphaMult;
    int maxIterLineSearch;
    double bndTol;
    double dXGrad;
    double dXHess;
    double xMinDiff;
    double minGrad2Norm;
    int maxIter;
    bool initHessFD;
    int verbose;
    std::vector<double> p0, p1;   // PNOL_OBJ_QUADRATIC: d[n], b[n]

  public:
    // same order as BFGS_Bnd::setParams (BFGS_bnd_linesearch.hpp:80-99); maxIter arrives as a double
    void setParams(double c1In, double c2In, double dalphaIn, double alphaGuessIn, double alphaTolIn,
                   double alphaMultIn, int maxIterLineSearchIn, double bndTolIn, double dXGradIn, double dXHessIn,
                   double maxIterIn, double xMinDiffIn, double minGrad2NormIn, bool initHessFDIn, int verboseIn) {
        c1 = c1In; c2 = c2In; dalpha = dalphaIn; alphaGuess = alphaGuessIn; alphaTol = alphaTolIn;
        alphaMult = alphaMultIn; maxIterLineSearch = maxIterLineSearchIn; bndTol = bndTolIn; dXGrad = dXGradIn;
        dXHess = dXHessIn; maxIter = (int)maxIterIn; xMinDiff = xMinDiffIn; minGrad2Norm = minGrad2NormIn;
        initHessFD = initHessFDIn; verbose = verboseIn;
    }
    // the data of PNOL_OBJ_QUADRATIC: f = sum_k (0.5 d_k x_k) x_k - b_k x_k + (0.25 x_k) x_{k+1}
    void setQuadraticData(const std::vector<double>& d, const std::vector<double>& b) { p0 = d; p1 = b; }

    // kind: PNOL_OBJ_ROSENBROCK, PNOL_OBJ_POWER (power: its exponent) or PNOL_OBJ_QUADRATIC.
    // X holds nstart * n values (the starts in, the optima out), Xlb / Xub the box (n values
    // each); f0 / fOpt: f at the start and at the optimum, iters: totalIter (the trips of all
    // recursion levels), info: the deepest recursion level in bits 0-7 and
    // PNOL_BFGS_BND_BATCH_CORNER for a corner end, per start.  Throws std::invalid_argument on
    // sizes that do not fit, std::runtime_error on a non-zero library status.
    void findMinBnd(int kind, int n, double power, std::vector<double>& X, const std::vector<double>& Xlb,
                    const std::vector<double>& Xub, std::vector<double>& f0, std::vector<double>& fOpt,
                    std::vector<int>& iters, std::vector<int>& info) {
        if (n <= 0 || X.empty() || X.size() % (std::size_t)n != 0)
            throw std::invalid_argument("BFGS_BndBatch::findMinBnd: X must hold nstart * n values");
        if (Xlb.size() != (std::size_t)n || Xub.size() != (std::size_t)n)
            throw std::invalid_argument("BFGS_BndBatch::findMinBnd: Xlb and Xub must hold n values");
        const std::size_t nstart = X.size() / (std::size_t)n;
        f0.assign(nstart, 0.0);
        fOpt.assign(nstart, 0.0);
        iters.assign(nstart, 0);
        info.assign(nstart, 0);
        std::vector<long long> evals(nstart, 0);
        const double params[15] = {c1, c2, dalpha, alphaGuess, alphaTol, alphaMult, (double)maxIterLineSearch,
                                   bndTol, dXGrad, dXHess, (double)maxIter, xMinDiff, minGrad2Norm,
                                   initHessFD ? 1.0 : 0.0, (double)verbose};
        const int st = pnol_run_bfgs_bnd_batch(kind, n, power, p0.empty() ? NULL : p0.data(), p0.size(),
                                               p1.empty() ? NULL : p1.data(), p1.size(), (long long)nstart, params,
                                               Xlb.data(), Xub.data(), X.data(), f0.data(), fOpt.data(), iters.data(),
                                               evals.data(), info.data());
        if (st != PNOL_OK)
            throw std::runtime_error(std::string("BFGS_BndBatch::findMinBnd: ") + pnol_status_string(st));
    }

    // BFGS_Bnd's defaults
    BFGS_BndBatch()
        : c1(1e-4), c2(0.9), dalpha(1e-6), alphaGuess(1), alphaTol(1e-20), alphaMult(2), maxIterLineSearch(50),
          bndTol(1e-5), dXGrad(1e-6), dXHess(1e-3), xMinDiff(1e-5), minGrad2Norm(1e-5), maxIter(10000),
          initHessFD(false), verbose(0) {}
    ~BFGS_BndBatch() {}
};

#endif /* PNOL_AMD_BFGS_BND_LINESEARCH_BATCH_HPP_ */
