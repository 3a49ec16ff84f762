/*
 * BFGS_with_linesearch_Batch.hpp  (MI355X-native PNOL addition)
 *
 * Multi-start BFGS in one GPU launch: nstart independent solves of one built-in scalar objective
 * (RosenbrockObject, PowerObject -- Source/ExampleObjectives.hpp:79-111, :206-234 -- or the
 * synthetic quadratic), each run through the whole of BFGS::findMin
 * (Source/BFGS_with_linesearch.cpp:12-432: FD gradient, cubic-interpolation Wolfe line search,
 * the update D <- M1 D M2 + M3) by one GPU lane in the reference's operation order.  Start s is
 * BFGS::findMin from the same X and parameters, bit for bit (PowerObject with power != 2
 * excepted: the device pow).  The reference has no batched class; this one stands where a host
 * loop of BFGS::findMin over starting points would.  setParams has BFGS's order and defaults;
 * initHessFD is not offered (the library reports it as unsupported), dXHess is unused and nothing
 * is printed whatever verbose says.  n <= PNOL_BFGS_BATCH_NMAX.
 *
 * Header-only over the C ABI (pnol_run_bfgs_batch, pnol_amd.h): link libpnol_amd.so.
 */
#ifndef PNOL_AMD_BFGS_WITH_LINESEARCH_BATCH_HPP_
#define PNOL_AMD_BFGS_WITH_LINESEARCH_BATCH_HPP_

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "pnol_amd.h"

class BFGSBatch {
  private:
    double c1, c2;
    double dalpha;
    double alphaGuess;
    int maxIterLineSearch;
    double dXGrad;
    double dXHess;
    double xMinDiff;
    double minGrad2Norm;
    int maxIter;
    bool initHessFD;
    bool verbose;
    std::vector<double> p0, p1;   // PNOL_OBJ_QUADRATIC: d[n], b[n]

  public:
    // same order as BFGS::setParams (BFGS_with_linesearch.hpp:62); maxIter arrives as a double
    void setParams(double c1In, double c2In, double dalphaIn, double alphaGuessIn, int maxIterLineSearchIn,
                   double dXGradIn, double dXHessIn, double maxIterIn, double xMinDiffIn, double minGrad2NormIn,
                   bool initHessFDIn, bool verboseIn) {
        c1 = c1In; c2 = c2In; dalpha = dalphaIn; alphaGuess = alphaGuessIn;
        maxIterLineSearch = maxIterLineSearchIn; dXGrad = dXGradIn; dXHess = dXHessIn;
        maxIter = (int)maxIterIn; xMinDiff = xMinDiffIn; minGrad2Norm = minGrad2NormIn;
        initHessFD = initHessFDIn; verbose = verboseIn;
    }
    // the data of PNOL_OBJ_QUADRATIC: f = sum_k (0.5 d_k x_k) x_k - b_k x_k + (0.25 x_k) x_{k+1}
    void setQuadraticData(const std::vector<double>& d, const std::vector<double>& b) { p0 = d; p1 = b; }

    // kind: PNOL_OBJ_ROSENBROCK, PNOL_OBJ_POWER (power: its exponent) or PNOL_OBJ_QUADRATIC.
    // X holds nstart * n values (the starts in, the optima out); f0 / fOpt: f at the start and
    // at the optimum, gnorm: the loop's last gradient 2-norm (above minGrad2Norm for a start
    // that ended through an exhausted line search or maxIter), iters: the loop's iter at exit,
    // per start.  Throws std::invalid_argument on sizes that do not fit, std::runtime_error on a
    // non-zero library status.
    void findMin(int kind, int n, double power, std::vector<double>& X, std::vector<double>& f0,
                 std::vector<double>& fOpt, std::vector<double>& gnorm, std::vector<int>& iters) {
        if (n <= 0 || X.empty() || X.size() % (std::size_t)n != 0)
            throw std::invalid_argument("BFGSBatch::findMin: X must hold nstart * n values");
        const std::size_t nstart = X.size() / (std::size_t)n;
        f0.assign(nstart, 0.0);
        fOpt.assign(nstart, 0.0);
        gnorm.assign(nstart, 0.0);
        iters.assign(nstart, 0);
        std::vector<long long> evals(nstart, 0);
        const double params[12] = {c1, c2, dalpha, alphaGuess, (double)maxIterLineSearch, dXGrad, dXHess,
                                   (double)maxIter, xMinDiff, minGrad2Norm, initHessFD ? 1.0 : 0.0,
                                   verbose ? 1.0 : 0.0};
        const int st = pnol_run_bfgs_batch(kind, n, power, p0.empty() ? NULL : p0.data(), p0.size(),
                                           p1.empty() ? NULL : p1.data(), p1.size(), (long long)nstart, params,
                                           X.data(), f0.data(), fOpt.data(), gnorm.data(), iters.data(), evals.data());
        if (st != PNOL_OK)
            throw std::runtime_error(std::string("BFGSBatch::findMin: ") + pnol_status_string(st));
    }

    BFGSBatch()
        : c1(1e-4), c2(0.9), dalpha(1e-6), alphaGuess(1), maxIterLineSearch(1000), dXGrad(1e-6), dXHess(1e-3),
          xMinDiff(1e-5), minGrad2Norm(1e-5), maxIter(10000), initHessFD(false), verbose(false) {}
    ~BFGSBatch() {}
};

#endif /* PNOL_AMD_BFGS_WITH_LINESEARCH_BATCH_HPP_ */
