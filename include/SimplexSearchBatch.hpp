/*
 * SimplexSearchBatch.hpp  (MI355X-native PNOL addition)
 *
 * Multi-start Nelder-Mead in one GPU launch: nstart independent searches of one built-in scalar
 * objective (RosenbrockObject, PowerObject -- Source/ExampleObjectives.hpp:79-111, :206-234 --
 * or the synthetic quadratic), each run through the whole of SimplexSearch::findMin
 * (Source/SimplexSearch.cpp:13-240) by one GPU lane in the reference's operation order.  Start s
 * draws its initial simplex from the stream seeded seed + s, so it is SimplexSearch with
 * setSeed(seed + s) from the same X, bit for bit (PowerObject with power != 2 excepted: the
 * device pow).  The reference has no batched class; this one stands where a host loop of
 * SimplexSearch::findMin over starting points would.  setSimplexParams has SimplexSearch's order
 * and defaults; nothing is printed whatever verbose says.  n <= PNOL_SIMPLEX_BATCH_NMAX.
 *
 * Header-only over the C ABI (pnol_run_simplex_batch, pnol_amd.h): link libpnol_amd.so.
 */
#ifndef PNOL_AMD_SIMPLEXSEARCHBATCH_HPP_
#define PNOL_AMD_SIMPLEXSEARCHBATCH_HPP_

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "pnol_amd.h"

class SimplexSearchBatch {
  private:
    double alpha, rho, gamma, sigma;
    double initRandMax, xMinDiff;
    int maxIter;
    bool verbose;
    unsigned long long seed;
    std::vector<double> p0, p1;   // PNOL_OBJ_QUADRATIC: d[n], b[n]

  public:
    void setSimplexParams(double alphaIn, double gammaIn, double rhoIn, double sigmaIn, int maxIterIn,
                          double initRandMaxIn, double xMinDiffIn, bool verboseIn) {
        alpha = alphaIn; gamma = gammaIn; rho = rhoIn; sigma = sigmaIn;
        maxIter = maxIterIn; initRandMax = initRandMaxIn; xMinDiff = xMinDiffIn; verbose = verboseIn;
    }
    // start s uses the stream seeded s0 + s (default 0)
    void setSeed(unsigned long long s0) { seed = s0; }
    // the data of PNOL_OBJ_QUADRATIC: f = sum_k (0.5 d_k x_k) x_k - b_k x_k + (0.25 x_k) x_{k+1}
    void setQuadraticData(const std::vector<double>& d, const std::vector<double>& b) { p0 = d; p1 = b; }

    // kind: PNOL_OBJ_ROSENBROCK, PNOL_OBJ_POWER (power: its exponent) or PNOL_OBJ_QUADRATIC.
    // X holds nstart * n values (the starts in, the optima out); f0 / fOpt: f at the start and
    // at the optimum, iters: the loop's iter at exit, per start.  Throws std::invalid_argument
    // on sizes that do not fit, std::runtime_error on a non-zero library status.
    void findMin(int kind, int n, double power, std::vector<double>& X, std::vector<double>& f0,
                 std::vector<double>& fOpt, std::vector<int>& iters) {
        if (n <= 0 || X.empty() || X.size() % (std::size_t)n != 0)
            throw std::invalid_argument("SimplexSearchBatch::findMin: X must hold nstart * n values");
        const std::size_t nstart = X.size() / (std::size_t)n;
        f0.assign(nstart, 0.0);
        fOpt.assign(nstart, 0.0);
        iters.assign(nstart, 0);
        std::vector<long long> evals(nstart, 0);
        const double params[8] = {alpha, gamma, rho, sigma, (double)maxIter, initRandMax, xMinDiff, verbose ? 1.0 : 0.0};
        const int st = pnol_run_simplex_batch(kind, n, power, p0.empty() ? NULL : p0.data(), p0.size(),
                                              p1.empty() ? NULL : p1.data(), p1.size(), (long long)nstart, params,
                                              seed, X.data(), f0.data(), fOpt.data(), iters.data(), evals.data());
        if (st != PNOL_OK)
            throw std::runtime_error(std::string("SimplexSearchBatch::findMin: ") + pnol_status_string(st));
    }

    SimplexSearchBatch()
        : alpha(1.0), rho(0.5), gamma(2.0), sigma(0.5), initRandMax(1), xMinDiff(1e-7), maxIter(10000),
          verbose(false), seed(0) {}
    ~SimplexSearchBatch() {}
};

#endif /* PNOL_AMD_SIMPLEXSEARCHBATCH_HPP_ */
