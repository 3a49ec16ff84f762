/*
 * LevenbergMarquardtBatch.hpp  (MI355X-native PNOL addition)
 *
 * Many small curve fits in one GPU launch: nprob independent ExpCurveObjective (n = 3) or
 * CubicObjective (n = 4) problems (Source/ExampleObjectives.hpp:113-201), each run through the
 * whole of LevMarq::findMin (Source/LevenbergMarquardt.cpp:11-167) by one GPU lane in the
 * reference's operation order.  The reference has no batched class; this one stands where a
 * host loop of LevMarq::setParams + findMin over problems would.  setParams has LevMarq's order
 * and defaults; nothing is printed whatever verbose says.
 *
 * Header-only over the C ABI (pnol_run_levmarq_batch, pnol_amd.h): link libpnol_amd.so.
 */
#ifndef PNOL_AMD_LEVENBERGMARQUARDTBATCH_HPP_
#define PNOL_AMD_LEVENBERGMARQUARDTBATCH_HPP_

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "pnol_amd.h"

class LevMarqBatch {
  private:
    double lambda0;
    double dXGrad;
    double xMinDiff;
    double maxIter;
    double lambdaFactor;   // > 1
    int verbose;

  public:
    void setParams(double lambda0In, double lambdaFactorIn, double dXGradIn, double maxIterIn, double xMinDiffIn,
                   int verboseIn) {
        maxIter = maxIterIn; xMinDiff = xMinDiffIn; verbose = verboseIn; dXGrad = dXGradIn;
        lambda0 = lambda0In; lambdaFactor = lambdaFactorIn;
    }

    // kind: PNOL_OBJ_EXPCURVE or PNOL_OBJ_CUBIC.  X holds nprob * n values (x0 in, optima out),
    // yData nprob * m ([nprob][m] row-major), xData m values (one grid for every problem) or
    // nprob * m.  chi0 / chi: chi^2 at x0 and at the optimum, iters: the loop's iter at exit, per
    // problem.  Throws std::invalid_argument on sizes that do not fit, std::runtime_error on a
    // non-zero library status.
    void findMin(int kind, const std::vector<double>& xData, const std::vector<double>& yData,
                 std::vector<double>& X, std::vector<double>& chi0, std::vector<double>& chi,
                 std::vector<int>& iters) {
        const int n = kind == PNOL_OBJ_EXPCURVE ? 3 : 4;
        const std::size_t nprob = X.size() / (std::size_t)n;
        if (nprob == 0 || X.size() != nprob * (std::size_t)n || yData.empty() || yData.size() % nprob != 0)
            throw std::invalid_argument("LevMarqBatch::findMin: X must hold nprob * n and yData nprob * m values");
        const std::size_t m = yData.size() / nprob;
        chi0.assign(nprob, 0.0);
        chi.assign(nprob, 0.0);
        iters.assign(nprob, 0);
        std::vector<long long> evals(nprob, 0);
        const double params[6] = {lambda0, lambdaFactor, dXGrad, maxIter, xMinDiff, (double)verbose};
        const int st = pnol_run_levmarq_batch(kind, n, (int)m, (long long)nprob, xData.data(), xData.size(),
                                              yData.data(), params, X.data(), chi0.data(), chi.data(), iters.data(),
                                              evals.data(), NULL, NULL);
        if (st != PNOL_OK)
            throw std::runtime_error(std::string("LevMarqBatch::findMin: ") + pnol_status_string(st));
    }

    LevMarqBatch() : lambda0(0.001), dXGrad(1e-7), xMinDiff(1e-7), maxIter(10000), lambdaFactor(10), verbose(1) {}
    ~LevMarqBatch() {}
};

#endif /* PNOL_AMD_LEVENBERGMARQUARDTBATCH_HPP_ */
