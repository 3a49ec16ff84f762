/*
 * SimplexSearch.hpp  (MI355X-native PNOL drop-in)
 *
 * The reference's Nelder-Mead simplex search (Source/SimplexSearch.hpp:24-66,
 * SimplexSearch.cpp:13-349): a random initial simplex around X, then per trip the centroid of
 * the n best vertices, reflection, expansion or contraction of the worst, or a shrink toward
 * the best, until the simplex is smaller than xMinDiff or maxIter trips ran.  The n + 1
 * vertices of the initial simplex and of a shrink are evaluated as ONE batch: on the device
 * when the objective provides deviceObjective() (pnol_dobj_eval_batch, each point in the
 * objective's own order), otherwise through Objective::objEvalBatch.  The trial points of a
 * trip are inherently sequential and evaluated one by one.  Many independent searches in one
 * GPU launch: SimplexSearchBatch.hpp.
 *
 * Differences from the reference, all documented in DESIGN.md (row f5):
 *  - timeRand() (UtilityFunctionLibrary, absent) is a uniform double from the GA's splitmix64
 *    stream (GARandom), seeded with time(0) like the reference's srand, or with setSeed();
 *  - simplexSort takes the first minimum among the vertices not yet placed (a stable sort by
 *    f), which is the reference's order whenever max f > 0 (its 2*max(f) sentinel breaks
 *    otherwise, as the GA's popSort: parity unpinned there).
 */
#ifndef PNOL_AMD_SIMPLEXSEARCH_HPP_
#define PNOL_AMD_SIMPLEXSEARCH_HPP_

#include <vector>

#include "GeneticAlgorithm.hpp"   // GARandom: the one random stream of the drop-in classes
#include "PNOL_Algorithm.hpp"

using namespace std;

class SimplexSearch : public Algorithm {
  private:
    // simplex parameters
    double alpha, rho, gamma, sigma;
    double initRandMax, xMinDiff;
    int maxIter;
    bool verbose;
    bool seeded;
    unsigned long long seed;
    int iterations;

  public:
    // main optimization function (SimplexSearch.cpp:13-240)
    void findMin(vector<double>& X, double& f0, double& fOpt);

    // f(x) of one vertex / of Nsimplex vertices (SimplexSearch.cpp:243-266); X is scratch of
    // the problem's size and ends as the last point evaluated
    double evaluateVariableArray(double* x, vector<double>& X);
    void evaluateVariableSet(double** xvec, int Nsimplex, vector<double>& X, double* fvec);

    void setSimplexParams(double alphaIn, double gammaIn, double rhoIn, double sigmaIn, int maxIterIn,
                          double initRandMaxIn, double xMinDiffIn, bool verboseIn) {
        alpha = alphaIn; gamma = gammaIn; rho = rhoIn; sigma = sigmaIn;
        maxIter = maxIterIn; initRandMax = initRandMaxIn; xMinDiff = xMinDiffIn; verbose = verboseIn;
    }

    // extensions: a reproducible initial simplex (default: time(0), as the reference's srand),
    // and the number of trips the last findMin ran
    void setSeed(unsigned long long s) { seed = s; seeded = true; }
    int getIterations() const { return iterations; }

    SimplexSearch()
        : alpha(1.0), rho(0.5), gamma(2.0), sigma(0.5), initRandMax(1), xMinDiff(1e-7), maxIter(10000),
          verbose(false), seeded(false), seed(0), iterations(0) {}
    ~SimplexSearch() {}
};

// the reference's free helpers (SimplexSearch.hpp:65-66): the Nd + 1 vertices ordered by f
// ascending, the first of equal values first; the largest |xvec[0][j] - xvec[k][j]| over k >= 1
void simplexSort(double* fvec, double** xvec, int Nd);
double simplexDiff(double** xvec, int Nd, int Nsimplex);

#endif /* PNOL_AMD_SIMPLEXSEARCH_HPP_ */
