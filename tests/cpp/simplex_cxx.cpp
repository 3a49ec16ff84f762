// simplex_cxx.cpp -- SimplexSearch (include/SimplexSearch.hpp) and SimplexSearchBatch
// (include/SimplexSearchBatch.hpp) from a C++11 program: a 10-D Rosenbrock as the reference's
// testSimplexSearch (Examples.cpp:456-485), then the same starts as one batch.  Compile check
// (g++ -std=c++0x -Wall -Werror -c); linked against libpnol_amd.so it runs on a GPU host.
#define PNOL_AMD_NO_MPI_BIND   // no MPI in this program, whatever headers the host has
#include <cstdio>
#include <exception>
#include <vector>

#include "SimplexSearch.hpp"
#include "SimplexSearchBatch.hpp"

class Rosenbrock : public Objective {
  public:
    double objEval(vector<double>& X) {
        double f = 0.0;
        for (size_t k = 0; k + 1 < X.size(); k++) {
            const double t = X[k + 1] - X[k] * X[k], u = 1.0 - X[k];
            f = f + (100.0 * (t * t) + u * u);
        }
        return f;
    }
};

int main() {
    const int n = 10;
    Rosenbrock obj;
    SimplexSearch simplex;
    simplex.setSimplexParams(1.0, 2.0, 0.5, 0.5, 400, 1.0, 1e-7, false);
    simplex.setSeed(20261021ull);
    simplex.setObjPtr(obj);
    vector<double> X(n, 3.0);
    double f0 = 0.0, fOpt = 0.0;
    simplex.findMin(X, f0, fOpt);
    std::printf("SimplexSearch: f0 %.17g fOpt %.17g iterations %d\n", f0, fOpt, simplex.getIterations());

    double* rows[3];
    double pts[3][2] = {{0.0, 0.0}, {1.0, 0.0}, {0.0, 2.0}};
    double fv[3] = {2.0, 1.0, 1.0};
    for (int k = 0; k < 3; k++) rows[k] = pts[k];
    simplexSort(fv, rows, 2);
    std::printf("simplexDiff %.17g\n", simplexDiff(rows, 2, 3));

    SimplexSearchBatch batch;
    batch.setSimplexParams(1.0, 2.0, 0.5, 0.5, 400, 1.0, 1e-7, false);
    batch.setSeed(20261021ull);
    std::vector<double> Xs(4 * n, 3.0), f0s, fOpts;
    std::vector<int> iters;
    try {
        batch.findMin(PNOL_OBJ_ROSENBROCK, n, 2.0, Xs, f0s, fOpts, iters);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::printf("SimplexSearchBatch: start 0 fOpt %.17g iterations %d\n", fOpts[0], iters[0]);
    return fOpts[0] == fOpt && iters[0] == simplex.getIterations() ? 0 : 1;
}
