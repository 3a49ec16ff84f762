// bfgs_batch_cxx.cpp -- BFGSBatch (include/BFGS_with_linesearch_Batch.hpp) from a C++11 program:
// 5-D Rosenbrock as the reference's testBFGS (Examples.cpp), from the first four starts of the
// tests' standard batch (start s at 3 - 0.01 s in every coordinate) as one batch.  Compiled with
// g++ -std=c++0x -Wall -Werror; linked against libpnol_amd.so it runs on a GPU host and prints,
// per start, a line "X x_0 .. x_4 f0 fOpt gnorm iterations" with %.17g doubles, which read back
// to the same bits (tests/test_gpu_bfgs_batch.py compares them with the restatement).
#include <cstdio>
#include <exception>
#include <vector>

#include "BFGS_with_linesearch_Batch.hpp"

int main() {
    const int n = 5, nstart = 4;
    BFGSBatch batch;
    batch.setParams(1e-4, 0.9, 1e-6, 1, 1000, 1e-7, 1e-3, 100, 1e-5, 1e-5, false, false);
    std::vector<double> d(n, 1.0), b(n, 0.0);
    batch.setQuadraticData(d, b);   // unused by Rosenbrock
    std::vector<double> X((std::size_t)nstart * n), f0, fOpt, gnorm;
    std::vector<int> iters;
    for (int s = 0; s < nstart; s++)
        for (int j = 0; j < n; j++) X[(std::size_t)s * n + j] = 3.0 - 0.01 * s;
    try {
        batch.findMin(PNOL_OBJ_ROSENBROCK, n, 2.0, X, f0, fOpt, gnorm, iters);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (int s = 0; s < nstart; s++) {
        std::printf("X");
        for (int j = 0; j < n; j++) std::printf(" %.17g", X[(std::size_t)s * n + j]);
        std::printf(" %.17g %.17g %.17g %d\n", f0[s], fOpt[s], gnorm[s], iters[s]);
    }
    return fOpt[0] < f0[0] ? 0 : 1;
}
