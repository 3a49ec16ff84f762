// bfgs_bnd_batch_cxx.cpp -- BFGS_BndBatch (include/BFGS_bnd_linesearch_Batch.hpp) from a C++11
// program: 3-D Rosenbrock in the box [-1, 5]^3 with the parameters of the reference's bounded
// example (Examples.cpp:75, silent), from the first four starts of the tests' standard grid
// (x0[s][j] = lb + (ub - lb) mod(0.37 s + 0.21 j + 0.05, 1)) as one batch.  Compiled with
// g++ -std=c++0x -Wall -Werror; linked against libpnol_amd.so it runs on a GPU host and prints,
// per start, a line "X x_0 x_1 x_2 f0 fOpt iterations info" with hex doubles
// (tests/test_gpu_bfgs_bnd_batch.py compares them with the batch).
#include <cmath>
#include <cstdio>
#include <exception>
#include <vector>

#include "BFGS_bnd_linesearch_Batch.hpp"

int main() {
    const int n = 3, nstart = 4;
    const double lb = -1.0, ub = 5.0;
    BFGS_BndBatch batch;
    batch.setParams(1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, false, -1);
    std::vector<double> d(n, 1.0), b(n, 0.0);
    batch.setQuadraticData(d, b);   // unused by Rosenbrock
    std::vector<double> X((std::size_t)nstart * n), Xlb(n, lb), Xub(n, ub), f0, fOpt;
    std::vector<int> iters, info;
    for (int s = 0; s < nstart; s++)
        for (int j = 0; j < n; j++) {
            const double a = 0.37 * s, c = 0.21 * j;
            const double t = a + c;
            X[(std::size_t)s * n + j] = lb + (ub - lb) * std::fmod(t + 0.05, 1.0);
        }
    try {
        batch.findMinBnd(PNOL_OBJ_ROSENBROCK, n, 2.0, X, Xlb, Xub, f0, fOpt, iters, info);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (int s = 0; s < nstart; s++) {
        std::printf("X");
        for (int j = 0; j < n; j++) std::printf(" %a", X[(std::size_t)s * n + j]);
        std::printf(" %a %a %d %d\n", f0[s], fOpt[s], iters[s], info[s]);
    }
    return fOpt[0] <= f0[0] ? 0 : 1;
}
