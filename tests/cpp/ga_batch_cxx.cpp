// ga_batch_cxx.cpp -- GeneticAlgorithmBatch (include/GeneticAlgorithmBatch.hpp) from a C++11
// program: 3-D Rosenbrock in the box [-2, 2]^3, four runs from x0 = -1 on the streams 1000 .. 1003
// with Npop = 40, maxGenerations = 200, NstaticGenerations = 20 (the first four runs of the tests'
// case "ros3") as one batch.  Compiled with g++ -std=c++0x -Wall -Werror; linked against
// libpnol_amd.so it runs on a GPU host and prints, per run, a line
// "X x_0 x_1 x_2 f0 fOpt generations evaluations info" with hex doubles
// (tests/test_gpu_ga_batch.py compares them with the batch).
#include <cstdio>
#include <exception>
#include <vector>

#include "GeneticAlgorithmBatch.hpp"

int main() {
    const int n = 3, nrun = 4;
    GeneticAlgorithmBatch batch;
    batch.setGAParams(40, 200, 0.1, 0.3, 0.2, 0.5, 0.01, 0.5, 20, false, false);
    batch.setSeed(1000);
    batch.setObjective(PNOL_OBJ_ROSENBROCK, n);
    std::vector<double> X((std::size_t)nrun * n, -1.0), Xlb(n, -2.0), Xub(n, 2.0), f0, fOpt;
    try {
        batch.findMinBnd(X, Xlb, Xub, f0, fOpt);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (int s = 0; s < nrun; s++) {
        std::printf("X");
        for (int j = 0; j < n; j++) std::printf(" %a", X[(std::size_t)s * n + j]);
        std::printf(" %a %a %d %lld %d\n", f0[s], fOpt[s], batch.getGenerations()[s], batch.getEvaluations()[s],
                    batch.getInfo()[s]);
    }
    return fOpt[0] <= f0[0] ? 0 : 1;
}
