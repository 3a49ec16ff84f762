// lm_batch_cxx.cpp -- LevMarqBatch (include/LevenbergMarquardtBatch.hpp) from a C++11 program.
// Usage: lm_batch_cxx FILE lambda0 lambdaFactor dXGrad maxIter xMinDiff
// FILE (binary, native endianness): four int64 {kind, nprob, m, xlen}, then xlen doubles of
// xData, nprob * m of yData, nprob * n of x0.  Prints per problem one line
// "X <n values %.17g> chi0 chi iters".  With no arguments: builds the object only (exit 0).
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "LevenbergMarquardtBatch.hpp"

static bool read_all(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    LevMarqBatch lm;
    if (argc < 7) return 0;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    long long hdr[4];
    if (!read_all(f, hdr, sizeof(hdr))) return 2;
    const int kind = (int)hdr[0];
    const size_t nprob = (size_t)hdr[1], m = (size_t)hdr[2], xlen = (size_t)hdr[3];
    const size_t n = kind == PNOL_OBJ_EXPCURVE ? 3 : 4;
    std::vector<double> x(xlen), y(nprob * m), X(nprob * n), chi0, chi;
    std::vector<int> iters;
    if (!read_all(f, x.data(), sizeof(double) * x.size()) || !read_all(f, y.data(), sizeof(double) * y.size()) ||
        !read_all(f, X.data(), sizeof(double) * X.size()))
        return 2;
    std::fclose(f);
    lm.setParams(std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6]), -1);
    try {
        lm.findMin(kind, x, y, X, chi0, chi, iters);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (size_t p = 0; p < nprob; ++p) {
        std::printf("X");
        for (size_t i = 0; i < n; ++i) std::printf(" %.17g", X[p * n + i]);
        std::printf(" %.17g %.17g %d\n", chi0[p], chi[p], iters[p]);
    }
    return 0;
}
