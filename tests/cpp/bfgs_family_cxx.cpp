// bfgs_family_cxx.cpp -- the five host BFGS drop-in classes driven directly from a C++11 program
// (g++ -std=c++0x -Wall -Werror, linked against libpnol_amd.so; needs a GPU), for what the C
// drivers do not reach: setinitialScalingVec / setGradVec and each class's printed text.
//
//   bfgs_family_cxx scaling     BFGS_Bnd ("alternating", n = 12) and BFGS_Bnd_MPI_SW (setPoolSize(4),
//                               the testBFGSBnd_MPI geometry, n = 10), each run three times: with
//                               neither vector set ("none"), with a scaling vector of all 1.0 and
//                               a dXGradVec of all dXGrad ("unit"), and with scaling alternating
//                               0.5 / 2.0 and dXGradVec alternating 1e-6 / 2e-6 ("pair").  One line
//                               per run: "R <class> <variant> <evals> <f0> <fOpt> <X...>", doubles as %a.
//   bfgs_family_cxx --record    the "pair" runs as the JSON of tests/golden/bfgs_family_parent.json
//   bfgs_family_cxx text <cls> [v]  one of BFGS, BFGS_MPI, BFGSBnd_MPI, BFGS_Bnd, BFGS_Bnd_MPI_SW at its
//                               loudest verbosity on Rosenbrock n = 3 from (-1, 2, 2), maxIter 6
//                               (the bounded ones in the box [-1, 5]^3, "lower-active"): stdout is
//                               the class's own text (tests/golden/bfgs_family_stdout_<cls>.txt).
//                               v: another verbosity for BFGS_Bnd / BFGS_Bnd_MPI_SW, whose messages
//                               have per-class thresholds (..._stdout_<cls>_v<v>.txt)
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "BFGS_bnd_linesearch.hpp"
#include "BFGS_bnd_linesearch_MPI_SW.hpp"
#include "BFGS_with_bnd_linesearch_MPI.hpp"
#include "BFGS_with_linesearch.hpp"
#include "BFGS_with_linesearch_MPI.hpp"
#include "ExampleObjectives.hpp"

struct Run {
    std::vector<double> X;
    double f0, fOpt;
    long evals;
};

// variant 0: neither vector; 1: the unit pair; 2: the alternating pair
template <class Solver>
static void set_vectors(Solver& b, int n, int variant, double dXGrad) {
    if (variant == 0) return;
    std::vector<double> scale(n, 1.0), dx(n, dXGrad);
    if (variant == 2)
        for (int i = 0; i < n; i++) {
            scale[i] = i % 2 ? 2.0 : 0.5;
            dx[i] = i % 2 ? 2e-6 : 1e-6;
        }
    b.setinitialScalingVec(scale);
    b.setGradVec(dx);
}

static Run run_bnd(int variant) {   // test_bfgs_bnd_matches_oracle's "alternating"
    const int n = 12;
    RosenbrockObject obj;
    BFGS_Bnd b;
    b.setParams(1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, false, -1);
    set_vectors(b, n, variant, 1e-6);
    b.setObjPtr(obj);
    Run r;
    r.X.resize(n);
    for (int i = 0; i < n; i++) r.X[i] = i % 2 ? -0.2 : 0.2;
    std::vector<double> lb(n, -0.3), ub(n, 0.6);
    b.findMinBnd(r.X, lb, ub, r.f0, r.fOpt);
    r.evals = (long)obj.getEvals();
    return r;
}

static Run run_sw(int variant) {   // test_bfgs_bnd_mpi_sw_box_cases' "testBFGSBnd_MPI-geometry"
    const int n = 10;
    RosenbrockObject obj;
    BFGS_Bnd_MPI_SW b;
    b.setParams(1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, false, -1);
    b.setPoolSize(4);
    set_vectors(b, n, variant, 1e-6);
    b.setObjPtr(obj);
    Run r;
    r.X.assign(n, 3.0);
    r.X[0] = -0.5;
    std::vector<double> lb(n, -5.0), ub(n, 5.0);
    lb[0] = -1.0;
    b.findMinBnd(r.X, lb, ub, r.f0, r.fOpt);
    r.evals = (long)obj.getEvals();
    return r;
}

static void print_line(const char* cls, const char* variant, const Run& r) {
    std::printf("R %s %s %ld %a %a", cls, variant, r.evals, r.f0, r.fOpt);
    for (std::size_t i = 0; i < r.X.size(); i++) std::printf(" %a", r.X[i]);
    std::printf("\n");
}

static void print_json(const char* cls, const Run& r, const char* tail) {
    std::printf("  \"%s\": {\"evals\": %ld, \"f0\": \"%a\", \"fOpt\": \"%a\", \"X\": [", cls, r.evals, r.f0, r.fOpt);
    for (std::size_t i = 0; i < r.X.size(); i++) std::printf("%s\"%a\"", i ? ", " : "", r.X[i]);
    std::printf("]}%s\n", tail);
}

static int text(const std::string& cls, const char* level) {
    RosenbrockObject obj;
    std::vector<double> X(3, 2.0), lb(3, -1.0), ub(3, 5.0);
    X[0] = -1.0;
    double f0 = 0, fOpt = 0;
    if (cls == "BFGS") {
        BFGS b;
        b.setParams(1e-4, 0.9, 1e-6, 1, 1000, 1e-7, 1e-3, 6, 1e-5, 1e-5, false, true);
        b.setObjPtr(obj);
        b.findMin(X, f0, fOpt);
    } else if (cls == "BFGS_MPI") {
        BFGS_MPI b;
        b.setParams(1e-4, 0.1, 4, 1, 1000, 1e-7, 1e-3, 6, 1e-5, 1e-5, false, true);
        b.setPoolSize(4);
        b.setObjPtr(obj);
        b.findMin(X, f0, fOpt);
    } else if (cls == "BFGSBnd_MPI") {
        BFGSBnd_MPI b;
        b.setParams(1e-4, 0.1, 1e-16, 4, 1, 1000, 1e-7, 1e-3, 6, 1e-5, 1e-5, 1e-5, false, true);
        b.setPoolSize(4);
        b.setObjPtr(obj);
        b.findMinBnd(X, lb, ub, f0, fOpt);
    } else if (cls == "BFGS_Bnd") {
        BFGS_Bnd b;
        b.setParams(1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 6, 1e-5, 1e-5, false, level ? std::atoi(level) : 2);
        b.setObjPtr(obj);
        b.findMinBnd(X, lb, ub, f0, fOpt);
    } else if (cls == "BFGS_Bnd_MPI_SW") {
        BFGS_Bnd_MPI_SW b;
        b.setParams(1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 6, 1e-5, 1e-5, false, level ? std::atoi(level) : 3);
        b.setPoolSize(4);
        b.setObjPtr(obj);
        b.findMinBnd(X, lb, ub, f0, fOpt);
    } else {
        std::fprintf(stderr, "unknown class %s\n", cls.c_str());
        return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "scaling";
    try {
        if (mode == "text" && argc > 2) return text(argv[2], argc > 3 ? argv[3] : 0);
        if (mode == "--record") {
            const Run a = run_bnd(2), b = run_sw(2);
            std::printf("{\n");   // after the runs: whatever the solvers printed comes before it
            print_json("BFGS_Bnd", a, ",");
            print_json("BFGS_Bnd_MPI_SW", b, "");
            std::printf("}\n");
            return 0;
        }
        if (mode == "scaling") {
            const char* names[3] = {"none", "unit", "pair"};
            for (int v = 0; v < 3; v++) {
                const Run a = run_bnd(v);
                print_line("BFGS_Bnd", names[v], a);
            }
            for (int v = 0; v < 3; v++) {
                const Run b = run_sw(v);
                print_line("BFGS_Bnd_MPI_SW", names[v], b);
            }
            return 0;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::fprintf(stderr, "usage: bfgs_family_cxx [scaling | --record | text <class> [verbose]]\n");
    return 2;
}
