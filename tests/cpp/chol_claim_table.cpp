// Prints the persistent Cholesky's worker claim order as the kernel computes it
// (csrc/chol_tasks.hpp, the header kernels/chol.hip includes) for tests/test_chol_claim_order.py.
//   chol_claim_table [Tmin Tmax]         every (order, split, rowmajor) for T = Tmin .. Tmax (2 .. 35)
//   chol_claim_table T order split rowmajor    that one table
// Output, one record per line:
//   guard <split> <need> <o(0)> <o(1)> ...   need: the smallest number of worker workgroups at which
//                                            a request for order 1 is kept; o(w): the order used
//                                            with w workers when order 1 is requested
//   table <T> <order> <split> <rowmajor> <ntasks>   followed by ntasks lines, claim index g = 0 ..:
//   <k> <i> <j> <h>
#include <cstdio>
#include <cstdlib>

#include "chol_tasks.hpp"

static void table(int T, int order, bool split, bool rowmajor) {
    const int nt = pnol::chol_step_task_count(T, split);
    std::printf("table %d %d %d %d %d\n", T, order, (int)split, (int)rowmajor, nt);
    for (int g = 0; g < nt; ++g) {
        const pnol::Task t = pnol::task_of(g, T, order, split, rowmajor);
        std::printf("%d %d %d %d\n", t.k, t.i, t.j, t.h);
    }
}

int main(int argc, char** argv) {
    constexpr int kGuardRow = 16;
    for (int split = 0; split < 2; ++split) {
        int need = 0;
        while (pnol::chol_claim_order(1, need, split != 0) != 1) ++need;
        std::printf("guard %d %d", split, need);
        for (int w = 0; w < kGuardRow; ++w) std::printf(" %d", pnol::chol_claim_order(1, w, split != 0));
        std::printf("\n");
    }
    if (argc == 5) {
        table(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]) != 0, std::atoi(argv[4]) != 0);
        return 0;
    }
    const int t0 = argc > 2 ? std::atoi(argv[1]) : 2, t1 = argc > 2 ? std::atoi(argv[2]) : 35;
    for (int T = t0; T <= t1; ++T)
        for (int order = 0; order < 2; ++order)
            for (int split = 0; split < 2; ++split)
                for (int rowmajor = 0; rowmajor < 2; ++rowmajor) table(T, order, split != 0, rowmajor != 0);
    return 0;
}
