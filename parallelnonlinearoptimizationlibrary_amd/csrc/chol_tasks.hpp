// chol_tasks.hpp -- the persistent tile Cholesky's worker claim order (kernels/chol.hip,
// k_chol_persist), in plain C++17 for the device and the host alike: the kernel and its launcher
// include it, and tests/cpp/chol_claim_table.cpp prints it for tests/test_chol_claim_order.py,
// which checks that the order is a permutation of the step tasks and that it drains.
#pragma once

#ifdef __HIPCC__
#define PNOL_HD __host__ __device__
#else
#define PNOL_HD
#endif

namespace pnol {

// The workers' claim order: claim index g -> step k and task -- a panel row i (L_ik, b_i), or
// an update tile (i, j) -= L_ik L_jk^T.  Step k (R = T-1-k panel rows) holds
// S_k = R + R (R + 1) / 2 - 1 tasks, local index l: panels l < R, then the update tiles in
// column order with the two the chain needs next first (l = R: (k+2, k+1), l = R+1: (k+2, k+2)).
//   order 0: step by step (every task waits only on tasks claimed before it).
//   order 1: each step's critical set C_k (l in {0, 1, R, R+1}; {0} for R = 1) one step early:
//            C_0, C_1, rest_0, C_2, rest_1, ..., C_{T-2}, rest_{T-3}, rest_{T-2}.  A task of C_{k+1}
//            may wait on a task of rest_k claimed after it: up to a whole critical set of workers
//            can wait on unclaimed tasks, so this order needs more workers than that
//            (chol_claim_order).
// (By tile column -- all of a column's updates before the next column's panels, every
// dependency claimed first -- measured 1.23 ms per solve against 0.60: the workers pile up on
// far-column tasks waiting for the chain while runnable updates stay unclaimed.)
// Order 1 against order 0: 6 of 6 same-box bench pairs faster, +0.5-1% LM iters/s.
struct Task {
    int k, i, j;   // j < 0: panel row i of step k
    int h;         // >= 0: the 32-row half h of a split critical update
};

// tasks of one critical set: panels k+1, k+2 and the two updates the chain needs next (as four
// halves when they are split)
PNOL_HD inline int chol_crit_tasks(bool split) { return split ? 6 : 4; }

// The order the workers use when `order` is asked for: order 1 lets each critical set's tasks
// wait on unclaimed ones, so it holds only with more worker workgroups (the chain's not counted)
// than one critical set has tasks; below that, step order.
PNOL_HD inline int chol_claim_order(int order, int workers, bool split) {
    return order == 1 && workers <= chol_crit_tasks(split) ? 0 : order;
}

// tasks of step k (R = T - 1 - k panel rows), with the split critical updates
PNOL_HD inline int step_tasks(int R, bool split) { return R + R * (R + 1) / 2 - 1 + (split && R >= 2 ? 2 : 0); }

// all the step tasks of a T-tile factorisation (steps 0 .. T-2)
PNOL_HD inline int chol_step_task_count(int T, bool split) {
    int n = 0;
    for (int R = T - 1; R >= 1; --R) n += step_tasks(R, split);
    return n;
}

// the reducing form's first tasks: b, then the T (T + 1) / 2 lower tiles
PNOL_HD inline int chol_reduce_task_count(int T) { return 1 + T * (T + 1) / 2; }

// split: the two critical updates (l = R, R + 1) are four half tasks (l = R .. R + 3), the other
// updates one index later by two.  rowmajor: the updates after the critical two by tile row
// (rows k+3, k+4, ..., each from column k+1 to the diagonal) instead of by tile column: the chain
// needs row d's tiles at step d - 1, so the rows near the diagonal come first.
PNOL_HD inline Task task_local(int k, int l, int T, bool split, bool rowmajor = false) {
    const int R = T - 1 - k;
    if (l < R) return {k, k + 1 + l, -1, -1};
    int q = l - R;
    if (split && R >= 2) {
        if (q < 4) return {k, k + 2, q < 2 ? k + 1 : k + 2, q & 1};
        q -= 2;
    }
    if (rowmajor && q >= 2) {
        int r = q - 2, i = k + 3;   // row i holds the tiles (i, k+1) .. (i, i): i - k of them
        while (r >= i - k) {
            r -= i - k;
            ++i;
        }
        return {k, i, k + 1 + r, -1};
    }
    // full column order f: column k+1 holds f = 0 .. R-1 (f = 0 is the chain's), column k+2
    // starts at f = R, ...
    int u = q == 0 ? 1 : (q == 1 ? R : (q < R ? q : q + 1));
    int j = k + 1;
    while (u >= T - j) {
        u -= T - j;
        ++j;
    }
    return {k, j + u, j, -1};
}

PNOL_HD inline Task task_of(int g, int T, int order, bool split, bool rowmajor = false) {
    if (order == 1) {
        const int nc = chol_crit_tasks(split);
        auto csz = [&](int kk) { return T - 1 - kk >= 2 ? nc : 1; };
        auto cmap = [&](int x, int RR) { return x < 2 ? x : RR + x - 2; };
        if (g < csz(0)) return task_local(0, cmap(g, T - 1), T, split, rowmajor);
        g -= csz(0);
        for (int kk = 0;; ++kk) {
            if (kk + 1 <= T - 2) {
                const int c1 = csz(kk + 1);
                if (g < c1) return task_local(kk + 1, cmap(g, T - 2 - kk), T, split, rowmajor);
                g -= c1;
            }
            const int RR = T - 1 - kk, S = step_tasks(RR, split), rest = S - csz(kk);
            if (g < rest || kk >= T - 2)   // rest_kk: the panels past the first two, the updates past C_kk's
                return task_local(kk, g < RR - 2 ? g + 2 : g + (RR >= 2 ? nc : 4), T, split, rowmajor);
            g -= rest;
        }
    }
    int k = 0, R = T - 1;
    for (;;) {
        const int S = step_tasks(R, split);
        if (g < S || R <= 1) break;
        g -= S;
        ++k;
        --R;
    }
    return task_local(k, g, T, split, rowmajor);
}

}  // namespace pnol
