// bfgs_helpers.hpp -- the small pure helpers of the host BFGS family (bfgs*.cpp; print_vec also
// levmarq.cpp): restatements of the reference's utility library, the in-place compaction of the
// active-set recursion, and the owner / slot arithmetic of the pooled line searches.  Standard
// library only -- no device, no communicator -- so tests/cpp/bfgs_common_check.cpp runs them
// under AddressSanitizer / UBSan as a stand-alone program.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <vector>

namespace pnol {

inline double sign_of(double x) { return x > 0 ? 1.0 : (x < 0 ? -1.0 : 0.0); }

inline void print_vec(const std::vector<double>& v) {
    for (double x : v) std::printf("%.17g ", x);
    std::printf("\n");
}

// the first minimum / maximum of v and its index
inline void vector_min(const std::vector<double>& v, double& val, int& idx) {
    val = v[0]; idx = 0;
    for (size_t i = 1; i < v.size(); ++i) if (v[i] < val) { val = v[i]; idx = (int)i; }
}
inline void vector_max(const std::vector<double>& v, double& val, int& idx) {
    val = v[0]; idx = 0;
    for (size_t i = 1; i < v.size(); ++i) if (v[i] > val) { val = v[i]; idx = (int)i; }
}

// v_i = a + i (b - a) / (N - 1)
inline void linspace(double a, double b, int N, std::vector<double>& v) {
    v.resize(N);
    for (int i = 0; i < N; ++i) v[i] = a + i * (b - a) / (N - 1);
}

// Xa = X + alpha p, the trial point of every lineSearchObj / lineSearchFDDerivative (alpha is
// the already-rounded step, alpha + dalpha included)
inline void line_point(const std::vector<double>& X, const std::vector<double>& p, double alpha,
                       std::vector<double>& Xa) {
    Xa.resize(X.size());
    for (size_t i = 0; i < X.size(); ++i) Xa[i] = X[i] + alpha * p[i];
}

// drop positions fk (ascending) of v[0, n): the kept entries slide down run by run
template <class T>
void drop_positions(std::vector<T>& v, const std::vector<int>& fk, int n) {
    if (fk.empty()) return;
    int dst = fk[0];
    for (size_t f = 0; f < fk.size(); ++f) {
        const int b = fk[f] + 1, e = f + 1 < fk.size() ? fk[f + 1] : n;
        std::copy(v.begin() + b, v.begin() + e, v.begin() + dst);
        dst += e - b;
    }
}
// the inverse: reopen the gaps at positions fk of v[0, n) (their contents are the caller's)
template <class T>
void reopen_positions(std::vector<T>& v, const std::vector<int>& fk, int n) {
    int hi = n;
    for (int f = (int)fk.size() - 1; f >= 0; --f) {
        const int b = fk[f] + 1;
        std::copy_backward(v.begin() + (b - f - 1), v.begin() + (hi - f - 1), v.begin() + hi);
        hi = fk[f];
    }
}

// A pool of N line-search entries dealt over P ranks: entry k is owned by rank k mod P as its
// slot k / P; every rank contributes `per` slots (at least one, so an empty pool still takes
// part in the collective) and the gathered buffer holds rank r's slots at [r per, (r + 1) per).
struct PoolSlots {
    int N, P, per;
    PoolSlots(int n, int p) : N(n), P(p), per((n + p - 1) / p > 0 ? (n + p - 1) / p : 1) {}
    int owner(int k) const { return k % P; }
    int slot(int k) const { return k / P; }
    size_t at(int k) const { return (size_t)owner(k) * per + slot(k); }   // in the gathered buffer
};

}  // namespace pnol
