// bfgs_common_check.cpp -- the pure helpers of the host BFGS family (csrc/host/bfgs_helpers.hpp).
// Built with -fsanitize=address,undefined by tests/test_bfgs_common.py; no device, no HIP.
//  - drop_positions / reopen_positions, for every n <= 8 and every subset fk of positions: the
//    compaction equals a naive gather of the kept entries, and reopening followed by writing
//    the held entries restores the original.  The vectors are exactly n long, so a copy past
//    either end is a sanitizer report.
//  - PoolSlots, for every N <= 12 and P <= 8: every entry has exactly one (owner, slot), all
//    slots are below per, and the gathered-buffer index round-trips.
//  - linspace's end points and vector_min / vector_max's first-extremum tie-breaking on literals.
// Exit 0 = clean.
#include <cstdio>
#include <vector>

#include "host/bfgs_helpers.hpp"

using namespace pnol;

template <class T>
static int check_positions(int n, unsigned mask) {
    std::vector<T> orig(n), kept;
    std::vector<int> fk;
    for (int i = 0; i < n; ++i) {
        orig[i] = (T)(100 + i);
        if (mask >> i & 1) fk.push_back(i);
        else kept.push_back(orig[i]);
    }
    std::vector<T> v = orig, held;
    for (int k : fk) held.push_back(v[k]);
    drop_positions(v, fk, n);
    v.resize(kept.size());
    v.shrink_to_fit();
    if (v != kept) return std::printf("drop_positions: n %d mask %#x\n", n, mask), 1;
    v.resize(n);
    v.shrink_to_fit();
    reopen_positions(v, fk, n);
    for (size_t f = 0; f < fk.size(); ++f) v[fk[f]] = held[f];
    if (v != orig) return std::printf("reopen_positions: n %d mask %#x\n", n, mask), 1;
    return 0;
}

static int check_pool(int N, int P) {
    const PoolSlots ps(N, P);
    const int cdiv = (N + P - 1) / P;
    if (ps.per != (cdiv > 0 ? cdiv : 1)) return std::printf("per: N %d P %d\n", N, P), 1;
    std::vector<int> entry((size_t)ps.per * P, -1);   // which entry sits at each gathered index
    for (int k = 0; k < N; ++k) {
        const int r = ps.owner(k), q = ps.slot(k);
        if (r < 0 || r >= P || q < 0 || q >= ps.per) return std::printf("range: N %d P %d k %d\n", N, P, k), 1;
        if (r + q * P != k) return std::printf("round trip: N %d P %d k %d\n", N, P, k), 1;
        if (ps.at(k) != (size_t)r * ps.per + q) return std::printf("at: N %d P %d k %d\n", N, P, k), 1;
        if (entry[ps.at(k)] != -1) return std::printf("shared slot: N %d P %d k %d\n", N, P, k), 1;
        entry[ps.at(k)] = k;
    }
    // rank r's q-th own entry (k = r, r + P, ...) is its slot q
    for (int r = 0; r < P; ++r) {
        int q = 0;
        for (int k = r; k < N; k += P, ++q)
            if (entry[(size_t)r * ps.per + q] != k) return std::printf("deal: N %d P %d k %d\n", N, P, k), 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    for (int n = 0; n <= 8; ++n)
        for (unsigned mask = 0; mask < (1u << n); ++mask) {
            bad += check_positions<double>(n, mask);
            bad += check_positions<int>(n, mask);
        }
    for (int N = 0; N <= 12; ++N)
        for (int P = 1; P <= 8; ++P) bad += check_pool(N, P);

    std::vector<double> v;
    linspace(0.1, 0.7, 4, v);
    if (v.size() != 4 || v[0] != 0.1 || v[3] != 0.1 + 3 * (0.7 - 0.1) / 3) bad += std::printf("linspace ends\n");
    linspace(2.0, -1.0, 7, v);
    if (v.size() != 7 || v[0] != 2.0 || v[6] != -1.0) bad += std::printf("linspace descending\n");
    double val;
    int idx;
    vector_min({3.0, 1.0, 2.0, 1.0, 5.0}, val, idx);
    if (val != 1.0 || idx != 1) bad += std::printf("vector_min tie\n");
    vector_min({4.0}, val, idx);
    if (val != 4.0 || idx != 0) bad += std::printf("vector_min single\n");
    vector_max({3.0, 5.0, 2.0, 5.0}, val, idx);
    if (val != 5.0 || idx != 1) bad += std::printf("vector_max tie\n");
    if (sign_of(-2.0) != -1.0 || sign_of(0.0) != 0.0 || sign_of(3.0) != 1.0) bad += std::printf("sign_of\n");
    std::vector<double> Xa;
    line_point({1.0, 2.0}, {0.5, -1.0}, 2.0, Xa);
    if (Xa.size() != 2 || Xa[0] != 2.0 || Xa[1] != 0.0) bad += std::printf("line_point\n");

    if (bad) return 1;
    std::printf("bfgs_common_check: clean\n");
    return 0;
}
