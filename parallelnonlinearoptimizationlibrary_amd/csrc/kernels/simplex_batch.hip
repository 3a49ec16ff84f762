// simplex_batch.hip -- batched Nelder-Mead: many independent simplex searches in one launch (gfx950).
//
// One lane owns one start and runs that start's whole SimplexSearch::findMin
// (SimplexSearch.cpp:13-240, host form: host/simplex.cpp), every statement in that order, so a
// start's result does not depend on the batch it is in and -- the built-in objectives being the
// sequential sum of scalar_term (scalar_terms.hpp), the expression the host objEval compiles --
// equals SimplexSearch with setSeed(seed + s) bit for bit (Power with power != 2 calls the
// device pow and is not bitwise against the host).
//
// State.  The row a lane touches (worst, best, a sorted position) differs per lane and is indexed
// at run time, so the simplex cannot live in registers (it would go to scratch).  It lives in
// LDS, lane-minor: slot q of lane l is lds[q * 64 + l], an 8-byte access whose bank depends on
// the lane alone -- conflict-free whatever slot each lane picks.  Slots per lane:
//     [0, (n+1) n)        the n + 1 vertices, physical row r at r * n
//     + n + 1             the values, by SORTED position
//     + n, + n, + n       xbar, xref, the second trial point (expansion or contraction)
// (n + 1)^2 + 3 n doubles per lane: n = 12 -> 205 x 512 B = 105 KB, one workgroup per CU;
// n = 10 -> 77 KB, two per CU; n <= 5 -> <= 26 KB.
//
// Sort.  Rows never move: a 4-bit-per-position permutation in one 64-bit register maps sorted
// position -> physical row (n + 1 <= 13 nibbles).  Outside a shrink only the replaced worst
// vertex moves; inserting it after every vertex whose value is <= its own is the order of the
// host's stable selection sort.  The initial simplex and a shrink run that insertion for every
// position in turn (a stable insertion sort).
//
// Divergence.  Lanes take different branches each trip; the objective is evaluated at three
// call sites the lanes reach together: every active lane's reflection, then the second point of
// every lane that needs one (expansion or contraction), then the n + 1 vertices of the rare
// lanes that shrink.
#include "lane_batch.hpp"

namespace pnol {
namespace {

// doubles of LDS per lane
constexpr int sx_slots(int n) { return (n + 1) * (n + 1) + 3 * n; }
static_assert(sizeof(double) * sx_slots(PNOL_SIMPLEX_BATCH_NMAX) * kLaneBatchLanes <= kLaneBatchLdsMax,
              "the largest simplex must fit one CU's LDS");
static_assert(4 * (PNOL_SIMPLEX_BATCH_NMAX + 1) <= 64, "one nibble per sorted position in the 64-bit permutation");

// physical row at sorted position k
__device__ __forceinline__ int sx_row(unsigned long long perm, int k) { return (int)((perm >> (4 * k)) & 15ull); }

// The vertex at sorted position k (value v, the values before it sorted) goes after every vertex
// whose value is <= v: values shift up, the permutation's nibble k moves down to the new place.
__device__ __forceinline__ void sx_insert(double* fv, unsigned long long& perm, int k, double v) {
    int p = k;
    while (p > 0) {
        const double prev = fv[(p - 1) * kLaneBatchLanes];
        if (!(prev > v)) break;
        fv[p * kLaneBatchLanes] = prev;
        --p;
    }
    fv[p * kLaneBatchLanes] = v;
    if (p != k) {
        const unsigned long long r = (perm >> (4 * k)) & 15ull;
        const unsigned long long lo = (1ull << (4 * p)) - 1ull;            // positions < p
        const unsigned long long upto = (1ull << (4 * k)) - 1ull;          // positions < k
        const unsigned long long hi = ~((1ull << (4 * (k + 1))) - 1ull);   // positions > k (k + 1 <= 13)
        perm = (perm & lo) | ((perm & upto & ~lo) << 4) | (r << (4 * p)) | (perm & hi);
    }
}

template <int KIND>
__global__ __launch_bounds__(kLaneBatchLanes) void k_simplex_batch(
    int n, size_t nstart, const double* __restrict__ p0, const double* __restrict__ p1, double power, double alpha,
    double gamma, double rho, double sigma, int maxIter, double initRandMax, double xMinDiff, unsigned long long seed,
    double* __restrict__ Xio, double* __restrict__ f0out, double* __restrict__ fopt, int* __restrict__ iters,
    long long* __restrict__ evals) {
    extern __shared__ __attribute__((aligned(16))) double sx_lds[];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * kLaneBatchLanes + lane;
    const bool valid = s < nstart;
    double* const xv = sx_lds + lane;                   // vertices: row r, coordinate j at (r * n + j)
    double* const fv = xv + (n + 1) * n * kLaneBatchLanes;     // values by sorted position
    double* const xbar = fv + (n + 1) * kLaneBatchLanes;
    double* const xref = xbar + n * kLaneBatchLanes;
    double* const x2 = xref + n * kLaneBatchLanes;
    const double dn = (double)n;

    // the initial simplex (SimplexSearch.cpp:46-67): vertex 0 is X, vertex i >= 1 adds
    // initRandMax * (u - 0.5) * 2.0 per coordinate, one draw per (i, j), i outer
    for (int j = 0; j < n; ++j) xv[j * kLaneBatchLanes] = valid ? Xio[s * (size_t)n + j] : 0.0;
    unsigned long long state = seed + (unsigned long long)s;
    for (int i = 1; i <= n; ++i)
        for (int j = 0; j < n; ++j) {
            unsigned long long z = (state += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            const double u = (double)(z >> 11) * 0x1.0p-53;
            xv[(i * n + j) * kLaneBatchLanes] = xv[j * kLaneBatchLanes] + initRandMax * (u - 0.5) * 2.0;
        }
    // all n + 1 vertices, f0 = the value of vertex 0, sort (:70-75)
    unsigned long long perm = 0xFEDCBA9876543210ull;
    double f0 = 0.0;
    for (int k = 0; k <= n; ++k) {
        const double v = lane_eval<KIND>(xv + k * n * kLaneBatchLanes, n, p0, p1, power);
        if (k == 0) f0 = v;
        sx_insert(fv, perm, k, v);
    }
    long long ev = n + 1;
    int iter = 0;
    double xdiff = xMinDiff * 2;
    bool active = valid && iter < maxIter && xdiff > xMinDiff;

    while (__any(active)) {
        double* const xw = xv + sx_row(perm, n) * n * kLaneBatchLanes;   // the worst vertex
        // ---- phase 1: centroid of the n best, reflection (:90-110)
        double fref = 0.0;
        if (active) {
            for (int i = 0; i < n; ++i) {
                double xb = 0.0;
                for (int k = 0; k < n; ++k) xb = xb + xv[(sx_row(perm, k) * n + i) * kLaneBatchLanes] / dn;
                xbar[i * kLaneBatchLanes] = xb;
                xref[i * kLaneBatchLanes] = xb + alpha * (xb - xw[i * kLaneBatchLanes]);
            }
            fref = lane_eval<KIND>(xref, n, p0, p1, power);
        }
        // ---- phase 2: expansion or contraction (:115-166)
        const double fbest = fv[0], fsecond = fv[(n - 1) * kLaneBatchLanes], fworst = fv[n * kLaneBatchLanes];
        const bool keepRef = active && fref >= fbest && fref < fsecond;
        const bool expand = active && !keepRef && fref < fbest;
        const bool second = active && !keepRef;
        double f2 = 0.0;
        if (second) {
            for (int i = 0; i < n; ++i) {
                const double xb = xbar[i * kLaneBatchLanes], w = xw[i * kLaneBatchLanes];
                x2[i * kLaneBatchLanes] = expand ? xb + gamma * (xb - w) : xb + rho * (w - xb);
            }
            f2 = lane_eval<KIND>(x2, n, p0, p1, power);
        }
        const bool take2 = second && (expand ? f2 < fref : f2 < fworst);
        const bool shrink = second && !expand && !take2;
        if (active && !shrink) {
            // the worst vertex is replaced and takes its sorted place (:117-173, :194)
            const double* src = take2 ? x2 : xref;
            for (int i = 0; i < n; ++i) xw[i * kLaneBatchLanes] = src[i * kLaneBatchLanes];
            sx_insert(fv, perm, n, take2 ? f2 : fref);
        }
        // ---- phase 3: shrink toward the best vertex, all n + 1 re-evaluated (:178-188)
        if (__any(shrink)) {
            const double* const x0 = xv + sx_row(perm, 0) * n * kLaneBatchLanes;
            if (shrink)
                for (int k = 1; k <= n; ++k) {
                    double* const xk = xv + sx_row(perm, k) * n * kLaneBatchLanes;
                    for (int i = 0; i < n; ++i) {
                        const double b = x0[i * kLaneBatchLanes];
                        xk[i * kLaneBatchLanes] = b + sigma * (xk[i * kLaneBatchLanes] - b);
                    }
                }
            for (int k = 0; k <= n; ++k)
                if (shrink) {
                    const double v = lane_eval<KIND>(xv + sx_row(perm, k) * n * kLaneBatchLanes, n, p0, p1, power);
                    sx_insert(fv, perm, k, v);
                }
        }
        if (active) {
            ev += 1 + (second ? 1 : 0) + (shrink ? n + 1 : 0);
            // xdiff = max |x0 - xk| over k >= 1 (simplexDiff, :331-349)
            const double* const x0 = xv + sx_row(perm, 0) * n * kLaneBatchLanes;
            double d = 0.0;
            for (int k = 1; k <= n; ++k) {
                const double* const xk = xv + sx_row(perm, k) * n * kLaneBatchLanes;
                for (int i = 0; i < n; ++i) {
                    const double diff = fabs(x0[i * kLaneBatchLanes] - xk[i * kLaneBatchLanes]);
                    if (diff > d) d = diff;
                }
            }
            xdiff = d;
            ++iter;
            active = iter < maxIter && xdiff > xMinDiff;
        }
    }

    if (valid) {
        const double* const x0 = xv + sx_row(perm, 0) * n * kLaneBatchLanes;
        for (int j = 0; j < n; ++j) Xio[s * (size_t)n + j] = x0[j * kLaneBatchLanes];
        f0out[s] = f0;
        fopt[s] = fv[0];
        iters[s] = iter;
        evals[s] = ev;
    }
}

}  // namespace

int launch_simplex_batch(pnol_ctx* ctx, const pnol_dobj* o, const double* params, unsigned long long seed,
                         long long nstart, double* X, double* f0, double* fopt, int* iters, long long* evals) {
    if (!ctx || !params || !X || !f0 || !fopt || !iters || !evals || nstart <= 0) return PNOL_ERR_ARG;
    PNOL_CHECK(scalar_batch_check(o, PNOL_SIMPLEX_BATCH_NMAX));
    const double* p = params;
    const size_t ns = (size_t)nstart, lds = sizeof(double) * (size_t)sx_slots(o->n) * kLaneBatchLanes;
    return scalar_batch_dispatch(o->kind, [&](auto kind) {
        return lane_batch_launch(ctx, "simplex_batch", &k_simplex_batch<decltype(kind)::value>, ns, lds, o->n, ns,
                                 (const double*)o->p0, (const double*)o->p1, o->power, p[0], p[1], p[2], p[3],
                                 (int)p[4], p[5], p[6], seed, X, f0, fopt, iters, evals);
    });
}

}  // namespace pnol
