// ga_batch.hip -- batched genetic algorithm: many independent GeneticAlgorithm runs in one launch
// (gfx950).
//
// One 64-lane workgroup (one wavefront) owns one run and takes it through every statement of
// GeneticAlgorithm::runGA (host form: host/genetic.cpp; GeneticAlgorithm.cpp:12-297) in order, the
// population's members on its lanes.  Run s draws from the stream seeded seed + s, so it is
// GeneticAlgorithm with setSeed(seed + s) from X[s], bit for bit, whatever batch it is in (the
// built-in objectives are the sequential sum of scalar_term, the expression the host objEval
// compiles; Power with power != 2 calls the device pow and is not bitwise against the host).
//
// Why not one lane per run: a run's state is two populations, F, Fnew and the fitness,
// (2 n + 3) Npop doubles -- 10.4 KB at Npop = 100, n = 5 -- and 64 of those do not fit a CU's LDS.
//
// State (dynamic LDS, sized per launch).  Members are stored member-minor in chunks of 64: with
// C = ceil(Npop / 64), coordinate j of member i is at ((i / 64) n + j) 64 + i % 64, so a lane
// that owns member i of a chunk reads its point with lane_eval's stride and without bank
// conflicts.
//     [0, 64 C n)            population A: Xpop, the sorted current generation
//     + 64 C n               population B: XpopNew, the children
//     + 64 C, + 64 C, + 64 C F, Fnew, fitness
//     + 64 C ints            evaluateIndicator (the serial sort's "taken" marks after evaluation)
//
// The stream.  GARandom is splitmix64, a counter generator: draw k (from 0) of the stream in
// state `st` is mix(st + (k + 1) g), g = 0x9E3779B97F4A7C15, so any lane computes any draw and the
// serial stream is consumed in parallel, in the host's order:
//   - selection (select_member, a rejection loop): lane t < W forms candidate pair t -- the
//     index draw 2 t, the accept draw 2 t + 1 -- one ballot finds the first accepting pair t*, the
//     state advances by 2 (t* + 1) draws; none: by 2 W, and round again.  W = 64, PNOL_GA_SPEC
//     (1..64) overrides it (a tuning and test knob: every width gives the same bits);
//   - bound repair: the flattened row-major (i, j) index 64 at a time; a violator's draw is
//     number popcount(ballot & lanes below), the state advances by popcount(ballot);
//   - identical-child repair: i ascending, the lanes compare member i with members k = i + 1...
//     64 at a time; at the first match k* member i is redrawn (n draws, j order) and flagged, and
//     the scan goes on from k* + 1 against the redrawn values, as the host's inner loop does.  The
//     call before the first evaluation runs on the all-zero XpopNew like the host's;
//   - mutations: n draws per random mutation once its member is selected, 2 n per elite child,
//     taken by the lanes in parallel.
// popSort is the host's repeated first minimum: the rank of member i is the number of k with
// F[k] < F[i], or F[k] == F[i] and k < i, and rows are scattered by rank into the other
// population (which is also the host's Xpop = XpopNew).  With a NaN among the F the host's scan
// is not an order (a NaN that comes first among the members left is taken first); lane 0 then
// runs the host's loop as written.
//
// Termination (the one departure from the host class).  A host selection never returns when no
// member past index 0 can be accepted.  A generation that starts not flat with no k >= 1 for
// which fitness[k] / maxFitness > 0 (one ballot), or a selection that has rejected
// PNOL_GA_BATCH_SELECT_CAP pairs, ends the run there: the current best member, F[0], the counts so
// far, PNOL_GA_BATCH_STUCK in info.  An all-NaN population is flat, selects uniformly like the host
// and ends by maxGenerations.
//
// Control flow is wave-uniform; a workgroup is one wave, so __syncthreads() between a phase's LDS
// writes and the next phase's reads is the only synchronisation.  No fma() in this file
// (-ffp-contract=off): every product and sum rounds as on the host.
#include "lane_batch.hpp"

#include "../pnol_env.hpp"

namespace pnol {
namespace {

constexpr unsigned long long kGaGolden = 0x9E3779B97F4A7C15ull;

constexpr int ga_chunks(int npop) { return (npop + kLaneBatchLanes - 1) / kLaneBatchLanes; }
// bytes of LDS of one run
constexpr size_t ga_lds(int n, int npop) {
    return (size_t)ga_chunks(npop) * kLaneBatchLanes * (sizeof(double) * (2 * n + 3) + sizeof(int));
}
static_assert(ga_lds(PNOL_GA_BATCH_NMAX, PNOL_GA_BATCH_NPOP_MAX) <= 64 * 1024,
              "the largest run must fit the 64 KB every kernel has");

struct GaArgs {
    int n, Npop, maxGen, Nelite, Ncross, Nrand, NeliteMut, W;
    double mutationSize, eliteMutationSize, NstaticGenerations, power;
    const double *p0, *p1, *lb, *ub;
    unsigned long long seed;
    double *X, *f0, *fopt;
    int* gens;
    long long* evals;
    int* info;
};

// draw k (from 0) of the stream in state st: GARandom::next() after k earlier calls
__device__ __forceinline__ double ga_draw(unsigned long long st, unsigned long long k) {
    unsigned long long z = st + (k + 1ull) * kGaGolden;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

// slot of coordinate j of member i
__device__ __forceinline__ int ga_at(int i, int j, int n) {
    return (((i >> 6) * n + j) << 6) + (i & (kLaneBatchLanes - 1));
}

// checkIndenticalChildAndReplace: returns the redraws made
__device__ int ga_identical(double* P, int* flag, int n, int Npop, const double* __restrict__ lb,
                            const double* __restrict__ ub, unsigned long long& st, int lane) {
    int hits = 0;
    for (int i = 0; i + 1 < Npop; ++i) {
        int k0 = i + 1;
        while (k0 < Npop) {
            const int k = k0 + lane;
            bool same = k < Npop;
            for (int j = 0; same && j < n; ++j) same = P[ga_at(i, j, n)] == P[ga_at(k, j, n)];
            const unsigned long long b = __ballot(same);
            if (b == 0ull) {
                k0 += kLaneBatchLanes;
                continue;
            }
            const int ks = k0 + __ffsll((long long)b) - 1;
            __syncthreads();
            if (lane < n) P[ga_at(i, lane, n)] = lb[lane] + (ub[lane] - lb[lane]) * ga_draw(st, lane);
            if (lane == 0) flag[i] = 1;
            st += (unsigned long long)n * kGaGolden;
            ++hits;
            __syncthreads();
            k0 = ks + 1;
        }
    }
    return hits;
}

// checkPopulationBoundsAndReplace
__device__ void ga_bounds(double* P, int* flag, int n, int Npop, const double* __restrict__ lb,
                          const double* __restrict__ ub, unsigned long long& st, int lane) {
    const int total = Npop * n;
    for (int e0 = 0; e0 < total; e0 += kLaneBatchLanes) {
        const int e = e0 + lane;
        const int i = e / n, j = e - i * n;
        bool viol = false;
        if (e < total) {
            const double x = P[ga_at(i, j, n)];
            viol = x > ub[j] || x < lb[j];
        }
        const unsigned long long b = __ballot(viol);
        if (viol) {
            const int k = __popcll(b & ((1ull << lane) - 1ull));
            P[ga_at(i, j, n)] = lb[j] + (ub[j] - lb[j]) * ga_draw(st, k);
            flag[i] = 1;
        }
        st += (unsigned long long)__popcll(b) * kGaGolden;
    }
}

// evaluatePopulation: the flagged members, one lane each; returns the evaluations
template <int KIND>
__device__ int ga_evaluate(const double* P, double* F, const int* flag, int n, int Npop,
                           const double* __restrict__ p0, const double* __restrict__ p1, double power, int lane) {
    int count = 0;
    for (int c = 0; c * kLaneBatchLanes < Npop; ++c) {
        const int i = c * kLaneBatchLanes + lane;
        const bool go = i < Npop && flag[i] != 0;
        if (go) F[i] = lane_eval<KIND>(P + c * n * kLaneBatchLanes + lane, n, p0, p1, power);
        count += __popcll(__ballot(go));
    }
    return count;
}

// popSort of (S, Fs) into (D, Fd); `taken` is scratch for the serial form
__device__ void ga_sort(const double* S, const double* Fs, double* D, double* Fd, int* taken, int n, int Npop,
                        int lane) {
    bool nan = false;
    for (int i = lane; i < Npop; i += kLaneBatchLanes) nan = nan || Fs[i] != Fs[i];
    if (__any(nan)) {
        // the host's loop as written (popSort, host/genetic.cpp)
        for (int i = lane; i < Npop; i += kLaneBatchLanes) taken[i] = 0;
        __syncthreads();
        for (int r = 0; r < Npop; ++r) {
            int best = -1;
            if (lane == 0) {
                for (int i = 0; i < Npop; ++i)
                    if (!taken[i] && (best < 0 || Fs[i] < Fs[best])) best = i;
                taken[best] = 1;
                Fd[r] = Fs[best];
            }
            best = __shfl(best, 0);
            if (lane < n) D[ga_at(r, lane, n)] = S[ga_at(best, lane, n)];
        }
    } else {
        for (int i = lane; i < Npop; i += kLaneBatchLanes) {
            const double fi = Fs[i];
            int r = 0;
            for (int k = 0; k < Npop; ++k) {
                const double fk = Fs[k];
                r += (fk < fi || (fk == fi && k < i)) ? 1 : 0;
            }
            for (int j = 0; j < n; ++j) D[ga_at(r, j, n)] = S[ga_at(i, j, n)];
            Fd[r] = fi;
        }
    }
    __syncthreads();
}

// select_member; -1: PNOL_GA_BATCH_SELECT_CAP pairs rejected
__device__ int ga_select(const double* fitness, double maxFitness, bool flat, int Npop, int W,
                         unsigned long long& st, int lane) {
    int pairs = 0;
    while (pairs < PNOL_GA_BATCH_SELECT_CAP) {
        const int w = min(W, PNOL_GA_BATCH_SELECT_CAP - pairs);
        bool accept = false;
        int k = 0;
        if (lane < w) {
            k = min((int)round(ga_draw(st, 2ull * lane) * Npop), Npop - 1);
            const double u = ga_draw(st, 2ull * lane + 1ull);
            accept = k != 0 && (flat || u <= fitness[k] / maxFitness);
        }
        const unsigned long long b = __ballot(accept);
        if (b != 0ull) {
            const int t = __ffsll((long long)b) - 1;
            st += 2ull * (unsigned long long)(t + 1) * kGaGolden;
            return __shfl(k, t);
        }
        st += 2ull * (unsigned long long)w * kGaGolden;
        pairs += w;
    }
    return -1;
}

template <int KIND>
__global__ __launch_bounds__(kLaneBatchLanes) void k_ga_batch(GaArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ga_lds_mem[];
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x;
    const int n = a.n, Npop = a.Npop;
    const int padded = ga_chunks(Npop) * kLaneBatchLanes;
    double* const cur = ga_lds_mem;                 // Xpop
    double* const nxt = cur + padded * n;           // XpopNew
    double* const F = nxt + padded * n;
    double* const Fnew = F + padded;
    double* const fitness = Fnew + padded;
    int* const flag = (int*)(fitness + padded);
    const double* __restrict__ lb = a.lb;
    const double* __restrict__ ub = a.ub;
    unsigned long long st = a.seed + (unsigned long long)s;
    long long ev = 0;

    // XpopNew, all zeros, through the identical-child check; every member to be evaluated
    for (int e = lane; e < padded * n; e += kLaneBatchLanes) cur[e] = 0.0;
    for (int i = lane; i < padded; i += kLaneBatchLanes) flag[i] = 1;
    // the initial population (in B): member 0 is X, member i >= 1 adds one draw per (i, j), i outer
    if (lane < n) nxt[ga_at(0, lane, n)] = a.X[s * (size_t)n + lane];
    __syncthreads();
    for (int e = lane; e < (Npop - 1) * n; e += kLaneBatchLanes) {
        const int i = e / n, j = e - i * n;
        nxt[ga_at(i + 1, j, n)] = nxt[ga_at(0, j, n)] + ((ub[j] - lb[j]) * ga_draw(st, e) + lb[j]);
    }
    st += (unsigned long long)((Npop - 1) * n) * kGaGolden;
    __syncthreads();
    ga_identical(cur, flag, n, Npop, lb, ub, st, lane);
    ga_bounds(nxt, flag, n, Npop, lb, ub, st, lane);
    __syncthreads();
    ev += ga_evaluate<KIND>(nxt, Fnew, flag, n, Npop, a.p0, a.p1, a.power, lane);
    __syncthreads();
    const double f0 = Fnew[0];
    ga_sort(nxt, Fnew, cur, F, flag, n, Npop, lane);

    double FbestPrev = F[0];
    int Nstatic = 0, iter = 0, info = 0;
    while (iter < a.maxGen) {
        const double Fworst = F[Npop - 1];
        for (int k = lane; k < Npop; k += kLaneBatchLanes) {
            const double d = Fworst - F[k];
            fitness[k] = d * d;
        }
        __syncthreads();
        const double maxFitness = fitness[0];
        bool pos = false, ratio = false;
        for (int k = lane; k < Npop; k += kLaneBatchLanes)
            if (k >= 1) {
                pos = pos || fitness[k] > 0.0;
                ratio = ratio || fitness[k] / maxFitness > 0.0;
            }
        const bool flat = maxFitness == 0.0 || !__any(pos);
        if (!flat && !__any(ratio)) {
            info = PNOL_GA_BATCH_STUCK;
            break;
        }
        // 1. elite children
        for (int i = lane; i < Npop; i += kLaneBatchLanes) {
            flag[i] = i < a.Nelite ? 0 : 1;
            if (i < a.Nelite) {
                Fnew[i] = F[i];
                for (int j = 0; j < n; ++j) nxt[ga_at(i, j, n)] = cur[ga_at(i, j, n)];
            }
        }
        int p = a.Nelite;
        bool stuck = false;
        // 2. crossovers
        for (int k = 0; k < a.Ncross && !stuck; ++k, ++p)
            for (int i = 0; i < n; ++i) {
                const int idx = ga_select(fitness, maxFitness, flat, Npop, a.W, st, lane);
                if (idx < 0) {
                    stuck = true;
                    break;
                }
                if (lane == 0) nxt[ga_at(p, i, n)] = cur[ga_at(idx, i, n)];
            }
        // 3. random mutations, the spread shrinking over the generations
        const double spreadRatio = a.mutationSize * (a.maxGen - iter) / a.maxGen;
        for (int k = 0; k < a.Nrand && !stuck; ++k, ++p) {
            const int idx = ga_select(fitness, maxFitness, flat, Npop, a.W, st, lane);
            if (idx < 0) {
                stuck = true;
                break;
            }
            if (lane < n) {
                const double mutation = spreadRatio * (ub[lane] - lb[lane]) * ga_draw(st, lane);
                nxt[ga_at(p, lane, n)] = cur[ga_at(idx, lane, n)] + mutation;
            }
            st += (unsigned long long)n * kGaGolden;
        }
        if (stuck) {
            info = PNOL_GA_BATCH_STUCK;
            break;
        }
        // 4. mutations of the elite: two draws per (child, coordinate)
        for (int e = lane; e < a.NeliteMut * n; e += kLaneBatchLanes) {
            const int k = e / n, j = e - k * n;
            const int el = min((int)round(ga_draw(st, 2ull * e) * a.Nelite), Npop - 1);
            const double mutation = a.eliteMutationSize * (ub[j] - lb[j]) * ga_draw(st, 2ull * e + 1ull);
            nxt[ga_at(p + k, j, n)] = cur[ga_at(el, j, n)] + mutation;
        }
        st += 2ull * (unsigned long long)(a.NeliteMut * n) * kGaGolden;
        __syncthreads();
        // 5. repair, 6. evaluate, 7. sort (into A: Xpop = XpopNew)
        ga_identical(nxt, flag, n, Npop, lb, ub, st, lane);
        ga_bounds(nxt, flag, n, Npop, lb, ub, st, lane);
        __syncthreads();
        ev += ga_evaluate<KIND>(nxt, Fnew, flag, n, Npop, a.p0, a.p1, a.power, lane);
        __syncthreads();
        ga_sort(nxt, Fnew, cur, F, flag, n, Npop, lane);
        const double Fbest = F[0];
        Nstatic = (Fbest == FbestPrev) ? Nstatic + 1 : 0;
        if (Nstatic > a.NstaticGenerations) break;
        FbestPrev = Fbest;
        ++iter;
    }

    if (lane < n) a.X[s * (size_t)n + lane] = cur[ga_at(0, lane, n)];
    if (lane == 0) {
        a.f0[s] = f0;
        a.fopt[s] = F[0];
        a.gens[s] = iter;
        a.evals[s] = ev;
        a.info[s] = info;
    }
}

// PNOL_GA_SPEC (tuning): the candidate pairs of a selection tested at once, 1..64
int ga_spec_env() {
    const int w = env_atoi("PNOL_GA_SPEC", kLaneBatchLanes);
    return w >= 1 && w <= kLaneBatchLanes ? w : kLaneBatchLanes;
}

}  // namespace

int launch_ga_batch(pnol_ctx* ctx, const pnol_dobj* o, const double* params, unsigned long long seed,
                    const double* Xlb, const double* Xub, long long nrun, double* X, double* f0, double* fopt,
                    int* gens, long long* evals, int* info) {
    if (!ctx || !Xlb || !Xub || !X || !f0 || !fopt || !gens || !evals || !info || nrun <= 0) return PNOL_ERR_ARG;
    GaCounts c;
    PNOL_CHECK(ga_batch_check_params(params, &c));
    PNOL_CHECK(scalar_batch_check(o, PNOL_GA_BATCH_NMAX));
    if (c.Npop > PNOL_GA_BATCH_NPOP_MAX) return PNOL_ERR_UNSUPPORTED;
    const GaArgs a = {o->n, c.Npop, c.maxGen, c.Nelite, c.Ncross, c.Nrand, c.NeliteMut, ga_spec_env(),
                      params[5], params[6], params[8], o->power,
                      (const double*)o->p0, (const double*)o->p1, Xlb, Xub,
                      seed, X, f0, fopt, gens, evals, info};
    return scalar_batch_dispatch(o->kind, [&](auto kind) {
        return wave_batch_launch(ctx, "ga_batch", &k_ga_batch<decltype(kind)::value>, (size_t)nrun,
                                 ga_lds(o->n, c.Npop), a);
    });
}

}  // namespace pnol
