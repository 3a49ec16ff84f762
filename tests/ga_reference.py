"""GeneticAlgorithm::runGA in plain Python, written from the host class's control flow
(csrc/host/genetic.cpp; GeneticAlgorithm.cpp:12-297): the yardstick of the batched-GA tests.
Python floats are IEEE doubles with no contraction, so every expression below gives the bits of
the C++ statement it restates; objective values come from the unchanged oracle (oracle.obj_eval).
The random stream is the drop-in classes' splitmix64 (GARandom) in 64-bit masked integers.

Two forms share the generation loop and differ in how they consume the stream:
  serial   rng.next() call by call, the host's loops as written;
  wave     random access to draw c of the stream, exactly as csrc/kernels/ga_batch.hip does: W-wide
           selection ballots, prefix-indexed bound-repair draws 64 flattened (i, j) at a time, the
           identical-child scan 64 members at a time, the rank sort, lanes' mutation draws.
Both apply the kernel's one departure from the host class, the stuck rule: a generation that
starts not flat with no k >= 1 for which fitness[k] / maxFitness > 0, or a selection that has
rejected `cap` candidate pairs, ends the run with info = STUCK."""
import math
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
LANES = 64
STUCK = 1                     # PNOL_GA_BATCH_STUCK
SELECT_CAP = 1 << 20          # PNOL_GA_BATCH_SELECT_CAP
DEFAULTS = (100, 1000, 0.1, 0.3, 0.2, 0.5, 0.01, 0.5, 50, 0)   # GeneticAlgorithm's constructor
SEED0 = 1000

Run = namedtuple("Run", "X f0 fopt gens evals info counters")
# counters: in-loop identical-child redraws, bound repairs, candidate pairs of all selections, the
# most pairs of one selection, flat (uniform) selections, selections, the stop reason, draws
Counters = namedtuple("Counters", "ident bounds pairs pairs_max flat selects stop draws")


def u01(seed, c):
    """Draw c (from 0) of the stream seeded `seed`: GARandom::next() after c earlier calls."""
    z = (seed + (c + 1) * GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return float(z >> 11) * 2.0 ** -53


def c_round(x):
    """std::round of a non-negative double: half away from zero."""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def member_counts(p):
    """(Nelite, NeliteMut, Ncross, Nrand) of GeneticAlgorithm.cpp:24-44."""
    npop = int(p[0])
    ne, nm, nc = (int(math.ceil(float(p[2]) * npop)), int(math.ceil(float(p[4]) * npop)),
                  int(math.ceil(float(p[3]) * npop)))
    return ne, nm, nc, npop - ne - nm - nc


def flat_and_stuck(fitness):
    """(flat, stuck) of a generation's fitness vector: select_member's flat, the kernel's pre-check."""
    mx = fitness[0]
    flat = mx == 0.0 or not any(f > 0.0 for f in fitness[1:])
    if flat:
        return True, False
    return False, not any(_div(f, mx) > 0.0 for f in fitness[1:])


def _div(a, b):
    """a / b of IEEE doubles (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


class _Stream:
    """The run's stream: `c` draws consumed so far."""

    def __init__(self, seed):
        self.seed = seed & M64
        self.c = 0

    def next(self):
        v = u01(self.seed, self.c)
        self.c += 1
        return v

    def at(self, k):
        return u01(self.seed, self.c + k)


# ---- the serial form: the host's loops as written ---------------------------------------------

class Serial:
    def __init__(self, cap=SELECT_CAP):
        self.cap = cap

    def initial(self, x0, lb, ub, npop, rng):
        n = len(x0)
        pop = [[float(v) for v in x0]]
        for _ in range(1, npop):
            pop.append([pop[0][j] + ((ub[j] - lb[j]) * rng.next() + lb[j]) for j in range(n)])
        return pop

    def identical(self, pop, lb, ub, flag, rng):
        n, npop, hits = len(lb), len(pop), 0
        col = [row[0] for row in pop]
        for i in range(npop):
            k = i + 1
            while k < npop:
                k = _first_equal(pop, col, i, k, npop)
                if k < 0:
                    break
                pop[i] = [lb[j] + (ub[j] - lb[j]) * rng.next() for j in range(n)]
                col[i] = pop[i][0]
                flag[i] = True
                hits += 1
                k += 1
        return hits

    def bounds(self, pop, lb, ub, flag, rng):
        n, reps = len(lb), 0
        for i, row in enumerate(pop):
            for j in range(n):
                if row[j] > ub[j] or row[j] < lb[j]:
                    row[j] = lb[j] + (ub[j] - lb[j]) * rng.next()
                    flag[i] = True
                    reps += 1
        return reps

    def sort(self, pop, F):
        return _host_sort(pop, F)

    def select(self, rng, fitness, mx, flat, npop):
        """(index or -1 when `cap` pairs were rejected, pairs consumed)."""
        pairs = 0
        while pairs < self.cap:
            r = min(c_round(rng.next() * npop), npop - 1)
            u = rng.next()
            pairs += 1
            if r != 0 and (flat or u <= _div(fitness[r], mx)):
                return r, pairs
        return -1, pairs

    def mutate(self, rng, row, spread, lb, ub):
        return [row[j] + spread * (ub[j] - lb[j]) * rng.next() for j in range(len(lb))]

    def elite_mutations(self, rng, cur, count, nelite, size, lb, ub):
        n, npop, out = len(lb), len(cur), []
        for _ in range(count):
            row = []
            for j in range(n):
                e = min(c_round(rng.next() * nelite), npop - 1)
                row.append(cur[e][j] + size * (ub[j] - lb[j]) * rng.next())
            out.append(row)
        return out


def _first_equal(pop, col, i, k0, end):
    """The first k in [k0, end) whose row equals row i in every coordinate (IEEE ==), or -1.  col
    holds the rows' first coordinates: list.index on it only narrows the candidates (it also
    accepts the same NaN object); the full comparison decides."""
    xi = pop[i]
    k = k0
    while True:
        try:
            k = col.index(xi[0], k, end)
        except ValueError:
            return -1
        if all(a == b for a, b in zip(xi, pop[k])):
            return k
        k += 1


def _host_sort(pop, F):
    """popSort: the first minimum among the members not yet placed, for every position.  Without a
    NaN that is the stable ascending order (Python's sort is stable); with one, the loop as
    written."""
    npop = len(F)
    if not any(f != f for f in F):
        order = sorted(range(npop), key=F.__getitem__)
    else:
        taken, order = [False] * npop, []
        for _ in range(npop):
            best = -1
            for i in range(npop):
                if not taken[i] and (best < 0 or F[i] < F[best]):
                    best = i
            taken[best] = True
            order.append(best)
    return [pop[i] for i in order], [F[i] for i in order]


# ---- the wave form: the stream by random access, as the kernel consumes it ---------------------

class Wave(Serial):
    def __init__(self, width=LANES, cap=SELECT_CAP):
        Serial.__init__(self, cap)
        assert 1 <= width <= LANES
        self.W = width

    def initial(self, x0, lb, ub, npop, rng):
        n = len(x0)
        pop = [[float(v) for v in x0]]
        for i in range(1, npop):
            pop.append([pop[0][j] + ((ub[j] - lb[j]) * rng.at((i - 1) * n + j) + lb[j]) for j in range(n)])
        rng.c += (npop - 1) * n
        return pop

    def identical(self, pop, lb, ub, flag, rng):
        n, npop, hits = len(lb), len(pop), 0
        col = [row[0] for row in pop]
        for i in range(npop - 1):
            k0 = i + 1
            while k0 < npop:
                ks = _first_equal(pop, col, i, k0, min(k0 + LANES, npop))   # one ballot over 64 members
                if ks < 0:
                    k0 += LANES
                    continue
                pop[i] = [lb[j] + (ub[j] - lb[j]) * rng.at(j) for j in range(n)]
                col[i] = pop[i][0]
                rng.c += n
                flag[i] = True
                hits += 1
                k0 = ks + 1
        return hits

    def bounds(self, pop, lb, ub, flag, rng):
        n, npop, reps = len(lb), len(pop), 0
        total = npop * n
        for e0 in range(0, total, LANES):
            lanes = range(e0, min(e0 + LANES, total))
            viol = [e for e in lanes if pop[e // n][e % n] > ub[e % n] or pop[e // n][e % n] < lb[e % n]]
            for below, e in enumerate(viol):       # popcount(ballot & lanes below)
                i, j = divmod(e, n)
                pop[i][j] = lb[j] + (ub[j] - lb[j]) * rng.at(below)
                flag[i] = True
            rng.c += len(viol)
            reps += len(viol)
        return reps

    def sort(self, pop, F):
        if any(f != f for f in F):
            return _host_sort(pop, F)             # lane 0 runs the host's loop
        Fa = np.array(F)
        idx = np.arange(len(F))
        before = (Fa[None, :] < Fa[:, None]) | ((Fa[None, :] == Fa[:, None]) & (idx[None, :] < idx[:, None]))
        rank = before.sum(axis=1)
        out, Fo = [None] * len(F), [None] * len(F)
        for i, r in enumerate(rank.tolist()):
            assert out[r] is None
            out[r], Fo[r] = pop[i], F[i]
        return out, Fo

    def select(self, rng, fitness, mx, flat, npop):
        pairs = 0
        while pairs < self.cap:
            w = min(self.W, self.cap - pairs)
            for t in range(w):
                k = min(c_round(rng.at(2 * t) * npop), npop - 1)
                u = rng.at(2 * t + 1)
                if k != 0 and (flat or u <= _div(fitness[k], mx)):
                    rng.c += 2 * (t + 1)
                    return k, pairs + t + 1
            rng.c += 2 * w
            pairs += w
        return -1, pairs

    def mutate(self, rng, row, spread, lb, ub):
        out = [row[j] + spread * (ub[j] - lb[j]) * rng.at(j) for j in range(len(lb))]
        rng.c += len(lb)
        return out

    def elite_mutations(self, rng, cur, count, nelite, size, lb, ub):
        n, npop = len(lb), len(cur)
        out = [[0.0] * n for _ in range(count)]
        for e in range(count * n):
            k, j = divmod(e, n)
            el = min(c_round(rng.at(2 * e) * nelite), npop - 1)
            out[k][j] = cur[el][j] + size * (ub[j] - lb[j]) * rng.at(2 * e + 1)
        rng.c += 2 * count * n
        return out


# ---- the run ----------------------------------------------------------------------------------

def run_ga(fn, x0, lb, ub, p, seed, form=None):
    """fn(list of n floats) -> float; p: the 10 setGAParams values without graph; form: Serial()
    (default) or Wave(width).  Returns a Run."""
    ops = form or Serial()
    npop, max_gen = int(p[0]), int(p[1])
    mut_size, elite_mut_size, nstatic_max = float(p[5]), float(p[6]), float(p[8])
    nelite, nelite_mut, ncross, nrand = member_counts(p)
    assert npop >= 2 and nrand > 0
    lb, ub = [float(v) for v in lb], [float(v) for v in ub]
    n = len(x0)
    rng = _Stream(seed)
    cnt = dict(ident=0, bounds=0, pairs=0, pairs_max=0, flat=0, selects=0)

    pop = ops.initial(x0, lb, ub, npop, rng)
    flag = [True] * npop
    zeros = [[0.0] * n for _ in range(npop)]
    ops.identical(zeros, lb, ub, flag, rng)       # the reference checks XpopNew (all zeros) here
    cnt["bounds"] += ops.bounds(pop, lb, ub, flag, rng)
    F = [fn(row) for row in pop]
    evals = npop
    f0 = F[0]
    pop, F = ops.sort(pop, F)

    fbest_prev, nstatic, it, info, stop = F[0], 0, 0, 0, "max"

    def select():
        idx, pairs = ops.select(rng, fitness, mx, flat, npop)
        cnt["selects"] += 1
        cnt["pairs"] += pairs
        cnt["pairs_max"] = max(cnt["pairs_max"], pairs)
        cnt["flat"] += 1 if flat else 0
        return idx

    while it < max_gen:
        fitness = []
        for k in range(npop):
            d = F[npop - 1] - F[k]
            fitness.append(d * d)
        mx = fitness[0]
        flat, stuck = flat_and_stuck(fitness)
        if stuck:
            info, stop = STUCK, "stuck"
            break
        new, Fnew, flag = [None] * npop, [0.0] * npop, [True] * npop
        for k in range(nelite):
            new[k], Fnew[k], flag[k] = list(pop[k]), F[k], False
        q = nelite
        for _ in range(ncross):
            idx = []
            for _i in range(n):
                idx.append(select())
                if idx[-1] < 0:
                    break
            if idx[-1] < 0:
                stuck = True
                break
            new[q] = [pop[idx[i]][i] for i in range(n)]
            q += 1
        spread = mut_size * (max_gen - it) / max_gen
        for _ in range(nrand):
            if stuck:
                break
            s = select()
            if s < 0:
                stuck = True
                break
            new[q] = ops.mutate(rng, pop[s], spread, lb, ub)
            q += 1
        if stuck:
            info, stop = STUCK, "stuck"
            break
        for row in ops.elite_mutations(rng, pop, nelite_mut, nelite, elite_mut_size, lb, ub):
            new[q] = row
            q += 1
        assert q == npop
        cnt["ident"] += ops.identical(new, lb, ub, flag, rng)
        cnt["bounds"] += ops.bounds(new, lb, ub, flag, rng)
        for i in range(npop):
            if flag[i]:
                Fnew[i] = fn(new[i])
                evals += 1
        pop, F = ops.sort(new, Fnew)
        nstatic = nstatic + 1 if F[0] == fbest_prev else 0
        if nstatic > nstatic_max:
            stop = "static"
            break
        fbest_prev = F[0]
        it += 1
    counters = Counters(cnt["ident"], cnt["bounds"], cnt["pairs"], cnt["pairs_max"], cnt["flat"], cnt["selects"],
                        stop, rng.c)
    return Run(np.array(pop[0]), f0, F[0], it, evals, info, counters)


def oracle_fn(oracle, obj):
    """fn for run_ga from an oracle objective."""
    return lambda v: oracle.obj_eval(obj, np.array(v, dtype=np.float64))


def make_obj(oracle, name, n):
    return {"rosenbrock": lambda: oracle.rosenbrock(n), "power2": lambda: oracle.power(n, 2.0),
            "quadratic": lambda: oracle.quadratic(n)}[name]()


def params(**kw):
    """The 10 setGAParams values (without graph), defaults overridden by name."""
    names = ("Npop", "maxGenerations", "eliteFrac", "crossFrac", "eliteMutationFrac", "mutationSize",
             "eliteMutationSize", "initialPopScaling", "NstaticGenerations", "verbose")
    p = list(DEFAULTS)
    for k, v in kw.items():
        p[names.index(k)] = v
    return tuple(p)


# The batches of the tests: name -> (objective, n, lb, ub, x0 value, runs, params).  Run s starts
# from x0 in every coordinate on the stream SEED0 + s.
CASES = {
    "ros3": ("rosenbrock", 3, -2.0, 2.0, -1.0, 65, (40, 200, 0.1, 0.3, 0.2, 0.5, 0.01, 0.5, 20, 0)),
    "small": ("rosenbrock", 2, -2.0, 2.0, -1.0, 65, params(Npop=8, maxGenerations=30, NstaticGenerations=5)),
    "n12": ("rosenbrock", 12, -2.0, 2.0, -1.0, 8, params(Npop=64, maxGenerations=30)),
    "npop130": ("rosenbrock", 3, -2.0, 2.0, -1.0, 6, params(Npop=130, maxGenerations=40, NstaticGenerations=10)),
    "defaults": ("rosenbrock", 5, -1.5, 1.2, 0.5, 3, params(maxGenerations=60)),
    "lds_max": ("rosenbrock", 12, -2.0, 2.0, -1.0, 2, params(Npop=256, maxGenerations=5)),
    "power": ("power2", 1, -2.0, 2.0, -1.0, 5, params(Npop=20, maxGenerations=40, NstaticGenerations=10)),
    "quadratic": ("quadratic", 5, -2.0, 2.0, -1.0, 5, params(Npop=40, maxGenerations=40, NstaticGenerations=10)),
    "gen0": ("rosenbrock", 3, -2.0, 2.0, -1.0, 3, params(Npop=40, maxGenerations=0)),
}
FINITE = tuple(CASES)

_CACHE = {}


def batch(oracle, name, n, lb, ub, x0, p, seed=SEED0, form=None, key=None):
    """The Runs of the rows of x0 (run s on the stream seed + s), cached under `key`."""
    k = None if key is None else (key, len(x0))
    if k is None or k not in _CACHE:
        fn = oracle_fn(oracle, make_obj(oracle, name, n))
        runs = [run_ga(fn, list(x0[s]), [lb] * n, [ub] * n, p, seed + s, form) for s in range(len(x0))]
        if k is None:
            return runs
        _CACHE[k] = runs
    return _CACHE[k]


def case_x0(case, nrun=None):
    _, n, _, _, x, runs, _ = CASES[case]
    return np.full((runs if nrun is None else nrun, n), x, dtype=np.float64)


def case_runs(oracle, case, nrun=None, form=None, tag="serial"):
    """The Runs of a case's first nrun runs (a prefix of the cached whole case)."""
    name, n, lb, ub, _, runs, p = CASES[case]
    whole = batch(oracle, name, n, lb, ub, case_x0(case), p, form=form, key=(case, tag))
    return whole[:runs if nrun is None else nrun]


def stacked(runs):
    """(X, f0, fopt, gens, evals, info) arrays of a list of Runs, with the library's dtypes."""
    return (np.array([r.X for r in runs]), np.array([r.f0 for r in runs]), np.array([r.fopt for r in runs]),
            np.array([r.gens for r in runs], dtype=np.int32), np.array([r.evals for r in runs], dtype=np.int64),
            np.array([r.info for r in runs], dtype=np.int32))
