"""SimplexSearch::findMin in plain Python, written from the reference's control flow
(SimplexSearch.cpp:13-349): the yardstick of the simplex tests.  Python floats are IEEE doubles
with no contraction, so every expression below gives the bits of the C++ statement it restates;
objective values come from the unchanged oracle (oracle.obj_eval).  The random stream is the
drop-in classes' splitmix64 (GARandom) in 64-bit masked integer arithmetic."""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
DEFAULTS = (1.0, 2.0, 0.5, 0.5, 10000, 1.0, 1e-7, 0)   # SimplexSearch's constructor
SEED0 = 20261021

Run = namedtuple("Run", "X f0 fopt iters evals outcomes")
# outcomes: counts of (reflection kept, expansion kept, reflection after a failed expansion,
# contraction kept, shrink)
OUTCOMES = ("reflect", "expand", "expand_failed", "contract", "shrink")


class SplitMix:
    def __init__(self, seed):
        self.state = seed & M64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        return float(z >> 11) * 2.0 ** -53


def params(**kw):
    """The 8 setSimplexParams values, defaults overridden by name."""
    names = ("alpha", "gamma", "rho", "sigma", "maxIter", "initRandMax", "xMinDiff", "verbose")
    p = list(DEFAULTS)
    for k, v in kw.items():
        p[names.index(k)] = v
    return tuple(p)


def _sort(f, x):
    """The first minimum among the vertices not yet placed, for every position (a stable sort)."""
    n1 = len(f)
    taken = [False] * n1
    fs, xs = [], []
    for _ in range(n1):
        best = -1
        for i in range(n1):
            if not taken[i] and (best < 0 or f[i] < f[best]):
                best = i
        taken[best] = True
        fs.append(f[best])
        xs.append(x[best])
    return fs, xs


def find_min(fn, x0, p, seed):
    """fn(list of n floats) -> float.  Returns a Run."""
    alpha, gamma, rho, sigma, max_iter, init_rand_max, x_min_diff = (float(p[0]), float(p[1]), float(p[2]),
                                                                     float(p[3]), int(p[4]), float(p[5]), float(p[6]))
    n = len(x0)
    rng = SplitMix(seed)
    x = [[float(v) for v in x0]]
    for _ in range(1, n + 1):
        x.append([x[0][j] + init_rand_max * (rng.next() - 0.5) * 2.0 for j in range(n)])
    f = [fn(v) for v in x]
    evals = n + 1
    f0 = f[0]
    f, x = _sort(f, x)
    out = dict.fromkeys(OUTCOMES, 0)
    it = 0
    xdiff = x_min_diff * 2
    while it < max_iter and xdiff > x_min_diff:
        xbar = [0.0] * n
        for i in range(n):
            for k in range(n):
                xbar[i] = xbar[i] + x[k][i] / float(n)
        xref = [xbar[i] + alpha * (xbar[i] - x[n][i]) for i in range(n)]
        fref = fn(xref)
        evals += 1
        if fref >= f[0] and fref < f[n - 1]:
            x[n], f[n] = xref, fref
            out["reflect"] += 1
        elif fref < f[0]:
            xe = [xbar[i] + gamma * (xbar[i] - x[n][i]) for i in range(n)]
            fe = fn(xe)
            evals += 1
            if fe < fref:
                x[n], f[n] = xe, fe
                out["expand"] += 1
            else:
                x[n], f[n] = xref, fref
                out["expand_failed"] += 1
        else:
            xc = [xbar[i] + rho * (x[n][i] - xbar[i]) for i in range(n)]
            fc = fn(xc)
            evals += 1
            if fc < f[n]:
                x[n], f[n] = xc, fc
                out["contract"] += 1
            else:
                for k in range(1, n + 1):
                    x[k] = [x[0][i] + sigma * (x[k][i] - x[0][i]) for i in range(n)]
                f = [fn(v) for v in x]
                evals += n + 1
                out["shrink"] += 1
        f, x = _sort(f, x)
        xdiff = 0.0
        for k in range(1, n + 1):
            for j in range(n):
                d = abs(x[0][j] - x[k][j])
                if d > xdiff:
                    xdiff = d
        it += 1
    return Run(np.array(x[0]), f0, f[0], it, evals, tuple(out[k] for k in OUTCOMES))


def oracle_fn(oracle, obj):
    """fn for find_min from an oracle objective."""
    return lambda v: oracle.obj_eval(obj, np.array(v, dtype=np.float64))


def standard_x0(nstart, n, first=0):
    """The standard batch: start s begins at 3 - 0.01 s in every coordinate."""
    return np.array([[3.0 - 0.01 * s] * n for s in range(first, first + nstart)], dtype=np.float64)


_CACHE = {}


def standard_batch(oracle, name, n, nstart, p=DEFAULTS, make_obj=None):
    """The Runs of starts 0 .. nstart-1 of the standard batch (stream SEED0 + s) on the oracle
    objective `name` ("rosenbrock", "power2" or "quadratic"), computed once per start and shared."""
    make = make_obj or {"rosenbrock": lambda: oracle.rosenbrock(n), "power2": lambda: oracle.power(n, 2.0),
                        "quadratic": lambda: oracle.quadratic(n)}[name]
    key = (name, n, tuple(p))
    runs = _CACHE.setdefault(key, [])
    if len(runs) < nstart:
        fn = oracle_fn(oracle, make())
        x0 = standard_x0(nstart, n)
        for s in range(len(runs), nstart):
            runs.append(find_min(fn, x0[s].tolist(), p, SEED0 + s))
    return runs[:nstart]


def stacked(runs):
    """(X, f0, fopt, iters, evals) arrays of a list of Runs, with the dtypes the library returns."""
    return (np.array([r.X for r in runs]), np.array([r.f0 for r in runs]), np.array([r.fopt for r in runs]),
            np.array([r.iters for r in runs], dtype=np.int32), np.array([r.evals for r in runs], dtype=np.int64))
