"""BFGS::findMin in plain Python, written from the reference's control flow
(BFGS_with_linesearch.cpp:12-432, Objective::gradientApproximation PNOL_Objective.cpp:12-34): the
yardstick of the batched-BFGS tests, with a counter on every branch of the line search so that a
test can prove its inputs take them (the oracle cannot say which branches a run took).

Scalars are np.float64 and vectors numpy arrays under np.errstate(all="ignore"): IEEE doubles
with no contraction, a division by a zero bracket width gives inf / NaN as in C (Python's own /
raises), and an elementwise numpy expression rounds every entry exactly as the C statement it
restates.  Every sum that the reference accumulates in order is accumulated in that order here
(over the summation index, vectorised only across independent entries).  Objective values come
from the unchanged oracle (oracle.obj_eval)."""
from collections import namedtuple

import numpy as np

# SURVEY 8(d) config 1, in BFGS::setParams order: c1, c2, dalpha, alphaGuess, maxIterLineSearch,
# dXGrad, dXHess, maxIter, xMinDiff, minGrad2Norm, initHessFD, verbose
DEFAULTS = (1e-4, 0.9, 1e-6, 1, 1000, 1e-7, 1e-3, 100, 1e-5, 1e-5, 0, 0)
NAMES = ("c1", "c2", "dalpha", "alphaGuess", "maxIterLineSearch", "dXGrad", "dXHess", "maxIter", "xMinDiff",
         "minGrad2Norm", "initHessFD", "verbose")

Run = namedtuple("Run", "X f0 fopt gnorm iters evals counts")
# counts, in this order:
COUNTERS = ("zoom_by_armijo",      # outer trip: phi(ai) > phi0 + c1 ai dphi0 -> zoom(aim1, ai)
            "zoom_by_rise",        # outer trip: phi(ai) >= phi(aim1) && it > 1 (Armijo held) -> zoom(aim1, ai)
            "zoom_by_slope",       # outer trip: dphi(ai) >= 0 -> zoom(ai, aim1)
            "accept_curvature",    # outer trip accepted: |dphi(ai)| <= |c2 dphi0|
            "step_doubled",        # outer trip: ai <- 2 ai
            "zoom_raise_hi",       # zoom trip: ahi <- aj
            "zoom_accept",         # zoom trip accepted on curvature
            "zoom_flip",           # zoom trip: dj (ahi - alo) >= 0, ahi <- alo
            "zoom_exhausted",      # zoom ran maxIterLineSearch trips: alphaOpt = 0
            "outer_exhausted",     # the outer search ran maxIterLineSearch trips: alphaOpt = 0
            "bisection",           # cubicInterpMin fell back to (ahi + alo) / 2
            "alo_eq_ahi",          # cubicInterpMin called with a zero bracket width
            "nan_step")            # cubicInterpMin returned NaN


def params(**kw):
    """The 12 BFGS::setParams values, DEFAULTS overridden by name."""
    p = list(DEFAULTS)
    for k, v in kw.items():
        p[NAMES.index(k)] = v
    return tuple(p)


def _dot(a, b):
    s = np.float64(0.0)
    for i in range(len(a)):
        s = s + a[i] * b[i]
    return s


def _cubic(alo, ahi, plo, phi, dlo, dhi, cnt):
    """cubicInterpMin, :359-385."""
    if alo == ahi:
        cnt["alo_eq_ahi"] += 1
    w = ahi - alo
    sg = np.float64(1.0 if w > 0 else (-1.0 if w < 0 else 0.0))
    d1 = dlo + dhi - 3 * (plo - phi) / (alo - ahi)
    d2 = sg * np.sqrt(d1 * d1 - dlo * dhi)
    an = ahi - (ahi - alo) * (dhi + d2 - d1) / (dhi - dlo + 2 * d2)
    if alo < ahi:
        if an < alo:
            an = (ahi + alo) / 2
            cnt["bisection"] += 1
    else:
        if an < ahi:
            an = (ahi + alo) / 2
            cnt["bisection"] += 1
    if np.isnan(an):
        cnt["nan_step"] += 1
    return an


def _update(D, y, s):
    """updateHessianInv, :389-432: D <- M1 D M2 + M3, every product entry summed over l ascending
    from 0.0."""
    n = len(y)
    rho = 1 / _dot(y, s)
    E = np.eye(n)
    M1 = E - (rho * s)[:, None] * y[None, :]
    M2 = E - (rho * y)[:, None] * s[None, :]
    M3 = (rho * s)[:, None] * s[None, :]
    A = np.zeros((n, n))
    for l in range(n):
        A = A + M1[:, l:l + 1] * D[l:l + 1, :]
    B = np.zeros((n, n))
    for l in range(n):
        B = B + A[:, l:l + 1] * M2[l:l + 1, :]
    return B + M3


def find_min(fn, x0, p):
    """fn(numpy array of n doubles) -> float.  Returns a Run."""
    with np.errstate(all="ignore"):
        return _find_min(fn, x0, p)


def _find_min(fn, x0, p):
    f8 = np.float64
    c1, c2, dalpha, alpha_guess = f8(p[0]), f8(p[1]), f8(p[2]), f8(p[3])
    max_ls, dx, max_iter = int(p[4]), f8(p[5]), int(p[7])
    x_min_diff, min_gnorm = f8(p[8]), f8(p[9])
    assert not p[10], "initHessFD is not restated"
    n = len(x0)
    cnt = dict.fromkeys(COUNTERS, 0)
    evals = [0]

    def f(x):
        evals[0] += 1
        return f8(fn(x))

    def gradient(X):
        # the base value first, then coordinate by coordinate
        Fb = f(X)
        g = np.zeros(n)
        for i in range(n):
            xd = X.copy()
            xd[i] = xd[i] + dx
            g[i] = (f(xd) - Fb) / dx
        return g

    def phi_dphi(X, pv, a):
        # lineSearchObj then lineSearchFDDerivative, :144-174
        pa = f(X + a * pv)
        fa = f(X + (a + dalpha) * pv)
        return pa, (fa - pa) / dalpha

    def zoom(alo, ahi, plo, phi, dlo, dhi, phi0, dphi0, X, pv):
        # lineSearchZoom, :296-356; None: exhausted
        for _ in range(max_ls):
            aj = _cubic(alo, ahi, plo, phi, dlo, dhi, cnt)
            pj, dj = phi_dphi(X, pv, aj)
            if pj > phi0 + c1 * aj * dphi0 or pj >= plo:
                ahi, phi, dhi = aj, pj, dj
                cnt["zoom_raise_hi"] += 1
            else:
                if abs(dj) <= abs(c2 * dphi0):
                    cnt["zoom_accept"] += 1
                    return aj, pj
                if dj * (ahi - alo) >= 0:
                    ahi, phi, dhi = alo, plo, dlo
                    cnt["zoom_flip"] += 1
                alo, plo, dlo = aj, pj, dj
        cnt["zoom_exhausted"] += 1
        return None

    def line_search(X, FX, g, pv):
        # cubicInterpolationLineSearch, :177-291; (0, FX) is the result of an exhausted search
        phi0, dphi0 = FX, _dot(g, pv)
        aim1, pim1, dim1 = f8(0.0), phi0, dphi0
        ai = alpha_guess
        for it in range(max_ls):
            pi, di = phi_dphi(X, pv, ai)
            armijo = pi > phi0 + c1 * ai * dphi0
            if armijo or (pi >= pim1 and it > 1):
                cnt["zoom_by_armijo" if armijo else "zoom_by_rise"] += 1
                return zoom(aim1, ai, pim1, pi, dim1, di, phi0, dphi0, X, pv) or (f8(0.0), FX)
            if abs(di) <= abs(c2 * dphi0):
                cnt["accept_curvature"] += 1
                return ai, pi
            if di >= 0:
                cnt["zoom_by_slope"] += 1
                return zoom(ai, aim1, pi, pim1, di, dim1, phi0, dphi0, X, pv) or (f8(0.0), FX)
            aim1, pim1, dim1 = ai, pi, di
            ai = 2 * ai
            cnt["step_doubled"] += 1
        cnt["outer_exhausted"] += 1
        return f8(0.0), FX

    X = np.array(x0, dtype=np.float64)
    D = np.eye(n)
    g = gradient(X)
    F = f(X)
    f0 = F
    it = 0
    xdiff, gnorm = x_min_diff * 2, 2 * min_gnorm
    while it < max_iter and xdiff > x_min_diff and gnorm > min_gnorm:
        gprev = g
        acc = np.zeros(n)
        for j in range(n):
            acc = acc + D[:, j] * g[j]
        pv = -acc
        alpha, Fopt = line_search(X, F, g, pv)
        Xprev = X
        X = X + alpha * pv
        F = Fopt
        g = gradient(X)
        D = _update(D, g - gprev, alpha * pv)
        xdiff = f8(0.0)
        for i in range(n):
            xdiff += abs(X[i] - Xprev[i])
        gnorm = np.sqrt(_dot(g, g))
        it += 1
    return Run(X, float(f0), float(F), float(gnorm), it, evals[0], tuple(cnt[k] for k in COUNTERS))


# An input whose OUTER search is exhausted: f = x^2 from x0 = 3 with alphaGuess = 1e-3.  p = -6, the
# slope at alpha is -36 + 72 alpha: negative and outside |0.9 * 36| for alpha = 1e-3, 2e-3, 4e-3,
# and Armijo holds there, so alpha doubles on each of the maxIterLineSearch = 3 trips.
OUTER_EXHAUSTED = ("power2", 1, (3.0,), params(alphaGuess=1e-3, maxIterLineSearch=3))


def oracle_fn(oracle, obj):
    """fn for find_min from an oracle objective."""
    return lambda v: oracle.obj_eval(obj, v)


def oracle_obj(oracle, name, n):
    return {"rosenbrock": lambda: oracle.rosenbrock(n), "power2": lambda: oracle.power(n, 2.0),
            "quadratic": lambda: oracle.quadratic(n)}[name]()


def standard_x0(nstart, n, first=0):
    """The standard batch: start s begins at 3 - 0.01 s in every coordinate."""
    return np.array([[3.0 - 0.01 * s] * n for s in range(first, first + nstart)], dtype=np.float64)


_CACHE = {}


def standard_batch(oracle, name, n, nstart, p=DEFAULTS):
    """The Runs of starts 0 .. nstart-1 of the standard batch on the oracle objective `name`
    ("rosenbrock", "power2" or "quadratic"), computed once per start and shared."""
    key = (name, n, tuple(p))
    runs = _CACHE.setdefault(key, [])
    if len(runs) < nstart:
        fn = oracle_fn(oracle, oracle_obj(oracle, name, n))
        x0 = standard_x0(nstart, n)
        for s in range(len(runs), nstart):
            runs.append(find_min(fn, x0[s], p))
    return runs[:nstart]


def stacked(runs):
    """(X, f0, fopt, gnorm, iters, evals) arrays of a list of Runs, with the dtypes the library returns."""
    return (np.array([r.X for r in runs]), np.array([r.f0 for r in runs]), np.array([r.fopt for r in runs]),
            np.array([r.gnorm for r in runs]), np.array([r.iters for r in runs], dtype=np.int32),
            np.array([r.evals for r in runs], dtype=np.int64))
