"""BFGS_Bnd::findMinBnd in plain Python, written from the reference's control flow
(BFGS_bnd_linesearch.cpp:15-750, Box_boundary_functions.cpp:11-40, Objective::objEvalRecur and
gradientApproximationRecur PNOL_Objective.cpp:303-360): the yardstick of the batched bounded-BFGS
tests, with a counter on every branch of the line search and of the active-set recursion so that a
test can prove its inputs take them (the oracle cannot say which branches a run took).

Scalars are np.float64 and vectors numpy arrays under np.errstate(all="ignore"), as in
tests/bfgs_reference.py: IEEE doubles with no contraction, every sum that the reference accumulates
in order accumulated in that order.  Objective values come from the unchanged oracle
(oracle.obj_eval) at the full-space point (frozen coordinates hold the value they were frozen at).

The level vectors stay in full space: a level's coordinates are exactly the coordinates that are
not frozen, ascending, so every reduced-order loop of the reference runs here over the free
indices in ascending order.

The corner end -- the one place this restatement (and the batched kernel) departs from the
reference.  An assessment at depth >= 1 that leaves no free coordinate makes the reference clear
optimFlag but keep those coordinates marked constant; the levels above clear only their own marks,
so from then on the constant indicator disagrees with the level vectors and the reference reads
past them (undefined behaviour: the C oracle aborts in malloc / free on such starts).  Here such a
start ends at that assessment: X is the full-space point (every coordinate at a bound with an
outward direction or gradient), fOpt the level's F, iterations and evaluations as counted up to
there (the trip that ends is not counted), and the run is flagged.  Everything before that moment
is the reference's arithmetic.  No free coordinate left at depth 0 is not a corner end: there the
reference is consistent and is followed exactly."""
from collections import namedtuple

import numpy as np

# Examples.cpp:75 (silent), in BFGS_Bnd::setParams order
P = (1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1)
NAMES = ("c1", "c2", "dalpha", "alphaGuess", "alphaTol", "alphaMult", "maxIterLineSearch", "bndTol", "dXGrad",
         "dXHess", "maxIter", "xMinDiff", "minGrad2Norm", "initHessFD", "verbose")

CORNER = 1 << 8   # PNOL_BFGS_BND_BATCH_CORNER: bit 8 of info

Run = namedtuple("Run", "X f0 fopt iters evals depth flagged counts")
# counts, in this order:
COUNTERS = ("zoom_hi_by_value",     # zoom trip: Armijo fails or phi_c >= min(phi_a, phi_b), phi_a < phi_b: b <- c
            "zoom_lo_by_value",     # the same test, phi_a >= phi_b: a <- c
            "zoom_accept",          # zoom trip accepted on curvature
            "zoom_lo_by_slope",     # zoom trip: dphi_c < 0: a <- c
            "zoom_hi_by_slope",     # zoom trip: dphi_c >= 0: b <- c
            "zoom_exit_iter",       # zoom left because iter_ls reached maxIterLineSearch
            "zoom_exit_width",      # zoom left because alpha_b - alpha_a <= alphaTol
            "zoom_result_a",        # zoom without success: phi_a < phi_b, the result is a
            "zoom_result_b",        # zoom without success: the result is b
            "guess_clipped",        # alphaGuess > alphaMax: the first step is alphaMax
            "outer_armijo",         # outer trip: phi(ai) > phi0 + c1 ai dphi0 -> zoom
            "outer_rise",           # outer trip: phi(ai) >= phi(aim1) and iter_ls > 1 (Armijo held) -> zoom
            "outer_accept",         # outer trip accepted on curvature
            "outer_slope",          # outer trip: dphi(ai) >= 0 -> zoom
            "at_bound",             # outer trip: ai == alphaMax, the search ends on the box
            "doubling",             # outer trip: ai <- 2 ai
            "doubling_clipped",     # ... and 2 ai > alphaMax: ai <- alphaMax
            "exhausted_previous",   # outer search exhausted: phi(aim1) < phi(ai), the previous point
            "exhausted_zero",       # outer search exhausted: phi0 < phi(ai), alpha = 0
            "exhausted_last",       # outer search exhausted: the last step
            "freeze_lower",         # a coordinate frozen at its lower bound
            "freeze_upper",         # a coordinate frozen at its upper bound
            "released",             # after a recursion: a released coordinate's gradient points inside (cont)
            "not_released",         # after a recursion: no released coordinate's does (optimFlag cleared)
            "multi_freeze",         # one assessment froze more than one coordinate
            "cubic_midpoint",       # cubicInterpMinSimple fell back to the midpoint
            "top_all_frozen",       # an assessment at depth 0 left no free coordinate
            "corner_end")           # an assessment at depth >= 1 left no free coordinate


def params(**kw):
    """The 15 BFGS_Bnd::setParams values, P overridden by name."""
    p = list(P)
    for k, v in kw.items():
        p[NAMES.index(k)] = v
    return tuple(p)


def grid_x0(nstart, n, lb, ub, first=0):
    """The standard start grid of the box [lb, ub]^n."""
    s = np.arange(first, first + nstart)[:, None]
    j = np.arange(n)[None, :]
    return lb + (ub - lb) * np.mod(0.37 * s + 0.21 * j + 0.05, 1.0)


def _cubic(aa, ab, pa, pb, da, db, cnt):
    """cubicInterpMinSimple, :736-750."""
    w = ab - aa
    sg = np.float64(1.0 if w > 0 else (-1.0 if w < 0 else 0.0))
    d1 = da + db - 3 * (pa - pb) / (aa - ab)
    d2 = sg * np.sqrt(d1 * d1 - da * db)
    an = ab - (ab - aa) * (db + d2 - d1) / (db - da + 2 * d2)
    if an < aa or an > ab or an != an:
        an = (aa + ab) / 2
        cnt["cubic_midpoint"] += 1
    return an


def _update(D, y, s):
    """updateHessianInv (BFGS_with_linesearch.cpp:389-432) on the level's coordinates."""
    n = len(y)
    ys = np.float64(0.0)
    for i in range(n):
        ys = ys + y[i] * s[i]
    rho = 1 / ys
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


class _Corner(Exception):
    pass


def find_min_bnd(fn, x0, lb, ub, p):
    """fn(numpy array of n doubles) -> float; lb, ub: the box, n values each.  Returns a Run."""
    with np.errstate(all="ignore"):
        return _Solver(fn, x0, lb, ub, p).run()


class _Solver:
    def __init__(self, fn, x0, lb, ub, p):
        f8 = np.float64
        self.fn = fn
        (self.c1, self.c2, self.dalpha, self.alpha_guess, self.alpha_tol) = (f8(v) for v in p[:5])
        self.max_ls, self.bnd_tol, self.dx = int(p[6]), f8(p[7]), f8(p[8])
        self.max_iter, self.x_min_diff, self.min_gnorm = int(p[10]), f8(p[11]), f8(p[12])
        assert not p[13], "initHessFD is not restated"
        self.n = len(x0)
        self.X = np.array(x0, dtype=f8)
        self.lb = np.array(lb, dtype=f8)
        self.ub = np.array(ub, dtype=f8)
        self.g = np.zeros(self.n)
        self.frozen = np.zeros(self.n, dtype=bool)
        self.cnt = dict.fromkeys(COUNTERS, 0)
        self.evals = 0
        self.total_iter = 0
        self.optim = True
        self.depth = 0
        self.max_depth = 0
        self.F = f8(0.0)

    def f(self, x):
        self.evals += 1
        return np.float64(self.fn(x))

    def free(self):
        return [i for i in range(self.n) if not self.frozen[i]]

    def gradient(self):
        """gradientApproximationRecur over the free coordinates: the base value first."""
        Fb = self.f(self.X)
        for i in self.free():
            xd = self.X.copy()
            xd[i] = xd[i] + self.dx
            self.g[i] = (self.f(xd) - Fb) / self.dx

    def phi_dphi(self, idx, pv, a):
        xa = self.X.copy()
        xb = self.X.copy()
        a2 = a + self.dalpha
        for i in idx:
            xa[i] = self.X[i] + a * pv[i]
            xb[i] = self.X[i] + a2 * pv[i]
        pa = self.f(xa)
        fa = self.f(xb)
        return pa, (fa - pa) / self.dalpha

    def alpha_bnd(self, idx, pv):
        """computeAlphaBnd, Box_boundary_functions.cpp:11-40."""
        bnd = np.float64(0.0)
        for k, i in enumerate(idx):
            a1 = (self.ub[i] - self.X[i]) / pv[i]
            a2 = (self.lb[i] - self.X[i]) / pv[i]
            ai = a1 if a1 > 0 else (a2 if a2 > 0 else np.float64(0.0))
            if k == 0:
                bnd = ai
            if bnd > ai:
                bnd = ai
        return bnd

    def zoom(self, aa, ab, pa, pb, da, db, phi0, dphi0, idx, pv, it):
        """lineSearchZoomBnd, :358-457; returns (alpha, phi, iter_ls)."""
        cnt = self.cnt
        while True:
            if not it < self.max_ls:
                cnt["zoom_exit_iter"] += 1
                break
            if not ab - aa > self.alpha_tol:
                cnt["zoom_exit_width"] += 1
                break
            ac = _cubic(aa, ab, pa, pb, da, db, cnt)
            pc, dc = self.phi_dphi(idx, pv, ac)
            pmin = pa
            if pb < pa:
                pmin = pb
            if pc > phi0 + self.c1 * ac * dphi0 or pc >= pmin:
                if pa < pb:
                    ab, pb, db = ac, pc, dc
                    cnt["zoom_hi_by_value"] += 1
                else:
                    aa, pa, da = ac, pc, dc
                    cnt["zoom_lo_by_value"] += 1
            else:
                if abs(dc) <= abs(self.c2 * dphi0):
                    cnt["zoom_accept"] += 1
                    return ac, pc, it
                if dc < 0:
                    aa, pa, da = ac, pc, dc
                    cnt["zoom_lo_by_slope"] += 1
                else:
                    ab, pb, db = ac, pc, dc
                    cnt["zoom_hi_by_slope"] += 1
            it += 1
        if pa < pb:
            cnt["zoom_result_a"] += 1
            return aa, pa, it
        cnt["zoom_result_b"] += 1
        return ab, pb, it

    def line_search(self, idx, pv):
        """cubicInterpolationLineSearchBnd, :203-353; returns (alpha, Fopt)."""
        f8 = np.float64
        cnt = self.cnt
        phi0 = self.F
        dphi0 = f8(0.0)
        for i in idx:
            dphi0 = dphi0 + self.g[i] * pv[i]
        aim1, pim1, dim1 = f8(0.0), phi0, dphi0
        amax = self.alpha_bnd(idx, pv)
        ai = self.alpha_guess
        if ai > amax:
            ai = amax
            cnt["guess_clipped"] += 1
        phii = f8(0.0)
        it = 0
        while it < self.max_ls:
            phii, di = self.phi_dphi(idx, pv, ai)
            armijo = phii > phi0 + self.c1 * ai * dphi0
            if armijo or (phii >= pim1 and it > 1):
                cnt["outer_armijo" if armijo else "outer_rise"] += 1
                a, ph, it = self.zoom(aim1, ai, pim1, phii, dim1, di, phi0, dphi0, idx, pv, it)
                return a, ph
            if abs(di) <= abs(self.c2 * dphi0):
                cnt["outer_accept"] += 1
                return ai, phii
            if di >= 0:
                cnt["outer_slope"] += 1
                a, ph, it = self.zoom(aim1, ai, pim1, phii, dim1, di, phi0, dphi0, idx, pv, it)
                return a, ph
            if ai == amax:
                cnt["at_bound"] += 1
                return ai, phii
            aim1, pim1, dim1 = ai, phii, di
            ai = 2 * ai
            cnt["doubling"] += 1
            if ai > amax:
                ai = amax
                cnt["doubling_clipped"] += 1
            it += 1
        if pim1 < phii:
            cnt["exhausted_previous"] += 1
            return aim1, pim1
        if phi0 < phii:
            cnt["exhausted_zero"] += 1
            return f8(0.0), phi0
        cnt["exhausted_last"] += 1
        return ai, phii

    def assess(self, idx, pv):
        """boundaryAssessment, :503-728.  Returns True when it re-optimised a reduced problem."""
        cnt = self.cnt
        hit = []
        for i in idx:
            if abs(self.X[i] - self.lb[i]) < self.bnd_tol and (pv[i] < 0 or self.g[i] > 0):
                hit.append(i)
                cnt["freeze_lower"] += 1
            elif abs(self.X[i] - self.ub[i]) < self.bnd_tol and (pv[i] > 0 or self.g[i] < 0):
                hit.append(i)
                cnt["freeze_upper"] += 1
        if len(hit) > 1:
            cnt["multi_freeze"] += 1
        nr = len(idx) - len(hit)
        if hit and nr > 0:
            for i in hit:
                self.frozen[i] = True
            self.depth += 1
            self.max_depth = max(self.max_depth, self.depth)
            self.main_loop()
            self.depth -= 1
            for i in hit:
                self.frozen[i] = False
            self.gradient()
            cont = False
            for i in hit:
                if abs(self.X[i] - self.lb[i]) < self.bnd_tol and self.g[i] < 0:
                    cont = True
                elif abs(self.X[i] - self.ub[i]) < self.bnd_tol and self.g[i] > 0:
                    cont = True
            cnt["released" if cont else "not_released"] += 1
            self.optim = cont
            return True
        if nr == 0:
            if self.depth >= 1:
                cnt["corner_end"] += 1
                raise _Corner()
            cnt["top_all_frozen"] += 1
            for i in hit:
                self.frozen[i] = True
            self.optim = False
        return False

    def main_loop(self):
        """mainBFGSLoop, :116-201, on the free coordinates at entry."""
        f8 = np.float64
        idx = self.free()
        nl = len(idx)
        D = np.eye(nl)
        it = 0
        xdiff, gnorm = self.x_min_diff * 2, 2 * self.min_gnorm
        while (self.optim and it < self.max_iter and xdiff > self.x_min_diff and gnorm > self.min_gnorm
               and self.total_iter < self.max_iter):
            gl = self.g[idx]
            acc = np.zeros(nl)
            for j in range(nl):
                acc = acc + D[:, j] * gl[j]
            pv = np.zeros(self.n)
            pv[idx] = -acc
            alpha, Fopt = self.line_search(idx, pv)
            Xprev = self.X.copy()
            for i in idx:
                self.X[i] = self.X[i] + alpha * pv[i]
            self.F = Fopt
            self.gradient()
            D = _update(D, self.g[idx] - gl, alpha * pv[idx])
            if self.assess(idx, pv):
                D = np.eye(nl)
            xdiff = f8(0.0)
            gg = f8(0.0)
            for i in idx:
                xdiff += abs(self.X[i] - Xprev[i])
                gg = gg + self.g[i] * self.g[i]
            gnorm = np.sqrt(gg)
            it += 1
            self.total_iter += 1

    def run(self):
        # checkBoxBounds, applied silently
        for i in range(self.n):
            if (self.X[i] - self.lb[i] < -abs(self.lb[i]) / 1000 or self.X[i] - self.ub[i] > abs(self.ub[i]) / 1000):
                self.X[i] = (self.lb[i] + self.ub[i]) / 2.0
        self.gradient()
        self.F = self.f(self.X)
        f0 = self.F
        flagged = False
        try:
            self.main_loop()
        except _Corner:
            flagged = True
        return Run(self.X.copy(), float(f0), float(self.F), self.total_iter, self.evals, self.max_depth, flagged,
                   tuple(self.cnt[k] for k in COUNTERS))


def oracle_fn(oracle, obj):
    return lambda v: oracle.obj_eval(obj, v)


def oracle_obj(oracle, name, n):
    return {"rosenbrock": lambda: oracle.rosenbrock(n), "power2": lambda: oracle.power(n, 2.0),
            "quadratic": lambda: oracle.quadratic(n)}[name]()


# The cases of the tests: name -> (objective, n, lb, ub, nstart, params)
CASES = {
    "A": ("rosenbrock", 3, -1.0, 5.0, 130, P),
    "B": ("rosenbrock", 8, -1.5, 1.2, 65, P),
    "C": ("rosenbrock", 3, -2.0, 0.5, 130, P),
    "D": ("rosenbrock", 3, -1.0, 5.0, 65, params(maxIterLineSearch=2)),
    "E": ("rosenbrock", 3, -1.0, 5.0, 65, params(alphaGuess=1e-3, maxIterLineSearch=3, maxIter=200)),
    "F": ("power2", 1, 0.5, 3.0, 65, P),
    "G": ("rosenbrock", 3, -1.0, 5.0, 65, params(maxIter=0)),
    "corners": ("rosenbrock", 2, 2.0, 3.0, 130, P),
    "quadratic": ("quadratic", 5, -0.5, 0.5, 65, P),
}

# three hand-made starts of case A's box with a coordinate outside it by more than |bound| / 1000:
# checkBoxBounds puts that coordinate on the midpoint
OUT_OF_BOX = np.array([[-1.5, 2.0, 3.0], [0.5, 5.1, 1.0], [7.0, -3.0, 2.5]])

_CACHE = {}


def batch(oracle, name, n, lb, ub, x0, p, key=None):
    """The Runs of the rows of x0 in the box [lb, ub]^n on the oracle objective `name`; with a
    key, computed once per start and shared."""
    runs = _CACHE.setdefault(key, []) if key is not None else []
    if len(runs) < len(x0):
        fn = oracle_fn(oracle, oracle_obj(oracle, name, n))
        lo, hi = np.full(n, lb), np.full(n, ub)
        for s in range(len(runs), len(x0)):
            runs.append(find_min_bnd(fn, x0[s], lo, hi, p))
    return runs[:len(x0)]


def case_x0(case, nstart=None, first=0):
    name, n, lb, ub, ns, p = CASES[case]
    return grid_x0(ns if nstart is None else nstart, n, lb, ub, first)


def case_runs(oracle, case, nstart=None):
    """The Runs of the first nstart starts of a case (all of them by default)."""
    name, n, lb, ub, ns, p = CASES[case]
    ns = ns if nstart is None else nstart
    return batch(oracle, name, n, lb, ub, grid_x0(ns, n, lb, ub), p, key=case)


def info_of(r):
    """The info word the library returns for a Run."""
    return r.depth | (CORNER if r.flagged else 0)


def stacked(runs):
    """(X, f0, fopt, iters, evals, info) arrays of a list of Runs, with the dtypes the library returns."""
    return (np.array([r.X for r in runs]), np.array([r.f0 for r in runs]), np.array([r.fopt for r in runs]),
            np.array([r.iters for r in runs], dtype=np.int32), np.array([r.evals for r in runs], dtype=np.int64),
            np.array([info_of(r) for r in runs], dtype=np.int32))
