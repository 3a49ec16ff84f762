"""Shared inputs of the batched Levenberg-Marquardt tests (test_lm_batch_cpu.py,
test_gpu_lm_batch.py): batches of noisy Cubic / ExpCurve fits and their per-problem oracle
solutions.  Every batch is drawn from np.random.default_rng(20261020) afresh, so a batch is a
function of its shape alone and the cached results below may be shared between tests (treat
them as read-only)."""
import functools

import numpy as np

SEED = 20261020
CUBIC_PARAMS = (0.001, 10, 1e-6, 10, 1e-5, -1)
EXP_PARAMS = (0.001, 10, 1e-6, 100, 1e-6, -1)
CUBIC_COEF = np.array([0.3, 1.1, -4.3, 7.3])
EXP_COEF = np.array([10.2, 0.4, 0.1])


@functools.lru_cache(maxsize=None)
def cubic_batch(nprob, m):
    """(xd, yd, x0): per-problem grids xd and data yd (nprob x m), x0 (nprob x 4)."""
    rng = np.random.default_rng(SEED)
    xd = np.linspace(-5, 5, m)[None, :] + 0.01 * rng.standard_normal((nprob, m))
    c = CUBIC_COEF[None, :] * (1 + 0.5 * rng.standard_normal((nprob, 4)))
    yd = c[:, 0:1] * xd ** 3 + c[:, 1:2] * xd ** 2 + c[:, 2:3] * xd + c[:, 3:4]
    yd = yd + 0.05 * rng.standard_normal((nprob, m))
    return np.ascontiguousarray(xd), np.ascontiguousarray(yd), np.full((nprob, 4), 0.1)


@functools.lru_cache(maxsize=None)
def exp_batch(nprob, m):
    """(xd, yd, x0): the shared grid xd (m), data yd (nprob x m), x0 (nprob x 3)."""
    rng = np.random.default_rng(SEED)
    xd = np.linspace(0, 5, m)
    c = EXP_COEF[None, :] * (1 + 0.2 * rng.standard_normal((nprob, 3)))
    yd = c[:, 0:1] * np.exp(c[:, 1:2] * xd[None, :]) + c[:, 2:3] + 0.01 * rng.standard_normal((nprob, m))
    return xd, np.ascontiguousarray(yd), np.full((nprob, 3), 0.1)


def oracle_solve(O, kind, xd, yd, x0, params):
    """The oracle's LevMarq::findMin problem by problem.  xd: one grid (m) or one per problem.
    Returns dict(X, chi0, chi, iters, evals, F0, FOpt) of arrays over the batch."""
    nprob, m = yd.shape
    n = x0.shape[1]
    out = dict(X=np.zeros((nprob, n)), chi0=np.zeros(nprob), chi=np.zeros(nprob),
               iters=np.zeros(nprob, dtype=np.int32), evals=np.zeros(nprob, dtype=np.int64),
               F0=np.zeros((nprob, m)), FOpt=np.zeros((nprob, m)))
    for p in range(nprob):
        o = O.Obj(kind, n, m, xd if xd.ndim == 1 else xd[p], yd[p])
        X, res, F0, FOpt, _ = O.lm_findmin(o, x0[p], params)
        out["X"][p], out["F0"][p], out["FOpt"][p] = X, F0, FOpt
        out["chi0"][p], out["chi"][p], out["iters"][p], out["evals"][p] = res.f0, res.fopt, res.iters, res.evals
    return out


_ORACLE_CACHE = {}


def cubic_oracle(O, nprob, m):
    key = ("cubic", nprob, m)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = oracle_solve(O, O.CUBIC, *cubic_batch(nprob, m), CUBIC_PARAMS)
    return _ORACLE_CACHE[key]


def exp_oracle(O, nprob, m):
    key = ("exp", nprob, m)
    if key not in _ORACLE_CACHE:
        xd, yd, x0 = exp_batch(nprob, m)
        _ORACLE_CACHE[key] = oracle_solve(O, O.EXPCURVE, xd, yd, x0, EXP_PARAMS)
    return _ORACLE_CACHE[key]
