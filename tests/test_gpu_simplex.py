"""Batched Nelder-Mead on the GPU (csrc/kernels/simplex_batch.hip): one lane per start.  The
built-in scalar objectives have no transcendental (Power with power = 2 is x * x), so every
start of a batch is compared bit for bit with the plain-Python restatement of
SimplexSearch::findMin (tests/simplex_reference.py) on the oracle's objective values."""
import numpy as np
import pytest

import simplex_reference as SR

pytestmark = pytest.mark.gpu

KEYS = ("X", "f0", "fopt", "iters", "evals")


@pytest.fixture(scope="module")
def ctx():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import Context
    if L.device_count() < 1:
        pytest.fail("no gfx950 device visible for a -m gpu run")
    return Context(0)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_bitwise(got, ref, rows=None, ref_rows=None):
    a = slice(None) if rows is None else rows
    b = a if ref_rows is None else ref_rows
    for k, g, r in zip(KEYS, got, ref):
        assert g[a].dtype == r[b].dtype, k
        assert g[a].shape == r[b].shape, k
        assert _bits(g[a]) == _bits(r[b]), k


def _dobj(ctx, name, n):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective
    if name == "rosenbrock":
        return DeviceObjective(ctx, L.OBJ_ROSENBROCK, n)
    if name == "power2":
        return DeviceObjective(ctx, L.OBJ_POWER, n, power=2.0)
    return DeviceObjective.synthetic(ctx, L.OBJ_QUADRATIC, n)   # the oracle's quadratic(n) data


_CACHE = {}


def _device(ctx, name, n, nstart, p=SR.DEFAULTS):
    """The device-pointer solution of the first nstart starts of the standard batch (solved once)."""
    from parallelnonlinearoptimizationlibrary_amd.device import run_simplex_batch
    key = (name, n, nstart, tuple(p))
    if key not in _CACHE:
        _CACHE[key] = run_simplex_batch(_dobj(ctx, name, n), SR.standard_x0(nstart, n), p, SR.SEED0)
    return _CACHE[key]


def _ref(oracle, name, n, nstart, p=SR.DEFAULTS):
    return SR.stacked(SR.standard_batch(oracle, name, n, nstart, p))


# ---- 1. Rosenbrock n = 3, bitwise per start ------------------------------------------------
@pytest.mark.parametrize("nstart", [1, 63, 64, 65, 130])
def test_batch_bitwise_against_restatement(ctx, oracle, nstart):
    """A partial wave, an exact wave, a wave plus one, two waves plus a tail."""
    if nstart == 130:
        # guards the inputs: neighbouring lanes must really leave the loop at different trips and
        # take every branch
        runs = SR.standard_batch(oracle, "rosenbrock", 3, 130)
        assert len(set(r.iters for r in runs)) >= 3
        total = np.sum([r.outcomes for r in runs], axis=0)
        assert all(total > 0), dict(zip(SR.OUTCOMES, total))
    _assert_bitwise(_device(ctx, "rosenbrock", 3, nstart), _ref(oracle, "rosenbrock", 3, nstart))


# ---- 2. n edges, 65 starts each: n = 1 (the accept test fref >= f[0] && fref < f[n-1] can never
# hold), n = 2, n = 10 (the reference's example size; start 6 shrinks), n = 12 (the LDS maximum),
# and the quadratic, whose data the kernel reads at wave-uniform addresses --------------------
EDGES = [("power2", 1, SR.DEFAULTS), ("rosenbrock", 2, SR.DEFAULTS), ("rosenbrock", 10, SR.params(maxIter=400)),
         ("rosenbrock", 12, SR.params(maxIter=200)), ("quadratic", 5, SR.DEFAULTS)]


@pytest.mark.parametrize("name,n,p", EDGES, ids=[f"{e[0]}-n{e[1]}" for e in EDGES])
def test_n_edges(ctx, oracle, name, n, p):
    if n == 10:
        assert SR.standard_batch(oracle, name, n, 65, p)[6].outcomes[SR.OUTCOMES.index("shrink")] > 0
    _assert_bitwise(_device(ctx, name, n, 65, p), _ref(oracle, name, n, 65, p))


# ---- 3. a start's result does not depend on the batch it is in -----------------------------
def test_batch_independence(ctx):
    from parallelnonlinearoptimizationlibrary_amd.device import run_simplex_batch
    whole = _device(ctx, "rosenbrock", 3, 130)
    part = run_simplex_batch(_dobj(ctx, "rosenbrock", 3), SR.standard_x0(10, 3, first=60), SR.DEFAULTS,
                             SR.SEED0 + 60)
    _assert_bitwise(whole, part, rows=slice(60, 70), ref_rows=slice(0, 10))


# ---- 4. maxIter = 0: the best vertex of the sorted initial simplex -------------------------
def test_max_iter_zero(ctx, oracle):
    p = SR.params(maxIter=0)
    got = _device(ctx, "rosenbrock", 3, 65, p)
    _assert_bitwise(got, _ref(oracle, "rosenbrock", 3, 65, p))
    X, f0, fopt, iters, evals = got
    assert np.all(iters == 0) and np.all(evals == 4)
    assert np.all(fopt <= f0)
    obj = oracle.rosenbrock(3)
    assert all(oracle.obj_eval(obj, X[s]) == fopt[s] for s in range(65))


# ---- 5. the one-problem path: SimplexSearch on the device objective ------------------------
@pytest.mark.parametrize("host_eval", [False, True])
def test_one_problem_path_equals_start_0(ctx, oracle, host_eval):
    from parallelnonlinearoptimizationlibrary_amd.device import run_simplex
    r = SR.standard_batch(oracle, "rosenbrock", 3, 1)[0]
    X, res = run_simplex(_dobj(ctx, "rosenbrock", 3), SR.standard_x0(1, 3)[0], SR.DEFAULTS, SR.SEED0,
                         host_eval=host_eval)
    bX, bf0, bfo, bit, bev = _device(ctx, "rosenbrock", 3, 1)
    for ref in ((r.X, r.f0, r.fopt, r.iters, r.evals), (bX[0], bf0[0], bfo[0], bit[0], bev[0])):
        assert _bits(X) == _bits(ref[0])
        assert _bits(np.float64(res.f0)) == _bits(np.float64(ref[1]))
        assert _bits(np.float64(res.fopt)) == _bits(np.float64(ref[2]))
        assert (res.iters, res.evals) == (int(ref[3]), int(ref[4]))


# ---- 6. a start whose objective is inf / NaN ends by maxIter and disturbs no other lane ----
def test_non_finite_start(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd.device import run_simplex_batch
    p = SR.params(maxIter=50)
    bad = 37
    x0 = SR.standard_x0(65, 3)
    x0[bad] = 1e200   # x^2 overflows: Rosenbrock is inf at the start and NaN (inf - inf) around it
    got = run_simplex_batch(_dobj(ctx, "rosenbrock", 3), x0, p, SR.SEED0)
    assert 0 <= got[3][bad] <= 50
    others = np.array([s for s in range(65) if s != bad])
    _assert_bitwise(got, _ref(oracle, "rosenbrock", 3, 65, p), rows=others)


# ---- 7. the host-pointer entry point runs the same launch ----------------------------------
def test_entry_points_agree(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_simplex_batch
    host = run_simplex_batch(None, SR.standard_x0(65, 3), SR.DEFAULTS, SR.SEED0, kind=L.OBJ_ROSENBROCK)
    _assert_bitwise(host, _device(ctx, "rosenbrock", 3, 65))
