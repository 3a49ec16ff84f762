"""Batched BFGS on the GPU (csrc/kernels/bfgs_batch.hip): one lane per start.  The built-in scalar
objectives have no transcendental (Power with power = 2 is x * x), so every start of a batch is
compared bit for bit -- X, f0, fOpt, the last gradient norm, iterations, evaluations -- with the
plain-Python restatement of BFGS::findMin (tests/bfgs_reference.py) on the oracle's objective
values; tests/test_bfgs_batch_cpu.py proves that restatement bitwise the oracle's bfgs_findmin and
that these inputs take every branch of the line search.  Every launch here is at most 130 lanes."""
import os
import subprocess

import numpy as np
import pytest

import bfgs_reference as BR
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("X", "f0", "fopt", "gnorm", "iters", "evals")


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


def _device(ctx, name, n, nstart, p=BR.DEFAULTS):
    """The device-pointer solution of the first nstart starts of the standard batch (solved once)."""
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_batch
    key = (name, n, nstart, tuple(p))
    if key not in _CACHE:
        _CACHE[key] = run_bfgs_batch(_dobj(ctx, name, n), BR.standard_x0(nstart, n), p)
    return _CACHE[key]


def _ref(oracle, name, n, nstart, p=BR.DEFAULTS):
    return BR.stacked(BR.standard_batch(oracle, name, n, nstart, p))


# ---- 1. Rosenbrock n = 3, bitwise per start ------------------------------------------------
@pytest.mark.parametrize("nstart", [1, 63, 64, 65, 130])
def test_batch_bitwise_against_restatement(ctx, oracle, nstart):
    """A partial wave, an exact wave, a wave plus one, two waves plus a tail."""
    if nstart == 130:
        # guards the inputs: neighbouring lanes leave the loop at different trips and take every
        # branch (the exhausted outer search has test 6)
        runs = BR.standard_batch(oracle, "rosenbrock", 3, 130)
        assert len(set(r.iters for r in runs)) >= 3
        total = dict(zip(BR.COUNTERS, np.sum([r.counts for r in runs], axis=0).tolist()))
        assert all(v > 0 for k, v in total.items() if k != "outer_exhausted"), total
    _assert_bitwise(_device(ctx, "rosenbrock", 3, nstart), _ref(oracle, "rosenbrock", 3, nstart))


# ---- 2. n edges, 65 starts each: n = 1 (a 1 x 1 D), n = 2, n = 5 (the testBFGS size: both the
# local minimum f = 3.93 and the global one are reached), n = 12 (the LDS maximum, dynamic LDS
# above 64 KB; some starts stop at maxIter = 100), and the quadratic, whose data the kernel reads
# at wave-uniform addresses ------------------------------------------------------------------
EDGES = [("power2", 1), ("rosenbrock", 2), ("rosenbrock", 5), ("rosenbrock", 12), ("quadratic", 5)]


@pytest.mark.parametrize("name,n", EDGES, ids=[f"{e[0]}-n{e[1]}" for e in EDGES])
def test_n_edges(ctx, oracle, name, n):
    ref = _ref(oracle, name, n, 65)
    if (name, n) == ("rosenbrock", 5):
        assert np.any(np.abs(ref[2] - 3.9308) < 1e-3) and np.any(ref[2] < 1e-8)
    if (name, n) == ("rosenbrock", 12):
        assert np.any(ref[4] == 100) and np.any(ref[4] < 100)
    _assert_bitwise(_device(ctx, name, n, 65), ref)


# ---- 3. a start's result does not depend on the batch it is in -----------------------------
def test_batch_independence(ctx):
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_batch
    whole = _device(ctx, "rosenbrock", 3, 130)
    part = run_bfgs_batch(_dobj(ctx, "rosenbrock", 3), BR.standard_x0(10, 3, first=60), BR.DEFAULTS)
    _assert_bitwise(whole, part, rows=slice(60, 70), ref_rows=slice(0, 10))


# ---- 4. maxIter = 0: the gradient and f0 are evaluated, nothing moves ----------------------
def test_max_iter_zero(ctx, oracle):
    p = BR.params(maxIter=0)
    got = _device(ctx, "rosenbrock", 3, 65, p)
    _assert_bitwise(got, _ref(oracle, "rosenbrock", 3, 65, p))
    X, f0, fopt, gnorm, iters, evals = got
    assert np.all(iters == 0) and np.all(evals == 3 + 2)
    assert _bits(X) == _bits(BR.standard_x0(65, 3))
    assert _bits(fopt) == _bits(f0)
    assert np.all(gnorm == 2 * p[9])


# ---- 5. maxIterLineSearch = 2: every start exhausts its zoom, alpha = 0 --------------------
def test_max_iter_line_search_two(ctx, oracle):
    p = BR.params(maxIterLineSearch=2)
    runs = BR.standard_batch(oracle, "rosenbrock", 3, 65, p)
    assert all(r.counts[BR.COUNTERS.index("zoom_exhausted")] == 1 for r in runs)
    got = _device(ctx, "rosenbrock", 3, 65, p)
    _assert_bitwise(got, BR.stacked(runs))
    assert np.all(got[4] == 1)
    assert _bits(got[0]) == _bits(BR.standard_x0(65, 3))


# ---- 6. the outer search exhausted (tests/test_bfgs_batch_cpu.py asserts the counter) ------
def test_outer_search_exhausted(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_batch
    name, n, x0, p = BR.OUTER_EXHAUSTED
    r = BR.find_min(BR.oracle_fn(oracle, BR.oracle_obj(oracle, name, n)), np.array(x0), p)
    assert r.counts[BR.COUNTERS.index("outer_exhausted")] >= 1
    got = run_bfgs_batch(_dobj(ctx, name, n), np.array([x0]), p)
    _assert_bitwise(got, BR.stacked([r]))


# ---- 7. the one-problem path: BFGS (exact update) on the device objective ------------------
@pytest.mark.parametrize("host_eval", [False, True])
def test_one_problem_path_equals_start_0(ctx, oracle, host_eval):
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    r = BR.standard_batch(oracle, "rosenbrock", 3, 1)[0]
    x0 = BR.standard_x0(1, 3)[0]
    # 13th value: update mode 1 = exact; the driver reports BFGS's iteration count with a profile
    X, res = run_bfgs(_dobj(ctx, "rosenbrock", 3), x0, list(BR.DEFAULTS) + [1], which=0, host_eval=host_eval,
                      profile={})
    oX, ores, _ = oracle.bfgs_findmin(oracle.rosenbrock(3), x0, BR.DEFAULTS)
    bX, bf0, bfo, _, bit, bev = _device(ctx, "rosenbrock", 3, 1)
    for ref in ((r.X, r.f0, r.fopt, r.iters, r.evals), (bX[0], bf0[0], bfo[0], bit[0], bev[0]),
                (oX, ores.f0, ores.fopt, ores.iters, ores.evals)):
        assert _bits(X) == _bits(ref[0])
        assert _bits(np.float64(res.f0)) == _bits(np.float64(ref[1]))
        assert _bits(np.float64(res.fopt)) == _bits(np.float64(ref[2]))
        assert (res.iters, res.evals) == (int(ref[3]), int(ref[4]))


# ---- 8. a start whose objective is inf / NaN ends by maxIter and disturbs no other lane ----
def test_non_finite_start(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_batch
    bad = 37
    x0 = BR.standard_x0(65, 3)
    x0[bad] = 1e200   # x^2 overflows: Rosenbrock is inf at the start and NaN (inf - inf) around it
    got = run_bfgs_batch(_dobj(ctx, "rosenbrock", 3), x0, BR.DEFAULTS)
    assert 0 <= got[4][bad] <= BR.DEFAULTS[7]
    others = np.array([s for s in range(65) if s != bad])
    _assert_bitwise(got, _ref(oracle, "rosenbrock", 3, 65), rows=others)


# ---- 9. the host-pointer entry point runs the same launch ----------------------------------
def test_entry_points_agree(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_batch
    host = run_bfgs_batch(None, BR.standard_x0(65, 3), BR.DEFAULTS, kind=L.OBJ_ROSENBROCK)
    _assert_bitwise(host, _device(ctx, "rosenbrock", 3, 65))


# ---- 10. the C++ header: BFGSBatch from a small program, as test_gpu_lm_batch.py runs LevMarqBatch
def test_cxx_header_program(oracle, tmp_path):
    """tests/cpp/bfgs_batch_cxx.cpp solves the first 4 starts of the Rosenbrock n = 5 standard batch
    with the DEFAULTS parameters and prints X, f0, fOpt, gnorm (%.17g) and iterations per start."""
    pkg = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")
    exe = str(tmp_path / "bfgs_batch_cxx")
    subprocess.run(["g++", "-O2", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "bfgs_batch_cxx.cpp"), "-L", pkg, "-lpnol_amd", "-pthread",
                    f"-Wl,-rpath,{pkg}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("X ")]
    assert len(rows) == 4 and all(len(row) == 5 + 4 for row in rows)
    vals = np.array([[float(v) for v in row[:8]] for row in rows])
    X, f0, fopt, gnorm, iters, _ = _ref(oracle, "rosenbrock", 5, 4)
    assert _bits(vals[:, :5]) == _bits(X)
    assert _bits(vals[:, 5]) == _bits(f0) and _bits(vals[:, 6]) == _bits(fopt) and _bits(vals[:, 7]) == _bits(gnorm)
    assert [int(row[8]) for row in rows] == iters.tolist()
