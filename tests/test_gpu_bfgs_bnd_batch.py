"""Batched box-bounded BFGS on the GPU (csrc/kernels/bfgs_bnd_batch.hip): one lane per start.  The
built-in scalar objectives have no transcendental (Power with power = 2 is x * x), so every start
of a batch is compared bit for bit -- X, f0, fOpt, iterations, evaluations, info -- with the
plain-Python restatement of BFGS_Bnd::findMinBnd (tests/bfgs_bnd_reference.py) on the oracle's
objective values; tests/test_bfgs_bnd_batch_cpu.py proves that restatement bitwise the oracle's
bfgs_bnd_findmin_ex on every start it does not flag and that these inputs take every reachable
branch.  Every launch here is at most 130 lanes."""
import os
import subprocess

import numpy as np
import pytest

import bfgs_bnd_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("X", "f0", "fopt", "iters", "evals", "info")


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


def _solve(ctx, name, n, lb, ub, x0, p):
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_bnd_batch
    return run_bfgs_bnd_batch(_dobj(ctx, name, n), x0, np.full(n, lb), np.full(n, ub), p)


_CACHE = {}


def _device(ctx, case, nstart=None):
    """The device-pointer solution of the first nstart starts of a case (solved once)."""
    name, n, lb, ub, ns, p = R.CASES[case]
    ns = ns if nstart is None else nstart
    if (case, ns) not in _CACHE:
        _CACHE[case, ns] = _solve(ctx, name, n, lb, ub, R.case_x0(case, ns), p)
    return _CACHE[case, ns]


def _ref(oracle, case, nstart=None):
    return R.stacked(R.case_runs(oracle, case, nstart))


# ---- 1. case A (Rosenbrock n = 3 in [-1, 5]^3), bitwise per start --------------------------
@pytest.mark.parametrize("nstart", [1, 63, 64, 65, 130])
def test_batch_bitwise_against_restatement(ctx, oracle, nstart):
    """A partial wave, an exact wave, a wave plus one, two waves plus a tail; lanes of one wave end
    at depths 0, 1 and 2 and at different trips."""
    if nstart == 130:
        runs = R.case_runs(oracle, "A")
        assert len(set(r.depth for r in runs)) >= 3 and len(set(r.iters for r in runs)) >= 3
    _assert_bitwise(_device(ctx, "A", nstart), _ref(oracle, "A", nstart))


# ---- 2. the other cases: B (n = 8, depths 2-5, multi-freeze), C (corner ends among ordinary
# starts), D (maxIterLineSearch = 2: zooms ended by iter_ls, exhausted outer searches), E (every
# start runs to maxIter through the shared totalIter), F (n = 1: all frozen at depth 0), G
# (maxIter = 0) ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["B", "C", "D", "E", "F", "G"])
def test_cases(ctx, oracle, case):
    ref = _ref(oracle, case)
    got = _device(ctx, case)
    if case == "C":
        flagged = (ref[5] & R.CORNER) != 0
        assert 0 < flagged.sum() < len(flagged)
        assert np.array_equal((got[5] & R.CORNER) != 0, flagged)
    if case == "G":
        assert np.all(ref[3] == 0) and _bits(got[0]) == _bits(R.case_x0("G"))
    _assert_bitwise(got, ref)


# ---- 3. every start a corner end -----------------------------------------------------------
def test_all_corner_ends(ctx, oracle):
    """Rosenbrock n = 2 in [2, 3]^2, 65 starts: both coordinates are frozen one after the other;
    info bit 8 is set on every start."""
    ref = _ref(oracle, "corners", 65)
    got = _device(ctx, "corners", 65)
    assert np.all(ref[5] & R.CORNER)
    assert np.all(got[5] & R.CORNER) and np.all((got[5] & 0xFF) >= 1)
    _assert_bitwise(got, ref)


# ---- 4. the quadratic, whose data the kernel reads at wave-uniform addresses ---------------
def test_quadratic(ctx, oracle):
    """The synthetic quadratic n = 5 in [-0.5, 0.5]^5, 65 starts."""
    _assert_bitwise(_device(ctx, "quadratic"), _ref(oracle, "quadratic"))


# ---- 5. n = NMAX: the LDS maximum, dynamic LDS above 64 KB ---------------------------------
def test_n_max(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    n = L.BFGS_BND_BATCH_NMAX
    assert 8 * 64 * (n * n + n * (n + 1) // 2 + 8 * n) > 64 * 1024
    x0 = R.grid_x0(65, n, -1.5, 1.2)
    runs = R.batch(oracle, "rosenbrock", n, -1.5, 1.2, x0, R.P, key="nmax")
    assert max(r.depth for r in runs) >= 3
    _assert_bitwise(_solve(ctx, "rosenbrock", n, -1.5, 1.2, x0, R.P), R.stacked(runs))


# ---- 6. checkBoxBounds ---------------------------------------------------------------------
def test_out_of_box_starts(ctx, oracle):
    name, n, lb, ub, _, p = R.CASES["A"]
    runs = R.batch(oracle, name, n, lb, ub, R.OUT_OF_BOX, p)
    _assert_bitwise(_solve(ctx, name, n, lb, ub, R.OUT_OF_BOX, p), R.stacked(runs))


# ---- 7. a start's result does not depend on the batch it is in -----------------------------
def test_batch_independence(ctx):
    name, n, lb, ub, _, p = R.CASES["A"]
    whole = _device(ctx, "A")
    part = _solve(ctx, name, n, lb, ub, R.case_x0("A", 10, first=60), p)
    _assert_bitwise(whole, part, rows=slice(60, 70), ref_rows=slice(0, 10))


# ---- 8. the host-pointer entry point runs the same launch ----------------------------------
def test_entry_points_agree(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_bnd_batch
    name, n, lb, ub, _, p = R.CASES["A"]
    host = run_bfgs_bnd_batch(None, R.case_x0("A", 65), np.full(n, lb), np.full(n, ub), p, kind=L.OBJ_ROSENBROCK)
    _assert_bitwise(host, _device(ctx, "A", 65))


# ---- 9. the one-problem class: BFGS_Bnd on the device objective ----------------------------
def test_one_problem_class_equals_batch_rows(ctx, oracle):
    """The first 4 unflagged starts of case A through run_bfgs(which=2) equal the batch rows
    bitwise in X, f0 and fOpt."""
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    name, n, lb, ub, _, p = R.CASES["A"]
    runs = R.case_runs(oracle, "A")
    x0 = R.case_x0("A")
    X, f0, fopt = _device(ctx, "A")[:3]
    rows = [s for s, r in enumerate(runs) if not r.flagged][:4]
    assert len(rows) == 4
    for s in rows:
        Xs, res = run_bfgs(_dobj(ctx, name, n), x0[s], list(p), which=2, lb=np.full(n, lb), ub=np.full(n, ub))
        assert _bits(Xs) == _bits(X[s]), s
        assert _bits(np.float64(res.f0)) == _bits(f0[s]), s
        assert _bits(np.float64(res.fopt)) == _bits(fopt[s]), s


# ---- 10. the C++ header: BFGS_BndBatch from a small program --------------------------------
def test_cxx_header_program(ctx, tmp_path):
    """tests/cpp/bfgs_bnd_batch_cxx.cpp solves the first 4 starts of case A and prints X, f0, fOpt
    (hex doubles), iterations and info per start."""
    pkg = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")
    exe = str(tmp_path / "bfgs_bnd_batch_cxx")
    subprocess.run(["g++", "-O2", "-std=c++0x", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bfgs_bnd_batch_cxx.cpp"), "-L",
                    pkg, "-lpnol_amd", "-pthread", f"-Wl,-rpath,{pkg}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("X ")]
    assert len(rows) == 4 and all(len(row) == 3 + 4 for row in rows)
    vals = np.array([[float.fromhex(v) for v in row[:5]] for row in rows])
    X, f0, fopt, iters, _, info = _device(ctx, "A", 4)
    assert _bits(vals[:, :3]) == _bits(X)
    assert _bits(vals[:, 3]) == _bits(f0) and _bits(vals[:, 4]) == _bits(fopt)
    assert [int(row[5]) for row in rows] == iters.tolist()
    assert [int(row[6]) for row in rows] == info.tolist()
