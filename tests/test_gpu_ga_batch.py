"""Batched genetic algorithm on the GPU (csrc/kernels/ga_batch.hip): one 64-lane workgroup per
run.  The built-in scalar objectives have no transcendental (Power with power = 2 is x * x), so
every run of a batch is compared bit for bit -- X, f0, fOpt, generations, evaluations, info --
with the plain-Python restatement of GeneticAlgorithm::runGA (tests/ga_reference.py) on the
oracle's objective values, and, wherever the oracle defines the run, with oracle.ga_findmin
itself; tests/test_ga_batch_reference.py proves the restatement's two forms.  The largest launch
here is 65 workgroups."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ga_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("X", "f0", "fopt", "gens", "evals", "info")


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


def _solve(ctx, name, n, lb, ub, x0, p, seed=R.SEED0):
    from parallelnonlinearoptimizationlibrary_amd.device import run_ga_batch
    return run_ga_batch(_dobj(ctx, name, n), x0, np.full(n, lb), np.full(n, ub), p, seed)


_CACHE = {}


def _device(ctx, case, nrun=None):
    """The device-pointer solution of the first nrun runs of a case (solved once)."""
    name, n, lb, ub, _, runs, p = R.CASES[case]
    ns = runs if nrun is None else nrun
    if (case, ns) not in _CACHE:
        _CACHE[case, ns] = _solve(ctx, name, n, lb, ub, R.case_x0(case, ns), p)
    return _CACHE[case, ns]


def _ref(oracle, case, nrun=None):
    return R.stacked(R.case_runs(oracle, case, nrun))


def _assert_oracle(oracle, case, got):
    """The first five outputs against oracle.ga_findmin run by run."""
    name, n, lb, ub, x, _, p = R.CASES[case]
    X, f0, fopt, gens, evals, info = got
    for s in range(len(f0)):
        Xo, res, st = oracle.ga_findmin(R.make_obj(oracle, name, n), [x] * n, [lb] * n, [ub] * n, list(p),
                                        R.SEED0 + s)
        assert st == 0 and info[s] == 0
        assert _bits(Xo) == _bits(X[s]), s
        assert _bits(np.float64(res.f0)) == _bits(f0[s]) and _bits(np.float64(res.fopt)) == _bits(fopt[s]), s
        assert (res.iters, res.evals) == (gens[s], evals[s]), s


# ---- 1. Rosenbrock n = 3, Npop = 40: runs that end at 54 different generations -------------
@pytest.mark.parametrize("nrun", [1, 3, 65])
def test_batch_bitwise_against_restatement(ctx, oracle, nrun):
    got = _device(ctx, "ros3", nrun)
    _assert_bitwise(got, _ref(oracle, "ros3", nrun))
    _assert_oracle(oracle, "ros3", got)


# ---- 2. a population smaller than a wave: identical-child redraws, selections of 32 pairs --
def test_small_population(ctx, oracle):
    got = _device(ctx, "small")
    _assert_bitwise(got, _ref(oracle, "small"))
    _assert_oracle(oracle, "small", got)


# ---- 3. the Npop and n edges: Npop = 64 at n = 12; Npop = 130 (three member chunks with a
# tail); the reference defaults' shape; the LDS maximum; Power-2 at n = 1; the quadratic, whose
# data the kernel reads at wave-uniform addresses; maxGenerations = 0 ------------------------
@pytest.mark.parametrize("case", ["n12", "npop130", "defaults", "lds_max", "power", "quadratic", "gen0"])
def test_cases(ctx, oracle, case):
    got = _device(ctx, case)
    ref = _ref(oracle, case)
    if case == "gen0":
        assert np.all(ref[3] == 0)
    _assert_bitwise(got, ref)
    _assert_oracle(oracle, case, got)


# ---- 4. the speculation width of the selection is a tuning knob ----------------------------
_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import ga_reference as R
from parallelnonlinearoptimizationlibrary_amd import _lib as L
from parallelnonlinearoptimizationlibrary_amd.device import Context, DeviceObjective, run_ga_batch
name, n, lb, ub, _, runs, p = R.CASES["small"]
ctx = Context(0)
out = run_ga_batch(DeviceObjective(ctx, L.OBJ_ROSENBROCK, n), R.case_x0("small"), np.full(n, lb), np.full(n, ub), p,
                   R.SEED0)
np.savez({out!r}, *out)
"""


@pytest.mark.parametrize("width", [1, 3])
def test_speculation_width_gives_the_same_bits(ctx, oracle, tmp_path, width):
    """PNOL_GA_SPEC = 1 and 3 in a fresh process: the bits of the default width."""
    out = str(tmp_path / "spec.npz")
    env = dict(os.environ, PNOL_GA_SPEC=str(width))
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    with np.load(out) as z:
        got = tuple(z[f"arr_{i}"] for i in range(6))
    _assert_bitwise(got, _device(ctx, "small"))
    _assert_bitwise(got, _ref(oracle, "small"))


# ---- 5. a run's result does not depend on the batch it is in -------------------------------
@pytest.mark.parametrize("s", [0, 37, 64])
def test_batch_independence(ctx, s):
    name, n, lb, ub, _, _, p = R.CASES["ros3"]
    whole = _device(ctx, "ros3")
    one = _solve(ctx, name, n, lb, ub, R.case_x0("ros3", 1), p, seed=R.SEED0 + s)
    _assert_bitwise(whole, one, rows=slice(s, s + 1), ref_rows=slice(0, 1))


# ---- 6. the host class with device evaluation ----------------------------------------------
def test_host_class_equals_run_0(ctx):
    from parallelnonlinearoptimizationlibrary_amd.device import run_ga
    name, n, lb, ub, x, _, p = R.CASES["ros3"]
    X, f0, fopt, gens, evals, info = _device(ctx, "ros3")
    Xh, res = run_ga(_dobj(ctx, name, n), [x] * n, np.full(n, lb), np.full(n, ub), list(p), R.SEED0, which=0)
    assert _bits(Xh) == _bits(X[0])
    assert _bits(np.float64(res.f0)) == _bits(f0[0]) and _bits(np.float64(res.fopt)) == _bits(fopt[0])
    assert (res.iters, res.evals, int(info[0])) == (gens[0], evals[0], 0)


# ---- 7. the host-pointer entry point runs the same launch ----------------------------------
def test_entry_points_agree(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_ga_batch
    name, n, lb, ub, _, _, p = R.CASES["ros3"]
    host = run_ga_batch(None, R.case_x0("ros3", 3), np.full(n, lb), np.full(n, ub), p, R.SEED0,
                        kind=L.OBJ_ROSENBROCK)
    _assert_bitwise(host, _device(ctx, "ros3", 3))


# ---- 8. non-finite runs --------------------------------------------------------------------
def test_non_finite_starts(ctx, oracle):
    """Runs 1 and 3 of four start from NaN and from inf.  The all-NaN population is flat, selects
    uniformly and runs to maxGenerations = 10; the inf start is repaired into the box; their
    neighbours are the runs they would be alone.  IEEE 754 leaves the sign of a NaN result open
    (x - NaN keeps the NaN's sign on the CPU and flips it on the GPU), so the NaN run's X, f0 and
    fOpt are compared as NaN, its counts and info exactly; the three other runs bit for bit."""
    n, lb, ub = 2, -2.0, 2.0
    p = R.params(Npop=20, maxGenerations=10)
    x0 = np.array([[-1.0] * n, [np.nan] * n, [-1.0] * n, [np.inf] * n])
    runs = R.batch(oracle, "rosenbrock", n, lb, ub, x0, p, key="nonfinite")
    got = _solve(ctx, "rosenbrock", n, lb, ub, x0, p)
    assert runs[1].gens == 10 and np.all(np.isnan(runs[1].X)) and np.isfinite(runs[3].fopt)
    ref = R.stacked(runs)
    finite = np.array([0, 2, 3])
    _assert_bitwise(got, ref, rows=finite)
    assert np.all(np.isnan(got[0][1])) and np.isnan(got[1][1]) and np.isnan(got[2][1])
    assert (got[3][1], got[4][1], got[5][1]) == (ref[3][1], ref[4][1], ref[5][1]) == (10, 200, 0)
    for s in (0, 2):
        Xo, res, st = oracle.ga_findmin(oracle.rosenbrock(n), x0[s], [lb] * n, [ub] * n, list(p), R.SEED0 + s)
        assert st == 0 and _bits(Xo) == _bits(got[0][s]) and (res.iters, res.evals) == (got[3][s], got[4][s])


# ---- 9. runs whose F overflows -------------------------------------------------------------
def test_overflowing_boxes(ctx, oracle):
    """Rosenbrock n = 2 from x0 = -1, one run each.  In [-1e77, 1e77]^2 about a third of the first
    population has a finite F below an inf worst, every fitness ratio is inf / inf, and the run ends
    with PNOL_GA_BATCH_STUCK at generation 0 where a host selection would never return.  In
    [-1e200, 1e200]^2 only member 0 has a finite F, so every fitness past index 0 is NaN and
    select_member's own rule calls the generation flat: the run is not stuck, it selects uniformly
    and ends by the static stop after 5 generations, as the host class does
    (tests/test_ga_batch_reference.py::test_overflowing_boxes).  Neither can hang: the pre-check
    and the cap bound every selection.  The oracle is not called on either."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    n = 2
    p = R.params(Npop=40, maxGenerations=50, NstaticGenerations=5)
    x0 = np.full((1, n), -1.0)
    stuck = R.batch(oracle, "rosenbrock", n, -1e77, 1e77, x0, p, key="box1e77")
    assert (stuck[0].info, stuck[0].gens, stuck[0].evals) == (R.STUCK, 0, 40)
    got = _solve(ctx, "rosenbrock", n, -1e77, 1e77, x0, p)
    assert got[5][0] == L.GA_BATCH_STUCK and got[3][0] == 0
    _assert_bitwise(got, R.stacked(stuck))
    flat = R.batch(oracle, "rosenbrock", n, -1e200, 1e200, x0, p, key="box1e200")
    assert (flat[0].info, flat[0].gens, flat[0].counters.stop) == (0, 5, "static")
    _assert_bitwise(_solve(ctx, "rosenbrock", n, -1e200, 1e200, x0, p), R.stacked(flat))


# ---- 10. refusals ---------------------------------------------------------------------------
def test_refusals(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    p = R.CASES["ros3"][6]
    for n, prm, status in ((L.GA_BATCH_NMAX + 1, p, L.PNOL_ERR_UNSUPPORTED),
                           (3, R.params(Npop=L.GA_BATCH_NPOP_MAX + 1), L.PNOL_ERR_UNSUPPORTED),
                           (3, R.params(eliteFrac=0.5, crossFrac=0.3, eliteMutationFrac=0.2), L.PNOL_ERR_ARG),
                           (3, R.params(eliteFrac=0.9), L.PNOL_ERR_ARG),
                           (3, R.params(Npop=1), L.PNOL_ERR_ARG),
                           (3, R.params(maxGenerations=-1), L.PNOL_ERR_ARG)):
        with pytest.raises(L.PnolError) as e:
            _solve(ctx, "rosenbrock", n, -2.0, 2.0, np.full((2, n), -1.0), prm)
        assert e.value.status == status, (n, prm)


# ---- 11. the C++ header: GeneticAlgorithmBatch from a small program ------------------------
def test_cxx_header_program(ctx, tmp_path):
    """tests/cpp/ga_batch_cxx.cpp runs the first 4 runs of case ros3 and prints X, f0, fOpt (hex
    doubles), generations, evaluations and info per run."""
    pkg = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")
    exe = str(tmp_path / "ga_batch_cxx")
    subprocess.run(["g++", "-O2", "-std=c++0x", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ga_batch_cxx.cpp"), "-L",
                    pkg, "-lpnol_amd", "-pthread", f"-Wl,-rpath,{pkg}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("X ")]
    assert len(rows) == 4 and all(len(row) == 3 + 5 for row in rows)
    vals = np.array([[float.fromhex(v) for v in row[:5]] for row in rows])
    X, f0, fopt, gens, evals, info = _device(ctx, "ros3", 65)
    assert _bits(vals[:, :3]) == _bits(X[:4])
    assert _bits(vals[:, 3]) == _bits(f0[:4]) and _bits(vals[:, 4]) == _bits(fopt[:4])
    assert [int(row[5]) for row in rows] == gens[:4].tolist()
    assert [int(row[6]) for row in rows] == evals[:4].tolist()
    assert [int(row[7]) for row in rows] == info[:4].tolist()
