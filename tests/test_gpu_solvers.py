"""Solver-level parity: the C++ drop-in classes (BFGS, BFGS_MPI, BFGS_Bnd, LevMarq, LevMarqMPI)
running on the GPU against the oracle and the reference outputs recorded in
tests/golden/reference_survey.json.  North-star tolerance: converged X within 1e-10
relative; bitwise wherever the device path follows the reference order (small n)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_survey.json")))


@pytest.fixture(scope="module")
def ctx():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import Context
    if L.device_count() < 1:
        pytest.fail("no gfx950 device visible for a -m gpu run")
    return Context(0)


def _obj(ctx, kind, n, m=0, p0=None, p1=None, power=2.0):
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective
    return DeviceObjective(ctx, kind, n, m, p0, p1, power)


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("key", ["bfgs_rosenbrock2_m12_1", "bfgs_rosenbrock2_3_3"])
def test_bfgs_rosenbrock2_matches_reference(ctx, key):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    g = GOLD[key]
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 2), g["x0"], g["params"])
    assert X.tolist() == g["X"]          # bitwise (reference-order device path at n=2)
    assert res.fopt == g["f"]
    assert res.evals == g["evals"]
    assert rel(X, g["X"]) <= 1e-10


def test_testBFGS_rosenbrock5(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    g = GOLD["testBFGS_rosenbrock5"]
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 5), g["x0"], g["params"][:11] + [0])
    Xo, reso, _ = oracle.bfgs_findmin(oracle.rosenbrock(5), g["x0"], g["params"])
    assert np.array_equal(X, Xo)
    assert res.fopt == g["f"]


def test_bfgs_host_eval_path_equals_device_path(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    g = GOLD["bfgs_rosenbrock2_m12_1"]
    o = _obj(ctx, L.OBJ_ROSENBROCK, 2)
    Xd, _ = run_bfgs(o, g["x0"], g["params"])
    Xh, _ = run_bfgs(o, g["x0"], g["params"], host_eval=True)
    assert np.array_equal(Xd, Xh)


def test_lm_expcurve(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    g = GOLD["testLMExp"]
    oe = oracle.expcurve()
    d = _obj(ctx, L.OBJ_EXPCURVE, 3, 100, oe.p0, oe.p1)
    # host objective (glibc exp, as the reference): bitwise with the reference output
    Xh, *_ = run_levmarq(d, g["x0"], g["params"], host_eval=True)
    assert Xh.tolist() == g["X"]
    # device FD batch (device exp): the north-star tolerance
    Xd, *_ = run_levmarq(d, g["x0"], g["params"])
    assert rel(Xd, g["X"]) <= 1e-10
    # LevMarqMPI, single rank: identical to LevMarq
    Xm, *_ = run_levmarq(d, g["x0"], g["params"], which=1, host_eval=True)
    assert Xm.tolist() == g["X"]


def test_lm_cubic_bitwise(ctx, oracle):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    g = GOLD["testLMCubicLinearCoef"]
    oc = oracle.cubic()
    d = _obj(ctx, L.OBJ_CUBIC, 4, 100, oc.p0, oc.p1)
    X, F0, FO, _ = run_levmarq(d, g["x0"], g["params"])
    assert X.tolist() == g["X"]


@pytest.mark.parametrize("m,n", [(600, 100), (3000, 257)])
def test_lm_linres_large(ctx, oracle, m, n):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    A, xs, y = oracle.linres_data(m, n)
    d = _obj(ctx, L.OBJ_LINRES, n, m, A, y)
    params = (0.001, 10, 1e-7, 6, 0.0, -1)
    X, F0, FO, _ = run_levmarq(d, np.zeros(n), params)
    Xo, *_ = oracle.lm_findmin(oracle.Obj(oracle.LINRES, n, m, A, y), np.zeros(n), params)
    assert rel(X, Xo) <= 1e-10
    assert rel(X, xs) <= 1e-8


@pytest.mark.parametrize("trips", [1, 2, 3])
def test_lm_cfg3_full_size_matches_oracle_trips(ctx, trips):
    """cfg 3 at the headline size (m = 16384, n = 2048, LevenbergMarquardt.cpp:50-136): the device
    LevMarq (FD Jacobian, MFMA J^T J, tile Cholesky) after 1, 2 and 3 loop trips against the
    oracle's X / chi^2 after the same trips (tests/golden/cfg3_lm_trips.npz, written by
    tests/golden/make_cfg3_lm_trips.py from the oracle's LU-based loop).  X within the north
    star's 1e-10 relative per trip (measured 2.9e-11 after trip 2); chi^2 within 1e-4 relative
    or the rounding floor; the evaluation count exact."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_levmarq
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "cfg3_lm_trips.npz"))
    m, n = int(g["m"]), int(g["n"])
    obj = DeviceObjective.synthetic(ctx, L.OBJ_LINRES, n, m)     # the oracle's splitmix64 stream
    params = tuple(g["params"][:3]) + (float(trips), 0.0, -1)
    X, F0, FO, res = run_levmarq(obj, np.zeros(n), params)
    obj.close()
    Xo = g["x_trips"][trips - 1]
    err = rel(X, Xo)
    print(f"trips {trips}: |X - X_oracle| / |X_oracle| = {err:.3e}, chi2 {res.fopt:.6e} vs {g['chi_trips'][trips - 1]:.6e}")
    assert err <= 1e-10, err
    assert res.f0 == float(g["chi0"]) or abs(res.f0 - float(g["chi0"])) <= 1e-12 * float(g["chi0"])
    # chi^2 after trip 2 is 2e-14 of chi0 (the residual of a point 3e-11 from the oracle's):
    # measured 7e-6 relative apart; after trip 3 it is at the rounding floor (6e-24 of chi0)
    chi_o = float(g["chi_trips"][trips - 1])
    assert abs(res.fopt - chi_o) <= max(1e-4 * chi_o, 1e-15 * float(g["chi0"])), (res.fopt, chi_o)
    assert res.evals == trips * (n + 2) + 1, res.evals


@pytest.mark.parametrize("m,n,lam0,iters", [(600, 100, 0.001, 12), (3000, 257, 0.001, 10), (2000, 300, 50.0, 9),
                                           (1000, 129, 1e-9, 12)])
def test_lm_one_wait_loop_equals_general_loop(ctx, oracle, m, n, lam0, iters):
    """The LM loop with one host wait per trip (n > PNOL_SEQ_MAX: the trip is queued whole, the
    trial point formed and evaluated on the device) replays the general loop exactly: X, F0,
    FOpt and the evaluation count are bitwise those of PNOL_LM_ASYNC=0, through accepted
    steps, the rejected ones after convergence (xMinDiff = 0 keeps the loop running) and a
    large starting lambda."""
    import os
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    A, xs, y = oracle.linres_data(m, n)
    params = (lam0, 10, 1e-7, iters, 0.0, -1)
    out = {}
    for mode in ("1", "0"):
        os.environ["PNOL_LM_ASYNC"] = mode
        try:
            d = _obj(ctx, L.OBJ_LINRES, n, m, A, y)
            out[mode] = run_levmarq(d, np.zeros(n), params)
        finally:
            os.environ.pop("PNOL_LM_ASYNC", None)
    (Xa, F0a, FOa, ra), (Xs, F0s, FOs, rs) = out["1"], out["0"]
    assert np.array_equal(Xa, Xs)
    assert np.array_equal(F0a, F0s) and np.array_equal(FOa, FOs)
    assert ra.evals == rs.evals
    assert rel(Xa, xs) <= 1e-8


def test_bfgs_mpi_pool_matches_oracle(ctx, oracle):
    """BFGS_MPI with Npool = 8 in one process equals the reference at np = 8, including the
    zero-pool defect (f = 0)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    P = [1e-4, 0.1, 4, 1, 1000, 1e-7, 1e-3, 200, 1e-5, 1e-5, 0, 0]   # testBFGS_MPI (verbose off)
    for npool in (2, 4, 8):
        X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 10), [10.0] * 10, P + [npool], which=1)
        Xo, reso = oracle.bfgs_mpi_findmin(oracle.rosenbrock(10), [10.0] * 10, P, npool)
        assert np.array_equal(X, Xo), npool
        assert res.fopt == reso.fopt
    assert res.fopt == 0.0
    # with the defect fixed the result is a real function value
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 10), [10.0] * 10, P + [8, 1], which=1)
    assert res.fopt > 0.0


@pytest.mark.parametrize("case", [
    ("testBFGSBnd", 5, [2.0] * 5, [-5.0] * 5, [5.0] * 5),
    ("lower-active", 3, [-1.0, 2.0, 2.0], [-1.0] * 3, [5.0] * 3),
    ("upper-active", 3, [0.0, 0.0, 0.0], [-2.0] * 3, [0.5] * 3),
    # frozen sets at interior and several positions at once (the in-place reduced vectors)
    ("alternating", 12, [0.2, -0.2] * 6, [-0.3] * 12, [0.6] * 12),
    ("upper-ramp", 16, list(np.linspace(-0.9, 0.9, 16)), [-1.0] * 16, [0.35] * 16),
    ("interior-lower", 9, [1.5] * 9, [0.2, 1.2, 0.2, 1.3, 0.2, 1.1, 0.2, 1.4, 0.2], [2.0] * 9),
])
def test_bfgs_bnd_matches_oracle(ctx, oracle, case):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    name, n, x0, lb, ub = case
    Pb = [1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1]   # Examples.cpp:75
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, n), x0, Pb, which=2, lb=lb, ub=ub)
    Xo, reso = oracle.bfgs_bnd_findmin(oracle.rosenbrock(n), x0, lb, ub, Pb)
    assert np.array_equal(X, Xo), name
    assert res.fopt == reso.fopt


@pytest.mark.parametrize("power", [2.0, 3.0])
def test_bfgs_bnd_power_recur(ctx, oracle, power):
    """BFGS_Bnd on PowerObject (ExampleObjectives.hpp:206-234) with every coordinate driven to its
    lower bound one recursion level at a time, so the Recur FD gradient (PNOL_Objective.cpp:337-360)
    runs at every level with frozen coordinates.  power = 2 takes the same-point reuse (values
    formed by the library's own host formula, the device kernel's bits); power = 3 calls pow,
    whose host and device results may differ in the last place, so its Recur gradients stay on
    the device.  Either way the run equals the oracle's (bitwise for power 2; power 3 within 1e-12,
    the oracle's glibc pow against the device's)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    n = 8
    x0 = list(np.linspace(-0.9, -0.2, n)) if power == 3.0 else list(np.linspace(0.9, 0.2, n))
    lb, ub = [-1.0] * n, [1.0] * n
    if power == 2.0:
        lb = list(np.linspace(0.1, 0.45, n))     # the minimiser of sum x^2 outside the box: all bounds active
    Pb = [1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1]   # Examples.cpp:75
    X, res = run_bfgs(_obj(ctx, L.OBJ_POWER, n, power=power), x0, Pb, which=2, lb=lb, ub=ub)
    Xo, reso = oracle.bfgs_bnd_findmin(oracle.power(n, power), x0, lb, ub, Pb)
    print(f"power {power}: max |X - Xo| = {np.max(np.abs(X - Xo)):.3e}, evals {res.evals} vs {reso.evals}")
    assert np.allclose(X, lb, atol=1e-5)
    if power == 2.0:
        assert np.array_equal(X, Xo) and res.fopt == reso.fopt and res.evals == reso.evals
    else:
        assert np.max(np.abs(X - Xo)) <= 1e-12 and abs(res.fopt - reso.fopt) <= 1e-12 * abs(reso.fopt)


BND_MPI_P = [1e-4, 0.1, 1e-16, 4, 1, 1000, 1e-7, 1e-3, 200, 1e-5, 1e-5, 1e-5, 0, 0]   # Examples.cpp:112


def _testBFGSBnd_MPI_start():
    n = 10      # Examples.cpp:90-105
    x0 = np.full(n, 3.0); x0[0] = -0.5; x0[1] = 3.0
    lb = np.full(n, -5.0); lb[0] = -1.0
    return n, x0, lb, np.full(n, 5.0)


@pytest.mark.parametrize("npool", [2, 3, 4, 8])
def test_bfgs_bnd_mpi_matches_oracle(ctx, oracle, npool):
    """BFGSBnd_MPI (testBFGSBnd_MPI, Examples.cpp:90-120) with Npool trial steps in one process
    equals the reference at np = Npool bitwise: X, fOpt and the evaluation count.  X[0] ends on
    its lower bound, so the run goes through boundaryAssessment's recursion."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    n, x0, lb, ub = _testBFGSBnd_MPI_start()
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, n), x0, BND_MPI_P + [npool], which=3, lb=lb, ub=ub)
    Xo, reso, st = oracle.bfgs_bnd_mpi_findmin(oracle.rosenbrock(n), x0, lb, ub, BND_MPI_P, npool)
    assert st == 0
    assert np.array_equal(X, Xo), (npool, X, Xo)
    assert res.fopt == reso.fopt and res.f0 == reso.f0
    assert res.evals == reso.evals
    assert np.all(X >= lb) and np.all(X <= ub)


@pytest.mark.parametrize("case", [
    ("lower-active", 3, [-1.0, 2.0, 2.0], [-1.0] * 3, [5.0] * 3),
    ("upper-active", 3, [0.0, 0.0, 0.0], [-2.0] * 3, [0.5] * 3),
    ("interior", 4, [2.0] * 4, [-5.0] * 4, [5.0] * 4),
])
def test_bfgs_bnd_mpi_box_cases(ctx, oracle, case):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    name, n, x0, lb, ub = case
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, n), x0, BND_MPI_P + [4], which=3, lb=lb, ub=ub)
    Xo, reso, st = oracle.bfgs_bnd_mpi_findmin(oracle.rosenbrock(n), x0, lb, ub, BND_MPI_P, 4)
    assert st == 0
    assert np.array_equal(X, Xo), name
    assert res.fopt == reso.fopt


def test_bfgs_bnd_mpi_quadratic_fast_mode(ctx, oracle):
    """n = 160 > PNOL_SEQ_MAX: fused lazy rank-2 passes, and the reduced problem starts from the
    free-free block of D gathered on the device (pnol_gather_submatrix_d).  Tolerance: the
    fused pass sums in a different order than the reference's O(n^3) update, so X is compared
    with the oracle within the FD-limited basin (h = 1e-6), as for BFGS fast mode."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    n = 160
    dd, bb = oracle.quadratic_data(n)
    lb, ub = np.full(n, -0.25), np.full(n, 0.25)
    P = [1e-4, 0.1, 1e-16, 4, 1, 200, 1e-6, 1e-3, 100, 1e-9, 1e-6, 1e-9, 0, 0]
    X, res = run_bfgs(DeviceObjective(ctx, L.OBJ_QUADRATIC, n, 0, dd, bb), np.zeros(n), P + [4], which=3,
                      lb=lb, ub=ub)
    Xo, reso, st = oracle.bfgs_bnd_mpi_findmin(oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb), np.zeros(n), lb, ub,
                                               P, 4)
    assert st == 0
    assert np.all(X >= lb) and np.all(X <= ub)
    assert res.fopt <= res.f0
    assert np.max(np.abs(X - Xo)) <= 2e-4, np.max(np.abs(X - Xo))
    assert abs(res.fopt - reso.fopt) <= 1e-6 * abs(reso.fopt)


SW_P = [1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1]   # Examples.cpp:37


@pytest.mark.parametrize("procs", [1, 2, 3, 4, 8])
def test_bfgs_bnd_mpi_sw_matches_oracle(ctx, oracle, procs):
    """BFGS_Bnd_MPI_SW (testBFGSBndMPISW, Examples.cpp:12-45) with the pools of a procs-rank run
    (procs + 1 bracketing, procs + 2 zoom) equals the reference at np = procs: X, fOpt, evals.
    At np = 1 the search is degenerate (it stops at x0 after two steps)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    x0, lb, ub = [-1.0, 2.0, 2.0], [-1.0] * 3, [5.0] * 3
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 3), x0, SW_P + [procs], which=4, lb=lb, ub=ub)
    Xo, reso = oracle.bfgs_bnd_mpi_sw_findmin(oracle.rosenbrock(3), x0, lb, ub, SW_P, procs)
    assert np.array_equal(X, Xo), (procs, X, Xo)
    assert res.fopt == reso.fopt and res.evals == reso.evals
    if procs > 1:
        np.testing.assert_allclose(X, 1.0, atol=1e-3)


@pytest.mark.parametrize("case", [
    ("testBFGSBnd-geometry", 5, [2.0] * 5, [-5.0] * 5, [5.0] * 5),
    ("upper-active", 3, [0.0, 0.0, 0.0], [-2.0] * 3, [0.5] * 3),
    ("testBFGSBnd_MPI-geometry", 10, [-0.5, 3.0] + [3.0] * 8, [-1.0] + [-5.0] * 9, [5.0] * 10),
])
def test_bfgs_bnd_mpi_sw_box_cases(ctx, oracle, case):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    name, n, x0, lb, ub = case
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, n), x0, SW_P + [4], which=4, lb=lb, ub=ub)
    Xo, reso = oracle.bfgs_bnd_mpi_sw_findmin(oracle.rosenbrock(n), x0, lb, ub, SW_P, 4)
    assert np.array_equal(X, Xo), name
    assert res.fopt == reso.fopt


@pytest.mark.parametrize("case", [
    # test_bfgs_bnd_matches_oracle's multi-freeze geometries: several coordinates freeze at
    # interior positions at once, so the in-place compaction of the reduced vectors is exercised
    ("alternating", 12, [0.2, -0.2] * 6, [-0.3] * 12, [0.6] * 12),
    ("upper-ramp", 16, list(np.linspace(-0.9, 0.9, 16)), [-1.0] * 16, [0.35] * 16),
    ("interior-lower", 9, [1.5] * 9, [0.2, 1.2, 0.2, 1.3, 0.2, 1.1, 0.2, 1.4, 0.2], [2.0] * 9),
])
def test_bfgs_bnd_mpi_sw_multi_freeze_matches_oracle(ctx, oracle, case):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    name, n, x0, lb, ub = case
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, n), x0, SW_P + [4], which=4, lb=lb, ub=ub)
    Xo, reso = oracle.bfgs_bnd_mpi_sw_findmin(oracle.rosenbrock(n), x0, lb, ub, SW_P, 4)
    print(f"{name}: fopt {res.fopt!r} vs {reso.fopt!r}, evals {res.evals} vs {reso.evals}")
    assert np.array_equal(X, Xo), name
    assert res.fopt == reso.fopt and res.evals == reso.evals


# ---- the drop-in classes driven from C++ (tests/cpp/bfgs_family_cxx.cpp) -------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["BFGS", "BFGS_MPI", "BFGSBnd_MPI", "BFGS_Bnd", "BFGS_Bnd_MPI_SW"]


@pytest.fixture(scope="module")
def family_exe(tmp_path_factory):
    import subprocess
    pkg = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")
    exe = str(tmp_path_factory.mktemp("bfgs_family") / "bfgs_family_cxx")
    subprocess.run(["g++", "-O2", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "bfgs_family_cxx.cpp"), "-L", pkg, "-lpnol_amd", "-pthread",
                    f"-Wl,-rpath,{pkg}", "-o", exe], check=True)
    return exe


def test_bfgs_family_scaling_and_grad_vectors(family_exe):
    """setinitialScalingVec / setGradVec of BFGS_Bnd and BFGS_Bnd_MPI_SW (the C drivers do not reach
    them; the oracle has no scaling vector).  A scaling of all 1.0 with a dXGradVec of all dXGrad
    is bitwise the run with neither set; the alternating pair is bitwise the run recorded from
    this program (--record) on the commit before the family shared its code
    (tests/golden/bfgs_family_parent.json)."""
    import subprocess
    r = subprocess.run([family_exe, "scaling"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("R "):
            _, cls, variant, evals, f0, fopt, *x = ln.split()
            rows[cls, variant] = {"evals": int(evals), "f0": f0, "fOpt": fopt, "X": x}
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "bfgs_family_parent.json")))
    for cls, n in (("BFGS_Bnd", 12), ("BFGS_Bnd_MPI_SW", 10)):
        assert len(rows[cls, "none"]["X"]) == n
        assert rows[cls, "unit"] == rows[cls, "none"], cls
        assert rows[cls, "pair"] == gold[cls], cls
        assert rows[cls, "pair"] != rows[cls, "none"], cls   # the pair does change the run


# each class at its loudest verbosity, and the two bounded classes at the levels where their
# thresholds differ (the step line: BFGS_Bnd above 1, the pooled class above 0; the lines after a
# recursion: above 0 / above 1; the boundary announcement: any non-zero level / above 0)
FAMILY_TEXT = [(cls, None) for cls in FAMILY] + [("BFGS_Bnd", 1), ("BFGS_Bnd", -1), ("BFGS_Bnd_MPI_SW", 1),
                                                 ("BFGS_Bnd_MPI_SW", 2)]


@pytest.mark.parametrize("cls,level", FAMILY_TEXT)
def test_bfgs_family_printed_text(family_exe, cls, level):
    """Each class on Rosenbrock n = 3 ("lower-active", maxIter 6): stdout byte for byte the text
    recorded on the commit before the family shared its code."""
    import subprocess
    r = subprocess.run([family_exe, "text", cls] + ([] if level is None else [str(level)]), capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    name = f"bfgs_family_stdout_{cls}" + ("" if level is None else f"_v{level}") + ".txt"
    gold = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
    assert len(gold) > (200 if level is None else 50)
    assert r.stdout == gold


def test_gather_submatrix(ctx):
    """pnol_gather_submatrix_d: D[idx][idx] bitwise (BFGS_with_bnd_linsearch_MPI.cpp:832-840)."""
    import torch
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    rng = np.random.default_rng(5)
    for n, k in ((7, 3), (300, 211), (1000, 999)):
        D = rng.standard_normal((n, n))
        idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
        dD = ctx.tensor(D)
        di = torch.from_numpy(idx).to(dD.device)
        out = ctx.empty(k, k)
        L.check(L.lib().pnol_gather_submatrix_d(ctx.h, dD.data_ptr(), n, n, di.data_ptr(), k, out.data_ptr(), k),
                "gather")
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), D[np.ix_(idx, idx)])


@pytest.mark.parametrize("n", [200, 1000])
def test_bfgs_quadratic_fast_mode(ctx, oracle, n):
    """n > PNOL_SEQ_MAX: fused lazy rank-2 passes; converges to the quadratic's minimiser and
    stays within the stated trajectory tolerance of the reference-form oracle."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    dd, bb = oracle.quadratic_data(n)
    P = [1e-4, 0.9, 1e-6, 1, 1000, 1e-6, 1e-3, 200, 1e-9, 1e-6, 0, 0]
    X, res = run_bfgs(DeviceObjective(ctx, L.OBJ_QUADRATIC, n, 0, dd, bb), np.zeros(n), P)
    H = np.diag(dd) + 0.25 * (np.eye(n, k=1) + np.eye(n, k=-1))
    xstar = np.linalg.solve(H, bb)
    # forward differences with h = 1e-6 bias the stationary point by O(h max d_i) ~ 1e-6
    assert rel(X, xstar) <= 2e-4
    Xo, reso, _ = oracle.bfgs_findmin(oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb), np.zeros(n), P)
    # Trajectory tolerance: the fused pass sums H.g in a different order than the reference's
    # O(n^3) update, so the two runs stop at different points inside the FD-limited basin
    # (gtol 1e-6 with h = 1e-6); both sit within O(h) of x*.  Measured 3.9e-5 at n = 1000.
    print(f"n={n}: |X - X_oracle| / |X_oracle| = {rel(X, Xo):.3e}, iterations {res.iters} vs {reso.iters}, "
          f"F {res.fopt!r} vs {reso.fopt!r}")
    assert rel(X, Xo) <= 2e-4


# cfg 2 (BFGS_with_linesearch.cpp:71-114 at n = 4096) against the oracle's rank-2 run, measured on
# MI355X (tools/cfg2_traj_probe.py, profiles/r04_cfg2_traj.json): max |X - Xo| / max |Xo| after
# maxIter iterations, and the evaluation counts (equal through iteration 8).  Iteration 1 starts
# from D = I, whose products are exact, so X is bitwise; from iteration 2 on the fused pass's
# H.g (row-tile partials) and the oracle's sequential matrixVectorMultiply differ in the last
# place, and the FD gradient (h = 1e-6) amplifies that by ~1/h per iteration.
CFG2_TRAJ = {1: 0.0, 2: 2.13e-10, 3: 5.47e-8}
CFG2_WHOLE_REL = 3.18e-5


@pytest.mark.parametrize("max_iter", sorted(CFG2_TRAJ))
def test_bfgs_cfg2_trajectory(ctx, oracle, max_iter):
    """cfg 2's first iterations: X after maxIter = 1, 2, 3 iterations within 2x the measured
    distance to the oracle's rank-2 run (bitwise after the first), the same evaluation counts."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    n = 4096
    dd, bb = oracle.quadratic_data(n)
    P = [1e-4, 0.9, 1e-6, 1, 1000, 1e-6, 1e-3, max_iter, 1e-9, 1e-6, 0, 0]
    prof = {}
    X, res = run_bfgs(DeviceObjective(ctx, L.OBJ_QUADRATIC, n, 0, dd, bb), np.zeros(n), P, profile=prof)
    Xo, reso, _ = oracle.bfgs_findmin(oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb), np.zeros(n), P, rank2=True)
    d = rel(X, Xo)
    print(f"maxIter={max_iter}: rel {d:.3e}, evals {res.evals} vs {reso.evals}")
    assert int(prof["iterations"]) == reso.iters == max_iter
    assert res.evals == reso.evals
    if CFG2_TRAJ[max_iter] == 0.0:
        assert np.array_equal(X, Xo) and res.fopt == reso.fopt
    else:
        assert d <= 2 * CFG2_TRAJ[max_iter]


def test_bfgs_cfg2_whole_solve(ctx, oracle):
    """cfg 2 to convergence: X within 2x the measured 3.18e-5 of the oracle's rank-2 run, the
    iteration count within one (measured 14 vs 15: the device run meets gtol one iteration
    earlier inside the FD-limited basin, at an F 4.3e-8 lower than the oracle's), and the
    evaluation count within one iteration's worth (an FD gradient of n + 1 points plus its line
    search)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    n = 4096
    dd, bb = oracle.quadratic_data(n)
    P = [1e-4, 0.9, 1e-6, 1, 1000, 1e-6, 1e-3, 200, 1e-9, 1e-6, 0, 0]
    prof = {}
    X, res = run_bfgs(DeviceObjective(ctx, L.OBJ_QUADRATIC, n, 0, dd, bb), np.zeros(n), P, profile=prof)
    Xo, reso, _ = oracle.bfgs_findmin(oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb), np.zeros(n), P, rank2=True)
    it = int(prof["iterations"])
    print(f"cfg 2: rel {rel(X, Xo):.3e}, iterations {it} vs {reso.iters}, evals {res.evals} vs {reso.evals}, "
          f"F {res.fopt!r} vs {reso.fopt!r}")
    assert rel(X, Xo) <= 2 * CFG2_WHOLE_REL
    assert abs(it - reso.iters) <= 1
    assert abs(res.evals - reso.evals) <= (n + 1) + 200
    assert abs(res.fopt - reso.fopt) <= 1e-9 * abs(reso.fopt)


# ---- config 5: BFGS_Bnd on the bounded quadratic (SURVEY 8(d) cfg 5) ----------------------
CFG5_P = [1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1]   # testBFGSBnd, Examples.cpp:75


def _box_qp_solution(d, b, lb, ub, sweeps=400):
    """The exact minimiser of the cfg-5 quadratic over the box: f = sum 0.5 d x^2 - b x +
    0.25 x_i x_{i+1} has the tridiagonal, strictly diagonally dominant Hessian diag(d) +
    0.25 (off-diagonals), so projected red-black Gauss-Seidel converges linearly (factor
    <= 0.5 / min d = 0.5 per sweep) to the unique KKT point."""
    n = len(d)
    x = np.zeros(n)
    for _ in range(sweeps):
        for par in (0, 1):
            i = np.arange(par, n, 2)
            nb = np.zeros(len(i))
            nb += np.where(i + 1 < n, x[np.minimum(i + 1, n - 1)], 0.0)
            nb += np.where(i - 1 >= 0, x[np.maximum(i - 1, 0)], 0.0)
            x[i] = np.clip((b[i] - 0.25 * nb) / d[i], lb[i], ub[i])
    return x


def _quad_grad(d, b, x):
    return d * x - b + 0.25 * (np.r_[x[1:], 0.0] + np.r_[0.0, x[:-1]])


@pytest.mark.parametrize("n", [200, 500, 1000, 2048])
def test_bfgs_bnd_fast_mode_cfg5_matches_oracle(ctx, oracle, n):
    """Serial BFGS_Bnd in fast mode (n > PNOL_SEQ_MAX: lazy rank-2 passes, the diagonal-D
    shortcuts, one borrowed device buffer for the whole active-set recursion) on the cfg-5
    quadratic (b x 4, box [-0.5, 0.5]^n, x0 = 0, testBFGSBnd params): about 70% of the
    coordinates end on a bound, each frozen by boundaryAssessment one level deeper.  Checked
    against the oracle's BFGS_Bnd with the rank-2 update form (the O(n^3) form agrees with it
    to 6e-17 at n = 200 / 300, tests/test_oracle_golden.py).  The device pass sums in another
    order, so the last reduced problem stops at a slightly different point inside the gradient
    tolerance (minGrad2Norm 1e-5 with FD steps of 1e-6): X is compared within 2e-6 (absolute,
    |X| <= 0.5; measured 4.3e-7 at n = 500), F within 1e-10 relative, the active set exactly,
    the iteration and evaluation counts within 5% (the recursion path is the same).  n = 2048:
    1385 recursion levels; the oracle's run takes ~1.5 min of one host core."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    dd, bb = oracle.quadratic_data(n, bscale=4.0)
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    X, res, tr = run_bfgs(DeviceObjective(ctx, L.OBJ_QUADRATIC, n, 0, dd, bb), np.zeros(n), CFG5_P, which=2,
                          lb=lb, ub=ub, trace_cap=100000)
    Xo, reso, tro, depth = oracle.bfgs_bnd_findmin_ex(oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb), np.zeros(n),
                                                      lb, ub, CFG5_P, rank2=True, trace_cap=100000)
    assert depth > n // 2                      # the recursion really is one level per bound
    assert np.all(X >= lb) and np.all(X <= ub)
    act = lambda x: (np.abs(x - lb) < 1e-5).astype(int) - (np.abs(x - ub) < 1e-5).astype(int)
    assert np.array_equal(act(X), act(Xo))
    info = (np.max(np.abs(X - Xo)), res.fopt, reso.fopt, res.iters, reso.iters, res.evals, reso.evals)
    assert np.max(np.abs(X - Xo)) <= 2e-6, info
    assert abs(res.fopt - reso.fopt) <= 1e-10 * abs(reso.fopt), info
    assert abs(res.iters - reso.iters) <= 0.05 * reso.iters and abs(res.evals - reso.evals) <= 0.05 * reso.evals, info
    assert len(tr) == res.iters and np.all(np.diff(tr) <= 0)
    xs = _box_qp_solution(dd, bb, lb, ub)
    assert np.max(np.abs(X - xs)) <= 1e-4


def test_bfgs_bnd_cfg5_full_size_properties(ctx):
    """Config 5 at full size, n = 16384 (D = 2.15 GB on the device): the bounded quadratic with
    data generated in HBM.  The oracle's update is O(n^2) per iteration over ~11k recursion
    levels (hours on a CPU), so the run is checked by properties: every iterate inside the box,
    F non-increasing along the trace, and X the box-constrained minimiser (the KKT point from
    projected Gauss-Seidel on the exact tridiagonal Hessian) to within the FD gradient's
    resolution (h = 1e-6, minGrad2Norm = 1e-5)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    import oracle as O
    n = 16384
    obj = DeviceObjective.synthetic(ctx, L.OBJ_QUADRATIC, n, 0, bscale=4.0)
    dd, bb = O.quadratic_data(n, bscale=4.0)        # the same splitmix64 stream (bitwise)
    lb, ub = np.full(n, -0.5), np.full(n, 0.5)
    X, res, tr = run_bfgs(obj, np.zeros(n), CFG5_P, which=2, lb=lb, ub=ub, trace_cap=1 << 20)
    assert np.all(X >= lb) and np.all(X <= ub)
    assert res.f0 == 0.0 and res.fopt < res.f0
    assert len(tr) == res.iters and np.all(np.diff(tr) <= 0) and tr[-1] == res.fopt
    xs = _box_qp_solution(dd, bb, lb, ub)
    g = _quad_grad(dd, bb, X)
    free = (X > lb + 1e-5) & (X < ub - 1e-5)
    # measured (profiles/r04_bench.json, bfgs_bnd_cfg5_solve): max |X - x*| = 9.99e-6; the bound is
    # 2x that, and the free gradient 4 (the largest diagonal entry) times it plus the FD step
    assert np.max(np.abs(g[free])) <= 1e-4, np.max(np.abs(g[free]))
    assert np.max(np.abs(X - xs)) <= 2e-5, np.max(np.abs(X - xs))
    act = lambda x: (np.abs(x - lb) < 1e-5).astype(int) - (np.abs(x - ub) < 1e-5).astype(int)
    assert np.mean(act(X) != act(xs)) <= 1e-3


def test_trial_points_on_device_bitwise(ctx, oracle, monkeypatch):
    """The line searches hand their trial points to objEvalBatch; PNOL_DEVICE_POINTS=1 makes
    the driver objective evaluate every batch on the device (pnol_dobj_eval_batch: one
    workgroup per point, the terms summed in index order).  The trajectories stay bitwise:
    BFGS on 2-D Rosenbrock vs the recorded reference output, BFGS_MPI pools and BFGS_Bnd
    (recursion, Recur scatter) vs the oracle."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    monkeypatch.setenv("PNOL_DEVICE_POINTS", "1")
    g = GOLD["bfgs_rosenbrock2_m12_1"]
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 2), g["x0"], g["params"])
    assert X.tolist() == g["X"] and res.fopt == g["f"] and res.evals == g["evals"]
    P = [1e-4, 0.1, 4, 1, 1000, 1e-7, 1e-3, 200, 1e-5, 1e-5, 0, 0]
    Xo, _ = oracle.bfgs_mpi_findmin(oracle.rosenbrock(10), [10.0] * 10, P, 4)
    X4, _ = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 10), [10.0] * 10, P + [4], which=1)
    assert np.array_equal(X4, Xo)
    Pb = [1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1]
    x0, lb, ub = [0.0, 0.0, 0.0], [-2.0] * 3, [0.5] * 3
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, 3), x0, Pb, which=2, lb=lb, ub=ub)
    Xo, reso = oracle.bfgs_bnd_findmin(oracle.rosenbrock(3), x0, lb, ub, Pb)
    assert np.array_equal(X, Xo) and res.evals == reso.evals


def test_eval_batch_abi_bitwise(ctx, oracle):
    """pnol_dobj_eval_batch on scalar kinds vs the oracle's objEval, point by point (n up to
    5000 crosses the kernel's 2048-term LDS chunks)."""
    import ctypes as C
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    rng = np.random.default_rng(3)
    for kind, n, o in [(L.OBJ_ROSENBROCK, 7, oracle.rosenbrock(7)), (L.OBJ_ROSENBROCK, 5000, oracle.rosenbrock(5000)),
                       (L.OBJ_QUADRATIC, 4097, oracle.quadratic(4097)), (L.OBJ_POWER, 300, oracle.power(300, 2))]:
        d = _obj(ctx, kind, n, 0, o.p0, o.p1, 2.0)
        Xs = np.ascontiguousarray(rng.uniform(-2, 2, (5, n)))
        f = np.zeros(5)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().pnol_dobj_eval_batch(ctx.h, d.h, Xs.ctypes.data_as(dp), 5, f.ctypes.data_as(dp)), "batch")
        assert f.tolist() == [oracle.obj_eval(o, x) for x in Xs], (kind, n)


@pytest.mark.parametrize("m,n", [(600, 100), (3000, 257)])
def test_lm_one_wait_loop_lu_fallback_equals_general_loop(ctx, oracle, m, n, monkeypatch):
    """The one-wait LM loop's fallback when the Cholesky reports a non-positive pivot (the
    solve status packed after sigma and F(x + sigma) in the pinned trip buffer -> redo the trip
    with the reference-order LU, levmarq.cpp redo_lu): forced on every trip by a test hook, the
    trajectory (X, F0, FOpt, evaluation count) is bitwise the general loop's, whose
    pnol_solve_d falls back to the same LU, and stays within 1e-10 of the oracle (whose
    luSolve is that LU)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    A, xs, y = oracle.linres_data(m, n)
    params = (0.001, 10, 1e-7, 8, 0.0, -1)
    monkeypatch.setenv("PNOL_CHOL_FORCE_FALLBACK", "1")
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PNOL_LM_ASYNC", mode)
        out[mode] = run_levmarq(_obj(ctx, L.OBJ_LINRES, n, m, A, y), np.zeros(n), params)
    (Xa, F0a, FOa, ra), (Xs, F0s, FOs, rs) = out["1"], out["0"]
    assert np.array_equal(Xa, Xs) and np.array_equal(F0a, F0s) and np.array_equal(FOa, FOs)
    assert ra.evals == rs.evals
    Xo, *_ = oracle.lm_findmin(oracle.Obj(oracle.LINRES, n, m, A, y), np.zeros(n), params)
    assert rel(Xa, Xo) <= 1e-10


@pytest.mark.parametrize("m,n,force,reduce", [(3000, 257, "0", "launch"), (2000, 700, "0", "launch"),
                                              (3000, 257, "1", "launch"), (2000, 700, "0", "tasks"),
                                              (3000, 257, "1", "tasks"), (2000, 700, "0", "tail"),
                                              (3000, 257, "1", "tail")])
def test_lm_fused_trip_loop_equals_general_loop(ctx, oracle, m, n, force, reduce, monkeypatch):
    """The one-wait LM loop with the fused trip (pnol_lm_trip_d, the default; its reduce as a
    launch into the Cholesky's matrix, or as the persistent launch's first tasks) replays the
    one-wait loop with the two calls (PNOL_LM_TRIP=0) and the general loop (PNOL_LM_ASYNC=0)
    bitwise -- X, F0, FOpt, evaluation count -- also with the LU fallback forced on every trip
    (force = 1: A formed from the trip's partials, pnol_lm_trip_normal_d); the fused trip's results
    reach the host alike written into the pinned block by its kernels (the default) or copied
    (PNOL_LM_ZEROCOPY=0), and with each next Jacobian queued behind a gate before the host's
    decision (the default) or after it (PNOL_LM_GATE=0)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    A, xs, y = oracle.linres_data(m, n)
    params = (0.001, 10, 1e-7, 8, 0.0, -1)
    monkeypatch.setenv("PNOL_CHOL_FORCE_FALLBACK", force)
    monkeypatch.setenv("PNOL_LM_REDUCE", reduce)
    out = {}
    for name, mode, trip, zc, gate in (("fused", "1", "1", "1", "1"), ("fused_nogate", "1", "1", "1", "0"),
                                       ("fused_copy", "1", "1", "0", "1"), ("two_call", "1", "0", "1", "1"),
                                       ("general", "0", "0", "1", "1")):
        monkeypatch.setenv("PNOL_LM_ASYNC", mode)
        monkeypatch.setenv("PNOL_LM_TRIP", trip)
        monkeypatch.setenv("PNOL_LM_ZEROCOPY", zc)
        monkeypatch.setenv("PNOL_LM_GATE", gate)
        out[name] = run_levmarq(_obj(ctx, L.OBJ_LINRES, n, m, A, y), np.zeros(n), params)
    for a, b in (("fused", "fused_nogate"), ("fused", "fused_copy"), ("fused", "two_call"), ("two_call", "general")):
        (Xa, F0a, FOa, ra), (Xs, F0s, FOs, rs) = out[a], out[b]
        assert np.array_equal(Xa, Xs), (a, b, rel(Xa, Xs))
        assert np.array_equal(F0a, F0s) and np.array_equal(FOa, FOs), (a, b)
        assert ra.evals == rs.evals, (a, b)
    assert rel(out["fused"][0], xs) <= 1e-8


def test_lm_gate_timeout_repeats_the_trip(ctx, oracle, monkeypatch, capfd):
    """A queued Jacobian's gate that gives up before the host decides (PNOL_LM_GATE_CAP=0: at
    once) makes that Jacobian launch return; the host sees it in the gate's report and runs the
    trip again whole -- the same X, F and evaluation count as without the gate."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    m, n = 3000, 257
    A, xs, y = oracle.linres_data(m, n)
    params = (0.001, 10, 1e-7, 6, 0.0, -1)
    out = {}
    for name, gate, cap in (("nogate", "0", None), ("gave_up", "1", "0")):
        monkeypatch.setenv("PNOL_LM_GATE", gate)
        if cap is None:
            monkeypatch.delenv("PNOL_LM_GATE_CAP", raising=False)
        else:
            monkeypatch.setenv("PNOL_LM_GATE_CAP", cap)
        out[name] = run_levmarq(_obj(ctx, L.OBJ_LINRES, n, m, A, y), np.zeros(n), params)
    err = capfd.readouterr().err
    assert "gate timed out" in err
    (Xa, F0a, FOa, ra), (Xb, F0b, FOb, rb) = out["nogate"], out["gave_up"]
    assert np.array_equal(Xa, Xb) and np.array_equal(F0a, F0b) and np.array_equal(FOa, FOb)
    assert ra.evals == rb.evals


@pytest.mark.parametrize("m,n,trip", [(3000, 257, "1"), (2000, 700, "1"), (2000, 700, "0")])
def test_lm_timed_out_trip_relaunches_cholesky(ctx, oracle, m, n, trip, monkeypatch, capfd):
    """A trip whose Cholesky reports a dependency wait past its spin cap (forced on every trip's
    reducing solve by PNOL_CHOL_FORCE_FALLBACK=-7) is a scheduling event, not a property of A: the
    loop redoes the trip's solve with the same Cholesky (never the LU; the relaunch is not forced)
    and reports it, so the trajectory -- X, F0, FOpt, evaluation count -- is bitwise the unforced
    run's.  (The reference's luSolve, LevenbergMarquardt.cpp:83, has no timing-dependent branch.)"""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq
    A, xs, y = oracle.linres_data(m, n)
    params = (0.001, 10, 1e-7, 6, 0.0, -1)
    monkeypatch.setenv("PNOL_LM_TRIP", trip)   # the fused trip (the default) or the two calls
    monkeypatch.setenv("PNOL_CHOL_FORCE_FALLBACK", "-7")
    Xt, F0t, FOt, rt = run_levmarq(_obj(ctx, L.OBJ_LINRES, n, m, A, y), np.zeros(n), params)
    err = capfd.readouterr().err
    assert err.count("Cholesky relaunched") == 6, err[-2000:]
    monkeypatch.delenv("PNOL_CHOL_FORCE_FALLBACK")
    X, F0, FO, r = run_levmarq(_obj(ctx, L.OBJ_LINRES, n, m, A, y), np.zeros(n), params)
    assert np.array_equal(Xt, X) and np.array_equal(F0t, F0) and np.array_equal(FOt, FO)
    assert rt.evals == r.evals


@pytest.mark.parametrize("n", [1, 7, 100, 300])
def test_matrix_inverse_bitwise(ctx, oracle, n):
    """pnol_matrix_inverse_d (one elimination of [B | I], per-column back substitution) equals
    the reference's matrixInverse -- luSolve per unit column -- bit for bit, row swaps included."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import _ptr
    import ctypes as C
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n)) + (0.5 * n) * np.eye(n)[::-1]   # anti-diagonal weight: pivots swap rows
    dB, out = ctx.tensor(B), ctx.empty(n, n)
    info = C.c_int(7)
    L.check(L.lib().pnol_matrix_inverse_d(ctx.h, _ptr(dB), n, n, _ptr(out), n, C.byref(info)), "matrix_inverse")
    assert info.value == 0
    assert np.array_equal(out.cpu().numpy(), oracle.matinv(B))


@pytest.mark.parametrize("n,x0", [(2, [-1.2, 1.0]), (5, [3.0] * 5), (10, [0.5] * 10)])
def test_bfgs_init_hess_fd_matches_oracle(ctx, oracle, n, x0):
    """BFGS with initHessFD (BFGS_with_linesearch.cpp:34-41): D0 = matrixInverse of the FD
    Hessian (hessianApproximation's points batched on the host, the inverse on the device);
    exact mode (n <= PNOL_SEQ_MAX), so X, fOpt and the evaluation count equal the oracle's."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs
    P = [1e-4, 0.9, 1e-6, 1, 1000, 1e-7, 1e-3, 100, 1e-5, 1e-5, 1, 0]
    X, res = run_bfgs(_obj(ctx, L.OBJ_ROSENBROCK, n), x0, P)
    Xo, reso, _ = oracle.bfgs_findmin(oracle.rosenbrock(n), x0, P)
    assert np.array_equal(X, Xo) and res.fopt == reso.fopt
    # the oracle's count starts after initHessFD; the objective's counter (ours) includes the
    # FD Hessian's 1 + 3 n (n + 1) / 2 evaluations, as the reference objective's does
    assert res.evals == reso.evals + 1 + 3 * n * (n + 1) // 2


def test_bfgs_init_hess_fd_fast_mode_quadratic(ctx, oracle):
    """initHessFD in fast mode (n = 300): the quadratic's FD Hessian is its tridiagonal Hessian
    to O(h), so D0 ~ H^{-1} and BFGS converges in a few iterations; trajectory tolerance vs the
    oracle as for the other fast-mode runs."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_bfgs
    n = 300
    dd, bb = oracle.quadratic_data(n)
    P = [1e-4, 0.9, 1e-6, 1, 1000, 1e-6, 1e-3, 50, 1e-9, 1e-6, 1, 0]
    prof = {}
    X, res = run_bfgs(DeviceObjective(ctx, L.OBJ_QUADRATIC, n, 0, dd, bb), np.zeros(n), P, profile=prof)
    Xo, reso, _ = oracle.bfgs_findmin(oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb), np.zeros(n), P)
    H = np.diag(dd) + 0.25 * (np.eye(n, k=1) + np.eye(n, k=-1))
    assert rel(X, np.linalg.solve(H, bb)) <= 2e-4
    assert rel(X, Xo) <= 2e-4
    assert prof["iterations"] <= 10


def _run_user_levmarq(tmp_path, A, y, x0, params, threads):
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "user_levmarq")
    if not os.path.exists(exe):   # normally built by __graft_entry__.build()
        subprocess.run(["make", "-s", "-C", os.path.join(root, "examples")], check=True, timeout=120)
    m, n = A.shape
    fin, fout = str(tmp_path / f"in{threads}.bin"), str(tmp_path / f"out{threads}.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", m, n, threads))
        f.write(np.asarray(params, dtype=np.float64).tobytes())
        for a in (A, y, x0):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    raw = open(fout, "rb").read()
    X = np.frombuffer(raw[:8 * n], dtype=np.float64)
    c0, c1 = np.frombuffer(raw[8 * n:8 * n + 16], dtype=np.float64)
    evals, batches = np.frombuffer(raw[8 * n + 16:], dtype=np.int64)
    return X, c0, c1, int(evals), int(batches)


@pytest.mark.parametrize("m,n", [(600, 100), (3000, 257)])
def test_user_program_own_multiobjective_levmarq(ctx, oracle, tmp_path, m, n):
    """A C++ user program (examples/user_levmarq.cpp, INTEGRATION.md's g++ build line) with its
    OWN MultiObjective (not a built-in: n > PNOL_SEQ_MAX, evaluated on the host through its
    objEvalBatch override, which spreads each batch over host threads) runs LevMarq with the
    J^T J / solve on the GPU.  Converged X within 1e-10 of the oracle's LevMarq; the thread
    count does not change a bit; every Jacobian's points arrived as batches."""
    A, xs, y = oracle.linres_data(m, n)
    params = (0.001, 10, 1e-7, 6, 0.0)
    X1, c01, c11, ev1, b1 = _run_user_levmarq(tmp_path, A, y, np.zeros(n), params, 1)
    X4, c04, c14, ev4, b4 = _run_user_levmarq(tmp_path, A, y, np.zeros(n), params, 4)
    assert np.array_equal(X1, X4) and c11 == c14 and ev1 == ev4
    Xo, reso, F0o, FOo, _ = oracle.lm_findmin(oracle.Obj(oracle.LINRES, n, m, A, y), np.zeros(n), params + (-1,))
    assert rel(X1, Xo) <= 1e-10
    assert rel(X1, xs) <= 1e-8
    assert ev1 == reso.evals, (ev1, reso.evals)
    assert b1 >= 6   # one batch (or more) of FD points per Jacobian, plus the trial points


GA_P = [40, 200, 0.1, 0.3, 0.2, 0.5, 0.01, 0.5, 20, 0]   # setGAParams without graph


@pytest.mark.parametrize("which,host_eval", [(0, False), (1, False), (0, True)])
def test_ga_matches_oracle(ctx, oracle, which, host_eval):
    """GeneticAlgorithm (0) / GeneticAlgorithmMPI on one rank (1) equal the restatement bitwise --
    X, f0, fOpt, generations, evaluations -- with every generation's population evaluated as
    one device batch (host_eval: through objEvalBatch on the host formula, the same bits).
    Rosenbrock n = 4 in [-2, 2]^4 and the cfg-2 quadratic at n = 100 (row f4)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_ga
    for kind, n, seed in ((L.OBJ_ROSENBROCK, 4, 12345), (L.OBJ_QUADRATIC, 100, 7)):
        lb, ub = np.full(n, -2.0), np.full(n, 2.0)
        x0 = np.full(n, -1.0)
        if kind == L.OBJ_ROSENBROCK:
            dobj, oobj = DeviceObjective(ctx, kind, n), oracle.rosenbrock(n)
        else:
            dd, bb = oracle.quadratic_data(n)
            dobj, oobj = DeviceObjective(ctx, kind, n, 0, dd, bb), oracle.Obj(oracle.QUADRATIC, n, 0, dd, bb)
        X, res = run_ga(dobj, x0, lb, ub, GA_P, seed, which=which, host_eval=host_eval)
        Xo, reso, st = oracle.ga_findmin(oobj, x0, lb, ub, GA_P[:9], seed, 0)
        assert st == 0
        assert np.array_equal(X, Xo), (kind, np.max(np.abs(X - Xo)))
        assert res.f0 == reso.f0 and res.fopt == reso.fopt, kind
        assert res.iters == reso.iters and res.evals == reso.evals, (kind, res.iters, reso.iters, res.evals, reso.evals)
        assert res.fopt < res.f0

