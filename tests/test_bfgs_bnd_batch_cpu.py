"""Batched box-bounded BFGS, the parts that need no GPU: the plain-Python restatement of
BFGS_Bnd::findMinBnd (tests/bfgs_bnd_reference.py) against the oracle bit for bit on every start
the restatement does not flag, proof that the cases take every reachable branch of the line search
and of the active-set recursion, the properties of the flagged (corner-end) starts, the argument
checks of the two entry points (all made before any device use), and the C++11 compile check of
the header.

The oracle is never called on a flagged start: past a corner end the reference reads beyond its
reduced vectors and the C oracle can corrupt the test process.  The restatement runs first and
decides which starts are flagged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bfgs_bnd_reference as R
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _against_oracle(oracle, name, n, lb, ub, x0, p, runs):
    """Every unflagged run equals oracle.bfgs_bnd_findmin_ex bitwise; returns how many were compared."""
    obj = R.oracle_obj(oracle, name, n)
    lo, hi = np.full(n, lb), np.full(n, ub)
    compared = 0
    for s, r in enumerate(runs):
        if r.flagged:
            continue
        X, res, _, depth = oracle.bfgs_bnd_findmin_ex(obj, x0[s], lo, hi, p)
        assert _bits(X) == _bits(r.X), s
        assert _bits(np.float64(res.f0)) == _bits(np.float64(r.f0)), s
        assert _bits(np.float64(res.fopt)) == _bits(np.float64(r.fopt)), s
        assert (res.iters, res.evals, depth) == (r.iters, r.evals, r.depth), s
        compared += 1
    return compared


# ---- 1. the restatement against the oracle -------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F", "G"])
def test_restatement_bitwise_against_oracle(oracle, case):
    """X, f0, fOpt, iterations, evaluations and depth of every unflagged start are
    oracle.bfgs_bnd_findmin_ex's.  Only case C has flagged starts (48 of 130 measured; at least 80
    must be unflagged)."""
    name, n, lb, ub, nstart, p = R.CASES[case]
    runs = R.case_runs(oracle, case)
    compared = _against_oracle(oracle, name, n, lb, ub, R.case_x0(case), p, runs)
    if case == "C":
        assert compared >= 80
    else:
        assert compared == nstart
    if case == "B":
        assert min(r.depth for r in runs) >= 2 and max(r.depth for r in runs) >= 5
    if case == "E":
        assert all(200 <= r.iters <= 202 for r in runs)
    if case == "F":
        assert all(r.depth == 0 for r in runs)
    if case == "G":
        assert all(r.iters == 0 and r.evals == 3 + 2 for r in runs)


def test_out_of_box_starts(oracle):
    """checkBoxBounds puts a coordinate outside the box by more than |bound| / 1000 on the midpoint."""
    name, n, lb, ub, _, p = R.CASES["A"]
    runs = R.batch(oracle, name, n, lb, ub, R.OUT_OF_BOX, p)
    assert _against_oracle(oracle, name, n, lb, ub, R.OUT_OF_BOX, p, runs) == len(R.OUT_OF_BOX)
    mid = (lb + ub) / 2.0
    fn = R.oracle_fn(oracle, R.oracle_obj(oracle, name, n))
    for x0, r in zip(R.OUT_OF_BOX, runs):
        moved = np.where((x0 < lb) | (x0 > ub), mid, x0)
        assert not np.array_equal(moved, x0)
        assert r.f0 == fn(moved)
        assert np.all(r.X >= lb - p[7]) and np.all(r.X <= ub + p[7])


# ---- 2. branch coverage --------------------------------------------------------------------
# The two counters no input of these tests reaches, and why:
#   exhausted_previous  the exhausted outer search returns the previous point when
#                       phi(aim1) < phi(ai), but every trip that goes on to double ends with
#                       (aim1, pim1) <- (ai, phii), so pim1 == phii when the loop runs out (and with
#                       maxIterLineSearch = 0 the test is phi0 < 0 against phii = 0 on an objective
#                       that is a sum of squares): unreachable.
#   exhausted_zero      needs phi0 < phi(ai) at the last trip although Armijo held there,
#                       phi(ai) <= phi0 + c1 ai dphi0: only with dphi0 > 0, an ascent direction, and
#                       every trip must also have measured a negative slope there.  D would have to
#                       lose positive definiteness first; a search over 10240 starts (Rosenbrock
#                       n = 2, 3, 5 and the quadratic in four boxes, maxIterLineSearch 1..4,
#                       alphaGuess 1e-3..1) found none.
UNREACHED = ("exhausted_previous", "exhausted_zero")


def test_cases_take_every_branch(oracle):
    """Guards the inputs of the bitwise tests: over cases A-F every branch counter is positive
    except UNREACHED (above), and case A spreads over at least 3 depths and at least 3 distinct
    iteration counts among neighbouring starts."""
    total = dict.fromkeys(R.COUNTERS, 0)
    for case in "ABCDEF":
        for r in R.case_runs(oracle, case):
            for k, v in zip(R.COUNTERS, r.counts):
                total[k] += v
    assert all(v > 0 for k, v in total.items() if k not in UNREACHED), total
    assert all(total[k] == 0 for k in UNREACHED), total
    a = R.case_runs(oracle, "A")
    assert len(set(r.depth for r in a)) >= 3
    assert max(len(set(r.iters for r in a[s:s + 8])) for s in range(0, 130, 8)) >= 3
    d = dict(zip(R.COUNTERS, np.sum([r.counts for r in R.case_runs(oracle, "D")], axis=0).tolist()))
    assert d["zoom_exit_iter"] > 0 and d["exhausted_last"] > 0


# ---- 3. flagged starts ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["C", "corners"])
def test_flagged_starts_end_at_a_corner(oracle, case):
    name, n, lb, ub, nstart, p = R.CASES[case]
    runs = R.case_runs(oracle, case)
    flagged = [r for r in runs if r.flagged]
    if case == "corners":
        assert len(flagged) == nstart
    else:
        assert 0 < len(flagged) <= nstart - 80
    for r in flagged:
        assert np.all((np.abs(r.X - lb) < p[7]) | (np.abs(r.X - ub) < p[7]))
        assert r.fopt <= r.f0
        assert r.depth >= 1
        assert R.info_of(r) & R.CORNER
    for r in runs:
        assert bool(R.info_of(r) & R.CORNER) == r.flagged
    X, f0, fopt, iters, evals, info = R.stacked(runs)
    assert X.shape == (nstart, n) and X.dtype == f0.dtype == fopt.dtype == np.float64
    assert iters.dtype == np.int32 and evals.dtype == np.int64 and info.dtype == np.int32


# ---- 4. ABI: argument checks before any device use, the same with or without a GPU ---------
def _batch(kind, n, nstart, params=R.P, len0=None, len1=None, null=None, lb=-1.0, ub=5.0):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    ns, nn = max(nstart, 1), max(n, 1)
    X = np.full(ns * nn, 2.0)
    lo, hi = np.full(nn, lb), np.full(nn, ub)
    f0, fo = np.zeros(ns), np.zeros(ns)
    iters, evals, info = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int64), np.zeros(ns, dtype=np.int32)
    p = np.array(params, dtype=np.float64)
    d = np.ones(nn)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    args = {"p": dp(p), "lb": dp(lo), "ub": dp(hi), "X": dp(X), "f0": dp(f0), "fopt": dp(fo), "iters": ip(iters),
            "evals": evals.ctypes.data_as(C.POINTER(C.c_longlong)), "info": ip(info)}
    if null:
        args[null] = None
    return L.lib().pnol_run_bfgs_bnd_batch(kind, n, 2.0, dp(d), d.size if len0 is None else len0, dp(d),
                                           d.size if len1 is None else len1, nstart, args["p"], args["lb"],
                                           args["ub"], args["X"], args["f0"], args["fopt"], args["iters"],
                                           args["evals"], args["info"])


def test_entry_points_exist():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    for name in ("pnol_bfgs_bnd_batch_solve_d", "pnol_run_bfgs_bnd_batch"):
        assert hasattr(L.lib(), name), name
        assert name in L.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "pnol_amd.h")).read()
    assert f"#define PNOL_BFGS_BND_BATCH_NMAX {L.BFGS_BND_BATCH_NMAX}" in hdr
    assert L.BFGS_BND_BATCH_NMAX >= 8
    assert f"#define PNOL_BFGS_BND_BATCH_CORNER {L.BFGS_BND_BATCH_CORNER}" in hdr
    assert L.BFGS_BND_BATCH_CORNER == R.CORNER == 1 << 8
    assert '"bfgs_bnd_batch"' in hdr   # the timer list names it


def test_bad_sizes_and_null_pointers_are_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, 3, 0) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 3, -5) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 0, 8) == L.PNOL_ERR_ARG
    for null in ("p", "lb", "ub", "X", "f0", "fopt", "iters", "evals", "info"):
        assert _batch(L.OBJ_ROSENBROCK, 3, 8, null=null) == L.PNOL_ERR_ARG, null
    # the device-pointer entry point without a context or an objective
    assert L.lib().pnol_bfgs_bnd_batch_solve_d(None, None, None, None, None, 8, None, None, None, None, None,
                                               None) == L.PNOL_ERR_ARG


def test_unsupported_requests():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, L.BFGS_BND_BATCH_NMAX + 1, 8) == L.PNOL_ERR_UNSUPPORTED
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, R.params(initHessFD=1)) == L.PNOL_ERR_UNSUPPORTED
    assert _batch(L.OBJ_LINRES, 3, 8) == L.PNOL_ERR_UNSUPPORTED


@pytest.mark.parametrize("which", ["maxIter", "maxIterLineSearch"])
@pytest.mark.parametrize("value", [-1, float("nan"), float("inf"), 2.0 ** 31])
def test_bad_iteration_caps_are_refused(which, value):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, R.params(**{which: value})) == L.PNOL_ERR_ARG


def test_short_quadratic_data_is_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len0=4) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len1=4) == L.PNOL_ERR_ARG


def test_inverted_box_is_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, lb=5.0, ub=-1.0) == L.PNOL_ERR_ARG


def test_no_device_is_reported_on_a_cpu_host():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _batch(L.OBJ_ROSENBROCK, 3, 8) == L.PNOL_ERR_NODEVICE
    assert _batch(L.OBJ_QUADRATIC, L.BFGS_BND_BATCH_NMAX, 1) == L.PNOL_ERR_NODEVICE
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, lb=2.0, ub=2.0) == L.PNOL_ERR_NODEVICE   # an empty box is a box
    from parallelnonlinearoptimizationlibrary_amd.device import run_bfgs_bnd_batch
    with pytest.raises(L.PnolError) as e:
        run_bfgs_bnd_batch(None, R.case_x0("A", 8), np.full(3, -1.0), np.full(3, 5.0), R.P, kind=L.OBJ_ROSENBROCK)
    assert e.value.status == L.PNOL_ERR_NODEVICE


# ---- 5. compile check ----------------------------------------------------------------------
def test_header_compiles_as_cxx11(tmp_path):
    """include/BFGS_bnd_linesearch_Batch.hpp in a C++11 program, warnings as errors (compile only)."""
    src = os.path.join(ROOT, "tests", "cpp", "bfgs_bnd_batch_cxx.cpp")
    subprocess.run(["g++", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                    "-o", str(tmp_path / "bfgs_bnd_batch_cxx.o")], check=True)
