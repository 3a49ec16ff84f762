"""SimplexSearch, the parts that need no GPU: the drop-in class on C callback objectives against
the plain-Python restatement (tests/simplex_reference.py) bit for bit, known answers that do not
depend on the restatement, the argument checks of the batched entry points (all made before any
device use), and the C++11 compile check of the two headers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import simplex_reference as SR
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _host_run(fn, x0, params, seed):
    from parallelnonlinearoptimizationlibrary_amd.device import host_run_simplex
    return host_run_simplex(fn, x0, params, seed)


CASES = [("rosenbrock", 2, SR.DEFAULTS), ("rosenbrock", 3, SR.DEFAULTS), ("rosenbrock", 10, SR.params(maxIter=400)),
         ("power2", 1, SR.DEFAULTS), ("power2", 5, SR.DEFAULTS)]


@pytest.mark.parametrize("name,n,p", CASES, ids=[f"{c[0]}-n{c[1]}" for c in CASES])
def test_host_class_bitwise_against_restatement(oracle, name, n, p):
    """pnol_host_run_simplex on Python callbacks over the first 8 starts of the standard batch:
    X, f0, fOpt, iterations and evaluations are the restatement's, bit for bit."""
    ref = SR.standard_batch(oracle, name, n, 8, p)
    obj = oracle.rosenbrock(n) if name == "rosenbrock" else oracle.power(n, 2.0)
    fn = lambda x: oracle.obj_eval(obj, x)
    x0 = SR.standard_x0(8, n)
    for s in range(8):
        X, res = _host_run(fn, x0[s], p, SR.SEED0 + s)
        r = ref[s]
        assert _bits(X) == _bits(r.X), s
        assert _bits(np.float64(res.f0)) == _bits(np.float64(r.f0)), s
        assert _bits(np.float64(res.fopt)) == _bits(np.float64(r.fopt)), s
        assert (res.iters, res.evals) == (r.iters, r.evals), s


def test_standard_batch_takes_every_outcome(oracle):
    """Guards the inputs of the bitwise test: over the first 8 Rosenbrock n = 3 starts every
    outcome is taken, the shrink in start 1."""
    ref = SR.standard_batch(oracle, "rosenbrock", 3, 8)
    total = np.sum([r.outcomes for r in ref], axis=0)
    assert all(total > 0), dict(zip(SR.OUTCOMES, total))
    assert ref[1].outcomes[SR.OUTCOMES.index("shrink")] > 0


def test_rosenbrock_2d_known_answer():
    calls = []

    def rosen(x):
        calls.append(x.copy())
        return 100.0 * (x[1] - x[0] * x[0]) ** 2 + (1.0 - x[0]) ** 2

    X, res = _host_run(rosen, [3.0, 3.0], SR.DEFAULTS, 7)
    assert np.max(np.abs(X - 1.0)) < 1e-5
    assert res.fopt < 1e-12
    assert res.f0 == rosen(np.array([3.0, 3.0]))
    # n + 1 at the start, then 1 or 2 per trip (a shrink: n + 1 more): every call is counted
    assert res.evals == len(calls) - 1
    assert 3 + res.iters <= res.evals
    assert np.array_equal(calls[0], [3.0, 3.0])


def test_one_trip_by_hand_power2_n1():
    """n = 1, f = x^2, one trip from x0 = 3.  The second vertex b = 3 + (u - 0.5) * 2 lies in
    [2, 4); this stream gives b > 3 (asserted), so 3 is the best vertex and b the worst:
    xbar = 3, the reflection 3 + (3 - b) = 6 - b in (2, 3) beats 3, the expansion
    3 + 2 (3 - b) = 9 - 2b in (1, 3) is smaller still (9 - 2b < 6 - b for b > 3) and is kept; it
    is the new best.  Four evaluations."""
    pts = []

    def sq(x):
        pts.append(float(x[0]))
        return x[0] * x[0]

    X, res = _host_run(sq, [3.0], SR.params(maxIter=1), SR.SEED0)
    assert pts[0] == 3.0
    b = pts[1]
    assert 3.0 < b < 4.0
    xbar = 3.0 / 1.0
    xref = xbar + 1.0 * (xbar - b)
    xe = xbar + 2.0 * (xbar - b)
    assert pts == [3.0, b, xref, xe]
    assert (res.iters, res.evals) == (1, 4)
    assert res.f0 == 9.0 and res.fopt == xe * xe and X[0] == xe


def _sort_diff(f, rows):
    """simplexSort then simplexDiff through the C++ free functions (tests/cpp/simplex_cxx.cpp links
    nothing; here they are called in the library by their C++ names)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    n1, nd = len(f), len(rows[0])
    fv = (C.c_double * n1)(*f)
    store = [(C.c_double * nd)(*r) for r in rows]
    xv = (C.POINTER(C.c_double) * n1)(*[C.cast(s, C.POINTER(C.c_double)) for s in store])
    sort = getattr(lib, "_Z11simplexSortPdPS_i")
    diff = getattr(lib, "_Z11simplexDiffPPdii")
    diff.restype = C.c_double
    sort(fv, xv, C.c_int(nd))
    d = diff(xv, C.c_int(nd), C.c_int(n1))
    return list(fv), [[xv[k][j] for j in range(nd)] for k in range(n1)], d


def test_simplex_sort_keeps_the_first_of_equal_values_first():
    f, x, _ = _sort_diff([2.0, 1.0, 3.0, 1.0, 2.0], [[0.0, 10.0, 0, 0], [1.0, 11.0, 0, 0], [2.0, 12.0, 0, 0],
                                                     [3.0, 13.0, 0, 0], [4.0, 14.0, 0, 0]])
    assert f == [1.0, 1.0, 2.0, 2.0, 3.0]
    assert [r[0] for r in x] == [1.0, 3.0, 0.0, 4.0, 2.0]
    assert [r[1] for r in x] == [11.0, 13.0, 10.0, 14.0, 12.0]
    # every value <= 0: the case the reference's 2 * max(f) sentinel gets wrong
    f, x, _ = _sort_diff([-1.0, -3.0, -2.0], [[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    assert f == [-3.0, -2.0, -1.0] and [r[0] for r in x] == [1.0, 2.0, 0.0]


def test_simplex_diff_on_a_hand_made_simplex():
    # already sorted; vertex 0 is (1, 1): |1 - 1.5| = 0.5, |1 - (-2)| = 3, |1 - 1.25| = 0.25
    _, _, d = _sort_diff([0.0, 1.0, 2.0], [[1.0, 1.0], [1.5, 1.0], [1.25, -2.0]])
    assert d == 3.0


# ---- argument checks: before any device use, so the same with or without a GPU ------------
def _batch(kind, n, nstart, params=SR.DEFAULTS, len0=None, len1=None, null=None):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    ns, nn = max(nstart, 1), max(n, 1)
    X = np.full(ns * nn, 3.0)
    f0, fo = np.zeros(ns), np.zeros(ns)
    iters, evals = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int64)
    p = np.array(params, dtype=np.float64)
    d = np.ones(nn)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args = {"p": dp(p), "X": dp(X), "f0": dp(f0), "fopt": dp(fo),
            "iters": iters.ctypes.data_as(C.POINTER(C.c_int)), "evals": evals.ctypes.data_as(C.POINTER(C.c_longlong))}
    if null:
        args[null] = None
    return L.lib().pnol_run_simplex_batch(kind, n, 2.0, dp(d), d.size if len0 is None else len0, dp(d),
                                          d.size if len1 is None else len1, nstart, args["p"], SR.SEED0, args["X"],
                                          args["f0"], args["fopt"], args["iters"], args["evals"])


def _host_status(params):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    p = np.array(params, dtype=np.float64)
    X = np.array([3.0, 3.0])
    res = L.Result()
    cb = L.HOST_SCALAR_FN(lambda xp, n, _u: 0.0)
    return L.lib().pnol_host_run_simplex(cb, None, p.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                         X.ctypes.data_as(C.POINTER(C.c_double)), 2, C.byref(res))


@pytest.mark.parametrize("max_iter", [-1, float("nan"), 2.0 ** 31])
def test_bad_max_iter_is_refused(max_iter):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    p = SR.params(maxIter=max_iter)
    assert _host_status(p) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, p) == L.PNOL_ERR_ARG


def test_bad_sizes_are_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, 3, 0) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 3, -5) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 0, 8) == L.PNOL_ERR_ARG
    assert L.SIMPLEX_BATCH_NMAX == 12
    assert _batch(L.OBJ_ROSENBROCK, 13, 8) == L.PNOL_ERR_UNSUPPORTED


def test_other_kinds_are_unsupported():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_LINRES, 3, 8) == L.PNOL_ERR_UNSUPPORTED
    assert _batch(L.OBJ_CUBIC, 4, 8) == L.PNOL_ERR_UNSUPPORTED


def test_null_pointers_are_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    for null in ("p", "X", "f0", "fopt", "iters", "evals"):
        assert _batch(L.OBJ_ROSENBROCK, 3, 8, null=null) == L.PNOL_ERR_ARG, null
    # the device-pointer entry point without a context or an objective
    assert L.lib().pnol_simplex_batch_solve_d(None, None, None, 1, 8, None, None, None, None, None) == L.PNOL_ERR_ARG


def test_short_quadratic_data_is_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len0=4) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len1=4) == L.PNOL_ERR_ARG


def test_refusal_precedence():
    """The order the refusals are applied in: parameters, then the kind, then non-positive sizes,
    then the NMAX limit, then the quadratic's data and the output pointers."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_LINRES, 3, 8, SR.params(maxIter=-1)) == L.PNOL_ERR_ARG           # parameters before kind
    assert _batch(L.OBJ_LINRES, 0, 8) == L.PNOL_ERR_UNSUPPORTED                          # kind before sizes
    assert _batch(L.OBJ_ROSENBROCK, L.SIMPLEX_BATCH_NMAX + 1, 0) == L.PNOL_ERR_ARG       # sizes before NMAX
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len0=4, null="fopt") == L.PNOL_ERR_ARG


def test_no_device_is_reported_on_a_cpu_host():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _batch(L.OBJ_ROSENBROCK, 3, 8) == L.PNOL_ERR_NODEVICE
    assert _batch(L.OBJ_QUADRATIC, 12, 1) == L.PNOL_ERR_NODEVICE
    from parallelnonlinearoptimizationlibrary_amd.device import run_simplex_batch
    with pytest.raises(L.PnolError) as e:
        run_simplex_batch(None, SR.standard_x0(8, 3), SR.DEFAULTS, SR.SEED0, kind=L.OBJ_ROSENBROCK)
    assert e.value.status == L.PNOL_ERR_NODEVICE


def test_entry_points_exist():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    for name in ("pnol_run_simplex", "pnol_host_run_simplex", "pnol_simplex_batch_solve_d",
                 "pnol_run_simplex_batch"):
        assert hasattr(L.lib(), name), name
        assert name in L.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "pnol_amd.h")).read()
    assert "#define PNOL_SIMPLEX_BATCH_NMAX 12" in hdr


def test_headers_compile_as_cxx11(tmp_path):
    """include/SimplexSearch.hpp and include/SimplexSearchBatch.hpp in a C++11 program, warnings as
    errors (compile only)."""
    src = os.path.join(ROOT, "tests", "cpp", "simplex_cxx.cpp")
    subprocess.run(["g++", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                    "-o", str(tmp_path / "simplex_cxx.o")], check=True)


def test_nan_objective_still_ends_by_max_iter():
    X, res = _host_run(lambda x: math.nan, [3.0, 3.0], SR.params(maxIter=25), 3)
    assert res.iters <= 25
