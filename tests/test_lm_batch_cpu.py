"""Batched Levenberg-Marquardt, the parts that need no GPU: the host-pointer entry point exists,
refuses bad shapes before it touches a device, reports a GPU-less host as such, and the
header-only C++ class compiles as C++11."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _call(kind, n, m, nprob, xlen, params=(0.001, 10, 1e-6, 10, 1e-5, -1)):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    np_ = max(nprob, 1)
    x = np.linspace(-1, 1, max(xlen, 1))
    y = np.zeros(np_ * max(m, 1))
    X = np.full(np_ * max(n, 1), 0.1)
    chi0, chi = np.zeros(np_), np.zeros(np_)
    iters, evals = np.zeros(np_, dtype=np.int32), np.zeros(np_, dtype=np.int64)
    p = np.array(params, dtype=np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    return L.lib().pnol_run_levmarq_batch(kind, n, m, nprob, dp(x), xlen, dp(y), dp(p), dp(X), dp(chi0), dp(chi),
                                          iters.ctypes.data_as(C.POINTER(C.c_int)),
                                          evals.ctypes.data_as(C.POINTER(C.c_longlong)), None, None)


def test_entry_points_exist():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    for name in ("pnol_lm_batch_create", "pnol_lm_batch_destroy", "pnol_lm_batch_solve_d", "pnol_run_levmarq_batch"):
        assert hasattr(L.lib(), name), name
        assert name in L.declared_symbols()


@pytest.mark.parametrize("kind,n,m,nprob,xlen", [
    (11, 4, 37, 0, 37),          # nprob <= 0
    (11, 4, 37, -3, 37),
    (11, 3, 37, 8, 37),          # Cubic has n = 4
    (10, 4, 37, 8, 37),          # ExpCurve has n = 3
    (11, 4, 37, 8, 38),          # xlen neither m nor nprob * m
    (11, 4, 37, 8, 8 * 37 - 1),
    (10, 3, 0, 8, 0),            # no data rows
])
def test_bad_shapes_are_refused_before_any_device_use(kind, n, m, nprob, xlen):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    # PNOL_ERR_ARG with or without a GPU: the shape checks come first
    assert _call(kind, n, m, nprob, xlen) == L.PNOL_ERR_ARG


def test_other_kinds_are_unsupported():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _call(L.OBJ_LINRES, 4, 37, 8, 37) == L.PNOL_ERR_UNSUPPORTED
    assert _call(L.OBJ_ROSENBROCK, 4, 37, 8, 37) == L.PNOL_ERR_UNSUPPORTED


def test_bad_max_iter_is_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _call(11, 4, 37, 8, 37, params=(0.001, 10, 1e-6, -1, 1e-5, -1)) == L.PNOL_ERR_ARG
    assert _call(11, 4, 37, 8, 37, params=(0.001, 10, 1e-6, float("nan"), 1e-5, -1)) == L.PNOL_ERR_ARG


def test_no_device_is_reported_on_a_cpu_host():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _call(11, 4, 37, 8, 37) == L.PNOL_ERR_NODEVICE
    assert _call(10, 3, 37, 8, 8 * 37) == L.PNOL_ERR_NODEVICE
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq_batch
    with pytest.raises(L.PnolError) as e:
        run_levmarq_batch(None, L.OBJ_CUBIC, np.linspace(-5, 5, 37), np.zeros((8, 37)), np.full((8, 4), 0.1),
                          (0.001, 10, 1e-6, 10, 1e-5, -1))
    assert e.value.status == L.PNOL_ERR_NODEVICE


def test_header_compiles_as_cxx11(tmp_path):
    """include/LevenbergMarquardtBatch.hpp in a C++11 program, warnings as errors (compile only)."""
    src = os.path.join(ROOT, "tests", "cpp", "lm_batch_cxx.cpp")
    subprocess.run(["g++", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                    "-o", str(tmp_path / "lm_batch_cxx.o")], check=True)
