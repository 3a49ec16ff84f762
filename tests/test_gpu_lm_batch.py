"""Batched Levenberg-Marquardt on the GPU (csrc/kernels/lm_batch.hip): one lane per problem.
Cubic has no transcendental, so every problem of a batch is compared with the oracle's
LevMarq::findMin bit for bit; ExpCurve is compared bit for bit with the library's one-problem
device path (the same device exp, the same residual expression, the same operation order)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import lm_batch_fixtures as FX
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("X", "chi0", "chi", "iters", "evals", "F0", "FOpt")
# max over the 65 ExpCurve problems of rel(X of the one-problem device path, X of the oracle), as
# measured on an MI355X (test_expcurve_loose_against_oracle prints it); the batch gets twice that
EXP_SINGLE_VS_ORACLE = 1.620e-10


@pytest.fixture(scope="module")
def ctx():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import Context
    if L.device_count() < 1:
        pytest.fail("no gfx950 device visible for a -m gpu run")
    return Context(0)


def _solve(kind, xd, yd, x0, params, ctx=None):
    from parallelnonlinearoptimizationlibrary_amd.device import run_levmarq_batch
    return dict(zip(KEYS, run_levmarq_batch(ctx, kind, xd, yd, x0, params, want_F=True)))


_CACHE = {}


def _cubic(nprob, m):
    """The device solution of FX.cubic_batch(nprob, m), host-pointer form (solved once)."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    if (nprob, m) not in _CACHE:
        _CACHE[(nprob, m)] = _solve(L.OBJ_CUBIC, *FX.cubic_batch(nprob, m), FX.CUBIC_PARAMS)
    return _CACHE[(nprob, m)]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_bitwise(got, ref, rows=None, ref_rows=None):
    a = slice(None) if rows is None else rows
    b = a if ref_rows is None else ref_rows
    for k in KEYS:
        assert got[k][a].dtype == ref[k][b].dtype, k
        assert _bits(got[k][a]) == _bits(ref[k][b]), k


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


# ---- 1. Cubic, bitwise against the oracle per problem ------------------------------------
@pytest.mark.parametrize("nprob", [1, 63, 64, 65, 130])
def test_cubic_bitwise_against_oracle(oracle, nprob):
    """A partial wave, an exact wave, a wave plus one, two waves plus a tail."""
    ref = FX.cubic_oracle(oracle, nprob, 37)
    if nprob == 130:
        # guards the inputs: neighbouring lanes must really leave the loop at different trips
        assert len(set(ref["iters"].tolist())) >= 3, sorted(set(ref["iters"].tolist()))
    _assert_bitwise(_cubic(nprob, 37), ref)


# ---- 2. m edges: with per-problem grids m = 4 and 33 stay resident in LDS (33: the largest m
# that does), m = 100 is staged in 32-row chunks with a 4-row tail (as m = 37 above: 32 + 5) ----
@pytest.mark.parametrize("m", [4, 33, 100])
def test_cubic_m_edges(oracle, m):
    _assert_bitwise(_cubic(65, m), FX.cubic_oracle(oracle, 65, m))


@pytest.mark.parametrize("rows", [7, 33, 100])
def test_staging_chunk_size_does_not_change_the_bits(monkeypatch, rows):
    """PNOL_LMB_ROWS (tuning): 7- and 33-row chunks, and all 100 rows of y, x and the cube table
    resident in LDS (155 KB of the CU's 160), against the default 32-row chunks."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    ref = _cubic(65, 100)
    monkeypatch.setenv("PNOL_LMB_ROWS", str(rows))
    _assert_bitwise(_solve(L.OBJ_CUBIC, *FX.cubic_batch(65, 100), FX.CUBIC_PARAMS), ref)


# ---- 3. a poisoned lane stays alone ---------------------------------------------------------
def test_poisoned_lane(oracle):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    xd, yd, x0 = FX.cubic_batch(130, 37)
    yd = yd.copy()
    yd[70, 5] = np.nan
    got = _solve(L.OBJ_CUBIC, xd, yd, x0, FX.CUBIC_PARAMS)
    assert _bits(got["X"][70]) == _bits(x0[70])
    assert got["iters"][70] == FX.CUBIC_PARAMS[3]
    assert np.isnan(got["chi"][70]) and np.isnan(got["chi0"][70])
    assert got["evals"][70] == 1 + 6 * FX.CUBIC_PARAMS[3]   # every trip ran and was rejected
    _assert_bitwise(got, FX.cubic_oracle(oracle, 130, 37), rows=[69, 71])


# ---- 4. a problem's result does not depend on its batch -------------------------------------
@pytest.mark.parametrize("p", [0, 63, 64, 129])
def test_batch_independence(p):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    xd, yd, x0 = FX.cubic_batch(130, 37)
    alone = _solve(L.OBJ_CUBIC, xd[p:p + 1], yd[p:p + 1], x0[p:p + 1], FX.CUBIC_PARAMS)
    _assert_bitwise(alone, _cubic(130, 37), rows=[0], ref_rows=[p])


# ---- 5. one shared grid == the same grid repeated -------------------------------------------
@pytest.mark.parametrize("kind_name", ["cubic", "exp"])
def test_shared_grid(kind_name):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    if kind_name == "cubic":
        xd, yd, x0 = FX.cubic_batch(65, 37)
        kind, grid, params = L.OBJ_CUBIC, np.ascontiguousarray(xd[3]), FX.CUBIC_PARAMS
    else:
        grid, yd, x0 = FX.exp_batch(65, 37)
        kind, params = L.OBJ_EXPCURVE, FX.EXP_PARAMS
    shared = _solve(kind, grid, yd, x0, params)
    repeated = _solve(kind, np.tile(grid, (65, 1)), yd, x0, params)
    _assert_bitwise(shared, repeated)
    assert len(set(shared["iters"].tolist())) >= 2   # the fits are not all alike


# ---- 6. maxIter = 0 -------------------------------------------------------------------------
def test_max_iter_zero():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    xd, yd, x0 = FX.cubic_batch(65, 37)
    got = _solve(L.OBJ_CUBIC, xd, yd, x0, (0.001, 10, 1e-6, 0, 1e-5, -1))
    assert _bits(got["X"]) == _bits(x0)
    assert np.all(got["iters"] == 0) and np.all(got["evals"] == 1)
    assert _bits(got["chi"]) == _bits(got["chi0"])
    assert _bits(got["F0"]) == _bits(got["FOpt"])
    assert _bits(got["chi0"]) == _bits(_cubic(65, 37)["chi0"])


# ---- 7. ExpCurve against the one-problem device path and, loosely, the oracle ---------------
@pytest.fixture(scope="module")
def exp_single(ctx):
    """The existing one-problem device path (LevMarq on a DeviceObjective) on every problem of
    the ExpCurve batch: X (65 x 3) and the evals counts.  Not the code under test."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_levmarq
    xd, yd, x0 = FX.exp_batch(65, 37)
    X, evals = np.zeros((65, 3)), np.zeros(65, dtype=np.int64)
    for p in range(65):
        d = DeviceObjective(ctx, L.OBJ_EXPCURVE, 3, 37, xd, yd[p])
        X[p], _, _, res = run_levmarq(d, x0[p], FX.EXP_PARAMS)
        evals[p] = res.evals
        d.close()
    return X, evals


@pytest.fixture(scope="module")
def exp_batch_dev():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    return _solve(L.OBJ_EXPCURVE, *FX.exp_batch(65, 37), FX.EXP_PARAMS)


@pytest.mark.parametrize("p", [0, 1, 31, 63, 64, 7, 22, 45])
def test_expcurve_bitwise_against_one_problem_path(exp_single, exp_batch_dev, p):
    """Bits of X and the trip count.  The one-problem driver reports no iteration count
    (pnol_result.iters is 0 there); its evals count, 1 + trips * (n + 2), gives the trips, and
    the loop's iter is trips - 1 when it stopped on xMinDiff and trips at maxIter."""
    Xs, evals = exp_single
    got = exp_batch_dev
    assert _bits(got["X"][p]) == _bits(Xs[p])
    assert got["evals"][p] == evals[p]
    trips, max_iter = (int(evals[p]) - 1) // 5, int(FX.EXP_PARAMS[3])
    assert (int(evals[p]) - 1) % 5 == 0
    if trips < max_iter:
        assert got["iters"][p] == trips - 1
    else:
        assert got["iters"][p] in (max_iter - 1, max_iter)


def test_expcurve_loose_against_oracle(oracle, exp_single, exp_batch_dev):
    """The batch against the oracle (glibc exp) within twice what the one-problem device path
    (device exp) differs from it: an ulp of exp moves the converged X of these noisy fits far
    more than 1e-10.  Measured on an MI355X: max over the batch of rel(X one-problem, X oracle)
    = 1.620e-10 (EXP_SINGLE_VS_ORACLE); the batch, bitwise that path, gave the same 1.620e-10."""
    ref = FX.exp_oracle(oracle, 65, 37)
    per = lambda X: max(rel(X[p], ref["X"][p]) for p in range(65))
    single, batch = per(exp_single[0]), per(exp_batch_dev["X"])
    print(f"expcurve: one-problem path vs oracle {single:.3e}, batch vs oracle {batch:.3e}")
    assert EXP_SINGLE_VS_ORACLE is not None, f"record the measured one-problem value: {single:.3e}"
    assert batch <= 2 * EXP_SINGLE_VS_ORACLE


def test_expcurve_noise_free_reference_data(ctx, oracle):
    """testLMExp's noise-free data (ExampleObjectives.hpp:113-154) as problem 0 of a batch: the
    one-problem device path meets 1e-10 against the reference output there (test_lm_expcurve),
    so the batch must too, and is bitwise that path."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_levmarq
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_survey.json")))["testLMExp"]
    oe = oracle.expcurve()
    _, y1, _ = FX.exp_batch(1, 100)
    yd = np.ascontiguousarray(np.vstack([oe.p1, y1[0]]))
    x0 = np.tile(np.array(g["x0"], dtype=np.float64), (2, 1))
    params = g["params"][:5] + [-1]   # the reference's parameters, silent
    got = _solve(L.OBJ_EXPCURVE, oe.p0, yd, x0, params)
    Xs, *_ = run_levmarq(DeviceObjective(ctx, L.OBJ_EXPCURVE, 3, 100, oe.p0, oe.p1), g["x0"], params)
    print(f"testLMExp: one-problem path vs reference {rel(Xs, g['X']):.3e}, batch {rel(got['X'][0], g['X']):.3e}")
    assert rel(Xs, g["X"]) <= 1e-10
    assert _bits(got["X"][0]) == _bits(Xs)
    assert rel(got["X"][0], g["X"]) <= 1e-10


# ---- 8. device form: torch tensors on the context's stream ----------------------------------
def test_device_form_equals_host_form(ctx):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import LMBatch
    xd, yd, x0 = FX.cubic_batch(130, 37)
    b = LMBatch(ctx, L.OBJ_CUBIC, 37, 130, xd)
    y_t, X_t = ctx.tensor(yd), ctx.tensor(x0)
    out = b.solve(y_t, X_t, FX.CUBIC_PARAMS, want_F=True)
    assert out[0] is X_t   # solved in place
    ctx.synchronize()
    got = dict(zip(KEYS, (a.cpu().numpy() for a in out)))
    b.close()
    _assert_bitwise(got, _cubic(130, 37))


# ---- 9. the C++ header ----------------------------------------------------------------------
def test_cxx_header_program(tmp_path):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    pkg = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")
    exe = str(tmp_path / "lm_batch_cxx")
    subprocess.run(["g++", "-O2", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lm_batch_cxx.cpp"), "-L", pkg, "-lpnol_amd", "-pthread",
                    f"-Wl,-rpath,{pkg}", "-o", exe], check=True)
    xd, yd, x0 = FX.cubic_batch(8, 37)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("4q", L.OBJ_CUBIC, 8, 37, xd.size))
        for a in (xd, yd, x0):
            f.write(_bits(a))
    r = subprocess.run([exe, str(data)] + [repr(float(v)) for v in FX.CUBIC_PARAMS[:5]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("X ")]
    assert len(rows) == 8
    vals = np.array([[float(v) for v in row[:6]] for row in rows])
    ref = _cubic(8, 37)
    assert _bits(vals[:, :4]) == _bits(ref["X"])
    assert _bits(vals[:, 4]) == _bits(ref["chi0"]) and _bits(vals[:, 5]) == _bits(ref["chi"])
    assert [int(row[6]) for row in rows] == ref["iters"].tolist()
