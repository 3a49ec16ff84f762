"""The yardstick of the batched genetic algorithm (csrc/kernels/ga_batch.hip) on the CPU:
tests/ga_reference.py restates GeneticAlgorithm::runGA in plain Python in two forms.  The serial
form is bitwise the oracle's ga_findmin on every finite batch of the GPU tests; the wave form --
the stream consumed by random access as the kernel does -- is bitwise the serial form at every
speculation width, with the same draws consumed.  The stuck rule and the selection cap, the one
departure from the host class, are checked on synthetic fitness vectors.  The C ABI's argument
checks run before any device use, so they are tested here too."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ga_reference as R
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b):
    return _bits(a.X) == _bits(b.X) and _bits(np.array(a[1:3])) == _bits(np.array(b[1:3])) and a[3:6] == b[3:6]


# ---- 1. the serial form against the oracle -------------------------------------------------
@pytest.mark.parametrize("case", R.FINITE)
def test_serial_form_bitwise_against_oracle(oracle, case):
    name, n, lb, ub, x, nrun, p = R.CASES[case]
    runs = R.case_runs(oracle, case)
    assert len(runs) == nrun
    for s, r in enumerate(runs):
        X, res, st = oracle.ga_findmin(R.make_obj(oracle, name, n), [x] * n, [lb] * n, [ub] * n, list(p), R.SEED0 + s)
        assert st == 0
        assert _bits(X) == _bits(r.X), s
        assert _bits(np.float64(res.f0)) == _bits(np.float64(r.f0)), s
        assert _bits(np.float64(res.fopt)) == _bits(np.float64(r.fopt)), s
        assert (res.iters, res.evals, r.info) == (r.gens, r.evals, 0), s


def test_cases_reach_what_they_are_there_for(oracle):
    """The counters of the restatement on the two large batches: many distinct generation counts,
    both stops, in-loop identical-child redraws, bound repairs, selections of many pairs."""
    ros3 = R.case_runs(oracle, "ros3")
    gens = sorted(set(r.gens for r in ros3))
    assert len(gens) == 54 and gens[0] == 23 and gens[-1] == 200
    assert sum(r.counters.stop == "static" for r in ros3) == 64 and sum(r.counters.stop == "max" for r in ros3) == 1
    assert sum(r.counters.ident for r in ros3) == 54
    assert sum(r.counters.bounds for r in ros3) > 80000
    assert max(r.counters.pairs_max for r in ros3) == 10
    small = R.case_runs(oracle, "small")
    assert len(set(r.gens for r in small)) == 22
    assert sum(r.counters.ident for r in small) == 165
    assert max(r.counters.pairs_max for r in small) == 32
    assert set(r.gens for r in R.case_runs(oracle, "npop130")) >= {10, 40}
    assert all(r.gens == 0 and r.evals == 40 for r in R.case_runs(oracle, "gen0"))


# ---- 2. the wave form against the serial form ----------------------------------------------
@pytest.mark.parametrize("width", [1, 3, 64])
@pytest.mark.parametrize("case", R.FINITE)
def test_wave_form_bitwise_against_serial(oracle, case, width):
    serial = R.case_runs(oracle, case)
    wave = R.case_runs(oracle, case, form=R.Wave(width), tag=f"wave{width}")
    for s, (a, b) in enumerate(zip(serial, wave)):
        assert _same(a, b), s
        assert a.counters == b.counters, s      # draws consumed included


def test_random_access_equals_the_sequential_stream():
    rng = R._Stream(R.SEED0)
    seq = [rng.next() for _ in range(200)]
    assert seq == [R.u01(R.SEED0, c) for c in range(200)]
    assert all(0.0 <= u < 1.0 for u in seq)


# ---- 3. non-finite runs --------------------------------------------------------------------
def test_all_nan_population_is_flat_and_ends_by_max_generations(oracle):
    fn = R.oracle_fn(oracle, oracle.rosenbrock(2))
    p = R.params(Npop=20, maxGenerations=10)
    for form in (None, R.Wave(3)):
        r = R.run_ga(fn, [math.nan] * 2, [-2.0] * 2, [2.0] * 2, p, R.SEED0, form)
        assert r.gens == 10 and r.info == 0 and r.counters.stop == "max"
        assert r.counters.flat == r.counters.selects > 0
        assert np.all(np.isnan(r.X)) and math.isnan(r.fopt)
    a = R.run_ga(fn, [math.inf] * 2, [-2.0] * 2, [2.0] * 2, p, R.SEED0)
    b = R.run_ga(fn, [math.inf] * 2, [-2.0] * 2, [2.0] * 2, p, R.SEED0, R.Wave(64))
    assert _same(a, b) and a.counters == b.counters
    assert math.isfinite(a.fopt) and a.info == 0     # every member repaired into the box


def test_mixed_nan_sort_is_the_hosts_loop():
    """popSort with a NaN among the F: a NaN that comes first among the members left is taken
    first (no order relation); both forms run the host's loop."""
    pop = [[float(i)] for i in range(5)]
    F = [2.0, math.nan, 1.0, math.nan, 0.5]
    for ops in (R.Serial(), R.Wave()):
        rows, Fs = ops.sort(list(pop), list(F))
        assert [r[0] for r in rows] == [4.0, 2.0, 0.0, 1.0, 3.0]
        assert Fs[:3] == [0.5, 1.0, 2.0] and math.isnan(Fs[3]) and math.isnan(Fs[4])
        rows, Fs = ops.sort(list(pop[:3]), [math.nan, 2.0, 1.0])
        assert [r[0] for r in rows] == [0.0, 2.0, 1.0] and math.isnan(Fs[0]) and Fs[1:] == [1.0, 2.0]
    rows, _ = R.Wave().sort(list(pop), [1.0, 0.0, 1.0, -0.0, 0.5])    # ties keep their index order
    assert [r[0] for r in rows] == [1.0, 3.0, 4.0, 0.0, 2.0]


# ---- 4. the stuck rule and the cap ---------------------------------------------------------
def test_stuck_rule_on_synthetic_fitness():
    inf, nan = math.inf, math.nan
    assert R.flat_and_stuck([0.0, 0.0, 0.0]) == (True, False)
    assert R.flat_and_stuck([nan, nan, nan]) == (True, False)          # an all-NaN population
    assert R.flat_and_stuck([inf, nan, nan]) == (True, False)          # one finite F, the rest inf
    assert R.flat_and_stuck([4.0, 1.0, 0.0]) == (False, False)
    assert R.flat_and_stuck([inf, inf, nan]) == (False, True)          # inf / inf
    assert R.flat_and_stuck([inf, 5.0, 0.0]) == (False, True)          # 5 / inf == 0
    assert R.flat_and_stuck([nan, 5.0, 0.0]) == (False, True)
    assert R.flat_and_stuck([1e300, 1e-300, 0.0]) == (False, True)     # the ratio underflows to 0
    assert R.flat_and_stuck([1.0, 1e-300, 0.0]) == (False, False)      # accepted once in 1e300 pairs


@pytest.mark.parametrize("width", [1, 3, 64])
def test_selection_cap(width):
    """A selection that accepts with probability 1e-300 rejects `cap` pairs and gives up, having
    consumed 2 * cap draws at every width."""
    fitness = [1.0, 1e-300, 0.0, 1e-300]
    a, b = R._Stream(7), R._Stream(7)
    assert R.Serial(cap=50).select(a, fitness, 1.0, False, 4) == (-1, 50)
    assert R.Wave(width, cap=50).select(b, fitness, 1.0, False, 4) == (-1, 50)
    assert a.c == b.c == 100
    # and an ordinary selection ends on the same pair in both forms
    fitness = [1.0, 0.5, 0.25, 0.0]
    for seed in range(20):
        a, b = R._Stream(seed), R._Stream(seed)
        assert R.Serial().select(a, fitness, 1.0, False, 4) == R.Wave(width).select(b, fitness, 1.0, False, 4)
        assert a.c == b.c


def test_capped_run_ends_stuck():
    """An objective whose best member is 1e150 below all others: the pre-check passes (ratios
    about 1e-29), the first selection runs into the (small) cap, the run ends at generation 0."""
    fn = lambda v: 0.0 if v[0] == -1.0 else 1e150 + v[0] * 1e135
    p = R.params(Npop=12, maxGenerations=10)
    runs = [R.run_ga(fn, [-1.0, -1.0], [-2.0] * 2, [2.0] * 2, p, 5, form)
            for form in (R.Serial(cap=40), R.Wave(1, cap=40), R.Wave(3, cap=40), R.Wave(64, cap=40))]
    for r in runs:
        assert (r.gens, r.evals, r.info, r.counters.stop) == (0, 12, R.STUCK, "stuck")
        assert r.fopt == 0.0 and r.X.tolist() == [-1.0, -1.0]
        assert r.counters.pairs == 40 and r.counters.draws == runs[0].counters.draws


def test_overflowing_boxes(oracle):
    """Rosenbrock n = 2 from x0 = -1.  In [-1e200, 1e200]^2 only member 0 has a finite F, every
    fitness past index 0 is NaN, so select_member's own rule calls the generation flat: the run
    selects uniformly and ends by the static stop like the host class -- it is not stuck.  In
    [-1e77, 1e77]^2 about a third of the members have a finite F below an inf worst: fitness is
    inf, every ratio inf / inf, and the pre-check ends the run at generation 0."""
    fn = R.oracle_fn(oracle, oracle.rosenbrock(2))
    p = R.params(Npop=40, maxGenerations=50, NstaticGenerations=5)
    r = R.run_ga(fn, [-1.0] * 2, [-1e200] * 2, [1e200] * 2, p, R.SEED0)
    assert (r.info, r.counters.stop, r.gens) == (0, "static", 5) and r.fopt == 404.0
    assert r.counters.flat == r.counters.selects > 0
    r = R.run_ga(fn, [-1.0] * 2, [-1e77] * 2, [1e77] * 2, p, R.SEED0)
    assert (r.info, r.counters.stop, r.gens, r.evals) == (R.STUCK, "stuck", 0, 40) and r.fopt == 404.0


# ---- 5. ABI: argument checks before any device use, the same with or without a GPU ---------
def _batch(kind, n, nrun, params=R.CASES["ros3"][6], len0=None, len1=None, null=None):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    ns, nn = max(nrun, 1), max(n, 1)
    X = np.full(ns * nn, -1.0)
    lo, hi = np.full(nn, -2.0), np.full(nn, 2.0)
    f0, fo = np.zeros(ns), np.zeros(ns)
    gens, evals, info = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int64), np.zeros(ns, dtype=np.int32)
    p = np.array(params, dtype=np.float64)
    d = np.ones(nn)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    args = {"p": dp(p), "lb": dp(lo), "ub": dp(hi), "X": dp(X), "f0": dp(f0), "fopt": dp(fo), "gens": ip(gens),
            "evals": evals.ctypes.data_as(C.POINTER(C.c_longlong)), "info": ip(info)}
    if null:
        args[null] = None
    return L.lib().pnol_run_ga_batch(kind, n, 2.0, dp(d), d.size if len0 is None else len0, dp(d),
                                     d.size if len1 is None else len1, nrun, args["p"], R.SEED0, args["lb"],
                                     args["ub"], args["X"], args["f0"], args["fopt"], args["gens"], args["evals"],
                                     args["info"])


def test_entry_points_exist():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    for name in ("pnol_ga_batch_solve_d", "pnol_run_ga_batch"):
        assert hasattr(L.lib(), name), name
        assert name in L.declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "pnol_amd.h")).read()
    assert f"#define PNOL_GA_BATCH_NMAX {L.GA_BATCH_NMAX}" in hdr and L.GA_BATCH_NMAX == 12
    assert f"#define PNOL_GA_BATCH_NPOP_MAX {L.GA_BATCH_NPOP_MAX}" in hdr and L.GA_BATCH_NPOP_MAX == 256
    assert f"#define PNOL_GA_BATCH_STUCK {L.GA_BATCH_STUCK}" in hdr and L.GA_BATCH_STUCK == R.STUCK == 1
    assert f"#define PNOL_GA_BATCH_SELECT_CAP {R.SELECT_CAP}" in hdr and R.SELECT_CAP == 1 << 20
    assert '"ga_batch"' in hdr   # the timer list names it


def test_bad_sizes_and_null_pointers_are_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, 3, 0) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 3, -5) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_ROSENBROCK, 0, 8) == L.PNOL_ERR_ARG
    for null in ("p", "lb", "ub", "X", "f0", "fopt", "gens", "evals", "info"):
        assert _batch(L.OBJ_ROSENBROCK, 3, 8, null=null) == L.PNOL_ERR_ARG, null
    # the device-pointer entry point without a context or an objective
    assert L.lib().pnol_ga_batch_solve_d(None, None, None, 0, None, None, 8, None, None, None, None, None,
                                         None) == L.PNOL_ERR_ARG


@pytest.mark.parametrize("over", [dict(Npop=1), dict(Npop=0), dict(Npop=-4), dict(Npop=float("nan")),
                                  dict(maxGenerations=-1), dict(maxGenerations=float("nan")),
                                  dict(maxGenerations=float("inf")), dict(maxGenerations=2.0 ** 31),
                                  dict(eliteFrac=0.5, crossFrac=0.3, eliteMutationFrac=0.2),     # Nrand = 0: "666"
                                  dict(eliteFrac=0.6, crossFrac=0.6), dict(crossFrac=float("nan")),
                                  dict(eliteFrac=-0.5)])
def test_bad_parameters_are_refused(over):
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, R.params(**over)) == L.PNOL_ERR_ARG


def test_unsupported_requests():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_ROSENBROCK, L.GA_BATCH_NMAX + 1, 8) == L.PNOL_ERR_UNSUPPORTED
    assert _batch(L.OBJ_ROSENBROCK, 3, 8, R.params(Npop=L.GA_BATCH_NPOP_MAX + 1)) == L.PNOL_ERR_UNSUPPORTED
    assert _batch(L.OBJ_LINRES, 3, 8) == L.PNOL_ERR_UNSUPPORTED


def test_short_quadratic_data_is_refused():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len0=4) == L.PNOL_ERR_ARG
    assert _batch(L.OBJ_QUADRATIC, 5, 8, len1=4) == L.PNOL_ERR_ARG


def test_no_device_is_reported_on_a_cpu_host():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    if L.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _batch(L.OBJ_ROSENBROCK, 3, 8) == L.PNOL_ERR_NODEVICE
    assert _batch(L.OBJ_QUADRATIC, L.GA_BATCH_NMAX, 1, R.params(Npop=L.GA_BATCH_NPOP_MAX)) == L.PNOL_ERR_NODEVICE
    from parallelnonlinearoptimizationlibrary_amd.device import run_ga_batch
    with pytest.raises(L.PnolError) as e:
        run_ga_batch(None, R.case_x0("ros3", 8), np.full(3, -2.0), np.full(3, 2.0), R.CASES["ros3"][6], R.SEED0,
                     kind=L.OBJ_ROSENBROCK)
    assert e.value.status == L.PNOL_ERR_NODEVICE


# ---- 6. compile check ----------------------------------------------------------------------
def test_header_compiles_as_cxx11(tmp_path):
    """include/GeneticAlgorithmBatch.hpp in a C++11 program, warnings as errors (compile only)."""
    src = os.path.join(ROOT, "tests", "cpp", "ga_batch_cxx.cpp")
    subprocess.run(["g++", "-std=c++0x", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                    "-o", str(tmp_path / "ga_batch_cxx.o")], check=True)
