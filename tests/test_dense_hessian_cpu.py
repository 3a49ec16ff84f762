"""The inputs of tests/test_gpu_dense_hessian.py, checked without a GPU: the reference's Fraction
product form equals the class's rank-2 lazy form on every dyadic fixture (so the algebra the GPU
tests hold the class to is the reference's), every dyadic fixture satisfies the exactness
condition that makes array_equal the right comparison, the accuracy bound of the random fixtures
is attained by an fp64 restatement of the lazy algebra, and the replay driver compiles."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dense_hessian_reference as R
from conftest import ROOT

DYADIC = [(n, k, scaled) for n, k in R.DYADIC_CASES for scaled in (False, True)]
IDS = [f"n{n}-{'diag' if scaled else 'I'}" for n, k, scaled in DYADIC]


@pytest.mark.parametrize("n,updates,scaled", DYADIC, ids=IDS)
def test_fraction_lazy_form_equals_product_form(n, updates, scaled):
    """p before any update, every pnext, the direction with the correction pending and on the
    folded D, and D after every update: the lazy form's Fractions are the product form's (at
    n = 5 the n^3 product too), and the audited dyadic run of the fixture gave the same numbers."""
    fx = R.dyadic_fixture(n, updates, scaled)
    m = R.fraction_model(fx)
    lazy = R.LazyModel(n, Fraction)
    lazy.ident(fx.scale)
    same = lambda *xs: all(np.array_equal(xs[0], x) for x in xs[1:])
    assert same(m.direction(fx.g), lazy.direction(fx.g), fx.lazy["p0"].fractions())
    for k, (y, s, g) in enumerate(fx.steps):
        lit = m.product_form_literal(y, s) if n <= 5 else None
        assert same(m.update(y, s, g), lazy.update(y, s, g), fx.lazy["pnext"][k].fractions())
        p = m.direction(fx.g)
        assert same(p, lazy.direction(fx.g), fx.lazy["ppend"][k].fractions())
        assert same(m.get(), lazy.get(), fx.lazy["D"][k].fractions())
        assert lit is None or same(m.get(), lit)
        assert same(p, lazy.direction(fx.g), fx.lazy["pfold"][k].fractions())


@pytest.mark.parametrize("n,updates,scaled", DYADIC, ids=IDS)
def test_dyadic_fixture_is_exact_in_fp64(n, updates, scaled):
    """Every value is a multiple of 2^-q and every sum's |terms| add up to less than 2^(53 - q), the
    updates are real ones (y.s a power of two other than 1, D changes), and the model's results
    convert to fp64 without rounding."""
    fx = R.dyadic_fixture(n, updates, scaled)
    au = fx.audit
    print(f"n={n} scaled={scaled}: y.s {float(fx.steps[0][0] @ fx.steps[0][1])} q {au.q} bits {au.max_bits} "
          f"max sum|terms| 2^{float(np.log2(float(au.max_abs_sum))):.1f}")
    assert au.holds()
    assert au.max_abs_sum < 2.0 ** (53 - au.q)
    assert len(fx.steps) == updates
    for y, s, g in fx.steps:
        ys = float(y @ s)
        assert ys > 1 and np.log2(ys) == int(np.log2(ys))
    D = [fx.lazy["D"][k].fractions() for k in range(updates)]
    for k in range(updates):
        R.to_f64(D[k])
        R.to_f64(fx.lazy["pnext"][k].fractions())
        assert k == 0 or not np.array_equal(D[k], D[k - 1])


def test_audit_rejects_inexact_inputs():
    """The condition has teeth: a sum whose |terms| reach 2^(53 - q) and a non-dyadic value fail."""
    v = lambda *x: np.array([Fraction(t) for t in x], dtype=object)
    au = R.Audit()
    au.dot(v(Fraction(1, 4), 2 ** 51), v(1, 1), Fraction(2 ** 51) + Fraction(1, 4))
    assert au.q == 2 and not au.holds()
    au = R.Audit()
    au.dot(v(Fraction(1, 4), 2 ** 50), v(1, 1), Fraction(2 ** 50) + Fraction(1, 4))
    assert au.q == 2 and au.holds()
    au = R.Audit()
    au.dot(R.Dy.of([0.25, 2.0 ** 51]), R.Dy.of([1.0, 1.0]), R.Dy.of(2.0 ** 51 + 0.25))
    assert au.q == 2 and not au.holds()
    assert np.array_equal(R.Dy.of([0.75, -3.0]).fractions(), v(Fraction(3, 4), -3))
    with pytest.raises(AssertionError):
        R.Audit().values(Fraction(1, 3))


@pytest.mark.parametrize("n", R.SPD_SIZES)
def test_fp64_lazy_algebra_attains_accuracy_bound(oracle, n):
    """The random fixtures of the GPU accuracy test: an fp64 restatement of the lazy algebra with
    sequential sums stays within e <= 8 max(e_oracle, 4 eps) of the longdouble product form, for D
    after six updates and for every pnext -- the bound is attainable by the algebra alone."""
    fx = R.spd_fixture(n)
    for y, s, g in fx.steps:
        assert y @ s > 0
    p_ref, D_ref = R.spd_reference(n)
    p_orc, D_orc = R.oracle_chain(oracle, fx)
    lazy = R.LazyModel(n, float)
    lazy.ident()
    p_lazy = [np.array(lazy.update(y, s, g)) for y, s, g in fx.steps]
    R.accuracy_bound(f"n={n} D", lazy.get(), D_orc, D_ref)
    for k in range(len(fx.steps)):
        R.accuracy_bound(f"n={n} pnext[{k}]", p_lazy[k], p_orc[k], p_ref[k])


def test_script_round_trip():
    """Script.parse reads back what the driver's record format holds (status, count, doubles)."""
    sc = R.Script()
    sc.new(0, 2, 2)
    sc.direction(0, [1.0, 2.0])
    sc.get(0)
    raw = np.array([0, 0, 0, 2, -1.0, -2.0, 1, 0], dtype="<f8").tobytes()
    out = sc.parse(raw)
    assert [t for t, _ in out] == [False, False, True]
    assert np.array_equal(out[1][1], [-1.0, -2.0]) and out[2][1].size == 0
    with pytest.raises(AssertionError):
        sc.parse(raw + raw[:8])


def test_driver_compiles(tmp_path):
    """tests/cpp/dense_hessian_ops.cpp as C++17, warnings as errors (compile only)."""
    pkg = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(pkg, "csrc"), "-I", os.path.join(pkg, "csrc", "host"), "-c",
                    os.path.join(ROOT, "tests", "cpp", "dense_hessian_ops.cpp"),
                    "-o", str(tmp_path / "dense_hessian_ops.o")], check=True)
