"""The input builders of tests/dense_fixtures.py do what tests/test_gpu_dense_anchor.py assumes
(CPU only)."""
import numpy as np
import pytest

import dense_fixtures as DF

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("n,h", [(300, 140), (200, 64), (130, 100), (64, 30), (5, 2)])
def test_exact_spd_plain_cholesky_reproduces_L_bitwise(n, h):
    A, x, b, L = DF.exact_spd(n, h, seed=n + h)
    assert np.array_equal(A, A.T)
    Lc, first = DF.plain_cholesky(A)
    assert first == -1
    assert np.array_equal(Lc, L)
    # pivots: powers of four; the solve by substitution returns the integer x exactly
    piv = np.diag(L) ** 2
    assert np.array_equal(np.log2(piv) % 2, np.zeros(n))
    z = np.zeros(n)
    for i in range(n):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    s = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s[i] = (z[i] - L[i + 1:, i] @ s[i + 1:]) / L[i, i]
    assert np.array_equal(s, x)
    assert np.abs(A).max() < 2.0 ** 30 and np.abs(b).max() < 2.0 ** 40   # far below 2^53


@pytest.mark.parametrize("n,p", [(200, 0), (200, 63), (200, 64), (200, 65), (200, 128), (200, 191), (200, 199),
                                 (130, 129)])
def test_broken_spd_first_bad_pivot_is_p(n, p):
    A, _ = DF.broken_spd(n, p, seed=n)
    A0, _ = DF.random_spd(n, seed=n)
    assert np.array_equal(A[:p, :p], A0[:p, :p]) and np.array_equal(A, A.T)
    L, first = DF.plain_cholesky(A)
    assert first == p
    piv = A[p, p] - L[p, :p] @ L[p, :p]
    assert abs(piv + 1.0) < 1e-8
    assert DF.plain_cholesky(A0)[1] == -1


def test_plain_cholesky_stops_at_nan_pivot():
    A, _ = DF.random_spd(200, seed=200)
    A[150, 150] = np.nan
    assert DF.plain_cholesky(A)[1] == 150


@pytest.mark.parametrize("n", [130, 700])
@pytest.mark.parametrize("cond", [1e2, 1e6, 1e10])
def test_graded_spd_condition_and_refined_reference(n, cond):
    A, b = DF.graded_spd(n, cond, seed=n)
    assert np.array_equal(A, A.T)
    ev = np.linalg.eigvalsh(A)
    assert ev[0] > 0 and abs(ev[-1] / ev[0] / cond - 1) < 1e-3
    assert np.finfo(np.longdouble).nmant >= 63
    x5, x6 = DF.refined_solve(A, b, 5), DF.refined_solve(A, b, 6)
    # the reference has converged: one more refinement moves it by far less than the fp64
    # solves' errors it is compared with (~ cond * eps)
    assert DF.rel_err(x6, x5) <= 1e-3 * cond * EPS
    # and its residual is at the extended format's rounding level
    r = b.astype(np.longdouble) - A.astype(np.longdouble) @ x5
    eps_ld = float(np.finfo(np.longdouble).eps)
    assert float(np.abs(r).max()) <= 4 * n * eps_ld * float(np.abs(A).max() * np.abs(x5).max())
    # an fp64 LAPACK Cholesky solve sits at the level the GPU solve is held to
    e = DF.rel_err(DF.lapack_cholesky_solve(A, b), x5)
    assert 0 < e <= cond * EPS * n


def test_normal_equations_exact_is_integer_arithmetic():
    J, F = DF.int_matrix(5000, 3, 1), DF.int_vector(5000, 2)
    for lam in (0.0, 0.5):
        A, d, rhs = DF.normal_equations_exact(J, F, lam)
        Ji, Fi = J.astype(np.int64), F.astype(np.int64)
        G = Ji.T @ Ji
        assert np.array_equal(d, np.diag(G).astype(np.float64))
        assert np.array_equal(rhs, -(Ji.T @ Fi).astype(np.float64))
        off = ~np.eye(3, dtype=bool)
        assert np.array_equal(A[off], G[off].astype(np.float64))
        assert np.array_equal(np.diag(A) * 2, (np.diag(G) * (2 if lam == 0 else 3)).astype(np.float64))
    assert np.abs(J).max() == 3 and np.abs(F).max() == 3


@pytest.mark.parametrize("n", [50, 300])
def test_lu_exchange_builders(n):
    A, _ = DF.lu_zero_first(n, seed=n)
    piv, before = DF.plain_lu_pivots(A)
    assert before[0] == 0.0 and piv[0] != 0
    A, _ = DF.lu_last_exchange(n, seed=n)
    piv, before = DF.plain_lu_pivots(A)
    assert before[n - 2] == 0.0 and piv[n - 2] == n - 1
    assert np.linalg.matrix_rank(A) == n


@pytest.mark.parametrize("n", [50, 300])
def test_equal_rows_singular(n):
    A, _ = DF.equal_rows_singular(n, seed=n)
    assert np.array_equal(A[n - 1], A[n // 3])
    assert np.linalg.matrix_rank(A) == n - 1
