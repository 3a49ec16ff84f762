"""CPU-only input builders and references for tests/test_gpu_dense_anchor.py.

Every builder is deterministic in its seed.  The integer / dyadic builders give inputs on which
each product and sum of the operation under test is exact in fp64, so the expected result is
numpy's and the comparison is array_equal; tests/test_dense_fixtures.py proves the properties
the GPU tests rely on.
"""
import numpy as np


def int_matrix(rows, cols, seed, lo=-3, hi=3):
    """rows x cols float64 matrix of integers in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(rows, cols)).astype(np.float64)


def int_vector(n, seed, lo=-3, hi=3):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=n).astype(np.float64)


def normal_equations_exact(J, F, lam):
    """(A, diag, rhs) of the LM normal equations for an integer J, F and a dyadic lambda:
    A = J^T J with A_ii = (1 + lam) (J^T J)_ii, diag = diag(J^T J), rhs = -J^T F.  All exact
    (|sums| <= 9 m, far below 2^53)."""
    JTJ = J.T @ J
    A = JTJ.copy()
    d = np.diag(JTJ).copy()
    A[np.diag_indices_from(A)] = (1.0 + lam) * d
    return A, d, -(J.T @ F)


def exact_spd(n, h, seed):
    """(A, x, b, L): A = L L^T with L = (I + N) diag(d), N nonzero only in rows >= h and columns
    < h (integers in [-2, 2]), d powers of two in [2^-3, 2^3]; x integer in [-3, 3]; b = A x.
    Every pivot of A's Cholesky is a power of four and every intermediate a small dyadic
    rational, so a correct fp64 Cholesky solve in any tile order returns x exactly."""
    rng = np.random.default_rng(seed)
    N = np.zeros((n, n))
    if 0 < h < n:
        N[h:, :h] = rng.integers(-2, 3, size=(n - h, h))
    d = 2.0 ** rng.integers(-3, 4, size=n)
    L = (np.eye(n) + N) * d[None, :]
    A = L @ L.T
    x = rng.integers(-3, 4, size=n).astype(np.float64)
    return A, x, A @ x, L


def random_spd(n, seed):
    """(A, b): A = J^T J + 0.5 I with J (n + 40) x n standard normal; b standard normal."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((n + 40, n))
    A = J.T @ J + 0.5 * np.eye(n)
    return (A + A.T) / 2, rng.standard_normal(n)


def graded_spd(n, cond, seed):
    """(A, b): A = Q diag(logspace(0, -log10 cond, n)) Q^T, symmetrised; b standard normal."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -np.log10(cond), n)
    A = (Q * s[None, :]) @ Q.T
    return (A + A.T) / 2, rng.standard_normal(n)


def broken_spd(n, p, seed):
    """(A, b): random_spd(n, seed) with A[p, p] replaced by A[p,:p] A[:p,:p]^{-1} A[:p,p] - 1, so
    the leading minors before p are unchanged and pivot p of a Cholesky is -1 up to rounding."""
    A, b = random_spd(n, seed)
    A = A.copy()
    s = float(A[p, :p] @ np.linalg.solve(A[:p, :p], A[:p, p])) if p > 0 else 0.0
    A[p, p] = s - 1.0
    return A, b


def plain_cholesky(A):
    """Plain-loop (left-looking, row by row) fp64 Cholesky.  Returns (L, first) where first is the
    index of the first non-positive (or NaN) pivot, or -1; L is valid up to that row."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        piv = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not piv > 0.0:
            return L, j
        L[j, j] = np.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, -1


def refined_solve(A, b, iters=5):
    """x = A^{-1} b: numpy.linalg.solve refined `iters` times with extended-precision residuals."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "np.longdouble is not an extended type here"
    Al, bl = A.astype(ld), b.astype(ld)
    x = np.linalg.solve(A, b).astype(ld)
    for _ in range(iters):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(ld)
    return x


def rel_err(x, x_ref):
    """|x - x_ref| / |x_ref| (2-norms), evaluated in x_ref's precision."""
    d = x.astype(x_ref.dtype) - x_ref
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(x_ref * x_ref)))


def lapack_cholesky_solve(A, b):
    import scipy.linalg as sl
    return sl.cho_solve(sl.cho_factor(A, lower=True), b)


def lu_zero_first(n, seed):
    """(A, b): standard normal with A[0, 0] = 0 (a row exchange at the first column)."""
    rng = np.random.default_rng(seed)
    A, b = rng.standard_normal((n, n)), rng.standard_normal(n)
    A[0, 0] = 0.0
    return A, b


def lu_last_exchange(n, seed):
    """(A, b): standard normal with row n-2 = e_{n-1}.  That row is never a pivot candidate before
    column n-2 and every multiplier on it is 0, so it reaches the last elimination step unchanged:
    the diagonal entry there is exactly 0 before pivoting and rows n-2, n-1 must be exchanged."""
    rng = np.random.default_rng(seed)
    A, b = rng.standard_normal((n, n)), rng.standard_normal(n)
    A[n - 2] = 0.0
    A[n - 2, n - 1] = 1.0
    return A, b


def plain_lu_pivots(A):
    """Partial-pivoting elimination (first maximal |entry| wins).  Returns (piv, diag_before):
    piv[k] the row exchanged into position k, diag_before[k] the diagonal entry before it."""
    M = A.copy()
    n = M.shape[0]
    piv, before = [], []
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        piv.append(p)
        before.append(M[k, k])
        if p != k:
            M[[k, p]] = M[[p, k]]
        if k + 1 < n:
            f = M[k + 1:, k] / M[k, k]
            M[k + 1:, k:] -= f[:, None] * M[k, k:][None, :]
    return piv, before


def equal_rows_singular(n, seed):
    """(A, b): integer matrix in [-3, 3] with two equal rows (exactly singular: the elimination
    meets an exact zero column, whatever the pivot order)."""
    A = int_matrix(n, n, seed)
    A[n - 1] = A[n // 3]
    return A, int_vector(n, seed + 1)
