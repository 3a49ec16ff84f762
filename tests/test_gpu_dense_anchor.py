"""The LM normal-equation kernels and the fused BFGS pass against exact references at the
dispatch edges.  Run on an MI355X: pytest -m gpu.

Most LM kernel tests elsewhere compare one path of the library with another.  Here the expected
values come from numpy (torch fp64 on the device for the large fused-pass cases) on inputs
built by tests/dense_fixtures.py: integer / dyadic inputs make every product and sum exact in
fp64, so the comparison is array_equal and one dropped, doubled or misplaced term fails it.  The
solve's accuracy is measured against an extended-precision reference and held to a small
multiple of an fp64 LAPACK Cholesky's error on the same system.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_fixtures as DF

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import Context
    if L.device_count() < 1:
        pytest.fail("no gfx950 device visible for a -m gpu run")
    return Context(0)


def _np(t):
    return t.cpu().numpy()


# ---- 1. SYRK and -J^T F: exact results at the dispatch edges -----------------------------------
# n <= 64 with m > 4096 (the MFMA path with fewer rows than one MFMA block), m below one m-slice
# (seven empty slices, zero stages), one row / column past a 64- and a 128-tile, odd m.
SHAPES = [(4097, 1), (4097, 64), (5000, 3), (1, 65), (5, 65), (63, 129), (64, 65), (65, 65), (513, 128),
          (513, 129), (1000, 257)]
STRIDED = [(513, 129), (1000, 257)]


@functools.lru_cache(maxsize=None)
def _normal_case(m, n):
    J, F = DF.int_matrix(m, n, 1000 * m + n), DF.int_vector(m, 7 * m + n)
    return J, F, {lam: DF.normal_equations_exact(J, F, lam) for lam in (0.0, 0.5)}


def _check_normal(ctx, JT, F, ref, lam, A=None):
    Aref, dref, rref = ref[lam]
    Ad, diag = ctx.jtj(JT, lam, A=A, want_diag=True)
    rhs = ctx.jtr(JT, F)
    Ah = _np(Ad)
    assert np.array_equal(Ah, Aref)
    assert np.array_equal(Ah, Ah.T)
    assert np.array_equal(_np(diag), dref)
    assert np.array_equal(_np(rhs), rref)


@pytest.mark.parametrize("t64", ["0", "1"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_normal_equations_exact(ctx, monkeypatch, m, n, t64):
    """pnol_jtj_d (A with the Marquardt diagonal, diag(J^T J), symmetry) and pnol_jtr_d on integer
    J, F and lambda in {0, 0.5}: every sum is exact, so both equal numpy's bitwise, with the
    128 x 128 and the 64 x 64 SYRK tiles."""
    monkeypatch.setenv("PNOL_SYRK_T64", t64)
    J, F, ref = _normal_case(m, n)
    JT, Ft = ctx.tensor(J.T.copy()), ctx.tensor(F)
    for lam in (0.0, 0.5):
        _check_normal(ctx, JT, Ft, ref, lam)


@pytest.mark.parametrize("t64", ["0", "1"])
@pytest.mark.parametrize("m,n", STRIDED)
def test_normal_equations_exact_strided_operands(ctx, monkeypatch, m, n, t64):
    """J^T as a view into a wider buffer (odd and even leading dimension, the padding NaN: it must
    never be read), J^T starting 8 bytes past a 16-byte boundary, and A written into a wider
    buffer whose columns >= n keep their sentinel."""
    import torch
    monkeypatch.setenv("PNOL_SYRK_T64", t64)
    J, F, ref = _normal_case(m, n)
    Ft = ctx.tensor(F)
    for pad in (3, 4):
        buf = ctx.tensor(np.full((n, m + pad), np.nan))
        buf[:, :m] = ctx.tensor(J.T.copy())
        JT = buf[:, :m]
        assert JT.stride(0) == m + pad
        _check_normal(ctx, JT, Ft, ref, 0.5)
    flat = ctx.tensor(np.full(n * m + 1, np.nan))
    assert flat.data_ptr() % 16 == 0
    flat[1:] = ctx.tensor(J.T.copy()).reshape(-1)
    JT = flat[1:].view(n, m)
    assert JT.data_ptr() % 16 == 8
    _check_normal(ctx, JT, Ft, ref, 0.5)
    # A into a wider buffer
    Abuf = ctx.tensor(np.full((n, n + 5), -77.0))
    _check_normal(ctx, ctx.tensor(J.T.copy()), Ft, ref, 0.5, A=Abuf[:, :n])
    assert bool(torch.all(Abuf[:, n:] == -77.0))


@pytest.mark.parametrize("m,n", [(5000, 3), (1000, 257)])
def test_jtr_accepts_8_byte_aligned_F(ctx, m, n):
    """pnol_jtr_d's slice GEMV with F 8 bytes past a 16-byte boundary: F is read with 8-byte
    loads and the result is the exact one (it used to be refused with PNOL_ERR_ARG); the same with
    a J^T whose rows are not 16-byte aligned either."""
    J, F, ref = _normal_case(m, n)
    Fbuf = ctx.tensor(np.concatenate([[np.nan], F]))
    Fv = Fbuf[1:]
    assert Fv.data_ptr() % 16 == 8
    JT = ctx.tensor(J.T.copy())
    assert np.array_equal(_np(ctx.jtr(JT, Fv)), ref[0.0][2])
    buf = ctx.tensor(np.full((n, m + 3), np.nan))
    buf[:, :m] = JT
    assert np.array_equal(_np(ctx.jtr(buf[:, :m], Fv)), ref[0.0][2])


def test_lm_small_n_large_m_matches_oracle(ctx, oracle):
    """The LM general loop with n <= 64 and m > 4096 (the MFMA SYRK and the slice GEMV on an
    8-row J^T, then the reference-order LU) against the oracle's loop: the LM contract, 1e-10."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import DeviceObjective, run_levmarq
    m, n = 5000, 8
    A, xs, y = oracle.linres_data(m, n)
    d = DeviceObjective(ctx, L.OBJ_LINRES, n, m, A, y)
    params = (0.001, 10, 1e-7, 6, 0.0, -1)
    X, _, _, _ = run_levmarq(d, np.zeros(n), params)
    Xo, *_ = oracle.lm_findmin(oracle.Obj(oracle.LINRES, n, m, A, y), np.zeros(n), params)
    assert np.max(np.abs(X - Xo)) / np.max(np.abs(Xo)) <= 1e-10


# ---- 2. the damped solve -----------------------------------------------------------------------
def _solve_async(ctx, At, bt):
    """pnol_solve_async_d through ctypes: (sigma, status read back)."""
    import torch
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import _ptr
    n = bt.numel()
    sigma = ctx.empty(n)
    info = torch.zeros(2, dtype=torch.int32, device=f"cuda:{ctx.device}")
    L.check(L.lib().pnol_solve_async_d(ctx.h, _ptr(At), At.stride(0), _ptr(bt), _ptr(sigma), n, _ptr(info)),
            "pnol_solve_async_d")
    return sigma, int(info[0].item())


@pytest.mark.parametrize("n,h", [(300, 140), (200, 64), (130, 100), (64, 30), (5, 2)])
def test_cholesky_exact_on_dyadic_factor(ctx, oracle, n, h):
    """A = L L^T with L = (I + N) diag(powers of two), b = A x for an integer x: every pivot is a
    power of four (the rsq estimate's third-order correction rounds to the exact power of two),
    the diagonal tiles' inverses (I - N_kk) diag(1/d) and every tile product are exact dyadic
    sums, so the tile Cholesky returns x bitwise in any tile order -- methods 4 and 5, method 0
    and pnol_solve_step_d.

    Method 0 at n <= PNOL_SEQ_MAX is by contract the reference-order LU (info 2), not a Cholesky:
    partial pivoting divides by pivots that are no powers of two, so that path is inexact on this
    matrix by design (the CPU oracle's luSolve misses x by 1.3e-9 at (64, 30) and by 2 ulp at
    (5, 2)); there method 0 is held to the LU's own exact contract, bitwise the oracle's."""
    A, x, b, _ = DF.exact_spd(n, h, seed=n + h)
    At, bt = ctx.tensor(A), ctx.tensor(b)
    for method in (4, 5):
        sigma, info = ctx.solve(At, bt, method=method)
        assert info == 1, method
        assert np.array_equal(_np(sigma), x), method
    assert np.array_equal(_np(At), A)
    x0 = DF.int_vector(n, n)
    sigma, xnext, st = ctx.solve_step(At, bt, ctx.tensor(x0))
    assert st == 0
    assert np.array_equal(_np(sigma), x) and np.array_equal(_np(xnext), x0 + x)
    sigma, info = ctx.solve(ctx.tensor(A), bt, method=0)
    if n > 64:
        assert info == 1
        assert np.array_equal(_np(sigma), x)
    else:
        assert info == 2
        assert np.array_equal(_np(sigma), oracle.lusolve(A, b))


@functools.lru_cache(maxsize=None)
def _spd_case(n):
    A, b = DF.random_spd(n, seed=n)
    return A, b, DF.refined_solve(A, b), DF.lapack_cholesky_solve(A, b)


def _accuracy_bound(tag, sigma, x_ref, x_lapack):
    """The bound of the accuracy test: e_gpu <= 8 max(e_lapack, 4 eps)."""
    e_gpu, e_lap = DF.rel_err(sigma, x_ref), DF.rel_err(x_lapack, x_ref)
    print(f"{tag}: e_gpu {e_gpu:.3e} e_lapack {e_lap:.3e} ratio {e_gpu / max(e_lap, 1e-300):.2f}")
    assert e_gpu <= 8 * max(e_lap, 4 * EPS), (tag, e_gpu, e_lap)


@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 127, 128, 129])
def test_cholesky_one_tile_and_first_boundary(ctx, n):
    """T = 1 (n <= 64: only the k = -1 step and the backward launch) and the first tile boundary:
    methods 4 and 5, pnol_solve_step_d and pnol_solve_async_d give the same bits, leave A intact,
    xnext is x + sigma, and the forward error is within the accuracy bound."""
    A, b, x_ref, x_lap = _spd_case(n)
    At, bt = ctx.tensor(A), ctx.tensor(b)
    s4, i4 = ctx.solve(At, bt, method=4)
    s5, i5 = ctx.solve(At, bt, method=5)
    x0 = np.random.default_rng(n).standard_normal(n)
    ss, xn, ist = ctx.solve_step(At, bt, ctx.tensor(x0))
    sa, ia = _solve_async(ctx, At, bt)
    assert i4 == 1 and i5 == 1 and ist == 0 and ia == 0
    s4 = _np(s4)
    assert np.array_equal(_np(s5), s4) and np.array_equal(_np(ss), s4) and np.array_equal(_np(sa), s4)
    assert np.array_equal(_np(At), A)
    assert np.array_equal(_np(xn), x0 + s4)
    _accuracy_bound(f"n={n}", s4, x_ref, x_lap)


@pytest.mark.parametrize("n", [1, 255, 257, 262145])
def test_add_bitwise(ctx, n):
    """pnol_add_d = the host's IEEE add, past the 1024-block grid cap too."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import _ptr
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n) * 1e-3
    xt, yt, z = ctx.tensor(x), ctx.tensor(y), ctx.tensor(np.full(n + 1, np.nan))
    L.check(L.lib().pnol_add_d(ctx.h, _ptr(xt), _ptr(yt), _ptr(z), n), "pnol_add_d")
    ctx.synchronize()
    zh = _np(z)
    assert np.array_equal(zh[:n], x + y) and np.isnan(zh[n])


@functools.lru_cache(maxsize=None)
def _graded_case(n, cond):
    A, b = DF.graded_spd(n, cond, seed=n)
    return A, b, DF.refined_solve(A, b), DF.lapack_cholesky_solve(A, b)


@pytest.mark.parametrize("method", [4, 5])
@pytest.mark.parametrize("cond", [1e2, 1e6, 1e10])
@pytest.mark.parametrize("n", [130, 700])
def test_cholesky_accuracy_vs_extended_reference(ctx, n, cond, method):
    """Graded SPD systems up to cond 1e10 (what a small lambda gives): the forward error against
    an extended-precision reference is at most 8 x that of an fp64 LAPACK Cholesky solve (both are
    rounding-error draws of algorithms with the same first-order bound; LAPACK's own LU and
    Cholesky differ by up to 2.6 x on these inputs).  Measured ratios: DESIGN.md "solve accuracy"."""
    assert np.finfo(np.longdouble).nmant >= 63
    A, b, x_ref, x_lap = _graded_case(n, cond)
    sigma, info = ctx.solve(ctx.tensor(A), ctx.tensor(b), method=method)
    assert info == 1
    _accuracy_bound(f"n={n} cond={cond:.0e} method={method}", _np(sigma), x_ref, x_lap)


@pytest.mark.parametrize("method", [4, 5])
@pytest.mark.parametrize("n", [130, 700])
def test_cholesky_power_of_four_scaling(ctx, n, method):
    """(4^k A) x = 4^k b: every operation of the factorisation and the solves scales by an exact
    power of two (sqrt(4^k) = 2^k), so sigma is bitwise the unscaled one unless a hidden absolute
    threshold exists."""
    A, b, _, _ = _spd_case(n)
    s0, i0 = ctx.solve(ctx.tensor(A), ctx.tensor(b), method=method)
    assert i0 == 1
    for k in (-50, 50):
        c = 4.0 ** k
        s, i = ctx.solve(ctx.tensor(A * c), ctx.tensor(b * c), method=method)
        assert i == 1, k
        assert np.array_equal(_np(s), _np(s0)), k


def _failing_solve_checks(ctx, oracle, capfd, A, b, lu_reference):
    Agood, bgood, _, _ = _spd_case(A.shape[0])
    Ag, bg = ctx.tensor(Agood), ctx.tensor(bgood)
    before, ib = ctx.solve(Ag, bg, method=5)
    assert ib == 1
    capfd.readouterr()
    At, bt = ctx.tensor(A), ctx.tensor(b)
    _, _, st = ctx.solve_step(At, bt, bt)
    assert st != 0 and st != -7, st
    if lu_reference:
        sigma, info = ctx.solve(At, bt, method=0)
        assert info == 2
        assert np.array_equal(_np(sigma), oracle.lusolve(A, b))
    ctx.synchronize()
    assert "relaunch" not in capfd.readouterr().err
    after, ia = ctx.solve(Ag, bg, method=5)
    s2, _, st2 = ctx.solve_step(Ag, bg, bg)
    assert ia == 1 and st2 == 0
    assert np.array_equal(_np(after), _np(before)) and np.array_equal(_np(s2), _np(before))


@pytest.mark.parametrize("n,p", [(200, 0), (200, 63), (200, 64), (200, 65), (200, 128), (200, 191), (200, 199),
                                 (130, 129)])
def test_cholesky_failure_position_sweep(ctx, oracle, capfd, n, p):
    """The first non-positive pivot at p (tile starts, tile ends, the last tile, the last pivot):
    method 0 falls back to the LU (info 2, bitwise the oracle's), pnol_solve_step_d reports a
    status that is no timeout, no wait ran to its cap (no relaunch line: the workers left through
    *info), and the context's next SPD solves give their earlier bits."""
    A, b = DF.broken_spd(n, p, seed=n)
    _failing_solve_checks(ctx, oracle, capfd, A, b, lu_reference=True)


def test_cholesky_nan_pivot(ctx, oracle, capfd):
    """A NaN at A[150, 150], n = 200 (a documented input: a NaN pivot takes the LU branch): a
    nonzero status that is no timeout, no relaunch, and a sound context afterwards."""
    A, b = DF.random_spd(200, seed=200)
    A = A.copy()
    A[150, 150] = np.nan
    _failing_solve_checks(ctx, oracle, capfd, A, b, lu_reference=False)


# ---- LU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_lu_sizes_around_launch_switch_bitwise(ctx, oracle, n):
    rng = np.random.default_rng(n + 300)
    A, b = rng.standard_normal((n, n)), rng.standard_normal(n)
    sigma, info = ctx.solve(ctx.tensor(A), ctx.tensor(b), method=2)
    assert info == 2
    assert np.array_equal(_np(sigma), oracle.lusolve(A, b))


@pytest.mark.parametrize("n", [50, 300])
@pytest.mark.parametrize("builder", ["lu_zero_first", "lu_last_exchange"])
def test_lu_row_exchanges_bitwise(ctx, oracle, builder, n):
    """A zero at A[0, 0], and an exact zero on the diagonal at the last elimination step (rows
    n-2 and n-1 must be exchanged), in the single-launch and the multi-launch form."""
    A, b = getattr(DF, builder)(n, seed=n)
    sigma, info = ctx.solve(ctx.tensor(A), ctx.tensor(b), method=2)
    assert info == 2
    ref = oracle.lusolve(A, b)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(_np(sigma), ref)


@pytest.mark.parametrize("n", [50, 300])
def test_lu_singular_status(ctx, n):
    A, b = DF.equal_rows_singular(n, seed=n)
    _, info = ctx.solve(ctx.tensor(A), ctx.tensor(b), method=2)
    assert info == -1


# ---- 3. fused BFGS pass at the tile heights large n selects --------------------------------------
@pytest.fixture(scope="module")
def pass_cases():
    cache = {}
    yield cache
    cache.clear()


def _pass_case(ctx, cache, n):
    """Integer D and vectors generated on the device, and the exact torch fp64 reference."""
    import torch
    if n not in cache:
        g = torch.Generator(device=f"cuda:{ctx.device}")
        g.manual_seed(n)
        dev = f"cuda:{ctx.device}"
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, device=dev).double()
        D = ri(-3, 3, n, n)
        sp, ap, bp, y, gv = (ri(-2, 2, n) for _ in range(5))
        Dc = D + torch.outer(sp, ap) + torch.outer(bp, sp)
        ref = {False: (D @ y, D.T @ y, D @ gv), True: (Dc @ y, Dc.T @ y, Dc @ gv)}
        cache[n] = (D, (sp, ap, bp), y, gv, Dc, ref)
    return cache[n]


@pytest.mark.parametrize("pending,wb", [(False, False), (True, True), (True, False)])
@pytest.mark.parametrize("n", [8192, 12288])
def test_bfgs_pass_exact_at_large_tile_heights(ctx, pass_cases, n, pending, wb):
    """n = 8192 runs the 256-row tiles and n = 12288, the smallest such n, the 32-row tiles (the
    override is read once per process, so the size cannot shrink): u, w, v and the written D on
    integer inputs equal torch's fp64 results bitwise (|sums| < 2^20: exact)."""
    import torch
    D0, pend, y, g, Dc, ref = _pass_case(ctx, pass_cases, n)
    D = D0.clone()
    u, w, v = ctx.bfgs_pass(D, y, g, pend if pending else None, wb)
    ru, rw, rv = ref[pending]
    assert torch.equal(u, ru) and torch.equal(w, rw) and torch.equal(v, rv)
    assert torch.equal(D, Dc if wb else D0)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n,pad", [(7, 1), (7, 2), (300, 1), (300, 2), (1031, 1), (1031, 2)])
def test_bfgs_pass_ident_padded_leading_dimension_exact(ctx, n, pad, scaled):
    """pnol_bfgs_pass_ident_d with ld = n + 1 and n + 2: one of the two is odd for every n (the
    identity source without vector loads, which no other test runs), the other even.  Bitwise the
    write-back pass over a real identity / diag(scale), and -- integer vectors, powers of two in
    scale -- exactly numpy's u, w, v and D; the never-read D buffer's NaN does not leak in and
    its padding columns stay untouched."""
    from parallelnonlinearoptimizationlibrary_amd import _lib as L
    from parallelnonlinearoptimizationlibrary_amd.device import _ptr
    rng = np.random.default_rng(n + 13 * scaled)
    y, g, sp, ap, bp = (rng.integers(-2, 3, size=n).astype(np.float64) for _ in range(5))
    scale = 2.0 ** rng.integers(-3, 4, size=n) if scaled else None
    ld = n + pad
    st = ctx.tensor(scale) if scaled else None
    pend = (ctx.tensor(sp), ctx.tensor(ap), ctx.tensor(bp))
    yt, gt = ctx.tensor(y), ctx.tensor(g)
    Dref = ctx.empty(n, ld)
    ctx.set_identity(Dref[:, :n], st)
    u0, w0, v0 = (_np(t) for t in ctx.bfgs_pass(Dref[:, :n], yt, gt, pend, True))
    Did = ctx.tensor(np.full((n, ld), np.nan))
    u1, w1, v1 = ctx.empty(n), ctx.empty(n), ctx.empty(n)
    L.check(L.lib().pnol_bfgs_pass_ident_d(ctx.h, _ptr(Did), ld, n, _ptr(st), _ptr(pend[0]), _ptr(pend[1]),
                                           _ptr(pend[2]), _ptr(yt), _ptr(gt), _ptr(u1), _ptr(w1), _ptr(v1)),
            "pnol_bfgs_pass_ident_d")
    ctx.synchronize()
    Dc = np.diag(scale if scaled else np.ones(n)) + np.outer(sp, ap) + np.outer(bp, sp)
    for got, same, exact in ((u1, u0, Dc @ y), (w1, w0, Dc.T @ y), (v1, v0, Dc @ g)):
        assert np.array_equal(_np(got), same) and np.array_equal(_np(got), exact)
    Dh = _np(Did)
    assert np.array_equal(Dh[:, :n], _np(Dref)[:, :n]) and np.array_equal(Dh[:, :n], Dc)
    assert np.all(np.isnan(Dh[:, n:]))
