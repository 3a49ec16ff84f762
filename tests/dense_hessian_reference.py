"""A plain dense model of pnol::DenseInverseHessian's interface (csrc/host/dense_hessian.hpp), the
fixtures of tests/test_dense_hessian_cpu.py and tests/test_gpu_dense_hessian.py, and the script
writer / result reader of the replay driver tests/cpp/dense_hessian_ops.cpp.

DenseModel keeps D as a full matrix: update is the reference product form
(I - rho s y^T) D (I - rho y s^T) + rho s s^T, direction is -D g, submatrix is D[idx][:, idx].  It
runs in fractions.Fraction (exact) or numpy.longdouble.  LazyModel restates the class's own
algebra -- a pending rank-2 correction (s, a, b), folded by the next pass -- with sequential sums,
in Fraction (to prove the two forms equal), in Dy (the same dyadic numbers held as integer arrays,
fast enough to audit the exactness of every fixture each time it is built) or in fp64 (to show
that the accuracy bound of the GPU test is attainable).
"""
import functools
import struct
from fractions import Fraction

import numpy as np

EPS = np.finfo(np.float64).eps
SEQ_MAX = 64   # PNOL_SEQ_MAX (include/pnol_amd.h): mode 0 is exact up to here


# ---- the dense model ---------------------------------------------------------------------------
def _frac_matrix(M):
    out = np.empty(np.shape(M), dtype=object)
    for k, v in np.ndenumerate(np.asarray(M)):
        out[k] = Fraction(v) if isinstance(v, Fraction) else Fraction(float(v))
    return out


class DenseModel:
    """D as a full matrix.  arith "fraction": object arrays of Fraction, every result exact;
    arith "longdouble": numpy.longdouble (at least a 64-bit significand, asserted)."""

    def __init__(self, n, arith):
        assert arith in ("fraction", "longdouble")
        if arith == "longdouble":
            assert np.finfo(np.longdouble).nmant >= 63
        self.n, self.arith, self.D = n, arith, None

    def _vec(self, v):
        return _frac_matrix(v) if self.arith == "fraction" else np.asarray(v, dtype=np.longdouble)

    def ident(self, scale=None):
        d = np.ones(self.n) if scale is None else np.asarray(scale, dtype=np.float64)
        self.setmatrix(np.diag(d))

    def setmatrix(self, M):
        assert np.shape(M) == (self.n, self.n)
        self.D = self._vec(M)

    def direction(self, g):
        return -(self.D.dot(self._vec(g)))

    def update(self, y, s, gnext=None):
        """The product form.  In longdouble the three matrices are formed and multiplied as
        written; in Fraction the same product is evaluated factor by factor through each factor's
        rank-1 part, (I - rho s y^T) D = D - rho s (y^T D), which is the same number exactly and
        O(n^2) (product_form_literal is the n^3 evaluation, compared at small n on the CPU)."""
        y, s = self._vec(y), self._vec(s)
        rho = 1 / y.dot(s)
        if self.arith == "longdouble":
            I = np.eye(self.n, dtype=np.longdouble)
            self.D = (I - rho * np.outer(s, y)).dot(self.D).dot(I - rho * np.outer(y, s)) + rho * np.outer(s, s)
        else:
            E = self.D - np.outer(rho * s, y.dot(self.D))
            self.D = E - np.outer(E.dot(y), rho * s) + np.outer(rho * s, s)
        return None if gnext is None else self.direction(gnext)

    def product_form_literal(self, y, s):
        """(I - rho s y^T) D (I - rho y s^T) + rho s s^T with both n^3 products (not applied)."""
        y, s = self._vec(y), self._vec(s)
        rho = 1 / y.dot(s)
        I = _frac_matrix(np.eye(self.n)) if self.arith == "fraction" else np.eye(self.n, dtype=np.longdouble)
        return (I - rho * np.outer(s, y)).dot(self.D).dot(I - rho * np.outer(y, s)) + rho * np.outer(s, s)

    def get(self):
        return self.D.copy()

    def submatrix(self, src, idx):
        idx = np.asarray(idx)
        assert len(idx) == self.n
        self.D = src.D[np.ix_(idx, idx)].copy()


def to_f64(a):
    """A Fraction / longdouble array as fp64; for a Fraction the conversion must be exact."""
    a = np.asarray(a)
    out = np.array(a, dtype=np.float64)
    if a.dtype == object:
        for k, v in np.ndenumerate(a):
            assert Fraction(float(out[k])) == v, "not an fp64 number"
    return out


# ---- dyadic arrays ---------------------------------------------------------------------------------
class Dy:
    """An array (or scalar) of dyadic rationals N * 2^-e: N a numpy object array of Python ints, so
    every operation is exact and runs in numpy's loops.  The same numbers as Fraction arrays
    (fractions() converts), many times faster; used to audit the dyadic fixtures."""

    __array_priority__ = 1000.0

    def __init__(self, N, e):
        self.N, self.e = np.asarray(N, dtype=object), int(e)

    @classmethod
    def of(cls, a):
        """Exactly the fp64 numbers of a."""
        a = np.asarray(a, dtype=np.float64)
        fr = [Fraction(float(x)) for x in a.ravel()]
        ex = [f.denominator.bit_length() - 1 for f in fr]
        e = max(ex, default=0)
        N = np.empty(len(fr), dtype=object)
        for k, (f, x) in enumerate(zip(fr, ex)):
            N[k] = f.numerator << (e - x)
        return cls(N.reshape(a.shape), e)

    def _align(self, o):
        e = max(self.e, o.e)
        return self.N * (1 << (e - self.e)), o.N * (1 << (e - o.e)), e

    def __add__(self, o):
        a, b, e = self._align(o)
        return Dy(a + b, e)

    def __sub__(self, o):
        a, b, e = self._align(o)
        return Dy(a - b, e)

    def __neg__(self):
        return Dy(-self.N, self.e)

    def __mul__(self, o):
        return Dy(self.N * o.N, self.e + o.e)

    def dot(self, o):
        return Dy(self.N.dot(o.N), self.e + o.e)

    def outer(self, o):
        return Dy(np.outer(self.N, o.N), self.e + o.e)

    @property
    def T(self):
        return Dy(self.N.T, self.e)

    def reciprocal(self):
        """1 / x for a scalar power of two."""
        x = int(self.N)
        assert x > 0 and x & (x - 1) == 0, "y.s is no power of two"
        k = x.bit_length() - 1              # x = 2^(k - e)
        return Dy(1 << max(self.e - k, 0), max(k - self.e, 0))

    def __float__(self):
        return float(Fraction(int(self.N), 1 << self.e))

    def _trailing(self):
        t = int(np.bitwise_or.reduce(self.N.ravel())) if self.N.size else 0
        return (t & -t).bit_length() - 1 if t else None

    def den_exp(self):
        """The largest denominator exponent among the entries."""
        tz = self._trailing()
        return 0 if tz is None else max(self.e - tz, 0)

    def bits(self):
        """An upper bound of numerator bits + denominator bits of any entry."""
        m = max((abs(int(x)) for x in self.N.ravel()), default=0)
        tz = self._trailing() or 0
        return (m >> tz).bit_length() + self.den_exp()

    def absf(self):
        return np.abs(np.array(self.N, dtype=np.float64)) * 2.0 ** -self.e

    def fractions(self):
        out = np.empty(self.N.shape, dtype=object)
        for k, x in np.ndenumerate(self.N):
            out[k] = Fraction(int(x), 1 << self.e)
        return out


def _outer(a, b):
    return a.outer(b) if isinstance(a, Dy) else np.outer(a, b)


def _recip(x):
    return x.reciprocal() if isinstance(x, Dy) else 1 / x


# ---- the class's lazy algebra --------------------------------------------------------------------
def _absf(X):
    return X.absf() if isinstance(X, Dy) else np.abs(np.array(X, dtype=np.float64))


class Audit:
    """Collects what makes a fixture exact in fp64 in any order of summation: every value the class
    forms, and every term of every sum, is a multiple of 2^-q (q = the largest denominator exponent
    registered), and for each sum the |terms| add up to less than 2^(53 - q).  Then every partial
    sum, in any grouping, is a multiple of 2^-q below 2^53 * 2^-q -- an fp64 number -- so no
    addition and no product rounds, fused or not.  Sufficient, not necessary: the terms of a
    product sum are taken as multiples of 1 / (largest denominator x largest denominator), and
    sum |terms| is computed in fp64 and rounded up by 2^-20."""

    def __init__(self):
        self.q, self.max_abs_sum, self.max_bits = 0, 0.0, 0

    def values(self, X):
        """Register Fractions or a Dy (a scalar or an array); returns their largest denominator."""
        if isinstance(X, Dy):
            q = X.den_exp()
            self.q, self.max_bits = max(self.q, q), max(self.max_bits, X.bits())
            return 1 << q
        den = 1
        for x in np.ravel(np.asarray(X, dtype=object)):
            d = x.denominator
            assert d & (d - 1) == 0, "not dyadic"
            den = max(den, d)
            self.max_bits = max(self.max_bits, abs(x.numerator).bit_length() + d.bit_length() - 1)
        self.q = max(self.q, den.bit_length() - 1)
        return den

    def terms(self, den, mag):
        """A sum whose terms are multiples of 1 / den and whose |terms| add up to mag (fp64)."""
        assert den & (den - 1) == 0
        self.q = max(self.q, den.bit_length() - 1)
        self.max_abs_sum = max(self.max_abs_sum, float(mag) * (1 + 2.0 ** -20))

    def dot(self, A, x, out):
        """out = A x (a matrix or a vector A): the terms A_ij x_j and the results."""
        self.terms(self.values(A) * self.values(x), np.max(_absf(A) @ _absf(x)))
        self.values(out)

    def holds(self):
        return self.q <= 53 and self.max_abs_sum < 2.0 ** (53 - self.q)


class LazyModel:
    """The algebra of DenseInverseHessian's fast mode: the stored D plus a pending (s, a, b) meaning
    D + s a^T + b s^T; update() folds the pending correction as the pass kernel does
    ((D_ij + s_i a_j) + b_i s_j), forms u = D y, w = D^T y, v = D g of the folded D, beta = y.u,
    c = rho^2 beta + rho, a = c s - rho w, b = -rho u and p = -(v + s (a.g) + b (s.g)).  The arrays
    are numpy object arrays of Fraction or of Python floats (fp64, unfused), whose dot products add
    in index order, or Dy arrays.  With an Audit (Fraction or Dy) every value and every sum is
    registered."""

    def __init__(self, n, scalar, audit=None):
        assert scalar in (Fraction, float, Dy) and (audit is None or scalar is not float)
        self.n, self.scalar, self.audit = n, scalar, audit
        self.D, self.pend = None, None

    def _arr(self, v):
        if self.scalar is Dy:
            return v if isinstance(v, Dy) else Dy.of(v)
        out = np.empty(np.shape(v), dtype=object)
        for k, x in np.ndenumerate(np.asarray(v)):
            out[k] = x if isinstance(x, Fraction) else self.scalar(float(x))
        return out

    def _dot(self, A, x):
        out = A.dot(x)
        if self.audit:
            self.audit.dot(A, x, out)
        return out

    def ident(self, scale=None):
        self.setmatrix(np.diag(np.ones(self.n) if scale is None else np.asarray(scale, dtype=np.float64)))

    def setmatrix(self, M):
        self.D, self.pend = self._arr(M), None

    def _fold(self):
        if self.pend is None:
            return
        s, a, b = self.pend
        sa, bs = _outer(s, a), _outer(b, s)
        D = (self.D + sa) + bs
        if self.audit:
            au = self.audit
            au.terms(max(au.values(self.D), au.values(sa), au.values(bs)), np.max(_absf(self.D) + _absf(sa) + _absf(bs)))
            au.values(D)
        self.D, self.pend = D, None

    def _p(self, v, g):
        """-(v + s (a.g) + b (s.g)) for the pending correction."""
        s, a, b = self.pend
        ag, sg = self._dot(a, g), self._dot(s, g)
        sag, bsg = s * ag, b * sg
        p = -((v + sag) + bsg)
        if self.audit:
            au = self.audit
            au.terms(max(au.values(v), au.values(sag), au.values(bsg)), np.max(_absf(v) + _absf(sag) + _absf(bsg)))
            au.values(p)
        return p

    def direction(self, g):
        g = self._arr(g)
        v = self._dot(self.D, g)
        return -v if self.pend is None else self._p(v, g)

    def update(self, y, s, gnext=None):
        y, s = self._arr(y), self._arr(s)
        self._fold()
        u, w = self._dot(self.D, y), self._dot(self.D.T, y)
        g = None if gnext is None else self._arr(gnext)
        v = None if gnext is None else self._dot(self.D, g)
        ys, beta = self._dot(y, s), self._dot(y, u)
        rho = _recip(ys)
        r2b = rho * rho * beta
        c = r2b + rho
        cs, rw = c * s, rho * w
        a, b = cs - rw, -(rho * u)
        if self.audit:
            au = self.audit
            au.terms(max(au.values(rho), au.values(rho * rho), au.values(r2b)), abs(float(r2b)) + abs(float(rho)))
            au.values(c)
            au.terms(max(au.values(cs), au.values(rw)), np.max(_absf(cs) + _absf(rw)))
            au.values(a)
            au.values(b)
        self.pend = (s, a, b)
        return None if gnext is None else self._p(v, g)

    def get(self):
        self._fold()
        if self.scalar is float:
            return np.array(self.D, dtype=np.float64)
        return self.D if self.scalar is Dy else self.D.copy()


def audit_exact_mode(D, y, s, audit):
    """The reference-order update of exact mode (M1 = I - rho s y^T, M2 = I - rho y s^T,
    M3 = rho s s^T; A = M1 D; D' = A M2 + M3) on a Dy D: registers every entry and, for the two
    matrix products, the terms M1_ik D_kj and A_ik M2_kj.  Returns D'."""
    y, s = Dy.of(y), Dy.of(s)
    ys = y.dot(s)
    audit.dot(y, s, ys)
    rho = ys.reciprocal()
    I = Dy.of(np.eye(len(y.N)))
    rs, ry = rho * s, rho * y
    M1, M2, M3 = I - rs.outer(y), I - ry.outer(s), rs.outer(s)
    A = D - rs.outer(y.dot(D))
    AM2 = A - A.dot(y).outer(rs)
    Dn = AM2 + M3
    dens = [audit.values(M) for M in (rs, ry, M1, M2, M3, D, A, AM2, Dn)]
    audit.terms(dens[2] * dens[5], np.max(M1.absf() @ D.absf()))
    audit.terms(dens[6] * dens[3], np.max(A.absf() @ M2.absf()))
    audit.terms(max(dens[7], dens[4]), np.max(AM2.absf() + M3.absf()))
    return Dn


# ---- dyadic fixtures -----------------------------------------------------------------------------
class Fixture:
    """n, scale (None: D0 = I), steps = [(y, s, gnext)] and a last direction vector g, as fp64
    arrays; a dyadic fixture carries its Audit and the lazy form's exact results (audit_fixture)."""

    def __init__(self, n, scale, steps, g):
        self.n, self.scale, self.steps, self.g, self.audit, self.lazy = n, scale, steps, g, None, None


def _dyadic_candidate(n, updates, scaled, seed, ys):
    rng = np.random.default_rng(seed)
    iv = lambda: rng.integers(-2, 3, size=n).astype(np.float64)
    scale = 2.0 ** rng.integers(-2, 3, size=n) if scaled else None
    steps = []
    for _ in range(updates):
        s, y, g = iv(), iv(), iv()
        k = int(rng.integers(0, n))
        s[k] = 1.0                       # the coordinate of y that makes y.s the power of two
        y[k] += ys - float(y @ s)
        assert float(y @ s) == ys
        steps.append((y, s, g))
    return Fixture(n, scale, steps, iv())


def audit_fixture(fx, exact_mode=True):
    """Run the class's fast-mode algebra in exact dyadic arithmetic (Dy) under one Audit -- a direction on the diagonal,
    then per step update with gnext, a direction with the correction pending, the fold, and a
    direction on the folded D (what a pass after getMatrix sums) -- and, with exact_mode, the
    reference-order update.  Returns (audit, results): results["p0"], ["pnext"], ["ppend"],
    ["pfold"] (lists per step) and ["D"] (after every step) are the lazy form's exact values (Dy)."""
    au = Audit()
    lazy = LazyModel(fx.n, Dy, au)
    lazy.ident(fx.scale)
    De = Dy.of(np.diag(np.ones(fx.n) if fx.scale is None else fx.scale))
    res = {"p0": lazy.direction(fx.g), "pnext": [], "ppend": [], "pfold": [], "D": []}
    for y, s, g in fx.steps:
        res["pnext"].append(lazy.update(y, s, g))
        res["ppend"].append(lazy.direction(fx.g))
        res["D"].append(lazy.get())
        res["pfold"].append(lazy.direction(fx.g))
        if exact_mode:
            De = audit_exact_mode(De, y, s, au)
    return au, res


@functools.lru_cache(maxsize=None)
def dyadic_fixture(n, updates, scaled, seed=0, exact_mode=True):
    """Integer s, y, g in [-2, 2] with one coordinate of y moved so that y.s is a power of two: rho,
    beta, c, a, b and every entry of every D are dyadic.  y.s is the first of 4, 8, 2, 16 (never 1:
    rho = 1 would hide a wrong power of rho) for which the exactness condition of Audit holds over
    everything the class forms (u, w, rho, rho^2 beta, c, a, b, the products s_i a_j and b_i s_j,
    the new D, a.g, s.g, p, and the reference-order products of exact mode); no fixture is
    returned without it."""
    tried = []
    for ys in (4.0, 8.0, 2.0, 16.0):
        fx = _dyadic_candidate(n, updates, scaled, 1000 * n + 10 * seed + scaled, ys)
        au, res = audit_fixture(fx, exact_mode)
        tried.append((ys, au.q, au.max_bits))
        if au.holds():
            fx.audit, fx.lazy = au, res
            return fx
    raise AssertionError(f"no exact dyadic fixture at n={n} updates={updates}: (y.s, q, bits) {tried}")


def fraction_model(fx):
    m = DenseModel(fx.n, "fraction")
    m.ident(fx.scale)
    return m


# ---- random fixtures -----------------------------------------------------------------------------
def random_fixture(n, updates, seed, scaled=True, zeros=False):
    """Random, non-dyadic y, s, g with y.s > 0 (y's sign chosen so) and a random positive scale.
    zeros (n >= 5): coordinates 0..2 of every vector hold signed zeros -- 0 and 1: s = -0 with
    y > 0 and y < 0, g = +0 and -0; 2: s = +0, y = -0 -- and the scale holds -0.0 at 0 and 1 and a
    negative entry at 2, so exact zero products of either sign, zero sums and a zero diagonal entry
    occur: the sign of a zero is then the only thing that can differ between two paths, and the
    only place where the shortcuts' `0.0 +` shows."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.5, 2.0, size=n) if scaled else None
    if zeros:
        assert n >= 5
        if scaled:
            scale[0], scale[1], scale[2] = -0.0, -0.0, -scale[2]
    steps = []
    for _ in range(updates + 1):
        s, y, g = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        if zeros:
            s[0], y[0], g[0] = -0.0, abs(y[0]), 0.0
            s[1], y[1], g[1] = -0.0, -abs(y[1]), -0.0
            s[2], y[2] = 0.0, -0.0
        if y @ s < 0:
            y = -y
        steps.append((y, s, g))
    return Fixture(n, scale, steps[:updates], steps[updates][2])


@functools.lru_cache(maxsize=None)
def spd_fixture(n, updates=6):
    """D0 = I, s random and y = H s for a fixed symmetric, strictly diagonally dominant H with a
    positive diagonal (so SPD: y.s = s^T H s > 0 without cancellation)."""
    rng = np.random.default_rng(4242 + n)
    B = rng.uniform(-1.0, 1.0, size=(n, n))
    H = (B + B.T) / 2
    np.fill_diagonal(H, 0.0)
    np.fill_diagonal(H, np.abs(H).sum(axis=1) + rng.uniform(1.0, 2.0, size=n))
    steps = []
    for _ in range(updates):
        s, g = rng.standard_normal(n), rng.standard_normal(n)
        steps.append((H @ s, s, g))
    return Fixture(n, None, steps, rng.standard_normal(n))


def rel_err(X, X_ref):
    """e(X) = max |X - X_ref| / max |X_ref|, the difference taken in X_ref's precision."""
    X_ref = np.asarray(X_ref)
    return float(np.max(np.abs(np.asarray(X, dtype=X_ref.dtype) - X_ref)) / np.max(np.abs(X_ref)))


@functools.lru_cache(maxsize=None)
def spd_reference(n):
    """The longdouble product-form chain on spd_fixture(n): ([-D_k g_k after update k], D_last)."""
    fx = spd_fixture(n)
    m = DenseModel(n, "longdouble")
    m.ident()
    ps = [m.update(y, s, g) for y, s, g in fx.steps]
    return ps, m.get()


def oracle_chain(oracle, fx):
    """The CPU oracle's update_hessian_inv chain (fp64, reference operation order) on fx:
    ([-matvec(D_k, g_k)], D_last)."""
    D = np.diag(np.ones(fx.n) if fx.scale is None else fx.scale)
    ps = []
    for y, s, g in fx.steps:
        D = oracle.update_hessian_inv(D, y, s)
        ps.append(-oracle.matvec(D, g))
    return ps, D


def accuracy_bound(tag, X, X_oracle, X_ref):
    """e(X) <= 8 max(e(X_oracle), 4 eps): two fp64 algorithms with the same first-order bound
    (the factor of tests/test_gpu_dense_anchor.py).  Prints the figures; returns the ratio."""
    e, eo = rel_err(X, X_ref), rel_err(X_oracle, X_ref)
    ratio = e / max(eo, 4 * EPS)
    print(f"{tag}: e_class {e:.3e} e_oracle {eo:.3e} ratio {ratio:.2f}")
    assert e <= 8 * max(eo, 4 * EPS), (tag, e, eo)
    return ratio


# ---- scripts of the replay driver ------------------------------------------------------------------
class Script:
    """Builds the binary script of tests/cpp/dense_hessian_ops.cpp and parses its results.  Every
    op returns its index into the list parse() gives: (threw, fp64 array)."""

    def __init__(self):
        self.buf, self.count, self.n = [], 0, {}

    def _op(self, code, oid, *parts):
        self.buf.append(struct.pack("<ii", code, oid))
        self.buf.extend(parts)
        self.count += 1
        return self.count - 1

    @staticmethod
    def _d(a, count):
        a = np.ascontiguousarray(a, dtype="<f8")
        assert a.size == count
        return a.tobytes()

    def new(self, oid, n, mode):
        self.n[oid] = n
        return self._op(0, oid, struct.pack("<ii", n, mode))

    def child(self, oid, parent, n, mode):
        self.n[oid] = n
        return self._op(1, oid, struct.pack("<iii", parent, n, mode))

    def drop(self, oid):
        return self._op(2, oid)

    def ident(self, oid, scale=None):
        if scale is None:
            return self._op(3, oid, struct.pack("<i", 0))
        return self._op(3, oid, struct.pack("<i", 1), self._d(scale, self.n[oid]))

    def setmatrix(self, oid, M):
        return self._op(4, oid, self._d(M, self.n[oid] ** 2))

    def direction(self, oid, g):
        return self._op(5, oid, self._d(g, self.n[oid]))

    def update(self, oid, y, s, gnext=None):
        n = self.n[oid]
        parts = [struct.pack("<i", gnext is not None), self._d(y, n), self._d(s, n)]
        if gnext is not None:
            parts.append(self._d(gnext, n))
        return self._op(6, oid, *parts)

    def get(self, oid):
        return self._op(7, oid)

    def submatrix(self, oid, src, idx):
        idx = np.ascontiguousarray(idx, dtype="<i4")
        assert idx.size == self.n[oid]
        return self._op(8, oid, struct.pack("<i", src), idx.tobytes())

    def exact(self, oid):
        return self._op(9, oid)

    def tobytes(self):
        return struct.pack("<i", self.count) + b"".join(self.buf)

    def parse(self, raw):
        a = np.frombuffer(raw, dtype="<f8")
        out, pos = [], 0
        for _ in range(self.count):
            threw, cnt = a[pos] != 0.0, int(a[pos + 1])
            out.append((bool(threw), a[pos + 2:pos + 2 + cnt].copy()))
            pos += 2 + cnt
        assert pos == a.size, "results do not match the script"
        return out


class Mirror:
    """A Script and, op for op, the DenseModel's result: want[k] is the model's p, pnext or matrix
    of op k.  Objects with the same history share one model state (the matrices are never changed
    in place), so a chain of updates is computed once however many objects replay it."""

    def __init__(self, arith="fraction"):
        self.script, self.arith, self.n, self.D, self.want = Script(), arith, {}, {}, {}
        self.memo = {}

    def _memo(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def _model(self, oid):
        m = DenseModel(self.n[oid], self.arith)
        m.D = self.D.get(oid)
        return m

    @staticmethod
    def _b(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()

    def new(self, oid, n, mode):
        self.n[oid] = n
        return self.script.new(oid, n, mode)

    def ident(self, oid, scale=None):
        def make():
            m = self._model(oid)
            m.ident(scale)
            return m.D
        self.D[oid] = self._memo(("ident", self.n[oid], self._b(scale)), make)
        return self.script.ident(oid, scale)

    def setmatrix(self, oid, M):
        m = self._model(oid)
        m.setmatrix(M)
        self.D[oid] = self._memo(("setmatrix", len(self.memo)), lambda: m.D)   # kept alive: ids are keys
        return self.script.setmatrix(oid, M)

    def _direction(self, oid, g):
        return self._memo((id(self.D[oid]), "direction", self._b(g)), lambda: self._model(oid).direction(g))

    def direction(self, oid, g):
        k = self.script.direction(oid, g)
        self.want[k] = self._direction(oid, g)
        return k

    def update(self, oid, y, s, gnext=None):
        k = self.script.update(oid, y, s, gnext)

        def make():
            m = self._model(oid)
            m.update(y, s)
            return m.D
        self.D[oid] = self._memo((id(self.D[oid]), "update", self._b(y), self._b(s)), make)
        if gnext is not None:
            self.want[k] = self._direction(oid, gnext)
        return k

    def get(self, oid):
        k = self.script.get(oid)
        self.want[k] = self.D[oid].reshape(-1)
        return k

    def submatrix(self, oid, src, idx):
        def make():
            m, ms = self._model(oid), self._model(src)
            m.submatrix(ms, idx)
            return m.D
        self.D[oid] = self._memo((id(self.D[src]), "submatrix", np.asarray(idx, dtype=np.int64).tobytes()), make)
        return self.script.submatrix(oid, src, idx)


# the dyadic fixtures of the GPU tests: (n, updates); each from I and from diag(2^e)
DYADIC_CASES = [(5, 4), (65, 4), (130, 3)]
SPD_SIZES = [65, 130]
