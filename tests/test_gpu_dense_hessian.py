"""pnol::DenseInverseHessian (csrc/host/dense_hessian.{hpp,cpp}), the state machine every fast-mode
BFGS solver keeps its inverse Hessian in, against a dense reference.  Run on an MI355X:
pytest -m gpu.

The class takes y, s and g directly, so nothing here goes through a forward-difference gradient:
on the dyadic fixtures of tests/dense_hessian_reference.py (every value and every sum exact in
fp64 in any order -- tests/test_dense_hessian_cpu.py proves the condition) the results are
array_equal to the Fraction product-form model; the host shortcuts of the lazy identity are held
bit for bit to the device path over a stored diagonal; lent storage is held bit for bit to a
stand-alone object; and random inputs are held to a few ulp of a longdouble model.

Each test writes one script, replays it with tests/cpp/dense_hessian_ops.cpp in one child process
(built once per module) and compares what came back.
"""
import os
import subprocess

import numpy as np
import pytest

import dense_hessian_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dense_hessian_ops") / "dense_hessian_ops")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                    "-I", os.path.join(PKG, "csrc", "host"),
                    os.path.join(ROOT, "tests", "cpp", "dense_hessian_ops.cpp"), "-L", PKG, "-lpnol_amd", "-pthread",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    return exe


def _run(driver, script, tmp_path):
    """Replay the script in one child process: [(threw, fp64 array)] per op."""
    src, dst = tmp_path / "script.bin", tmp_path / "results.bin"
    src.write_bytes(script.tobytes())
    r = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return script.parse(dst.read_bytes())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _assert_none_threw(out, skip=()):
    for k, (threw, _) in enumerate(out):
        assert threw == (k in skip), f"op {k}"


def _assert_model(out, mirror):
    """Every result the Mirror has an expectation for equals the model's, converted to fp64
    without rounding."""
    assert mirror.want
    for k, want in mirror.want.items():
        threw, got = out[k]
        assert not threw, f"op {k}"
        assert np.array_equal(got, R.to_f64(np.asarray(want).reshape(-1))), f"op {k}"


def _assert_same_bits(out, ops_a, ops_b):
    assert len(ops_a) == len(ops_b) and ops_a
    for ka, kb in zip(ops_a, ops_b):
        (ta, a), (tb, b) = out[ka], out[kb]
        assert not ta and not tb, (ka, kb)
        assert a.size == b.size and a.size > 0, (ka, kb)
        assert _bits(a) == _bits(b), (ka, kb, int(np.sum(a.view(np.uint64) != b.view(np.uint64))))


# ---- (a) exact results on dyadic fixtures --------------------------------------------------------
@pytest.mark.parametrize("n,updates", R.DYADIC_CASES)
def test_exact_on_dyadic_fixtures(driver, tmp_path, n, updates):
    """From I and from diag(2^e): p before any update, every pnext, a direction after an update made
    without gnext (pending over the diagonal, and pending over a stored D), getMatrix after 1, 2
    and k updates, a second getMatrix straight after, a direction and an update after getMatrix --
    in fast mode (2), exact mode (1) and auto (0: exact at n = 5, fast at 65 and 130): all equal
    the Fraction product-form model."""
    mr, oid = R.Mirror("fraction"), 0
    flags = {}
    for scaled in (False, True):
        fx = R.dyadic_fixture(n, updates, scaled)
        for mode in (2, 1, 0):
            # A: pnext of every update, then D
            mr.new(oid, n, mode)
            flags[mr.script.exact(oid)] = mode == 1 or (mode == 0 and n <= R.SEQ_MAX)
            mr.ident(oid, fx.scale)
            mr.direction(oid, fx.g)
            for y, s, g in fx.steps:
                mr.update(oid, y, s, g)
            mr.get(oid)
            mr.get(oid)
            mr.direction(oid, fx.g)
            oid += 1
            # B: updates without gnext, each followed by direction, D, D again, direction
            mr.new(oid, n, mode)
            mr.ident(oid, fx.scale)
            for y, s, g in fx.steps:
                mr.update(oid, y, s)
                mr.direction(oid, g)
                mr.get(oid)
                mr.get(oid)
                mr.direction(oid, fx.g)
            oid += 1
        # C: a correction pending over a stored D when direction / getMatrix come (fast mode)
        mr.new(oid, n, 2)
        mr.ident(oid, fx.scale)
        (y0, s0, _), rest = fx.steps[0], fx.steps[1:]
        mr.update(oid, y0, s0)
        for y, s, g in rest:
            mr.update(oid, y, s, g)
        mr.direction(oid, fx.g)
        mr.get(oid)
        oid += 1
    out = _run(driver, mr.script, tmp_path)
    _assert_none_threw(out)
    for k, want in flags.items():
        assert out[k][1][0] == float(want)
    _assert_model(out, mr)


# ---- (b) the host shortcuts against the device path ---------------------------------------------
def _shortcut_sequences(sc, fx, make):
    """The four op sequences of (b) on fresh objects from make(); the op indices with results."""
    ops = []
    (y0, s0, g0), (y1, s1, g1), (y2, s2, g2) = fx.steps[:3]
    o = make()
    ops.append(sc.direction(o, fx.g))
    o = make()
    ops += [sc.update(o, y0, s0, g0), sc.update(o, y1, s1, g1), sc.update(o, y2, s2, g2), sc.get(o)]
    o = make()
    sc.update(o, y0, s0)
    ops += [sc.direction(o, g0), sc.get(o)]
    o = make()
    ops.append(sc.update(o, y0, s0, g0))
    ops.append(sc.get(o))
    ops += [sc.update(o, y1, s1, g1), sc.direction(o, fx.g), sc.get(o)]
    return ops


class _Ids:
    def __init__(self):
        self.next = 0

    def __call__(self):
        self.next += 1
        return self.next - 1


@pytest.mark.parametrize("n", [5, 65, 130])
def test_identity_shortcuts_bitwise_device_path(driver, tmp_path, n):
    """The same ops on a lazy `ident [scale]` object (direction() on a diagonal, updateIdentFused,
    the 0.0 + d_i v_i products, the synthesised diagonal of the first fold) and on an object given
    diag(scale) with setMatrix (a real pass over a real matrix): every p, pnext and D bit for bit,
    on random y, s, g with y.s > 0 -- and on vectors that also hold +0.0 and -0.0 (with one
    negative scale entry), where the sign of an exact zero is the only thing that can differ."""
    sc, ids = R.Script(), _Ids()
    pairs = []
    for scaled, zeros in ((False, False), (True, False), (False, True), (True, True)):
        fx = R.random_fixture(n, 3, seed=7 * n + scaled, scaled=scaled, zeros=zeros)
        diag = np.diag(np.ones(n) if fx.scale is None else fx.scale)

        def lazy():
            o = ids()
            sc.new(o, n, 2)
            sc.ident(o, fx.scale)
            return o

        def stored():
            o = ids()
            sc.new(o, n, 2)
            sc.setmatrix(o, diag)
            return o

        pairs.append((_shortcut_sequences(sc, fx, lazy), _shortcut_sequences(sc, fx, stored)))
    out = _run(driver, sc, tmp_path)
    _assert_none_threw(out)
    for a, b in pairs:
        _assert_same_bits(out, a, b)


# ---- (c) non-finite operands ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 130])
def test_non_finite_operands_take_device_path(driver, tmp_path, n):
    """g with one inf (on the diagonal and with a correction pending), gnext with one NaN, y with
    one inf, scale with one inf: the lazy object leaves its shortcuts and poisons exactly as the
    device path over a stored diagonal does -- identical bytes, NaN positions included (ordinary
    data: no value is asserted beyond that)."""
    sc, ids = R.Script(), _Ids()
    fx = R.random_fixture(n, 2, seed=31 * n, scaled=True)
    (y0, s0, g0), (y1, s1, g1) = fx.steps
    k = n // 2

    def poisoned(v, x):
        v = v.copy()
        v[k] = x
        return v

    def case(make, which):
        ops = []
        if which == "g":
            o = make(fx.scale)
            ops.append(sc.direction(o, poisoned(fx.g, np.inf)))
            sc.update(o, y0, s0)
            ops += [sc.direction(o, poisoned(fx.g, -np.inf)), sc.direction(o, fx.g), sc.get(o)]
        elif which == "gnext":
            o = make(fx.scale)
            ops += [sc.update(o, y0, s0, poisoned(g0, np.nan)), sc.update(o, y1, s1, g1), sc.get(o)]
        elif which == "y":
            o = make(fx.scale)
            ops += [sc.update(o, poisoned(y0, np.inf), s0, g0), sc.direction(o, fx.g), sc.get(o)]
        else:
            o = make(poisoned(fx.scale, np.inf))
            ops += [sc.direction(o, fx.g), sc.update(o, y0, s0, g0), sc.direction(o, fx.g), sc.get(o)]
        return ops

    def lazy(scale):
        o = ids()
        sc.new(o, n, 2)
        sc.ident(o, scale)
        return o

    def stored(scale):
        o = ids()
        sc.new(o, n, 2)
        sc.setmatrix(o, np.diag(scale))
        return o

    pairs = [(w, case(lazy, w), case(stored, w)) for w in ("g", "gnext", "y", "scale")]
    out = _run(driver, sc, tmp_path)
    _assert_none_threw(out)
    for w, a, b in pairs:
        _assert_same_bits(out, a, b)
        assert not np.all(np.isfinite(np.concatenate([out[i][1] for i in a]))), w


# ---- (d) setSubmatrixOf from every source state --------------------------------------------------
@pytest.mark.parametrize("n,updates", R.DYADIC_CASES)
def test_submatrix_from_every_source_state(driver, tmp_path, n, updates):
    """idx a sorted random subset (about 60 %, first and last index kept) of a source that is the
    lazy identity, a lazy diag(scale), a diagonal with a pending correction, a stored matrix with a
    pending correction, and a stored matrix with nothing pending: the result's D is
    D_exact[idx][:, idx], its direction -D_sub g (for the lazy diagonal -scale[idx] g exactly), and
    the source still gives the exact direction and D afterwards."""
    fx = R.dyadic_fixture(n, updates, True)
    rng = np.random.default_rng(n)
    keep = rng.random(n) < 0.6
    keep[0] = keep[-1] = True
    if keep.all():
        keep[n // 2] = False
    idx = np.flatnonzero(keep)
    m = len(idx)
    assert 2 <= m < n
    gsub = fx.steps[0][2][idx]
    (y0, s0, _), (y1, s1, _) = fx.steps[:2]
    mr = R.Mirror("fraction")

    def prepare(src, state):
        mr.new(src, n, 2)
        mr.ident(src, None if state == "identity" else fx.scale)
        if state in ("diag+pending", "stored+pending", "stored"):
            mr.update(src, y0, s0)
        if state in ("stored+pending", "stored"):
            mr.update(src, y1, s1)
        if state == "stored":
            mr.get(src)

    lazy_p = None
    for k, state in enumerate(("identity", "diag", "diag+pending", "stored+pending", "stored")):
        src, sub = 2 * k, 2 * k + 1
        prepare(src, state)
        mr.new(sub, m, 2)
        mr.submatrix(sub, src, idx)
        p = mr.direction(sub, gsub)
        if state == "diag":
            lazy_p = p
        mr.get(sub)
        mr.direction(sub, gsub)
        mr.direction(src, fx.g)
        mr.get(src)
        mr.direction(src, fx.g)
    out = _run(driver, mr.script, tmp_path)
    _assert_none_threw(out)
    _assert_model(out, mr)
    assert np.array_equal(out[lazy_p][1], -(fx.scale[idx] * gsub))


# ---- (e) lending -----------------------------------------------------------------------------------
def _life(sc, o, fx, nsteps=3):
    """ident scale -> updates with gnext -> getMatrix -> direction; the op indices with results."""
    sc.ident(o, fx.scale)
    ops = [sc.update(o, y, s, g) for y, s, g in fx.steps[:nsteps]]
    return ops + [sc.get(o), sc.direction(o, fx.g)]


def _busy_parent(sc, o, n, seed):
    """A parent with a random stored matrix, one folded update and one pending."""
    fx = R.random_fixture(n, 2, seed=seed, scaled=False)
    rng = np.random.default_rng(seed + 1)
    sc.new(o, n, 2)
    sc.setmatrix(o, np.eye(n) + rng.standard_normal((n, n)))
    for y, s, g in fx.steps:
        sc.update(o, y, s, g)
    return fx


def test_lent_storage_shows_nothing_of_the_parent(driver, tmp_path):
    """A parent (n = 130, random stored matrix, two updates, the second pending) lends to a child
    (n = 90, mode 2): the child's pnext, D and p are bit for bit a stand-alone object's, the
    parent's direction after the loan throws (D used while lent), and after setIdentity the parent
    is bit for bit a fresh object.  The same for a child larger than its parent's buffer (5 -> 65:
    own storage) and for the innermost level of a chain parent -> child -> grandchild, in fast
    and in exact mode."""
    sc = R.Script()
    same, threw = [], []
    P, C, S, F = 0, 1, 2, 3
    pfx = _busy_parent(sc, P, 130, seed=130)
    cfx = R.random_fixture(90, 3, seed=90)
    sc.child(C, P, 90, 2)
    got = _life(sc, C, cfx)
    sc.new(S, 90, 2)
    same.append((got, _life(sc, S, cfx)))
    sc.drop(C)
    threw.append(sc.direction(P, pfx.g))
    threw.append(sc.get(P))
    ffx = R.random_fixture(130, 3, seed=131)
    got = _life(sc, P, ffx)
    sc.new(F, 130, 2)
    same.append((got, _life(sc, F, ffx)))
    # a child that does not fit its parent's buffer
    P2, C2, S2 = 4, 5, 6
    _busy_parent(sc, P2, 5, seed=5)
    c2fx = R.random_fixture(65, 3, seed=65)
    sc.child(C2, P2, 65, 2)
    got = _life(sc, C2, c2fx)
    sc.new(S2, 65, 2)
    same.append((got, _life(sc, S2, c2fx)))
    sc.drop(C2)
    # parent -> child -> grandchild, as BFGS_Bnd's active-set recursion nests them
    P3, C3, G, SG, GX, SGX = 7, 8, 9, 10, 11, 12
    _busy_parent(sc, P3, 130, seed=133)
    sc.child(C3, P3, 90, 2)
    sc.ident(C3, cfx.scale)
    sc.update(C3, *cfx.steps[0][:2])
    sc.update(C3, *cfx.steps[1])          # a stored matrix and a pending correction in the middle
    gfx = R.random_fixture(40, 3, seed=40)
    sc.child(G, C3, 40, 2)
    got = _life(sc, G, gfx)
    sc.new(SG, 40, 2)
    same.append((got, _life(sc, SG, gfx)))
    sc.drop(G)
    threw.append(sc.direction(C3, cfx.g))
    sc.child(GX, C3, 40, 1)
    got = _life(sc, GX, gfx)
    sc.new(SGX, 40, 1)
    same.append((got, _life(sc, SGX, gfx)))
    sc.drop(GX)
    sc.drop(C3)
    threw.append(sc.direction(P3, pfx.g))
    out = _run(driver, sc, tmp_path)
    _assert_none_threw(out, skip=threw)
    for a, b in same:
        _assert_same_bits(out, a, b)


# ---- (f) accuracy on random inputs -----------------------------------------------------------------
@pytest.mark.parametrize("n", R.SPD_SIZES)
def test_accuracy_against_extended_precision(driver, tmp_path, oracle, n):
    """D0 = I, six updates with s random and y = H s (H SPD, diagonally dominant): with
    e(X) = max |X - X_ref| / max |X_ref| against the longdouble product-form model,
    e(D_class) <= 8 max(e(D_oracle), 4 eps) and the same for every pnext against -D_ref g, where
    the oracle is the CPU restatement's update_hessian_inv chain (fp64, reference operation
    order).  Measured ratios: DESIGN.md "BFGS inverse-Hessian state"."""
    fx = R.spd_fixture(n)
    p_ref, D_ref = R.spd_reference(n)
    p_orc, D_orc = R.oracle_chain(oracle, fx)
    sc = R.Script()
    sc.new(0, n, 2)
    sc.ident(0)
    ups = [sc.update(0, y, s, g) for y, s, g in fx.steps]
    get = sc.get(0)
    out = _run(driver, sc, tmp_path)
    _assert_none_threw(out)
    R.accuracy_bound(f"n={n} D", out[get][1].reshape(n, n), D_orc, D_ref)
    for k, op in enumerate(ups):
        R.accuracy_bound(f"n={n} pnext[{k}]", out[op][1], p_orc[k], p_ref[k])


# ---- (g) exact mode through the class ----------------------------------------------------------------
def test_exact_mode_bitwise_oracle(driver, tmp_path, oracle):
    """Mode 1 at n = 5, 64 and 65 and mode 0 at n = 64 are exact, mode 0 at n = 65 and mode 2 are
    not; ident scale -> update -> direction in exact mode at n <= 64 (the lazy identity written out
    by ensureDevice before the reference-order kernels run) gives the oracle's
    update_hessian_inv(diag(scale), y, s) and -matvec(D, g) bit for bit."""
    sc = R.Script()
    checks, flags = [], []
    # (n, mode, exact?, compared): at n = 65 the direction's sums are no longer in reference order
    cases = [(5, 1, True, True), (64, 1, True, True), (64, 0, True, True), (65, 1, True, False),
             (65, 0, False, False), (65, 2, False, False), (5, 2, False, False)]
    for o, (n, mode, exact, compared) in enumerate(cases):
        sc.new(o, n, mode)
        flags.append((sc.exact(o), exact))
        if not compared:
            continue
        fx = R.random_fixture(n, 1, seed=1000 * mode + n)
        y, s, g = fx.steps[0]
        sc.ident(o, fx.scale)
        sc.update(o, y, s)
        D = oracle.update_hessian_inv(np.diag(fx.scale), y, s)
        checks.append((sc.direction(o, g), -oracle.matvec(D, g)))
        checks.append((sc.get(o), D.reshape(-1)))
    out = _run(driver, sc, tmp_path)
    _assert_none_threw(out)
    for k, want in flags:
        assert out[k][1][0] == float(want), k
    for k, want in checks:
        assert _bits(out[k][1]) == _bits(want), k
