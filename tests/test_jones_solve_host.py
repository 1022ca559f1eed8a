"""CPU tests of the Jones solve on a resident model (``simulate_vis_jones_solve``, ``fv_jones_solve``,
``fv_jones_normal_rows``): the numpy reference against the already-pinned ``jones_refs.chi2_jones`` and against the
properties of the iteration and of the rank rule, the C surface, and the argument errors raised before any engine exists
or any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import jones_refs
from tests import jones_solve_refs as jsr
from tests.gain_solve_refs import used_weights
from tests.test_derivative_api_host import _cfg, _vis
from tests.test_jones_host import _case, _shapes


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def per_row(J, nt):
    return np.broadcast_to(J, (J.shape[0], nt) + J.shape[2:])


def jones_case(noise, leakage=0.05, seed=0, nant=8, lead=(2, 2), cross=1.0):
    """``nant`` antennas, all pairs plus autos, a model whose cross-hands are ``cross`` times as strong as its parallel
    hands, data from true time-constant matrices -- diagonal ``1 + 0.3 N(0, 1)``, off-diagonal ``leakage N(0, 1)`` -- and
    noise of standard deviation ``noise``.  Returns (V, d, w, true matrices (nfreqs, 1, 2, 2, nant), a1, a2)."""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(nant, 0)
    a1, a2 = i.astype(np.int32), j.astype(np.int32)
    shape = lead + (2, 2, len(a1))

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    V = c(shape)
    V[..., 0, 1, :] *= cross
    V[..., 1, 0, :] *= cross
    J = leakage * c(lead[:1] + (1, 2, 2, nant))
    for f in range(2):
        J[..., f, f, :] = 1 + 0.3 * c(lead[:1] + (1, nant))
    d = jones_refs.apply_jones(V, per_row(J, lead[1]), a1, a2) + noise * c(shape) / np.sqrt(2)
    return V, d, np.ones(shape), J, a1, a2


def test_reference_normal_systems_are_the_pinned_jones_gradient():
    """With the autos flagged ``gjones[:, c, a] = 2 (A Gamma_a[:, c] - b)``."""
    for seed in (0, 5):
        V, d, w, J, a1, a2 = _case(seed)
        assert (a1 == a2).any() and (w == 0).any() and np.isnan(d).any()
        A, b = jsr.normal_sums(V, d, w, J, a1, a2)
        gj = jones_refs.chi2_jones(V, d, used_weights(V, w, a1, a2), J, a1, a2)[3]
        worst = float(np.abs(jsr.gradient(A, b, J) - gj).max() / np.abs(gj).max())
        print("jones solve reference: 2 (A Gamma - b) against gjones", worst)
        assert A.shape == J.shape[:2] + (4, 2, J.shape[-1]) and A.dtype == np.float64 and b.shape == J.shape and worst <= 1e-12
        assert np.all(A[..., -1] == 0) and np.all(b[..., -1] == 0)  # (the last antenna has no baseline)
        det = A[..., 0, :, :] * A[..., 1, :, :] - A[..., 2, :, :] ** 2 - A[..., 3, :, :] ** 2
        assert np.all(det >= -1e-13 * A[..., 0, :, :] * A[..., 1, :, :])  # (Cauchy-Schwarz)
        both = jsr.normal_sums(V, d, w, J, a1, a2, with_abs=True)
        assert np.array_equal(both[0], A) and np.array_equal(both[1], b)
        assert np.all(both[2] >= np.abs(A) * (1 - 1e-14)) and np.all(both[3] >= np.abs(b) * (1 - 1e-14))


def test_true_matrices_on_noiseless_data_are_a_fixed_point():
    V, d, w, J, a1, a2 = jones_case(0.0, leakage=0.3)
    for max_iter in (1, 2):
        got, changes, chi2, solved, _ = jsr.solve(V, d, w, J, a1, a2, False, max_iter, 0.0)
        print("jones solve reference: fixed point", max_iter, float(changes[-1].max()), float(chi2.max()))
        assert solved.all() and changes[-1].max() <= 1e-13 and np.abs(got - J).max() <= 1e-13 and chi2.max() <= 1e-24
    Jt = per_row(J, V.shape[1]).copy()  # per-time matrices: every (frequency, time) on its own
    got, changes, _, solved, _ = jsr.solve(V, d, w, Jt, a1, a2, True, 1, 0.0)
    assert got.shape == Jt.shape and changes[0].shape == V.shape[:2] and solved.all() and np.abs(got - Jt).max() <= 1e-13


def test_reference_recovers_the_data_and_lowers_chi2():
    for leakage in (0.05, 0.3):
        V, d, w, J, a1, a2 = jones_case(0.0, leakage=leakage)
        eye = jones_refs.diagonal(np.ones((2, 1, 2, 8), complex))
        got, changes, chi2, solved, _ = jsr.solve(V, d, w, eye, a1, a2, False, 200, 1e-10)
        used = used_weights(V, w, a1, a2) > 0
        worst = float(np.abs(jones_refs.apply_jones(V, per_row(got, 2), a1, a2) - d)[used].max())
        print("jones solve reference: recovery", leakage, len(changes), worst)
        assert len(changes) < 200 and solved.all() and worst <= 1e-8
    V, d, w, J, a1, a2 = jones_case(0.05, seed=1)
    start = jsr.chi2_rows(V, d, w, per_row(eye, 2), a1, a2).sum()
    values = [start] + [jsr.solve(V, d, w, eye, a1, a2, False, n, 0.0)[2].sum() for n in (1, 2, 5, 40)]
    print("jones solve reference: chi2 on noisy data", values)
    assert values[-1] < 0.1 * start and values[-1] <= min(values)


def test_reference_is_slow_with_weak_cross_hands():
    """The figures the documentation quotes: with cross-hands at 10 % of the parallel hands the leakage terms are barely
    constrained; with cross-hands as strong as the parallel hands the same cases converge in about fifty iterations."""
    eye = jones_refs.diagonal(np.ones((2, 1, 2, 8), complex))
    slow, counts = [], []
    for leakage, seed in ((0.05, 0), (0.05, 1), (0.3, 2)):
        V, d, w, _, a1, a2 = jones_case(0.0, leakage, seed, cross=0.1)
        changes = jsr.solve(V, d, w, eye, a1, a2, False, 400, 1e-10)[1]
        assert len(changes) == 400
        slow.append(float(changes[-1].max()))
        V, d, w, _, a1, a2 = jones_case(0.0, leakage, seed)
        counts.append(len(jsr.solve(V, d, w, eye, a1, a2, False, 400, 1e-10)[1]))
    print("jones solve reference: change at iteration 400 with weak cross-hands", slow, "iterations with strong ones", counts)
    assert all(5e-8 < c < 3e-5 for c in slow) and all(46 <= n <= 52 for n in counts)


def test_rank_rule():
    V, d, w, J, a1, a2 = jones_case(0.05, seed=2)
    nt = V.shape[1]
    # an antenna without used samples: neither column is solved, the matrix keeps its bits
    w0 = w.copy()
    w0[..., (a1 == 3) | (a2 == 3)] = 0
    got, _, _, solved, (A, b) = jsr.solve(V, d, w0, J, a1, a2, False, 3, 0.0)
    assert not solved[..., 3].any() and solved.sum() == solved.size - 4 and np.array_equal(got[..., 3], J[..., 3])
    assert np.all(A[..., 3] == 0) and np.all(b[..., 3] == 0)
    # a column with one used sample: antenna 5's only baseline is (2, 5), where it is a2 and its feed is x; of column
    # x = 1 one of the two samples is flagged at the one time that is used
    w1 = w.copy()
    w1[..., ((a1 == 5) | (a2 == 5)) & ~((a1 == 2) & (a2 == 5))] = 0
    k = int(np.flatnonzero((a1 == 2) & (a2 == 5))[0])
    w1[:, 1:, :, :, k] = 0
    w1[:, 0, 1, 0, k] = 0
    got, _, _, solved, (A, b) = jsr.solve(V, d, w1, J, a1, a2, False, 3, 0.0)
    assert solved[..., 0, 5].all() and not solved[..., 1, 5].any() and solved.sum() == solved.size - 2
    assert np.array_equal(got[:, :, :, 1, 5], J[:, :, :, 1, 5]) and not np.array_equal(got[:, :, :, 0, 5], J[:, :, :, 0, 5])
    a00, a11 = A[..., 0, 1, 5], A[..., 1, 1, 5]
    det = a00 * a11 - A[..., 2, 1, 5] ** 2 - A[..., 3, 1, 5] ** 2
    print("jones solve reference: det of a rank-one column over A00 A11", float(np.abs(det / (a00 * a11)).max()))
    assert np.all(a00 > 0) and np.all(a11 > 0) and np.all(np.abs(det) <= 34 * 2.0**-52 * a00 * a11)
    # a diagonal model with flagged cross-hands: every column is rank one and nothing is solved
    Vd, wd = V.copy(), w.copy()
    Vd[..., 0, 1, :] = Vd[..., 1, 0, :] = 0
    wd[..., 0, 1, :] = wd[..., 1, 0, :] = 0
    D = jones_refs.diagonal(J[..., [0, 1], [0, 1], :])
    got, changes, _, solved, (A, _) = jsr.solve(Vd, d, wd, D, a1, a2, False, 2, 0.0)
    assert not solved.any() and np.array_equal(got, D) and not changes[-1].any()
    assert np.all(A[..., 0, 0, :] > 0) and np.all(A[..., 1, 1, :] > 0)  # (each column sees its own parallel hand only)
    assert np.abs(per_row(got, nt) - per_row(D, nt)).max() == 0


_NEW = {"fv_jones_normal_rows": 13, "fv_jones_solve": 22}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_jones_normal_rows\(int device, int precision, int64_t nrows, int64_t nbls, int nant, "
                     r"const int \*ant1,\s+const int \*ant2,\s+const void \*jones, const void \*vis, const void \*data, "
                     r"const void \*weights,\s+double \*A_out,\s+void \*b_out\);", header, re.M)
    assert re.search(r"^int fv_jones_solve\(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int nant, "
                     r"const int \*ant1,\s+const int \*ant2,\s+int per_time, const void \*vis, int vis_on_device, "
                     r"const void \*data, int data_on_device,\s+const void \*weights,\s+int weights_on_device, void \*jones, "
                     r"int max_iter, double tol, int \*niter_out,\s+double \*change_out,\s+double \*chi2_ft_out, "
                     r"int \*solved_out\);", header, re.M)
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    gain = _lib.SYMBOLS["fv_gain_solve"][1]
    assert _lib.SYMBOLS["fv_jones_solve"][1] == gain[:5] + gain[6:]  # (fv_gain_solve argument for argument, without tpol)
    flat = " ".join(header.split()).replace(" * ", " ")
    for stated in ("A[i, j] += w[x, y] conj(Z[i, y]) Z[j, y] b[i] += w[x, y] conj(Z[i, y]) d[x, y]",
                   "A[i, j] += w[x, y] Y[x, i] conj(Y[x, j]) b[i] += w[x, y] Y[x, i] conj(d[x, y])",
                   "gjones[:, c, a] = 2 (A Gamma_a[:, c] - b)", "det = A00 A11 - |A01|^2 > 2^-30 A00 A11",
                   "Gamma <- Gamma^ for odd i and (Gamma^ + Gamma) / 2 for even i",
                   "change[unit] = max |new - old| / max |new|"):
        assert stated in flat, stated


def test_exported_with_the_gain_solve_s_signature():
    own = inspect.signature(adjoint.simulate_vis_jones_solve).parameters
    gain = inspect.signature(adjoint.simulate_vis_gain_solve).parameters
    assert [("jones" if n == "gains" else n) for n in gain] == list(own)
    assert all(own["jones" if n == "gains" else n].kind == gain[n].kind and own["jones" if n == "gains" else n].default == gain[n].default
               for n in gain)
    assert fftvis_amd.simulate_vis_jones_solve is adjoint.simulate_vis_jones_solve
    doc = " ".join(adjoint.simulate_vis_jones_solve.__doc__.split())
    for word in ("StefCal", "polarized=True", "det A > 2^-30 A00 A11", "simulate_vis_gain_solve", "common unitary factor",
                 "7e-8 to 2e-5 at iteration 400", "Not differentiable", "explicit ``baselines``", "a joint sky and Jones solve",
                 "sharding"):
        assert word in doc, word
    for fn in (adjoint.simulate_vis_jones_chi2, adjoint.simulate_vis_gain_solve):
        assert "simulate_vis_jones_solve" in fn.__doc__


def _call(data=None, **changes):
    cfg = dict(_cfg(), polarized=True)
    cfg.update(changes)
    return adjoint.simulate_vis_jones_solve(_vis(cfg) if data is None else data, **cfg)


def test_bad_arguments():
    import torch

    cfg = dict(_cfg(), polarized=True)
    const, per_time = _shapes(cfg)
    nant, nf = const[0], const[-1]
    shape = _vis(cfg).shape
    ones = np.ones(const, complex)
    with _raises(ValueError, "jones needs polarized=True: a 2 x 2 matrix per antenna mixes the two feeds"):
        adjoint.simulate_vis_jones_solve(_vis(_cfg()), **_cfg())
    for bad in ((nant, 2, nf), const[:-1], const + (1, 1), (nant + 1,) + const[1:], per_time[:-1] + (per_time[-1] + 1,),
                (2, 2, nant, nf)):
        with _raises(ValueError, f"jones must have shape {const} or {per_time}, got {bad}"):
            _call(jones=np.ones(bad, complex))
    with _raises(ValueError, "jones must be complex (one 2 x 2 matrix per antenna and channel)"):
        _call(jones=np.ones(const))
    for value in (np.nan, complex(1, np.inf)):
        j = np.ones(per_time, complex)
        j[(0,) * j.ndim] = value
        with _raises(ValueError, "jones must be finite"):
            _call(jones=j)
    with _raises(ValueError, f"per_time=True needs per-time jones of shape {per_time}, got {const}"):
        _call(jones=ones, per_time=True)
    with _raises(ValueError, f"data must have simulate_vis's output shape {shape}, got {shape[:-1]}"):
        _call(data=np.zeros(shape[:-1], complex))
    with _raises(ValueError, f"weights must have data's shape {shape}, got {shape[1:]}"):
        _call(weights=np.ones(shape[1:]))
    with _raises(ValueError, "weights must be real (inverse variances; 0 flags a sample)"):
        _call(weights=np.ones(shape, complex))
    for model in (np.zeros(shape[:-1] + (shape[-1] + 1,), complex), torch.zeros(shape[1:], dtype=torch.complex128)):
        with _raises(ValueError, f"model must have simulate_vis's output shape {shape}, got {tuple(model.shape)}"):
            _call(model=model)

    class Elsewhere(torch.Tensor):  # (what _run_device looks at, without a second GPU -- or any)
        device = torch.device("cuda", 1)

    with _raises(ValueError, "model lives on cuda:1, the run is on cuda:0"):
        _call(model=torch.zeros(shape, dtype=torch.complex128).as_subclass(Elsewhere))
    with _raises(ValueError, "data lives on cuda:1, the run is on cuda:0"):
        _call(data=torch.zeros(shape, dtype=torch.complex128).as_subclass(Elsewhere))
    with _raises(ValueError, "weights lives on cuda:1, the run is on cuda:0"):
        _call(weights=torch.ones(shape, dtype=torch.float64).as_subclass(Elsewhere))
    with _raises(ValueError, "ref_ant must be a key of ants, got 1000"):
        _call(ref_ant=1000)
    for bad in (0, -3, 2.5):
        with _raises(ValueError, f"max_iter must be a positive integer, got {bad!r}"):
            _call(max_iter=bad)
    for bad in (-1e-3, float("nan")):
        with _raises(ValueError, f"tol must be non-negative, got {bad!r}"):
            _call(tol=bad)
    with _raises(ValueError, "fluxes must have shape (nsources, nfreqs[, 4])"):  # (without model= the forward's checks)
        _call(fluxes=np.ones((3, 3)))
    with pytest.raises(TypeError, match="gains"):
        _call(gains=np.ones((nant, 2, nf), complex))
    with pytest.raises(TypeError, match="jones"):
        adjoint.simulate_vis_gain_solve(_vis(cfg), **dict(cfg, jones=ones))


def test_a_valid_call_reaches_the_engine(monkeypatch):
    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)
    cfg = dict(_cfg(), polarized=True)
    for kw in (dict(), dict(per_time=True), dict(jones=np.ones(_shapes(cfg)[1], complex), per_time=True, ref_ant=0, tol=0.0)):
        with pytest.raises(Reached):
            _call(**kw)


def test_the_start_and_the_result_keep_their_layout():
    """The block the library takes and the shapes that come back, without a device."""
    from types import SimpleNamespace

    nant, nf, nt = 3, 2, 4
    run = SimpleNamespace(ants={10: 0, 11: 0, 12: 0}, nfreqs=nf, ntimes=nt, args=dict(polarized=True), cdt=np.complex128)
    block, shape, own = adjoint._jones_solve_start(run, None, True)
    assert block.shape == (nf, nt, 2, 2, nant) and shape == (nant, 2, 2, nf, nt) and own
    assert np.array_equal(block, jones_refs.diagonal(np.ones((nf, nt, 2, nant), complex)))
    rng = np.random.default_rng(0)
    j = rng.normal(size=(nant, 2, 2, nf)) + 1j * rng.normal(size=(nant, 2, 2, nf))
    block, shape, own = adjoint._jones_solve_start(run, j, False)
    assert block.shape == (nf, 1, 2, 2, nant) and shape == j.shape and not own and block.flags.c_contiguous
    assert all(block[f, 0, i, c, a] == j[a, i, c, f] for f in range(nf) for i in range(2) for c in range(2) for a in range(nant))
    assert np.array_equal(adjoint._jones_solve_result(block, shape), j)


def test_fv_jones_normal_rows_argument_checks():
    L = _lib.lib()
    fn = L.fv_jones_normal_rows
    buf = (ctypes.c_double * 256)()
    a = (ctypes.c_int * 3)(0, 1, 2)

    def call(precision=2, nrows=1, nbls=3, nant=3, a1=a, a2=a, j=buf, v=buf, d=buf, A=buf, b=buf):
        return fn(0, precision, nrows, nbls, nant, a1, a2, j, v, d, None, A, b)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for kw in (dict(nrows=-1), dict(nbls=-1)):
        assert call(**kw) == 1 and b"fv_jones_normal_rows: negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and b"fv_jones_normal_rows: nant must be positive" in L.fv_last_error()
    for kw in (dict(j=None), dict(A=None), dict(b=None)):
        assert call(**kw) == 1 and b"fv_jones_normal_rows: null jones, A_out or b_out" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(v=None), dict(d=None)):
        assert call(**kw) == 1 and b"fv_jones_normal_rows: null pairs, vis or data" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2) == 1 and b"fv_jones_normal_rows: antenna index outside [0, nant)" in L.fv_last_error()
    # no baseline: zeros, without a device; no row: nothing
    A, b = np.full((2, 4, 2, 3), 7.0), np.full((2, 2, 2, 3), 7.0, dtype=complex)
    assert fn(0, 2, 2, 0, 3, None, None, buf, None, None, None, _lib.ptr(A), _lib.ptr(b)) == 0
    assert np.all(A == 0) and np.all(b == 0)
    assert fn(0, 2, 0, 3, 3, a, a, None, None, None, None, None, None) == 0


def test_fv_jones_solve_argument_checks():
    L = _lib.lib()
    fn = L.fv_jones_solve
    buf = (ctypes.c_double * 256)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    niter = (ctypes.c_int * 1)(-1)

    def call(precision=2, nfreqs=1, ntimes=1, nbls=3, nant=3, a1=a, a2=a, per_time=0, v=buf, d=buf, flags=(0, 0, 0), j=buf,
             max_iter=5, tol=1e-8, n=niter, change=buf, chi2=buf, solved=buf):
        return fn(0, precision, nfreqs, ntimes, nbls, nant, a1, a2, per_time, v, flags[0], d, flags[1], None, flags[2], j,
                  max_iter, tol, n, change, chi2, solved)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for kw in (dict(nfreqs=-1), dict(ntimes=-1), dict(nbls=-1)):
        assert call(**kw) == 1 and b"fv_jones_solve: negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and b"fv_jones_solve: nant must be positive" in L.fv_last_error()
    for bad in (0, -1):
        assert call(max_iter=bad) == 1 and b"fv_jones_solve: max_iter must be positive" in L.fv_last_error()
    for bad in (-1e-9, float("nan")):
        assert call(tol=bad) == 1 and b"fv_jones_solve: tol must be non-negative" in L.fv_last_error()
    for kw in (dict(per_time=2), dict(flags=(2, 0, 0)), dict(flags=(0, -1, 0)), dict(flags=(0, 0, 3))):
        assert call(**kw) == 1 and b"fv_jones_solve: per_time and the on_device flags must be 0 or 1" in L.fv_last_error()
    assert call(n=None) == 1 and b"fv_jones_solve: null niter_out" in L.fv_last_error()
    for kw in (dict(j=None), dict(change=None), dict(chi2=None), dict(solved=None)):
        assert call(**kw) == 1 and b"fv_jones_solve: null jones, change_out, chi2_ft_out or solved_out" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(v=None), dict(d=None)):
        assert call(**kw) == 1 and b"fv_jones_solve: null pairs, vis or data" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2) == 1 and b"fv_jones_solve: antenna index outside [0, nant)" in L.fv_last_error()
    assert niter[0] == -1  # (nothing ran)
    # no baseline: the start matrices, chi2 0, nothing solved, without a device
    j = np.arange(2 * 3 * 4 * 3, dtype=complex).reshape(2, 3, 2, 2, 3) + 1j
    start = j.copy()
    change, chi2, solved = np.full((2, 3), 7.0), np.full((2, 3), 7.0), np.full((2, 3, 2, 3), 7, dtype=np.int32)
    assert fn(0, 1, 2, 3, 0, 3, None, None, 1, None, 0, None, 0, None, 0, _lib.ptr(j), 5, 0.0, niter, _lib.ptr(change),
              _lib.ptr(chi2), _lib.ptr(solved)) == 0, L.fv_last_error()
    assert niter[0] == 0 and np.array_equal(j, start) and not change.any() and not chi2.any() and not solved.any()
