"""CPU tests of the gain solve on a resident model (``simulate_vis_gain_solve``, ``fv_gain_solve``,
``fv_gain_normal_rows``): the numpy reference against the already-pinned ``gain_refs.chi2_gains`` and against the properties
of the iteration, the C surface, and the argument errors raised before any engine exists or any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import gain_refs
from tests import gain_solve_refs as gsr
from tests.test_derivative_api_host import _cfg, _vis
from tests.test_gains_host import _case, _shapes


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def solve_case(polarized, noise, seed=0, nant=8, lead=(2, 2), flag_cross=True):
    """``nant`` antennas, all pairs plus autos, data from true time-constant gains ``1 + 0.3 N(0, 1)`` and noise of standard
    deviation ``noise``; polarized: cross-hand model visibilities at 10 % of the parallel hands, flagged with ``flag_cross``.
    Returns (V, d, w, true gains (nfreqs, 1, nfeed, nant), a1, a2)."""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(nant, 0)
    a1, a2 = i.astype(np.int32), j.astype(np.int32)
    shape = lead + ((2, 2, len(a1)) if polarized else (len(a1),))

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    V = c(shape)
    w = np.ones(shape)
    if polarized:
        V[..., 0, 1, :] *= 0.1
        V[..., 1, 0, :] *= 0.1
        if flag_cross:
            w[..., 0, 1, :] = 0
            w[..., 1, 0, :] = 0
    g = 1 + 0.3 * c(lead[:1] + (1, 2 if polarized else 1, nant))
    d = gain_refs.apply_gains(V, np.broadcast_to(g, lead + g.shape[2:]), a1, a2) + noise * c(shape) / np.sqrt(2)
    return V, d, w, g, a1, a2


@pytest.mark.parametrize("polarized", [False, True])
def test_reference_normal_sums_are_the_pinned_gain_gradient(polarized):
    """With the autos flagged ``ggains = 2 (den g - num)``."""
    for seed in (0, 5):
        V, d, w, g, a1, a2 = _case(polarized, seed)
        assert (a1 == a2).any() and (w == 0).any() and np.isnan(d).any()
        num, den = gsr.normal_sums(V, d, w, g, a1, a2)
        gg = gain_refs.chi2_gains(V, d, gsr.used_weights(V, w, a1, a2), g, a1, a2)[3]
        worst = float(np.abs(2 * (den * g - num) - gg).max() / np.abs(gg).max())
        print("gain solve reference: 2 (den g - num) against ggains", polarized, worst)
        assert num.shape == g.shape and den.shape == g.shape and den.dtype == np.float64 and worst <= 1e-12
        assert np.all(den[..., -1] == 0) and np.all(num[..., -1] == 0)  # (the last antenna has no baseline)
        both = gsr.normal_sums(V, d, w, g, a1, a2, with_abs=True)
        assert np.array_equal(both[0], num) and np.all(both[2] >= np.abs(num) * (1 - 1e-14))


def test_reference_chi2_does_not_increase_on_noisy_data():
    V, d, w, g, a1, a2 = solve_case(False, 0.05)
    g0 = np.ones_like(g)
    start = gsr.chi2_rows(V, d, w, np.broadcast_to(g0, V.shape[:2] + g0.shape[2:]), a1, a2).sum()
    values = [start] + [gsr.solve(V, d, w, g0, a1, a2, False, n, 0.0)[2].sum() for n in range(1, 41)]
    print("gain solve reference: chi2 per iteration", values[:6], values[-1])
    # strictly down while chi2 is still above its floor by more than the sum's own rounding (2 * 2 * 36 terms, each to a
    # few ulps: 1e-13 relative); once it has stalled there, a rise of that rounding is all that is allowed
    moving = [a - values[-1] > 1e-13 * a for a in values[:-1]]
    assert sum(moving) >= 30 and moving == sorted(moving, reverse=True)
    assert all(b < a if m else b <= a * (1 + 1e-13) for a, b, m in zip(values, values[1:], moving))
    assert values[-1] < 0.05 * start


def test_reference_crawls_with_cross_hands_and_converges_with_them_flagged():
    """The figures the documentation quotes: cross-hand model visibilities at 10 % of the parallel hands leave the phase
    between the feeds barely constrained."""
    counts = {}
    for flag_cross, max_iter in ((True, 200), (False, 400)):
        V, d, w, g, a1, a2 = solve_case(True, 0.0, flag_cross=flag_cross)
        _, changes, _, _ = gsr.solve(V, d, w, np.ones_like(g), a1, a2, False, max_iter, 1e-10)
        counts[flag_cross] = (len(changes), [float(c.max()) for c in changes])
    print("gain solve reference: cross-hands flagged", counts[True][0], "unflagged after 200 and 400", counts[False][1][199],
          counts[False][1][-1])
    assert abs(counts[True][0] - 56) <= 1 and counts[True][1][-1] < 1e-10
    slow = counts[False][1]
    assert counts[False][0] == 400 and 1e-5 < slow[199] < 2e-5 and 5e-7 < slow[-1] < 6e-7


@pytest.mark.parametrize("polarized", [False, True])
def test_reference_converges_to_a_stationary_point(polarized):
    V, d, w, g, a1, a2 = solve_case(polarized, 0.05, seed=1)
    g0 = np.ones_like(g)
    wu = gsr.used_weights(V, w, a1, a2)

    def gradient(x):  # of the time-constant gains: the per-time gradients added
        return gain_refs.chi2_gains(V, d, wu, np.broadcast_to(x, V.shape[:2] + x.shape[2:]), a1, a2)[3].sum(axis=1)

    got, changes, chi2, solved = gsr.solve(V, d, w, g0, a1, a2, False, 1000, 1e-12)
    ratio = float(np.linalg.norm(gradient(got)) / np.linalg.norm(gradient(g0)))
    print("gain solve reference: iterations, gradient ratio", polarized, len(changes), ratio)
    assert len(changes) < 1000 and changes[-1].max() < 1e-12 and ratio <= 1e-8
    assert got.shape == g0.shape and chi2.shape == V.shape[:2] and solved.all()


def test_reference_per_time_units_are_independent_solves():
    V, d, w, g, a1, a2 = solve_case(True, 0.05, seed=2)
    w[0, 1, ..., a1 == 3] = 0  # antenna 3 has no used sample in unit (0, 1)
    w[0, 1, ..., a2 == 3] = 0
    g0 = np.ones(V.shape[:2] + g.shape[2:], dtype=complex)
    got, changes, chi2, solved = gsr.solve(V, d, w, g0, a1, a2, True, 7, 0.0)
    assert len(changes) == 7 and changes[0].shape == V.shape[:2]
    assert not solved[0, 1, :, 3].any() and solved.sum() == solved.size - 2 and np.all(got[0, 1, :, 3] == 1)
    one, _, chi2_one, _ = gsr.solve(V[1:, :1], d[1:, :1], w[1:, :1], g0[1:, :1], a1, a2, True, 7, 0.0)
    assert np.array_equal(one, got[1:, :1]) and np.array_equal(chi2_one, chi2[1:, :1])


_NEW = {"fv_gain_normal_rows": 14, "fv_gain_solve": 23}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_gain_normal_rows\(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, "
                     r"const int \*ant1,\s+const int \*ant2, const void \*gains, const void \*vis, const void \*data, "
                     r"const void \*weights, void \*num,\s+double \*den\);", header, re.M)
    assert re.search(r"^int fv_gain_solve\(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, "
                     r"const int \*ant1,\s+const int \*ant2, int per_time, const void \*vis, int vis_on_device, "
                     r"const void \*data, int data_on_device,\s+const void \*weights, int weights_on_device, void \*gains, "
                     r"int max_iter, double tol, int \*niter_out,\s+double \*change_out, double \*chi2_ft_out, "
                     r"int \*solved_out\);", header, re.M)
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    flat = " ".join(header.split()).replace(" * ", " ")
    for stated in ("side 0 (a = ant1[k], f = p, every q): num += w g[q, ant2] V conj(d) den += w |g[q, ant2]|^2 |V|^2",
                   "side 1 (a = ant2[k], f = q, every p): num += w g[p, ant1] conj(V) d den += w |g[p, ant1]|^2 |V|^2",
                   "ggains = 2 (den g - num)", "g <- g^ for odd i and (g^ + g) / 2 for even i",
                   "change[unit] = max |g_new - g| / max |g_new|"):
        assert stated in flat, stated


def test_exported_with_the_gain_objective_s_run_keywords():
    own = inspect.signature(adjoint.simulate_vis_gain_solve).parameters
    chi2 = inspect.signature(adjoint.simulate_vis_gain_chi2).parameters
    mine = ["gains", "per_time", "weights", "model", "return_model", "max_iter", "tol", "ref_ant"]
    dropped = {"gains", "weights", "wrt", "chi2_per", "return_gvis", "adjoint_path"}
    names = list(chi2)
    assert list(own) == names[:9] + mine + [n for n in names[9:] if n not in dropped]
    assert all(own[n].kind == chi2[n].kind and own[n].default == chi2[n].default for n in own if n not in mine)
    defaults = dict(gains=None, per_time=False, weights=None, model=None, return_model=False, max_iter=100, tol=1e-8, ref_ant=None)
    assert all(own[n].kind.name == "KEYWORD_ONLY" and own[n].default == v for n, v in defaults.items())
    assert fftvis_amd.simulate_vis_gain_solve is adjoint.simulate_vis_gain_solve
    doc = " ".join(adjoint.simulate_vis_gain_solve.__doc__.split())
    for word in ("Flag the cross-hands (weight 0) to solve each feed on its parallel hand", "autos", "StefCal", "leakage",
                 "a joint sky and gain solve", "``model=`` in ``simulate_vis_gain_chi2`` and ``simulate_vis_gain_gauss_newton``",
                 "sharding", "Not differentiable", "explicit ``baselines``"):
        assert word in doc, word
    for fn in (adjoint.simulate_vis_gain_chi2, adjoint.simulate_vis_gain_gauss_newton):
        assert "simulate_vis_gain_solve" in fn.__doc__ and "keeping V resident" not in " ".join(fn.__doc__.split())


def _call(basis=False, data=None, **changes):
    cfg = _cfg(basis)
    return adjoint.simulate_vis_gain_solve(_vis(cfg) if data is None else data, **dict(cfg, **changes))


@pytest.mark.parametrize("basis", [False, True])
def test_bad_arguments(basis):
    import torch

    cfg = _cfg(basis)
    const, per_time = _shapes(cfg)
    shape = _vis(cfg).shape
    ones = np.ones(const, complex)
    for bad in (const[:-1], const + (1, 1), (const[0] + 1,) + const[1:], per_time[:-1] + (per_time[-1] + 1,)):
        with _raises(ValueError, f"gains must have shape {const} or {per_time}, got {bad}"):
            _call(basis, gains=np.ones(bad, complex))
    with _raises(ValueError, "gains must be complex (one gain per antenna, feed and channel)"):
        _call(basis, gains=np.ones(const))
    for value in (np.nan, complex(1, np.inf)):
        g = np.ones(per_time, complex)
        g[(0,) * g.ndim] = value
        with _raises(ValueError, "gains must be finite"):
            _call(basis, gains=g)
    with _raises(ValueError, f"per_time=True needs per-time gains of shape {per_time}, got {const}"):
        _call(basis, gains=ones, per_time=True)
    with _raises(ValueError, f"data must have simulate_vis's output shape {shape}, got {shape[:-1]}"):
        _call(basis, data=np.zeros(shape[:-1], complex))
    with _raises(ValueError, f"weights must have data's shape {shape}, got {shape[1:]}"):
        _call(basis, weights=np.ones(shape[1:]))
    with _raises(ValueError, "weights must be real (inverse variances; 0 flags a sample)"):
        _call(basis, weights=np.ones(shape, complex))
    for model in (np.zeros(shape[:-1] + (shape[-1] + 1,), complex), torch.zeros(shape[1:], dtype=torch.complex128)):
        with _raises(ValueError, f"model must have simulate_vis's output shape {shape}, got {tuple(model.shape)}"):
            _call(basis, model=model)

    class Elsewhere(torch.Tensor):  # (what _run_device looks at, without a second GPU -- or any)
        device = torch.device("cuda", 1)

    with _raises(ValueError, "model lives on cuda:1, the run is on cuda:0"):
        _call(basis, model=torch.zeros(shape, dtype=torch.complex128).as_subclass(Elsewhere))
    with _raises(ValueError, "data lives on cuda:1, the run is on cuda:0"):
        _call(basis, data=torch.zeros(shape, dtype=torch.complex128).as_subclass(Elsewhere))
    with _raises(ValueError, "weights lives on cuda:1, the run is on cuda:0"):
        _call(basis, weights=torch.ones(shape, dtype=torch.float64).as_subclass(Elsewhere))
    with _raises(ValueError, "ref_ant must be a key of ants, got 1000"):
        _call(basis, ref_ant=1000)
    for bad in (0, -3, 2.5):
        with _raises(ValueError, f"max_iter must be a positive integer, got {bad!r}"):
            _call(basis, max_iter=bad)
    for bad in (-1e-3, float("nan")):
        with _raises(ValueError, f"tol must be non-negative, got {bad!r}"):
            _call(basis, tol=bad)
    with _raises(ValueError, "fluxes must have shape (nsources, nfreqs[, 4])"):  # (without model= the forward's checks)
        _call(basis, fluxes=np.ones((3, 3)))
    if not basis:
        with pytest.raises(ValueError, match="^Basis decomposition is not compatible with unpolarized simulations"):
            _call(basis, beam_coefs=np.ones((len(cfg["ants"]), 1, 2), complex))


def test_a_valid_call_reaches_the_engine(monkeypatch):
    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)
    cfg = _cfg()
    for kw in (dict(), dict(per_time=True), dict(gains=np.ones(_shapes(cfg)[1], complex), per_time=True, ref_ant=0, tol=0.0)):
        with pytest.raises(Reached):
            _call(**kw)


def test_fv_gain_normal_rows_argument_checks():
    L = _lib.lib()
    fn = L.fv_gain_normal_rows
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)

    def call(precision=2, nrows=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, g=buf, v=buf, d=buf, num=buf, den=buf):
        return fn(0, precision, nrows, nbls, tpol, nant, a1, a2, g, v, d, None, num, den)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and b"fv_gain_normal_rows: tpol must be 1 or 4" in L.fv_last_error()
    for kw in (dict(nrows=-1), dict(nbls=-1)):
        assert call(**kw) == 1 and b"fv_gain_normal_rows: negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and b"fv_gain_normal_rows: nant must be positive" in L.fv_last_error()
    for kw in (dict(g=None), dict(num=None), dict(den=None)):
        assert call(**kw) == 1 and b"fv_gain_normal_rows: null gains, num or den" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(v=None), dict(d=None)):
        assert call(**kw) == 1 and b"fv_gain_normal_rows: null pairs, vis or data" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2, tpol=4) == 1 and b"fv_gain_normal_rows: antenna index outside [0, nant)" in L.fv_last_error()
    # no baseline: zeros, without a device
    num, den = np.full((2, 1, 3), 7.0, dtype=complex), np.full((2, 1, 3), 7.0)
    assert fn(0, 2, 2, 0, 1, 3, None, None, buf, None, None, None, _lib.ptr(num), _lib.ptr(den)) == 0
    assert np.all(num == 0) and np.all(den == 0)


def test_fv_gain_solve_argument_checks():
    L = _lib.lib()
    fn = L.fv_gain_solve
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    niter = (ctypes.c_int * 1)(-1)

    def call(precision=2, nfreqs=1, ntimes=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, per_time=0, v=buf, d=buf, flags=(0, 0, 0), g=buf,
             max_iter=5, tol=1e-8, n=niter, change=buf, chi2=buf, solved=buf):
        return fn(0, precision, nfreqs, ntimes, nbls, tpol, nant, a1, a2, per_time, v, flags[0], d, flags[1], None, flags[2], g,
                  max_iter, tol, n, change, chi2, solved)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and b"fv_gain_solve: tpol must be 1 or 4" in L.fv_last_error()
    for kw in (dict(nfreqs=-1), dict(ntimes=-1), dict(nbls=-1)):
        assert call(**kw) == 1 and b"fv_gain_solve: negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and b"fv_gain_solve: nant must be positive" in L.fv_last_error()
    for bad in (0, -1):
        assert call(max_iter=bad) == 1 and b"fv_gain_solve: max_iter must be positive" in L.fv_last_error()
    for bad in (-1e-9, float("nan")):
        assert call(tol=bad) == 1 and b"fv_gain_solve: tol must be non-negative" in L.fv_last_error()
    for kw in (dict(per_time=2), dict(flags=(2, 0, 0)), dict(flags=(0, -1, 0)), dict(flags=(0, 0, 3))):
        assert call(**kw) == 1 and b"fv_gain_solve: per_time and the on_device flags must be 0 or 1" in L.fv_last_error()
    assert call(n=None) == 1 and b"fv_gain_solve: null niter_out" in L.fv_last_error()
    for kw in (dict(g=None), dict(change=None), dict(chi2=None), dict(solved=None)):
        assert call(**kw) == 1 and b"fv_gain_solve: null gains, change_out, chi2_ft_out or solved_out" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(v=None), dict(d=None)):
        assert call(**kw) == 1 and b"fv_gain_solve: null pairs, vis or data" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2, tpol=4) == 1 and b"fv_gain_solve: antenna index outside [0, nant)" in L.fv_last_error()
    assert niter[0] == -1  # (nothing ran)
    # no baseline: the start gains, chi2 0, nothing solved, without a device
    g = np.arange(2 * 3 * 2 * 3, dtype=complex).reshape(2, 3, 2, 3) + 1j
    start = g.copy()
    change, chi2, solved = np.full((2, 3), 7.0), np.full((2, 3), 7.0), np.full(g.shape, 7, dtype=np.int32)
    assert fn(0, 1, 2, 3, 0, 4, 3, None, None, 1, None, 0, None, 0, None, 0, _lib.ptr(g), 5, 0.0, niter, _lib.ptr(change),
              _lib.ptr(chi2), _lib.ptr(solved)) == 0, L.fv_last_error()
    assert niter[0] == 0 and np.array_equal(g, start) and not change.any() and not chi2.any() and not solved.any()
