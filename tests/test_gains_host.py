"""CPU tests of the per-antenna gains in the fused objective (``simulate_vis_gain_chi2``, ``fv_gain_residual_chi2``,
``fv_sim_set_gain_pairs``, ``fv_sim_run_residual_gains``): the numpy references against finite differences of their own
chi2, the C surface, and the argument errors raised before any engine exists or any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import gain_refs
from tests.test_derivative_api_host import _cfg, _vis


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _case(polarized, seed=0, nant=5, nbls=9, lead=(2, 3)):
    rng = np.random.default_rng(seed)
    shape = lead + ((2, 2, nbls) if polarized else (nbls,))

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    a1, a2 = rng.integers(0, nant - 1, nbls), rng.integers(0, nant - 1, nbls)  # (the last antenna has no baseline)
    a1[0] = a2[0] = 1  # an auto-correlation
    V, d, g = c(shape), c(shape), 1 + 0.3 * c(lead + (2 if polarized else 1, nant))
    w = rng.uniform(0.5, 2.0, size=shape)
    flagged = rng.random(shape) < 0.2
    w[flagged] = 0
    d[flagged] = np.nan
    return V, d, w, g, a1, a2


@pytest.mark.parametrize("polarized", [False, True])
def test_reference_gain_gradient_is_the_stencil_of_its_own_chi2(polarized):
    V, d, w, g, a1, a2 = _case(polarized)
    rows, Gp, G, gg = gain_refs.chi2_gains(V, d, w, g, a1, a2)
    assert rows.shape == V.shape[:2] and gg.shape == g.shape and np.all(gg[..., -1] == 0) and np.isfinite(G).all()
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4):
        dg = rng.normal(size=g.shape) + 1j * rng.normal(size=g.shape)
        fd = gain_refs.five_point(lambda h: gain_refs.chi2_gains(V, d, w, g + h * dg, a1, a2)[0].sum(), 0.25)
        an = np.sum(np.conj(gg) * dg).real
        worst = max(worst, abs(fd - an) / abs(an))
    print("gain reference: stencil against ggains", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("polarized", [False, True])
def test_reference_gvis_is_the_derivative_in_v(polarized):
    V, d, w, g, a1, a2 = _case(polarized, seed=3)
    G = gain_refs.chi2_gains(V, d, w, g, a1, a2)[2]
    rng = np.random.default_rng(2)
    dV = rng.normal(size=V.shape) + 1j * rng.normal(size=V.shape)

    def chi2(h):
        return gain_refs.chi2_gains(V + h * dV, d, w, g, a1, a2)[0].sum()

    fd = (chi2(0.5) - chi2(-0.5)) / 1.0  # chi2 is quadratic in V: the central difference is exact up to rounding
    an = np.sum(np.conj(G) * dV).real
    assert abs(fd - an) <= 1e-12 * abs(an)
    assert np.array_equal(gain_refs.apply_gains(V, np.ones_like(g), a1, a2), V)
    used = w != 0
    Vp = gain_refs.apply_gains(V, g, a1, a2)
    assert np.allclose(gain_refs.chi2_gains(V, d, w, g, a1, a2)[1][used], (2 * w * (Vp - d))[used], rtol=1e-15)


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_gain_residual_chi2\(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, "
                     r"const int \*ant1,\s+const int \*ant2, const void \*gains, void \*vis, const void \*data, "
                     r"const void \*weights,\s+double \*chi2_rows, void \*ggains\);", header, re.M)
    assert re.search(r"^int fv_sim_set_gain_pairs\(fv_sim \*h, int nant, const int \*ant1, const int \*ant2\);", header, re.M)
    assert re.search(r"^int fv_sim_run_residual_gains\(fv_sim \*h, int t0, int t1, int f0, int f1, const void \*data, "
                     r"int data_on_device,\s+const void \*weights, int weights_on_device, const void \*gains, "
                     r"int gains_on_device, void \*gvis,\s+int gvis_on_device, double \*chi2_ft, void \*ggains, "
                     r"int ggains_on_device\);", header, re.M)
    arity = {"fv_gain_residual_chi2": 14, "fv_sim_set_gain_pairs": 4, "fv_sim_run_residual_gains": 16}
    for name, n in arity.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_gain_residual) and callable(gpu_simulate.SimHandle.set_gain_pairs)
    plain = inspect.signature(adjoint.simulate_vis_chi2).parameters
    own = inspect.signature(adjoint.simulate_vis_gain_chi2).parameters
    # simulate_vis_chi2's parameters and, first of the keywords, the required gains
    assert list(own) == list(plain)[:9] + ["gains"] + list(plain)[9:]
    assert all(own[n].kind == plain[n].kind and own[n].default == plain[n].default for n in plain)
    assert own["gains"].kind.name == "KEYWORD_ONLY" and own["gains"].default is inspect.Parameter.empty
    assert "gains" not in inspect.signature(adjoint.simulate_vis_gauss_newton).parameters
    assert fftvis_amd.simulate_vis_gain_chi2 is adjoint.simulate_vis_gain_chi2
    for word in ("simulate_vis_gauss_newton", "leakage", "gains in ``simulate_vis`` itself", "sharding", "explicit ``baselines``",
                 "NOT"):
        assert word in adjoint.simulate_vis_gain_chi2.__doc__, word


def _call(basis=False, **changes):
    cfg = _cfg(basis)
    changes.setdefault("gains", None)
    return adjoint.simulate_vis_gain_chi2(_vis(cfg), **dict(cfg, **changes))


def _shapes(cfg):
    nant, nf, nt = len(cfg["ants"]), np.size(cfg["freqs"]), len(cfg["times"])
    lead = (nant, 2) if cfg.get("polarized") else (nant,)
    return lead + (nf,), lead + (nf, nt)


@pytest.mark.parametrize("basis", [False, True])
def test_bad_gains(basis):
    cfg = _cfg(basis)
    const, per_time = _shapes(cfg)
    for bad in (const[:-1], const + (1, 1), (const[0] + 1,) + const[1:], per_time[:-1] + (per_time[-1] + 1,),
                const[1:] + const[:1]):
        with _raises(ValueError, f"gains must have shape {const} or {per_time}, got {bad}"):
            _call(basis, gains=np.ones(bad, complex))
    with _raises(ValueError, "gains must be complex (one gain per antenna, feed and channel)"):
        _call(basis, gains=np.ones(const))
    for value in (np.nan, complex(1, np.inf)):
        g = np.ones(per_time, complex)
        g[(0,) * g.ndim] = value
        with _raises(ValueError, "gains must be finite"):
            _call(basis, gains=g)
    for wrt in ("gains", ("fluxes", "gains")):
        with _raises(ValueError, "wrt='gains' needs gains="):
            _call(basis, wrt=wrt)
    with pytest.raises(ValueError, match="^wrt must name "):
        _call(basis, wrt=("gains", "gains"), gains=np.ones(const, complex))
    with _raises(ValueError, "wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and 'gains', "
                             "got 'antennas'"):
        _call(basis, wrt="antennas", gains=np.ones(const, complex))
    for wrt in ("gains", ("fluxes", "gains")):  # simulate_vis_chi2 itself does not know the name
        with pytest.raises(ValueError, match="^wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs', got"):
            adjoint.simulate_vis_chi2(_vis(cfg), **dict(cfg, wrt=wrt))
    with pytest.raises(TypeError, match="gains"):
        adjoint.simulate_vis_chi2(_vis(cfg), **dict(cfg, gains=np.ones(const, complex)))


def test_torch_entry_point_checks_the_gains_before_an_engine_exists():
    import torch

    cfg = _cfg()
    const, _ = _shapes(cfg)
    F = torch.ones(20, 2, dtype=torch.float64)
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    g = torch.ones(const[:-1], dtype=torch.complex128, requires_grad=True)
    with pytest.raises(ValueError, match=r"^gains must have shape "):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, gains=g, **kw)
    with pytest.raises(ValueError, match=r"^gains must be complex"):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, gains=torch.ones(const, dtype=torch.float64), **kw)


def test_fv_gain_residual_chi2_argument_checks():
    L = _lib.lib()
    fn = L.fv_gain_residual_chi2
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    for precision in (0, 3):
        assert fn(0, precision, 1, 3, 1, 3, a, a, buf, buf, buf, None, buf, None) == 1
        assert b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert fn(0, 2, 1, 3, tpol, 3, a, a, buf, buf, buf, None, buf, None) == 1
        assert b"tpol must be 1 or 4" in L.fv_last_error()
    for nrows, nbls in [(-1, 3), (1, -1)]:
        assert fn(0, 2, nrows, nbls, 1, 3, a, a, buf, buf, buf, None, buf, None) == 1
        assert b"negative shape" in L.fv_last_error()
    assert fn(0, 2, 1, 3, 1, 3, a, a, None, buf, buf, None, buf, None) == 1
    assert b"null gains" in L.fv_last_error()
    for a1, a2, v, d, c in [(None, a, buf, buf, buf), (a, None, buf, buf, buf), (a, a, None, buf, buf), (a, a, buf, None, buf),
                            (a, a, buf, buf, None)]:
        assert fn(0, 2, 1, 3, 1, 3, a1, a2, buf, v, d, None, c, None) == 1
        assert b"null pairs, vis, data or chi2_rows" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert fn(0, 2, 1, 3, 4, 3, a1, a2, buf, buf, buf, None, buf, buf) == 1
        assert b"antenna index outside [0, nant)" in L.fv_last_error()
    assert fn(0, 2, 1, 3, 1, 0, a, a, buf, buf, buf, None, buf, None) == 1
    assert b"nant must be positive" in L.fv_last_error()


def test_handle_entry_points_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    a = (ctypes.c_int * 2)(0, 1)
    assert L.fv_sim_set_gain_pairs(None, 2, a, a) == 1 and b"null handle" in L.fv_last_error()
    fn = L.fv_sim_run_residual_gains
    assert fn(None, 0, 1, 0, 1, buf, 0, None, 0, buf, 0, buf, 0, buf, None, 0) == 1
    assert b"null handle" in L.fv_last_error()
    for d, g, v, c in [(None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)]:
        assert fn(None, 0, 1, 0, 1, d, 0, buf, 0, g, 0, v, 0, c, None, 0) == 1
        assert b"null data, gains, gvis or chi2_ft" in L.fv_last_error()
    for flags in [(2, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, 3, 0, 0), (0, 0, 0, 2, 0), (0, 0, 0, 0, -1)]:
        assert fn(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], buf, flags[2], buf, flags[3], buf, buf, flags[4]) == 1
        assert b"on_device" in L.fv_last_error()
