"""CPU tests of the Jones gains in the fused objective (``simulate_vis_jones_chi2``, ``fv_jones_residual_chi2``,
``fv_sim_run_residual_jones``): the numpy references against finite differences of their own chi2 and against the
diagonal gains' references, the C surface, and the argument errors raised before any engine exists or any device is
touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import gain_refs, jones_refs
from tests.test_derivative_api_host import _cfg, _vis


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _case(seed=0, nant=5, nbls=9, lead=(2, 3)):
    """Random blocks with an auto-correlation, an antenna without a baseline, 20 % flags with NaN data under them, one
    baseline with every sample flagged."""
    rng = np.random.default_rng(seed)
    shape = lead + (2, 2, nbls)

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    a1, a2 = rng.integers(0, nant - 1, nbls), rng.integers(0, nant - 1, nbls)  # (the last antenna has no baseline)
    a1[0] = a2[0] = 1  # an auto-correlation
    V, d = c(shape), c(shape)
    J = 0.4 * c(lead + (2, 2, nant))
    J[..., 0, 0, :] += 1
    J[..., 1, 1, :] += 1
    w = rng.uniform(0.5, 2.0, size=shape)
    flagged = rng.random(shape) < 0.2
    flagged[..., 3] = True
    w[flagged] = 0
    d[flagged] = np.nan
    return V, d, w, J, a1, a2


def test_reference_gradient_is_the_stencil_of_its_own_chi2():
    V, d, w, J, a1, a2 = _case()
    rows, Gp, G, gj = jones_refs.chi2_jones(V, d, w, J, a1, a2)
    assert rows.shape == V.shape[:2] and gj.shape == J.shape and np.all(gj[..., -1] == 0) and np.isfinite(G).all()
    assert np.all(Gp[w == 0] == 0) and np.all(G[..., 3] == 0) and np.count_nonzero(gj[..., :-1]) == gj[..., :-1].size
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4):
        dJ = rng.normal(size=J.shape) + 1j * rng.normal(size=J.shape)
        fd = jones_refs.five_point(lambda h: jones_refs.chi2_jones(V, d, w, J + h * dJ, a1, a2)[0].sum(), 0.25)
        an = np.sum(np.conj(gj) * dJ).real
        worst = max(worst, abs(fd - an) / abs(an))
    print("jones reference: stencil against gjones", worst)
    assert worst <= 1e-12


def test_reference_gvis_is_the_derivative_in_v():
    V, d, w, J, a1, a2 = _case(seed=3)
    G = jones_refs.chi2_jones(V, d, w, J, a1, a2)[2]
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(3):
        dV = rng.normal(size=V.shape) + 1j * rng.normal(size=V.shape)
        fd = jones_refs.five_point(lambda h: jones_refs.chi2_jones(V + h * dV, d, w, J, a1, a2)[0].sum(), 0.25)
        an = np.sum(np.conj(G) * dV).real
        worst = max(worst, abs(fd - an) / abs(an))
    print("jones reference: stencil against G", worst)
    assert worst <= 1e-12
    eye = jones_refs.diagonal(np.ones(J.shape[:2] + (2, J.shape[-1])))
    assert np.array_equal(jones_refs.apply_jones(V, eye, a1, a2), V)
    used = w != 0
    Vp = jones_refs.apply_jones(V, J, a1, a2)
    assert np.allclose(jones_refs.chi2_jones(V, d, w, J, a1, a2)[1][used], (2 * w * (Vp - d))[used], rtol=1e-15)


def test_majorant_bounds_the_gradient_terms():
    V, d, w, J, a1, a2 = _case(seed=4)
    gj, A = jones_refs.chi2_jones(V, d, w, J, a1, a2, with_abs=True)[3:]
    assert A.shape == J.shape and np.all(A >= np.abs(gj)) and np.all(A[..., -1] == 0)


def test_diagonal_matrices_are_the_gains():
    V, d, w, J, a1, a2 = _case(seed=5)
    rng = np.random.default_rng(6)
    g = 1 + 0.3 * (rng.normal(size=J.shape[:2] + (2, J.shape[-1])) + 1j * rng.normal(size=J.shape[:2] + (2, J.shape[-1])))
    D = jones_refs.diagonal(g)
    rows, Gp, G, gj = jones_refs.chi2_jones(V, d, w, D, a1, a2)
    rows_g, Gp_g, G_g, gg = gain_refs.chi2_gains(V, d, w, g, a1, a2)

    def close(a, b):
        return np.abs(a - b).max() <= 1e-13 * np.abs(b).max()

    assert close(jones_refs.apply_jones(V, D, a1, a2), gain_refs.apply_gains(V, g, a1, a2))
    assert close(rows, rows_g) and close(Gp, Gp_g) and close(G, G_g)
    assert close(gj[..., 0, 0, :], gg[..., 0, :]) and close(gj[..., 1, 1, :], gg[..., 1, :])
    assert np.abs(gj[..., 0, 1, :]).max() > 0.1  # (the leakage entries have a gradient of their own at diagonal matrices)


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_jones_residual_chi2\(int device, int precision, int64_t nrows, int64_t nbls, int nant, "
                     r"const int \*ant1,\s+const int \*ant2, const void \*jones, void \*vis, const void \*data, "
                     r"const void \*weights,\s+double \*chi2_rows, void \*gjones\);", header, re.M)
    assert re.search(r"^int fv_sim_run_residual_jones\(fv_sim \*h, int t0, int t1, int f0, int f1, const void \*data, "
                     r"int data_on_device,\s+const void \*weights, int weights_on_device, const void \*jones, "
                     r"int jones_on_device, void \*gvis,\s+int gvis_on_device, double \*chi2_ft, void \*gjones, "
                     r"int gjones_on_device\);", header, re.M)
    arity = {"fv_jones_residual_chi2": 13, "fv_sim_run_residual_jones": 16}
    for name, n in arity.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_jones_residual)
    plain = inspect.signature(adjoint.simulate_vis_chi2).parameters
    own = inspect.signature(adjoint.simulate_vis_jones_chi2).parameters
    # simulate_vis_chi2's parameters and, first of the keywords, the required jones
    assert list(own) == list(plain)[:9] + ["jones"] + list(plain)[9:]
    assert all(own[n].kind == plain[n].kind and own[n].default == plain[n].default for n in plain)
    assert own["jones"].kind.name == "KEYWORD_ONLY" and own["jones"].default is inspect.Parameter.empty
    assert "jones" not in inspect.signature(adjoint.simulate_vis_gain_chi2).parameters
    assert fftvis_amd.simulate_vis_jones_chi2 is adjoint.simulate_vis_jones_chi2
    for word in ("leakage", "polarized=True", "explicit ``baselines``", "NOT", "Gauss-Newton", "sharding"):
        assert word in adjoint.simulate_vis_jones_chi2.__doc__, word
    assert "simulate_vis_jones_chi2" in adjoint.simulate_vis_gain_chi2.__doc__


def _call(**changes):
    cfg = dict(_cfg(), polarized=True)
    changes.setdefault("jones", None)
    cfg.update(changes)
    return adjoint.simulate_vis_jones_chi2(_vis(cfg), **cfg)


def _shapes(cfg):
    nant, nf, nt = len(cfg["ants"]), np.size(cfg["freqs"]), len(cfg["times"])
    return (nant, 2, 2, nf), (nant, 2, 2, nf, nt)


def test_bad_jones():
    cfg = _cfg()
    const, per_time = _shapes(cfg)
    nant, nf = const[0], const[-1]
    for bad in ((nant, 2, nf), (nant, nf), const[:-1], const + (1, 1), (nant + 1,) + const[1:],
                per_time[:-1] + (per_time[-1] + 1,), (2, 2, nant, nf), (nant, 2, 3, nf)):
        with _raises(ValueError, f"jones must have shape {const} or {per_time}, got {bad}"):
            _call(jones=np.ones(bad, complex))
    with _raises(ValueError, "jones must be complex (one 2 x 2 matrix per antenna and channel)"):
        _call(jones=np.ones(const))
    for value in (np.nan, complex(1, np.inf)):
        j = np.ones(per_time, complex)
        j[(0,) * j.ndim] = value
        with _raises(ValueError, "jones must be finite"):
            _call(jones=j)
    with _raises(ValueError, "jones needs polarized=True: a 2 x 2 matrix per antenna mixes the two feeds"):
        _call(jones=np.ones(const, complex), polarized=False)
    for wrt in ("jones", ("fluxes", "jones")):
        with _raises(ValueError, "wrt='jones' needs jones="):
            _call(wrt=wrt)
    with pytest.raises(ValueError, match="^wrt must name "):
        _call(wrt=("jones", "jones"), jones=np.ones(const, complex))
    for wrt in ("antennas", "gains"):  # (the gains are simulate_vis_gain_chi2's)
        with _raises(ValueError, "wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and 'jones', "
                                 f"got '{wrt}'"):
            _call(wrt=wrt, jones=np.ones(const, complex))
    pol = dict(cfg, polarized=True)
    for wrt in ("jones", ("fluxes", "jones")):  # the other two functions do not know the name
        with pytest.raises(ValueError, match="^wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs', got"):
            adjoint.simulate_vis_chi2(_vis(pol), **dict(pol, wrt=wrt))
        with pytest.raises(ValueError, match="^wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and "
                                             "'gains', got"):
            adjoint.simulate_vis_gain_chi2(_vis(pol), **dict(pol, wrt=wrt, gains=np.ones((nant, 2, nf), complex)))
    with pytest.raises(TypeError, match="jones"):
        adjoint.simulate_vis_chi2(_vis(pol), **dict(pol, jones=np.ones(const, complex)))
    with pytest.raises(TypeError, match="jones"):
        adjoint.simulate_vis_gain_chi2(_vis(pol), **dict(pol, gains=np.ones((nant, 2, nf), complex), jones=np.ones(const, complex)))


def test_objective_of_takes_the_matrices_in_a_form_of_their_own():
    from fftvis_amd.gpu import gpu_simulate as gs

    blk = np.ones((2, 2, 2, 2, 7), complex)
    assert gs._is_jones(("jones", blk)) and not gs._is_jones(blk) and not gs._is_jones(None) and not gs._is_jones((blk, None))
    gs._check_objective((None, None, {"gjones": blk}, ("jones", blk)), False)
    with _raises(ValueError, "objective_of: gjones needs the matrices (a fourth element ('jones', block))"):
        gs._check_objective((None, None, {"gjones": blk}, blk[:, :, 0]), False)
    with _raises(ValueError, "objective_of: ggains needs the gains (a fourth element)"):
        gs._check_objective((None, None, {"ggains": blk}, ("jones", blk)), False)
    with _raises(ValueError, "objective_of: the fourth element is the gains, or ('jones', block)"):
        gs._check_objective((None, None, {}, ("leakage", blk)), False)


def test_torch_entry_point_checks_jones_before_an_engine_exists():
    import torch

    cfg = dict(_cfg(), polarized=True)
    const, _ = _shapes(cfg)
    F = torch.ones(20, 2, dtype=torch.float64)
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    j = torch.ones(const[:-1], dtype=torch.complex128, requires_grad=True)
    with pytest.raises(ValueError, match=r"^jones must have shape "):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, jones=j, **kw)
    with pytest.raises(ValueError, match=r"^jones must be complex"):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, jones=torch.ones(const, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match=r"^jones needs polarized=True"):
        fftvis_amd.torch_simulate_vis_chi2(_vis(_cfg()), F, jones=torch.ones(const, dtype=torch.complex128),
                                           **dict(kw, polarized=False))
    with pytest.raises(TypeError, match=r"gains= or jones=, not both"):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, jones=torch.ones(const, dtype=torch.complex128),
                                           gains=torch.ones((const[0], 2, const[-1]), dtype=torch.complex128), **kw)


def test_fv_jones_residual_chi2_argument_checks():
    L = _lib.lib()
    fn = L.fv_jones_residual_chi2
    buf = (ctypes.c_double * 256)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    for precision in (0, 3):
        assert fn(0, precision, 1, 3, 3, a, a, buf, buf, buf, None, buf, None) == 1
        assert b"precision must be 1 or 2" in L.fv_last_error()
    for nrows, nbls in [(-1, 3), (1, -1)]:
        assert fn(0, 2, nrows, nbls, 3, a, a, buf, buf, buf, None, buf, None) == 1
        assert b"negative shape" in L.fv_last_error()
    assert fn(0, 2, 1, 3, 3, a, a, None, buf, buf, None, buf, None) == 1
    assert b"null jones" in L.fv_last_error()
    for a1, a2, v, d, c in [(None, a, buf, buf, buf), (a, None, buf, buf, buf), (a, a, None, buf, buf), (a, a, buf, None, buf),
                            (a, a, buf, buf, None)]:
        assert fn(0, 2, 1, 3, 3, a1, a2, buf, v, d, None, c, None) == 1
        assert b"null pairs, vis, data or chi2_rows" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert fn(0, 2, 1, 3, 3, a1, a2, buf, buf, buf, None, buf, buf) == 1
        assert b"antenna index outside [0, nant)" in L.fv_last_error()
    assert fn(0, 2, 1, 3, 0, a, a, buf, buf, buf, None, buf, None) == 1
    assert b"nant must be positive" in L.fv_last_error()
    # no rows and no baselines need no device: nothing, and zeros
    assert fn(0, 2, 0, 3, 3, a, a, None, None, None, None, None, None) == 0
    rows, gj = (ctypes.c_double * 2)(7.0, 7.0), (ctypes.c_double * 48)(*([7.0] * 48))
    assert fn(0, 2, 2, 0, 3, None, None, buf, None, None, None, rows, gj) == 0
    assert list(rows) == [0.0, 0.0] and not any(gj)


def test_handle_entry_point_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    fn = L.fv_sim_run_residual_jones
    assert fn(None, 0, 1, 0, 1, buf, 0, None, 0, buf, 0, buf, 0, buf, None, 0) == 1
    assert b"null handle" in L.fv_last_error()
    for d, j, v, c in [(None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)]:
        assert fn(None, 0, 1, 0, 1, d, 0, buf, 0, j, 0, v, 0, c, None, 0) == 1
        assert b"null data, jones, gvis or chi2_ft" in L.fv_last_error()
    for flags in [(2, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, 3, 0, 0), (0, 0, 0, 2, 0), (0, 0, 0, 0, -1)]:
        assert fn(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], buf, flags[2], buf, flags[3], buf, buf, flags[4]) == 1
        assert b"on_device" in L.fv_last_error()
