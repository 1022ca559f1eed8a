"""CPU tests of the fused objective's surface (``simulate_vis_chi2``, ``torch_simulate_vis_chi2``, ``fv_residual_chi2``,
``fv_sim_run_residual``): the exports, the signatures, the argument errors raised before any engine exists --
``wrapper.create_simulation_engine`` is replaced by a function that fails the test, as in ``test_derivative_api_host`` --
and the C entry points' argument checks through a null handle and null pointers."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import objective_refs
from tests.test_derivative_api_host import REQUIRED, Mgr, _cfg, _vis
from tests.test_sky_adjoint_host import _COMMON, _TAIL

_HEAD = [(n, "POSITIONAL_OR_KEYWORD", REQUIRED)
         for n in ("data", "ants", "fluxes", "ra", "dec", "freqs", "times", "beam", "telescope_loc")]
_OWN = [("weights", "KEYWORD_ONLY", None), ("wrt", "KEYWORD_ONLY", ("fluxes",)), ("beam_coefs", "KEYWORD_ONLY", None),
        ("chi2_per", "KEYWORD_ONLY", "total"), ("return_gvis", "KEYWORD_ONLY", False),
        ("adjoint_path", "KEYWORD_ONLY", "type3"), ("full_stokes", "KEYWORD_ONLY", None)]


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _call(data=None, basis=False, **changes):
    cfg = _cfg(basis)
    return adjoint.simulate_vis_chi2(_vis(cfg) if data is None else data, **dict(cfg, **changes))


def test_exported_with_the_documented_signatures():
    got = [(p.name, p.kind.name, p.default) for p in inspect.signature(adjoint.simulate_vis_chi2).parameters.values()]
    # after its own keywords, the keywords simulate_vis_sky_adjoint takes (beam_coefs moved up)
    assert got == _HEAD + _OWN + _COMMON + _TAIL
    sky = [p.name for p in inspect.signature(adjoint.simulate_vis_sky_adjoint).parameters.values()]
    assert set(sky) - {"vis"} <= {p[0] for p in got}
    assert fftvis_amd.simulate_vis_chi2 is adjoint.simulate_vis_chi2
    assert fftvis_amd.torch_simulate_vis_chi2 is adjoint.torch_simulate_vis_chi2
    got = [(p.name, p.kind.name, p.default) for p in inspect.signature(adjoint.torch_simulate_vis_chi2).parameters.values()]
    assert got == [("data", "POSITIONAL_OR_KEYWORD", REQUIRED), ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED),
                   ("weights", "KEYWORD_ONLY", None), ("beam_coefs", "KEYWORD_ONLY", None), ("antpos", "KEYWORD_ONLY", None),
                   ("antnums", "KEYWORD_ONLY", None), ("radec", "KEYWORD_ONLY", None), ("kwargs", "VAR_KEYWORD", REQUIRED)]


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_residual_chi2\(int device, int precision, int64_t nrows, int64_t row_len, void \*vis, "
                     r"const void \*data,\s+const void \*weights, double \*chi2_rows\);", header, re.M)
    assert re.search(r"^int fv_sim_run_residual\(fv_sim \*h, int t0, int t1, int f0, int f1, const void \*data, "
                     r"int data_on_device, const void \*weights,\s+int weights_on_device, void \*gvis, int gvis_on_device, "
                     r"double \*chi2_ft\);", header, re.M)
    assert len(_lib.SYMBOLS["fv_residual_chi2"][1]) == 8 and len(_lib.SYMBOLS["fv_sim_run_residual"][1]) == 12
    assert hasattr(_lib.lib(), "fv_residual_chi2") and hasattr(_lib.lib(), "fv_sim_run_residual")
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_residual)
    assert "objective_of" in inspect.signature(gpu_simulate.GPUSimulationEngine.simulate).parameters


def test_the_reference_itself():
    rng = np.random.default_rng(0)
    V = rng.normal(size=(2, 3, 5)) + 1j * rng.normal(size=(2, 3, 5))
    d = rng.normal(size=V.shape) + 1j * rng.normal(size=V.shape)
    w = rng.uniform(0.5, 2.0, size=V.shape)
    w[0, 1, 2] = 0.0
    d[0, 1, 2] = np.nan
    chi2, G = objective_refs.chi2_and_gvis(V, d, w)
    assert chi2.shape == (2, 3) and np.isfinite(chi2).all() and G[0, 1, 2] == 0
    keep = w != 0
    assert np.allclose(chi2.sum(), np.sum(w[keep] * np.abs(V[keep] - d[keep]) ** 2), rtol=1e-14)
    assert np.allclose(G[keep], 2 * w[keep] * (V[keep] - d[keep]), rtol=1e-15)
    c1, G1 = objective_refs.chi2_and_gvis(V, np.zeros_like(V))
    assert np.array_equal(G1, 2 * V) and np.allclose(c1, (np.abs(V) ** 2).sum(axis=-1), rtol=1e-14)
    assert objective_refs.row_major_sum(chi2) == float(np.cumsum(chi2.ravel())[-1])


@pytest.mark.parametrize("basis", [False, True])
def test_wrong_data_or_weights(basis):
    vis = _vis(_cfg(basis))
    for bad in (vis[:1], vis[..., :-1]):
        with _raises(ValueError, f"data must have simulate_vis's output shape {vis.shape}, got {bad.shape}"):
            _call(bad, basis)
        with _raises(ValueError, f"weights must have data's shape {vis.shape}, got {bad.shape}"):
            _call(vis, basis, weights=np.ones(bad.shape))
    with _raises(ValueError, "weights must be real (inverse variances; 0 flags a sample)"):
        _call(vis, basis, weights=np.ones(vis.shape, complex))


def test_bad_wrt():
    with _raises(ValueError, "wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs', got "
                             "'antennas'"):
        _call(wrt="antennas")
    for wrt in (("fluxes", "fluxes"), ("topo", "radec", "topo"), ("fluxes", "positions")):
        with pytest.raises(ValueError, match="^wrt must name "):
            _call(wrt=wrt)
    for wrt in ("beam_coefs", ("fluxes", "beam_coefs")):
        with _raises(ValueError, "wrt='beam_coefs' needs beam_coefs (basis beams)"):
            _call(wrt=wrt)
    with _raises(ValueError, "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to "
                             "use beam_coefs."):
        _call(basis=True, polarized=False, data=_vis(_cfg(False)))
    with _raises(ValueError, "beam_coefs must have shape (nant, nbasis, nfreqs)"):
        _call(basis=True, beam_coefs=np.ones((7, 3, 2), complex))


@pytest.mark.parametrize("wrt", ["radec", ("fluxes", "radec"), ("ants", "radec", "fluxes")])
@pytest.mark.parametrize("basis", [False, True])
def test_radec_follows_the_source_adjoints_coordinate_rules(basis, wrt):
    with _raises(ValueError, "wrt='radec' needs this package's own chain from (ra, dec) to the topocentric vectors; with "
                             "coord_mgr= the chain is the manager's: ask for wrt='topo' and apply its Jacobian"):
        _call(basis=basis, wrt=wrt, coord_mgr=Mgr())
    with _raises(ValueError, "wrt='radec' needs coord_method='SiderealRotation' or device astrometry (astrom= / "
                             "device_astrometry=True); coord_method='CoordinateRotationERFA' builds a matvis manager "
                             "whose chain is its own: ask for wrt='topo'"):
        _call(basis=basis, wrt=wrt, coord_method=inspect.signature(adjoint.simulate_vis_chi2).parameters["coord_method"].default)


def test_chi2_per_adjoint_path_backend_and_fluxes():
    with _raises(ValueError, "chi2_per must be 'total' or 'freq_time', got 'row'"):
        _call(chi2_per="row")
    with _raises(ValueError, "adjoint_path must be 'type3', 'type2' or 'auto', got 'type1'"):
        _call(adjoint_path="type1")
    for wrt in ((), "fluxes", ("ants", "topo")):
        with _raises(ValueError, "Unsupported backend: cpu"):
            _call(backend="cpu", wrt=wrt)
    with _raises(ValueError, "fluxes must have shape (nsources, nfreqs[, 4])"):
        _call(fluxes=np.ones((19, 2)))
    with _raises(ValueError, "full_stokes=True does not match fluxes of shape (20, 2)"):
        _call(full_stokes=True, polarized=True, data=_vis(_cfg(True)))


def test_torch_entry_point_refuses_what_it_decides_itself():
    import torch

    cfg = _cfg()
    F = torch.ones(20, 2, dtype=torch.float64)
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    for name in ("wrt", "chi2_per", "return_gvis"):
        with pytest.raises(TypeError, match=f"does not take {name}="):
            fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, **dict(kw, **{name: "fluxes"}))
    with pytest.raises(TypeError, match="not ants="):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, antpos=torch.zeros(7, 3, dtype=torch.float64), **kw)
    with pytest.raises(TypeError, match="not both"):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, radec=torch.zeros(20, 2, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match=r"radec must be a real \(nsrc, 2\) tensor"):
        fftvis_amd.torch_simulate_vis_chi2(_vis(cfg), F, radec=torch.zeros(20, 3, dtype=torch.float64),
                                           **{k: v for k, v in kw.items() if k not in ("ra", "dec")})


def test_fv_sim_run_residual_argument_checks():
    L = _lib.lib()
    fn = L.fv_sim_run_residual
    buf = (ctypes.c_double * 8)()
    assert fn(None, 0, 1, 0, 1, buf, 0, buf, 0, buf, 0, buf) == 1
    assert b"null handle" in L.fv_last_error()
    assert fn(None, 0, 1, 0, 1, buf, 0, None, 0, buf, 0, buf) == 1  # weights may be null: the handle is what is missing
    assert b"null handle" in L.fv_last_error()
    for d, g, c in [(None, buf, buf), (buf, None, buf), (buf, buf, None)]:
        assert fn(None, 0, 1, 0, 1, d, 0, buf, 0, g, 0, c) == 1
        assert b"null data, gvis or chi2_ft" in L.fv_last_error()
    for flags in [(2, 0, 0), (0, -1, 0), (0, 0, 3), (3, 3, 3)]:
        assert fn(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], buf, flags[2], buf) == 1
        assert b"on_device" in L.fv_last_error()


def test_fv_residual_chi2_argument_checks():
    L = _lib.lib()
    fn = L.fv_residual_chi2
    buf = (ctypes.c_double * 8)()
    for precision in (0, 3):
        assert fn(0, precision, 1, 1, buf, buf, None, buf) == 1
        assert b"precision must be 1 or 2" in L.fv_last_error()
    for nrows, row_len in [(-1, 1), (1, -1)]:
        assert fn(0, 2, nrows, row_len, buf, buf, None, buf) == 1
        assert b"negative shape" in L.fv_last_error()
    for v, d, c in [(None, buf, buf), (buf, None, buf), (buf, buf, None)]:
        assert fn(0, 2, 1, 1, v, d, None, c) == 1
        assert b"null vis, data or chi2_rows" in L.fv_last_error()
