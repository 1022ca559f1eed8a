"""CPU tests of the joint sky adjoint's surface (``simulate_vis_sky_adjoint``, ``simulate_vis_basis_sky_adjoint``,
``fv_sim_run_sky_adjoint``, ``fv_sim_run_basis_sky_adjoint``): the exports, the signatures, the argument errors raised
before any engine exists -- ``wrapper.create_simulation_engine`` is replaced by a function that fails the test, as in
``test_derivative_api_host`` -- and the C entry points' argument checks through a bare handle."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests.test_derivative_api_host import INF, REQUIRED, Mgr, _cfg, _vis

_COMMON = [
    ("beam_idx", "KEYWORD_ONLY", None), ("baselines", "KEYWORD_ONLY", None), ("precision", "KEYWORD_ONLY", 2),
    ("polarized", "KEYWORD_ONLY", False), ("eps", "KEYWORD_ONLY", None), ("upsample_factor", "KEYWORD_ONLY", 2),
    ("beam_spline_opts", "KEYWORD_ONLY", None), ("use_feed", "KEYWORD_ONLY", 'x'),
    ("flat_array_tol", "KEYWORD_ONLY", 1e-06), ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'),
    ("nprocesses", "KEYWORD_ONLY", 1), ("nthreads", "KEYWORD_ONLY", None),
    ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'), ("coord_method_params", "KEYWORD_ONLY", None),
    ("force_use_type3", "KEYWORD_ONLY", False), ("force_use_ray", "KEYWORD_ONLY", False),
    ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'), ("max_memory", "KEYWORD_ONLY", INF),
    ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0),
]
_TAIL = [
    ("device", "KEYWORD_ONLY", 0), ("coord_mgr", "KEYWORD_ONLY", None), ("reference_compat", "KEYWORD_ONLY", True),
    ("astrom", "KEYWORD_ONLY", None), ("device_astrometry", "KEYWORD_ONLY", False),
]
_HEAD = [(n, "POSITIONAL_OR_KEYWORD", REQUIRED) for n in ("vis", "ants", "fluxes", "ra", "dec", "freqs", "times", "beam")]
_WRT = [("wrt", "KEYWORD_ONLY", ("fluxes", "radec")), ("full_stokes", "KEYWORD_ONLY", None)]

SIGNATURES = {
    # simulate_vis_source_adjoint's keywords after wrt and full_stokes
    "simulate_vis_sky_adjoint": _HEAD + [("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED)] + _WRT + _COMMON
    + [("beam_coefs", "KEYWORD_ONLY", None)] + _TAIL,
    # simulate_vis_basis_source_adjoint's: beam_coefs positional, polarized on by default
    "simulate_vis_basis_sky_adjoint": _HEAD + [("beam_coefs", "POSITIONAL_OR_KEYWORD", REQUIRED),
                                               ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED)] + _WRT
    + [("polarized", "KEYWORD_ONLY", True) if p[0] == "polarized" else p for p in _COMMON] + _TAIL,
}
SYMBOLS = ("fv_sim_run_sky_adjoint", "fv_sim_run_basis_sky_adjoint")
BASIS = {"simulate_vis_sky_adjoint": False, "simulate_vis_basis_sky_adjoint": True}


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _call(name, vis=None, **changes):
    cfg = _cfg(BASIS[name])
    return getattr(adjoint, name)(_vis(cfg) if vis is None else vis, **dict(cfg, **changes))


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_exported_with_the_documented_signature(name):
    got = [(p.name, p.kind.name, p.default) for p in inspect.signature(getattr(adjoint, name)).parameters.values()]
    assert got == SIGNATURES[name]
    assert getattr(fftvis_amd, name) is getattr(adjoint, name)
    assert "adjoint_path" not in inspect.signature(getattr(adjoint, name)).parameters


def test_the_keywords_after_wrt_are_those_of_the_source_passes():
    for joint, single in (("simulate_vis_sky_adjoint", "simulate_vis_source_adjoint"),
                          ("simulate_vis_basis_sky_adjoint", "simulate_vis_basis_source_adjoint")):
        a = [(p.name, p.default) for p in inspect.signature(getattr(adjoint, joint)).parameters.values()]
        b = [(p.name, p.default) for p in inspect.signature(getattr(adjoint, single)).parameters.values()]
        assert [p for p in a if p[0] not in ("wrt", "full_stokes")] == [p for p in b if p[0] != "wrt"]


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"^int %s\(fv_sim \*h, int t0, int t1, int f0, int f1, const void \*gvis, int gvis_on_device, "
                         r"void \*gflux,\s+int gflux_on_device, double \*gtopo, int gtopo_on_device, int accumulate\);" % sym,
                         header, re.M), sym
        assert sym in _lib.SYMBOLS and len(_lib.SYMBOLS[sym][1]) == 12
        assert hasattr(_lib.lib(), sym)
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_sky_adjoint)
    assert "sky_of" in inspect.signature(gpu_simulate.GPUSimulationEngine.simulate).parameters


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_bad_wrt(name):
    with _raises(ValueError, "wrt must name some of 'fluxes', 'topo' and 'radec', got 'antennas'"):
        _call(name, wrt="antennas")
    for wrt in ((), ("fluxes", "fluxes"), ("topo", "radec", "topo"), ("fluxes", "beam_coefs"), ("fluxes", "ants")):
        with pytest.raises(ValueError, match="^wrt must name "):
            _call(name, wrt=wrt)


@pytest.mark.parametrize("wrt", [("fluxes", "topo"), "fluxes", "topo", ("radec",)])
@pytest.mark.parametrize("name", list(SIGNATURES))
def test_wrong_backend(name, wrt):
    with _raises(ValueError, "Unsupported backend: cpu"):
        _call(name, backend="cpu", wrt=wrt)


@pytest.mark.parametrize("wrt", [("fluxes", "topo"), ("fluxes",), "topo"])
@pytest.mark.parametrize("name", list(SIGNATURES))
def test_wrong_vis_shape(name, wrt):
    vis = _vis(_cfg(BASIS[name]))
    for bad in (vis[:1], vis[..., :-1]):
        with _raises(ValueError, f"vis must have simulate_vis's output shape {vis.shape}, got {bad.shape}"):
            _call(name, vis=bad, wrt=wrt, coord_method="SiderealRotation")


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_wrong_fluxes_shape(name):
    for bad in (np.ones((19, 2)), np.ones((20, 3)), np.ones((20, 2, 3))):
        with _raises(ValueError, "fluxes must have shape (nsources, nfreqs[, 4])"):
            _call(name, fluxes=bad)
    with _raises(ValueError, "a full-Stokes sky needs polarized=True"):
        _call("simulate_vis_sky_adjoint", fluxes=np.ones((20, 2, 4)))


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_full_stokes_mismatch_has_the_basis_adjoints_message(name):
    with _raises(ValueError, "full_stokes=True does not match fluxes of shape (20, 2)"):
        _call(name, full_stokes=True, polarized=True)
    with _raises(ValueError, "full_stokes=False does not match fluxes of shape (20, 2, 4)"):
        _call(name, full_stokes=False, polarized=True, fluxes=np.ones((20, 2, 4)))
    with _raises(ValueError, "full_stokes=True does not match fluxes of shape (20, 2)"):  # the message it borrows
        adjoint.simulate_vis_basis_adjoint(_vis(_cfg(True)), **_cfg(True), full_stokes=True)


def test_beam_coefs_on_the_plain_function_and_missing_from_the_basis_function():
    with _raises(NotImplementedError, "simulate_vis_sky_adjoint does not support basis beams (beam_coefs): "
                                      "simulate_vis_basis_sky_adjoint does"):
        _call("simulate_vis_sky_adjoint", beam_coefs=np.ones((7, 1, 2), complex))
    with _raises(ValueError, "simulate_vis_basis_sky_adjoint needs beam_coefs (without basis beams "
                             "simulate_vis_sky_adjoint is the pass)"):
        _call("simulate_vis_basis_sky_adjoint", beam_coefs=None)
    with _raises(ValueError, "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to "
                             "use beam_coefs."):
        _call("simulate_vis_basis_sky_adjoint", polarized=False)
    with _raises(ValueError, "beam_coefs must have shape (nant, nbasis, nfreqs)"):
        _call("simulate_vis_basis_sky_adjoint", beam_coefs=np.ones((7, 3, 2), complex))


@pytest.mark.parametrize("wrt", ["radec", ("fluxes", "radec"), ("topo", "radec", "fluxes")])
@pytest.mark.parametrize("name", list(SIGNATURES))
def test_radec_follows_the_source_adjoints_coordinate_rules(name, wrt):
    with _raises(ValueError, "wrt='radec' needs this package's own chain from (ra, dec) to the topocentric vectors; with "
                             "coord_mgr= the chain is the manager's: ask for wrt='topo' and apply its Jacobian"):
        _call(name, wrt=wrt, coord_mgr=Mgr())
    with _raises(ValueError, "wrt='radec' needs coord_method='SiderealRotation' or device astrometry (astrom= / "
                             "device_astrometry=True); coord_method='CoordinateRotationERFA' builds a matvis manager "
                             "whose chain is its own: ask for wrt='topo'"):
        _call(name, wrt=wrt, coord_method=inspect.signature(getattr(adjoint, name)).parameters["coord_method"].default)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_c_entry_point_argument_checks(sym):
    L = _lib.lib()
    fn = getattr(L, sym)
    buf = (ctypes.c_double * 8)()
    assert fn(None, 0, 1, 0, 1, buf, 0, buf, 0, buf, 0, 0) == 1
    assert b"handle" in L.fv_last_error()
    for g, gf, gt in [(None, buf, buf), (buf, None, buf), (buf, buf, None)]:
        assert fn(None, 0, 1, 0, 1, g, 0, gf, 0, gt, 0, 0) == 1
        assert b"null adjoint" in L.fv_last_error()
    for flags in [(2, 0, 0), (0, -1, 0), (0, 0, 3), (3, 3, 3)]:
        assert fn(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], buf, flags[2], 0) == 1
        assert b"on_device" in L.fv_last_error()
    for acc in (2, -1):
        assert fn(None, 0, 1, 0, 1, buf, 0, buf, 0, buf, 0, acc) == 1
        assert b"accumulate" in L.fv_last_error()
