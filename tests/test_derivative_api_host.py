"""CPU tests of the host layer the derivative entry points of ``fftvis_amd.adjoint`` share: their signatures, the argument
errors they raise alike before any engine exists, and the time-block walker of ``gpu_simulate`` their engine loops run on.
No GPU work and no built library: ``wrapper.create_simulation_engine`` is replaced by a function that fails the test.

The public passes are six -- ``simulate_vis_adjoint``, ``_basis_adjoint``, ``_position_adjoint``, ``_source_adjoint``,
``_jvp`` and ``_basis_jvp`` -- and the torch operations five.  The signature table was generated once with
``inspect.signature`` from the commit before the host layer was factored out, and is compared by equality."""

import inspect
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import adjoint, synth, wrapper
from fftvis_amd.gpu import gpu_simulate

REQUIRED = inspect.Parameter.empty
INF = float("inf")

SIGNATURES = {
    "simulate_vis_adjoint": [
        ("vis", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ants", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("ra", "POSITIONAL_OR_KEYWORD", REQUIRED), ("dec", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("freqs", "POSITIONAL_OR_KEYWORD", REQUIRED), ("times", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("beam", "POSITIONAL_OR_KEYWORD", REQUIRED), ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("full_stokes", "KEYWORD_ONLY", False), ("beam_idx", "KEYWORD_ONLY", None), ("baselines", "KEYWORD_ONLY", None),
        ("precision", "KEYWORD_ONLY", 2), ("polarized", "KEYWORD_ONLY", False), ("eps", "KEYWORD_ONLY", None),
        ("upsample_factor", "KEYWORD_ONLY", 2), ("beam_spline_opts", "KEYWORD_ONLY", None),
        ("use_feed", "KEYWORD_ONLY", 'x'), ("flat_array_tol", "KEYWORD_ONLY", 1e-06),
        ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'), ("nprocesses", "KEYWORD_ONLY", 1),
        ("nthreads", "KEYWORD_ONLY", None), ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'),
        ("coord_method_params", "KEYWORD_ONLY", None), ("force_use_type3", "KEYWORD_ONLY", False),
        ("force_use_ray", "KEYWORD_ONLY", False), ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'),
        ("max_memory", "KEYWORD_ONLY", INF), ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0),
        ("beam_coefs", "KEYWORD_ONLY", None), ("device", "KEYWORD_ONLY", 0), ("coord_mgr", "KEYWORD_ONLY", None),
        ("reference_compat", "KEYWORD_ONLY", True), ("astrom", "KEYWORD_ONLY", None),
        ("device_astrometry", "KEYWORD_ONLY", False), ("adjoint_path", "KEYWORD_ONLY", 'type3'),
    ],
    "simulate_vis_basis_adjoint": [
        ("vis", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ants", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ra", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("dec", "POSITIONAL_OR_KEYWORD", REQUIRED), ("freqs", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("times", "POSITIONAL_OR_KEYWORD", REQUIRED), ("beam", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("beam_coefs", "POSITIONAL_OR_KEYWORD", REQUIRED), ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("wrt", "KEYWORD_ONLY", ('fluxes', 'beam_coefs')), ("full_stokes", "KEYWORD_ONLY", None),
        ("beam_idx", "KEYWORD_ONLY", None), ("baselines", "KEYWORD_ONLY", None), ("precision", "KEYWORD_ONLY", 2),
        ("polarized", "KEYWORD_ONLY", True), ("eps", "KEYWORD_ONLY", None), ("upsample_factor", "KEYWORD_ONLY", 2),
        ("beam_spline_opts", "KEYWORD_ONLY", None), ("use_feed", "KEYWORD_ONLY", 'x'),
        ("flat_array_tol", "KEYWORD_ONLY", 1e-06), ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'),
        ("nprocesses", "KEYWORD_ONLY", 1), ("nthreads", "KEYWORD_ONLY", None),
        ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'), ("coord_method_params", "KEYWORD_ONLY", None),
        ("force_use_type3", "KEYWORD_ONLY", False), ("force_use_ray", "KEYWORD_ONLY", False),
        ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'), ("max_memory", "KEYWORD_ONLY", INF),
        ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0), ("device", "KEYWORD_ONLY", 0),
        ("coord_mgr", "KEYWORD_ONLY", None), ("reference_compat", "KEYWORD_ONLY", True), ("astrom", "KEYWORD_ONLY", None),
        ("device_astrometry", "KEYWORD_ONLY", False),
    ],
    "simulate_vis_position_adjoint": [
        ("vis", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ants", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ra", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("dec", "POSITIONAL_OR_KEYWORD", REQUIRED), ("freqs", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("times", "POSITIONAL_OR_KEYWORD", REQUIRED), ("beam", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED), ("wrt", "KEYWORD_ONLY", 'ants'),
        ("beam_idx", "KEYWORD_ONLY", None), ("baselines", "KEYWORD_ONLY", None), ("precision", "KEYWORD_ONLY", 2),
        ("polarized", "KEYWORD_ONLY", False), ("eps", "KEYWORD_ONLY", None), ("upsample_factor", "KEYWORD_ONLY", 2),
        ("beam_spline_opts", "KEYWORD_ONLY", None), ("use_feed", "KEYWORD_ONLY", 'x'),
        ("flat_array_tol", "KEYWORD_ONLY", 1e-06), ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'),
        ("nprocesses", "KEYWORD_ONLY", 1), ("nthreads", "KEYWORD_ONLY", None),
        ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'), ("coord_method_params", "KEYWORD_ONLY", None),
        ("force_use_type3", "KEYWORD_ONLY", False), ("force_use_ray", "KEYWORD_ONLY", False),
        ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'), ("max_memory", "KEYWORD_ONLY", INF),
        ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0), ("beam_coefs", "KEYWORD_ONLY", None),
        ("device", "KEYWORD_ONLY", 0), ("coord_mgr", "KEYWORD_ONLY", None), ("reference_compat", "KEYWORD_ONLY", True),
        ("astrom", "KEYWORD_ONLY", None), ("device_astrometry", "KEYWORD_ONLY", False),
    ],
    "simulate_vis_source_adjoint": [
        ("vis", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ants", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("ra", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("dec", "POSITIONAL_OR_KEYWORD", REQUIRED), ("freqs", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("times", "POSITIONAL_OR_KEYWORD", REQUIRED), ("beam", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED), ("wrt", "KEYWORD_ONLY", 'radec'),
        ("beam_idx", "KEYWORD_ONLY", None), ("baselines", "KEYWORD_ONLY", None), ("precision", "KEYWORD_ONLY", 2),
        ("polarized", "KEYWORD_ONLY", False), ("eps", "KEYWORD_ONLY", None), ("upsample_factor", "KEYWORD_ONLY", 2),
        ("beam_spline_opts", "KEYWORD_ONLY", None), ("use_feed", "KEYWORD_ONLY", 'x'),
        ("flat_array_tol", "KEYWORD_ONLY", 1e-06), ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'),
        ("nprocesses", "KEYWORD_ONLY", 1), ("nthreads", "KEYWORD_ONLY", None),
        ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'), ("coord_method_params", "KEYWORD_ONLY", None),
        ("force_use_type3", "KEYWORD_ONLY", False), ("force_use_ray", "KEYWORD_ONLY", False),
        ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'), ("max_memory", "KEYWORD_ONLY", INF),
        ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0), ("beam_coefs", "KEYWORD_ONLY", None),
        ("device", "KEYWORD_ONLY", 0), ("coord_mgr", "KEYWORD_ONLY", None), ("reference_compat", "KEYWORD_ONLY", True),
        ("astrom", "KEYWORD_ONLY", None), ("device_astrometry", "KEYWORD_ONLY", False),
    ],
    "simulate_vis_jvp": [
        ("ants", "POSITIONAL_OR_KEYWORD", REQUIRED), ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("ra", "POSITIONAL_OR_KEYWORD", REQUIRED), ("dec", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("freqs", "POSITIONAL_OR_KEYWORD", REQUIRED), ("times", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("beam", "POSITIONAL_OR_KEYWORD", REQUIRED), ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("d_ants", "KEYWORD_ONLY", None), ("d_baselines", "KEYWORD_ONLY", None), ("d_radec", "KEYWORD_ONLY", None),
        ("d_topo", "KEYWORD_ONLY", None), ("d_fluxes", "KEYWORD_ONLY", None), ("beam_idx", "KEYWORD_ONLY", None),
        ("baselines", "KEYWORD_ONLY", None), ("precision", "KEYWORD_ONLY", 2), ("polarized", "KEYWORD_ONLY", False),
        ("eps", "KEYWORD_ONLY", None), ("upsample_factor", "KEYWORD_ONLY", 2), ("beam_spline_opts", "KEYWORD_ONLY", None),
        ("use_feed", "KEYWORD_ONLY", 'x'), ("flat_array_tol", "KEYWORD_ONLY", 1e-06),
        ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'), ("nprocesses", "KEYWORD_ONLY", 1),
        ("nthreads", "KEYWORD_ONLY", None), ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'),
        ("coord_method_params", "KEYWORD_ONLY", None), ("force_use_type3", "KEYWORD_ONLY", False),
        ("force_use_ray", "KEYWORD_ONLY", False), ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'),
        ("max_memory", "KEYWORD_ONLY", INF), ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0),
        ("beam_coefs", "KEYWORD_ONLY", None), ("device", "KEYWORD_ONLY", 0), ("coord_mgr", "KEYWORD_ONLY", None),
        ("reference_compat", "KEYWORD_ONLY", True), ("astrom", "KEYWORD_ONLY", None),
        ("device_astrometry", "KEYWORD_ONLY", False),
    ],
    "simulate_vis_basis_jvp": [
        ("ants", "POSITIONAL_OR_KEYWORD", REQUIRED), ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("ra", "POSITIONAL_OR_KEYWORD", REQUIRED), ("dec", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("freqs", "POSITIONAL_OR_KEYWORD", REQUIRED), ("times", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("beam", "POSITIONAL_OR_KEYWORD", REQUIRED), ("beam_coefs", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("telescope_loc", "POSITIONAL_OR_KEYWORD", REQUIRED), ("d_beam_coefs", "KEYWORD_ONLY", None),
        ("d_fluxes", "KEYWORD_ONLY", None), ("d_ants", "KEYWORD_ONLY", None), ("d_baselines", "KEYWORD_ONLY", None),
        ("beam_idx", "KEYWORD_ONLY", None), ("baselines", "KEYWORD_ONLY", None), ("precision", "KEYWORD_ONLY", 2),
        ("polarized", "KEYWORD_ONLY", True), ("eps", "KEYWORD_ONLY", None), ("upsample_factor", "KEYWORD_ONLY", 2),
        ("beam_spline_opts", "KEYWORD_ONLY", None), ("use_feed", "KEYWORD_ONLY", 'x'),
        ("flat_array_tol", "KEYWORD_ONLY", 1e-06), ("interpolation_function", "KEYWORD_ONLY", 'az_za_map_coordinates'),
        ("nprocesses", "KEYWORD_ONLY", 1), ("nthreads", "KEYWORD_ONLY", None),
        ("coord_method", "KEYWORD_ONLY", 'CoordinateRotationERFA'), ("coord_method_params", "KEYWORD_ONLY", None),
        ("force_use_type3", "KEYWORD_ONLY", False), ("force_use_ray", "KEYWORD_ONLY", False),
        ("trace_mem", "KEYWORD_ONLY", False), ("backend", "KEYWORD_ONLY", 'gpu'), ("max_memory", "KEYWORD_ONLY", INF),
        ("min_chunks", "KEYWORD_ONLY", 1), ("source_buffer", "KEYWORD_ONLY", 1.0), ("device", "KEYWORD_ONLY", 0),
        ("coord_mgr", "KEYWORD_ONLY", None), ("reference_compat", "KEYWORD_ONLY", True), ("astrom", "KEYWORD_ONLY", None),
        ("device_astrometry", "KEYWORD_ONLY", False),
    ],
    "torch_simulate_vis": [
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("kwargs", "VAR_KEYWORD", REQUIRED),
    ],
    "torch_simulate_vis_basis": [
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("beam_coefs", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("kwargs", "VAR_KEYWORD", REQUIRED),
    ],
    "torch_simulate_vis_basis_array": [
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("beam_coefs", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("antpos", "POSITIONAL_OR_KEYWORD", REQUIRED), ("antnums", "KEYWORD_ONLY", None),
        ("kwargs", "VAR_KEYWORD", REQUIRED),
    ],
    "torch_simulate_vis_array": [
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("antpos", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("antnums", "KEYWORD_ONLY", None), ("kwargs", "VAR_KEYWORD", REQUIRED),
    ],
    "torch_simulate_vis_sky": [
        ("fluxes", "POSITIONAL_OR_KEYWORD", REQUIRED), ("radec", "POSITIONAL_OR_KEYWORD", REQUIRED),
        ("kwargs", "VAR_KEYWORD", REQUIRED),
    ],
}


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_signatures_are_the_documented_ones(name):
    got = [(p.name, p.kind.name, p.default) for p in inspect.signature(getattr(adjoint, name)).parameters.values()]
    assert got == SIGNATURES[name]
    assert getattr(fftvis_amd, name) is getattr(adjoint, name)


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


class Mgr:
    """A caller's coordinate manager: only its presence matters to the checks."""


def _cfg(basis=False):
    """HERA-7, 20 sources, 2 channels, 2 times; ``basis``: two Airy dishes as basis beams, polarized."""
    cfg = synth.make_config("C1", nsrc=20, nfreq=2, ntimes=2)
    if basis:
        cfg.update(polarized=True, beam=[fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(13.0)],
                   beam_coefs=np.ones((len(cfg["ants"]), 2, 2), complex))
    return cfg


def _vis(cfg):
    nbls = len(cfg["baselines"])
    return np.zeros((2, 2, 2, 2, nbls) if cfg["polarized"] else (2, 2, nbls), complex)


# pass: (basis beams, takes vis, takes fluxes)
PASSES = {
    "simulate_vis_adjoint": (False, True, False),
    "simulate_vis_basis_adjoint": (True, True, True),
    "simulate_vis_position_adjoint": (False, True, True),
    "simulate_vis_source_adjoint": (False, True, True),
    "simulate_vis_jvp": (False, False, True),
    "simulate_vis_basis_jvp": (True, False, True),
}


def _call(name, vis=None, **changes):
    """The pass on the smallest configuration with ``changes`` to its keywords (``vis``: another gradient)."""
    basis, takes_vis, takes_fluxes = PASSES[name]
    cfg = _cfg(basis)
    if not takes_fluxes:
        del cfg["fluxes"]
    kw = dict(cfg, **changes)
    fn = getattr(adjoint, name)
    return fn(_vis(cfg) if vis is None else vis, **kw) if takes_vis else fn(**kw)


NO_BASIS = {
    "simulate_vis_adjoint": "simulate_vis_adjoint does not support basis beams (beam_coefs)",
    "simulate_vis_position_adjoint": "simulate_vis_position_adjoint does not support basis beams (beam_coefs): "
                                     "simulate_vis_basis_adjoint(wrt='ants') does",
    "simulate_vis_source_adjoint": "simulate_vis_source_adjoint does not support basis beams (beam_coefs)",
    "simulate_vis_jvp": "simulate_vis_jvp does not support basis beams (beam_coefs): simulate_vis_basis_jvp(d_ants=) does",
}
BAD_WRT = {
    "simulate_vis_basis_adjoint": "wrt must name some of 'fluxes', 'beam_coefs', 'ants' and 'baselines', got 'antennas'",
    "simulate_vis_position_adjoint": "wrt must name 'ants', 'baselines' or both, got 'antennas'",
    "simulate_vis_source_adjoint": "wrt must name 'topo', 'radec' or both, got 'antennas'",
}


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


@pytest.mark.parametrize("name", list(PASSES))
def test_wrong_backend(name):
    with _raises(ValueError, "Unsupported backend: cpu"):
        _call(name, backend="cpu")


@pytest.mark.parametrize("name", [n for n, p in PASSES.items() if p[1]])
def test_wrong_vis_shape(name):
    vis = _vis(_cfg(PASSES[name][0]))
    with _raises(ValueError, f"vis must have simulate_vis's output shape {vis.shape}, got {vis[:1].shape}"):
        _call(name, vis=vis[:1])
    with _raises(ValueError, f"vis must have simulate_vis's output shape {vis.shape}, got {vis[..., :-1].shape}"):
        _call(name, vis=vis[..., :-1])


@pytest.mark.parametrize("name", [n for n, p in PASSES.items() if p[2]])
def test_wrong_fluxes_shape(name):
    for bad in (np.ones((19, 2)), np.ones((20, 3)), np.ones((20, 2, 3))):
        with _raises(ValueError, "fluxes must have shape (nsources, nfreqs[, 4])"):
            _call(name, fluxes=bad)


@pytest.mark.parametrize("name", list(NO_BASIS))
def test_beam_coefs_where_unsupported(name):
    with _raises(NotImplementedError, NO_BASIS[name]):
        _call(name, beam_coefs=np.ones((7, 1, 2), complex))


@pytest.mark.parametrize("name", list(BAD_WRT))
def test_bad_wrt(name):
    with _raises(ValueError, BAD_WRT[name]):
        _call(name, wrt="antennas")
    for wrt in ((), ("ants", "ants"), ("topo", "topo"), ("fluxes", "positions")):
        with pytest.raises(ValueError, match="^wrt must name "):
            _call(name, wrt=wrt)


@pytest.mark.parametrize("name", ["simulate_vis_jvp", "simulate_vis_basis_jvp"])
def test_antenna_tangent_given_twice(name):
    with _raises(ValueError, "give the antenna tangent as d_ants or as d_baselines, not both"):
        _call(name, d_ants=np.zeros((7, 3)), d_baselines=np.zeros((21, 3)))


def test_source_tangent_given_twice():
    with _raises(ValueError, "give the source tangent as d_radec or as d_topo, not both"):
        _call("simulate_vis_jvp", d_radec=np.zeros((20, 2)), d_topo=np.zeros((2, 20, 3)))


def test_radec_chain_with_a_coordinate_manager():
    with _raises(ValueError, "wrt='radec' needs this package's own chain from (ra, dec) to the topocentric vectors; with "
                             "coord_mgr= the chain is the manager's: ask for wrt='topo' and apply its Jacobian"):
        _call("simulate_vis_source_adjoint", wrt="radec", coord_mgr=Mgr())
    with _raises(ValueError, "d_radec needs this package's own chain from (ra, dec) to the topocentric vectors; with "
                             "coord_mgr= the chain is the manager's: apply its Jacobian and pass d_topo"):
        _call("simulate_vis_jvp", d_radec=np.zeros((20, 2)), coord_mgr=Mgr())
    # ... and with a matvis manager the engine would build
    with _raises(ValueError, "wrt='radec' needs coord_method='SiderealRotation' or device astrometry (astrom= / "
                             "device_astrometry=True); coord_method='CoordinateRotationERFA' builds a matvis manager "
                             "whose chain is its own: ask for wrt='topo'"):
        _call("simulate_vis_source_adjoint", wrt=("topo", "radec"), coord_method="CoordinateRotationERFA")
    with _raises(ValueError, "d_radec needs coord_method='SiderealRotation' or device astrometry (astrom= / "
                             "device_astrometry=True); coord_method='CoordinateRotationERFA' builds a matvis manager "
                             "whose chain is its own: pass d_topo"):
        _call("simulate_vis_jvp", d_radec=np.zeros((20, 2)), coord_method="CoordinateRotationERFA")


def test_the_tangents_of_nothing_are_zeros_without_an_engine():
    for name in ("simulate_vis_jvp", "simulate_vis_basis_jvp"):
        z = _call(name)
        assert z.shape == _vis(_cfg(PASSES[name][0])).shape and z.dtype == np.complex128 and not z.any()


class Handle:
    """Records what the block loops ask of a ``SimHandle``."""

    def __init__(self):
        self.calls = []

    def set_topo(self, topo):
        self.calls.append(("set_topo", topo.shape, topo[:, 0, 0].tolist()))

    def __getattr__(self, name):
        if not name.startswith("run_"):
            raise AttributeError(name)
        return lambda ta, te_, f0, f1, *rest: self.calls.append((name, ta, te_, f0, f1) + tuple(
            x if isinstance(x, bool) else None if x is None else tuple(x.shape) for x in rest))


class TopoMgr:
    """A matvis-style manager of 4 sources whose vectors at time index ti are all ti."""

    def rotate(self, ti):
        self.all_coords_topo = np.full((3, 4), float(ti))


def test_time_blocks_without_a_coordinate_manager():
    h = Handle()
    assert list(gpu_simulate._time_blocks(h, 1, 6, 2, None)) == [(1, 3, 1, 3), (3, 5, 3, 5), (5, 6, 5, 6)]
    assert h.calls == []
    assert list(gpu_simulate._time_blocks(h, 1, 6, 0, None))[0] == (1, 2, 1, 2)  # a block is one step at least
    assert list(gpu_simulate._time_blocks(h, 1, 6, 9, None)) == [(1, 6, 1, 6)]
    assert list(gpu_simulate._time_blocks(h, 3, 3, 2, None)) == []


def test_time_blocks_stream_a_coordinate_manager():
    """The handle runs every block as (0, its length) on the vectors of the block's own time indices, set before the
    block is yielded."""
    h = Handle()
    seen = []
    for blk in gpu_simulate._time_blocks(h, 1, 6, 2, TopoMgr()):
        seen.append((blk, len(h.calls)))
    assert seen == [((1, 3, 0, 2), 1), ((3, 5, 0, 2), 2), ((5, 6, 0, 1), 3)]
    assert h.calls == [("set_topo", (2, 3, 4), [1.0, 2.0]), ("set_topo", (2, 3, 4), [3.0, 4.0]), ("set_topo", (1, 3, 4), [5.0])]


@pytest.mark.parametrize("mgr", [None, TopoMgr()])
def test_adjoint_loop_accumulates_after_the_first_block(mgr):
    h = Handle()
    g, gflux = np.zeros((2, 5, 21), complex), np.ones((20, 2))
    assert gpu_simulate._run_adjoint(h, g, gflux, 1, 6, 0, 2, 2, mgr) is gflux
    runs = [c for c in h.calls if c[0] == "run_adjoint"]
    ranges = [(0, 2), (0, 2), (0, 1)] if mgr is not None else [(1, 3), (3, 5), (5, 6)]
    assert [c[1:3] for c in runs] == ranges
    assert [c[5] for c in runs] == [(2, 2, 21), (2, 2, 21), (2, 1, 21)]  # each block's slice of g
    assert [c[-1] for c in runs] == [False, True, True]  # accumulate
    assert len([c for c in h.calls if c[0] == "set_topo"]) == (3 if mgr is not None else 0)


def test_adjoint_loop_variants_and_the_empty_range():
    g = np.zeros((2, 5, 2, 2, 21), complex)
    h = Handle()
    gflux, gcoefs, gbls = np.ones((20, 2)), np.ones((7, 2, 2), complex), np.ones((21, 3))
    out = gpu_simulate._run_adjoint(h, g, gflux, 0, 5, 0, 2, 3, None, gcoefs=gcoefs, basis=True, gbls=gbls)
    assert out[0] is gflux and out[1] is gcoefs and out[2] is gbls
    assert [(c[0], c[1], c[2], c[-1]) for c in h.calls] == [
        ("run_basis_adjoint", 0, 3, False), ("run_basis_position_adjoint", 0, 3, False),
        ("run_basis_adjoint", 3, 5, True), ("run_basis_position_adjoint", 3, 5, True)]
    h = Handle()  # the sources' rows are per block, never accumulated
    gtopo = np.ones((5, 20, 3))
    gpu_simulate._run_adjoint(h, g, gtopo, 0, 5, 0, 2, 2, None, sources=True)
    assert [(c[1], c[2], c[6], c[-1]) for c in h.calls] == [(0, 2, (2, 20, 3), False), (2, 4, (2, 20, 3), False),
                                                           (4, 5, (1, 20, 3), False)]
    h = Handle()  # no time steps: nothing runs and the outputs are zeroed
    gpu_simulate._run_adjoint(h, g[:, :0], gflux, 2, 2, 0, 2, 2, None, gcoefs=gcoefs, basis=True, gbls=gbls)
    assert h.calls == [] and not gflux.any() and not gcoefs.any() and not gbls.any()
    gpos = np.ones((21, 3))
    gpu_simulate._run_adjoint(h, g[:, :0], gpos, 2, 2, 0, 2, 2, None, positions=True)
    assert h.calls == [] and not gpos.any()


@pytest.mark.parametrize("axis", [1, 2])
def test_tangent_loops_write_whole_results_in_place_and_blocks_through_scratch(axis):
    shape = (2, 5, 21) if axis == 1 else (3, 2, 5, 21)
    dv = np.zeros(shape, complex)
    blk, dst = gpu_simulate._result_block(dv, axis, 0, 5, True)
    assert blk is dv and dst is None
    blk, dst = gpu_simulate._result_block(dv, axis, 1, 3, False)
    assert blk.shape == shape[:axis] + (2,) + shape[axis + 1:] and blk.flags.c_contiguous and blk.dtype == dv.dtype
    blk[...] = 1
    dst[...] = blk
    assert dv.take(range(1, 3), axis=axis).all() and not dv.take([0, 3, 4], axis=axis).any()
    h = Handle()
    run = gpu_simulate._run_tangent if axis == 1 else gpu_simulate._run_basis_tangent
    tangents = (np.zeros((21, 3)), np.zeros((5, 20, 3))) if axis == 1 else (np.zeros((3, 7, 2, 2), complex),)
    assert run(h, *tangents, dv, 0, 5, 0, 2, 2, None) is dv
    assert [c[1:3] for c in h.calls] == [(0, 2), (2, 4), (4, 5)]
    assert [c[-1] for c in h.calls] == [shape[:axis] + (n,) + shape[axis + 1:] for n in (2, 2, 1)]
    if axis == 1:  # every block takes its rows of dtopo
        assert [c[-2] for c in h.calls] == [(2, 20, 3), (2, 20, 3), (1, 20, 3)]
    h = Handle()  # one block that is the whole result is written in place
    run(h, *tangents, dv, 0, 5, 0, 2, 5, None)
    assert [c[1:3] for c in h.calls] == [(0, 5)] and h.calls[0][-1] == shape
