"""CPU tests of the Gauss-Newton product's surface (``simulate_vis_gauss_newton``, ``fv_weight_rows``,
``fv_sim_weight_block``): the exports, the signatures, the argument errors raised before any engine exists --
``wrapper.create_simulation_engine`` is replaced by a function that fails the test, as in ``test_objective_host`` -- the C
entry points' argument checks through a null handle and null pointers, and the numpy references themselves."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import gauss_newton_refs as gnr
from tests.objective_refs import row_sums_exact
from tests.test_derivative_api_host import REQUIRED, Mgr, _cfg, _vis
from tests.test_sky_adjoint_host import _COMMON, _TAIL

_HEAD = [(n, "POSITIONAL_OR_KEYWORD", REQUIRED)
         for n in ("ants", "fluxes", "ra", "dec", "freqs", "times", "beam", "telescope_loc")]
_OWN = [("d_fluxes", "KEYWORD_ONLY", None), ("d_ants", "KEYWORD_ONLY", None), ("d_baselines", "KEYWORD_ONLY", None),
        ("d_radec", "KEYWORD_ONLY", None), ("d_topo", "KEYWORD_ONLY", None), ("d_beam_coefs", "KEYWORD_ONLY", None),
        ("weights", "KEYWORD_ONLY", None), ("wrt", "KEYWORD_ONLY", None), ("quad_per", "KEYWORD_ONLY", "total"),
        ("return_gvis", "KEYWORD_ONLY", False), ("adjoint_path", "KEYWORD_ONLY", "type3"), ("beam_coefs", "KEYWORD_ONLY", None),
        ("full_stokes", "KEYWORD_ONLY", None)]


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _call(basis=False, **changes):
    cfg = _cfg(basis)
    if not any(k.startswith("d_") for k in changes):
        changes["d_fluxes"] = np.ones_like(cfg["fluxes"])
    return adjoint.simulate_vis_gauss_newton(**dict(cfg, **changes))


def test_exported_with_the_documented_signature():
    fn = adjoint.simulate_vis_gauss_newton
    got = [(p.name, p.kind.name, p.default) for p in inspect.signature(fn).parameters.values()]
    # after its own keywords, the keywords simulate_vis_chi2 takes
    assert got == _HEAD + _OWN + _COMMON + _TAIL
    chi2 = [p.name for p in inspect.signature(adjoint.simulate_vis_chi2).parameters.values()]
    assert set(chi2) - {"data", "chi2_per"} <= {p[0] for p in got}
    assert fftvis_amd.simulate_vis_gauss_newton is fn
    for word in ("the gradient in the same call", "damping", "several directions per call", "hvp", "sharding"):
        assert word in fn.__doc__, word
    assert "J^T J product" not in adjoint.simulate_vis_chi2.__doc__


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_weight_rows\(int device, int precision, int64_t nrows, int64_t row_len, int nparts, "
                     r"const void \*const \*parts,\s+const void \*weights, double \*q_rows\);", header, re.M)
    assert re.search(r"^int fv_sim_weight_block\(fv_sim \*h, int t0, int t1, int f0, int f1, int nparts, "
                     r"void \*const \*parts_dev, const void \*weights,\s+int weights_on_device, double \*q_ft\);", header, re.M)
    assert len(_lib.SYMBOLS["fv_weight_rows"][1]) == 8 and len(_lib.SYMBOLS["fv_sim_weight_block"][1]) == 10
    assert hasattr(_lib.lib(), "fv_weight_rows") and hasattr(_lib.lib(), "fv_sim_weight_block")
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.weight_block)
    assert "gauss_newton_of" in inspect.signature(gpu_simulate.GPUSimulationEngine.simulate).parameters


def test_the_references_compute_what_the_header_and_the_docstring_state():
    header = " ".join(open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read().split())
    header = header.replace(" * ", " ")  # (the comment's line starts)
    # the order of the adds, the rounding of G and the flag rule of gnr.weight_rows are fv_weight_rows' documented ones
    for stated in ("U = ((P_0 + P_1) + P_2) + P_3", "G = 2 (w U) (one rounding per component and an exact doubling)",
                   "q_rows[i] = sum over row i of w |U|^2 with every term formed and added in fp64",
                   "A weight of exactly 0 flags its sample: G is exactly 0 there, nothing is added and the parts are not used"):
        assert stated in header, stated
    doc = " ".join(adjoint.simulate_vis_gauss_newton.__doc__.split())
    for stated in ("``quad = sum w |U|^2``", "``G = 2 w U``", "``<p, H p> = 2 quad``"):  # gnr.quad_and_gvis, gnr.inner
        assert stated in doc, stated
    rng = np.random.default_rng(0)
    for cdt, rdt in ((np.complex128, np.float64), (np.complex64, np.float32)):
        parts = [(rng.normal(size=(3, 5)) + 1j * rng.normal(size=(3, 5))).astype(cdt) for _ in range(3)]
        w = rng.uniform(0.5, 2.0, size=(3, 5)).astype(rdt)
        w[1, 2] = 0
        parts[1][1, 2] = np.nan
        G, U, terms = gnr.weight_rows(parts, w)
        assert G.dtype == cdt and U.dtype == cdt and terms.dtype == np.float64 and np.isfinite(G).all()
        assert G[1, 2] == 0 and U[1, 2] == 0 and terms[1, 2] == 0
        keep = w != 0
        exact = sum(p.astype(np.complex128) for p in parts)
        tol = 8 * np.finfo(rdt).eps
        assert np.allclose(U[keep], exact[keep], rtol=tol, atol=tol)
        assert np.allclose(G[keep], 2 * w[keep] * exact[keep], rtol=tol, atol=tol)
        assert np.array_equal(gnr.weight_rows(parts[:1])[0], 2 * parts[0])  # no weights, one part: an exact doubling
        q = row_sums_exact(terms)
        assert q.shape == (3,) and np.allclose(q, (w * np.abs(U) ** 2).sum(axis=-1), rtol=tol)
    U = rng.normal(size=(2, 3, 4)) + 1j * rng.normal(size=(2, 3, 4))
    w = rng.uniform(0.5, 2.0, size=U.shape)
    w[0, 0, 0] = 0
    rows, G = gnr.quad_and_gvis(np.where(w != 0, U, np.nan), w)
    assert rows.shape == (2, 3) and G[0, 0, 0] == 0 and np.allclose(rows.sum(), (w * np.abs(U) ** 2).sum(), rtol=1e-14)
    assert np.allclose(gnr.inner(U, G), 2 * rows.sum(), rtol=1e-14)  # <U, 2 w U> = 2 quad


def test_no_direction_and_exclusive_directions():
    cfg = _cfg()
    with _raises(ValueError, "simulate_vis_gauss_newton needs a direction: d_fluxes, d_ants, d_baselines, d_radec, d_topo or "
                             "d_beam_coefs"):
        adjoint.simulate_vis_gauss_newton(**cfg)
    with _raises(ValueError, "give the antenna tangent as d_ants or as d_baselines, not both"):
        _call(d_ants=np.zeros((7, 3)), d_baselines=np.zeros((len(cfg["baselines"]), 3)))
    with _raises(ValueError, "give the source tangent as d_radec or as d_topo, not both"):
        _call(d_radec=np.zeros((20, 2)), d_topo=np.zeros((2, 20, 3)), coord_method="SiderealRotation")


@pytest.mark.parametrize("basis", [False, True])
def test_wrong_shapes(basis):
    cfg = _cfg(basis)
    nbls = len(cfg["baselines"])
    sid = dict(coord_method="SiderealRotation")
    with _raises(ValueError, "d_fluxes must have fluxes' shape (20, 2), got (19, 2)"):
        _call(basis, d_fluxes=np.ones((19, 2)))
    with _raises(ValueError, "d_ants must have shape (7, 3), got (6, 3)"):
        _call(basis, d_ants=np.zeros((6, 3)))
    with _raises(ValueError, f"d_baselines must have shape ({nbls}, 3), got ({nbls}, 2)"):
        _call(basis, d_baselines=np.zeros((nbls, 2)))
    with _raises(ValueError, "d_radec must have shape (20, 2), got (20, 3)"):
        _call(basis, d_radec=np.zeros((20, 3)), **sid)
    with _raises(ValueError, "d_topo must have shape (2, 20, 3), got (1, 20, 3)"):
        _call(basis, d_topo=np.zeros((1, 20, 3)))
    vis = _vis(cfg)
    with _raises(ValueError, f"weights must have simulate_vis's output shape {vis.shape}, got {vis[:1].shape}"):
        _call(basis, weights=np.ones(vis[:1].shape))
    with _raises(ValueError, "weights must be real (inverse variances; 0 flags a sample)"):
        _call(basis, weights=np.ones(vis.shape, complex))
    with _raises(ValueError, "fluxes must have shape (nsources, nfreqs[, 4])"):
        _call(basis, fluxes=np.ones((19, 2)))


def test_beam_coefs_directions():
    with _raises(ValueError, "d_beam_coefs needs beam_coefs (basis beams)"):
        _call(d_beam_coefs=np.ones((7, 2, 2), complex))
    with _raises(ValueError, "wrt='beam_coefs' needs beam_coefs (basis beams)"):
        _call(wrt=("fluxes", "beam_coefs"))
    with _raises(ValueError, "d_beam_coefs must be one direction of beam_coefs' shape (7, 2, 2) (a stack is not covered), got "
                             "(3, 7, 2, 2)"):
        _call(True, d_beam_coefs=np.ones((3, 7, 2, 2), complex))
    with _raises(ValueError, "d_beam_coefs must be one direction of beam_coefs' shape (7, 2, 2) (a stack is not covered), got "
                             "(7, 2, 1)"):
        _call(True, d_beam_coefs=np.ones((7, 2, 1), complex))
    with _raises(ValueError, "d_beam_coefs must be complex, like beam_coefs"):
        _call(True, d_beam_coefs=np.ones((7, 2, 2)))
    with _raises(ValueError, "Basis decomposition is not compatible with unpolarized simulations. Set polarized=True to "
                             "use beam_coefs."):
        _call(True, polarized=False)
    with _raises(ValueError, "beam_coefs must have shape (nant, nbasis, nfreqs)"):
        _call(True, beam_coefs=np.ones((7, 3, 2), complex))


def test_bad_wrt_quad_per_adjoint_path_and_backend():
    with _raises(ValueError, "wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs', got "
                             "'antennas'"):
        _call(wrt="antennas")
    for wrt in (("fluxes", "fluxes"), ("topo", "radec", "topo"), ("fluxes", "positions")):
        with pytest.raises(ValueError, match="^wrt must name "):
            _call(wrt=wrt)
    with _raises(ValueError, "quad_per must be 'total' or 'freq_time', got 'row'"):
        _call(quad_per="row")
    with _raises(ValueError, "adjoint_path must be 'type3', 'type2' or 'auto', got 'type1'"):
        _call(adjoint_path="type1")
    for wrt in (None, (), "fluxes", ("ants", "topo")):
        with _raises(ValueError, "Unsupported backend: cpu"):
            _call(backend="cpu", wrt=wrt)
    with _raises(ValueError, "full_stokes=True does not match fluxes of shape (20, 2)"):
        _call(full_stokes=True, polarized=True)


@pytest.mark.parametrize("basis", [False, True])
def test_radec_follows_the_jvps_and_the_adjoints_coordinate_rules(basis):
    default = inspect.signature(adjoint.simulate_vis_gauss_newton).parameters["coord_method"].default
    for asked, kw in (("d_radec", dict(d_radec=np.zeros((20, 2)), wrt="fluxes")), ("wrt='radec'", dict(wrt=("fluxes", "radec")))):
        with _raises(ValueError, f"{asked} needs this package's own chain from (ra, dec) to the topocentric vectors; with "
                                 "coord_mgr= the chain is the manager's: pass d_topo and ask for wrt='topo', and apply its "
                                 "Jacobian"):
            _call(basis, coord_mgr=Mgr(), **kw)
        with _raises(ValueError, f"{asked} needs coord_method='SiderealRotation' or device astrometry (astrom= / "
                                 f"device_astrometry=True); coord_method='CoordinateRotationERFA' builds a matvis manager "
                                 "whose chain is its own: pass d_topo and ask for wrt='topo'"):
            _call(basis, coord_method=default, **kw)


def test_fv_weight_rows_argument_checks():
    L = _lib.lib()
    fn = L.fv_weight_rows
    buf = (ctypes.c_double * 8)()
    parts = (ctypes.c_void_p * 4)(*[ctypes.addressof(buf)] * 4)
    hole = (ctypes.c_void_p * 2)(ctypes.addressof(buf), None)
    for precision in (0, 3):
        assert fn(0, precision, 1, 1, 1, parts, None, buf) == 1
        assert b"precision must be 1 or 2" in L.fv_last_error()
    for nrows, row_len in [(-1, 1), (1, -1)]:
        assert fn(0, 2, nrows, row_len, 1, parts, None, buf) == 1
        assert b"negative shape" in L.fv_last_error()
    for nparts in (0, 5, -1):
        assert fn(0, 2, 1, 1, nparts, parts, None, buf) == 1
        assert b"nparts must be 1 .. 4" in L.fv_last_error()
    assert fn(0, 2, 1, 1, 1, None, None, buf) == 1
    assert fn(0, 2, 1, 1, 2, hole, None, buf) == 1
    assert b"null part" in L.fv_last_error()
    assert fn(0, 2, 1, 1, 1, parts, None, None) == 1
    assert b"null q_rows" in L.fv_last_error()


def test_fv_sim_weight_block_argument_checks():
    L = _lib.lib()
    fn = L.fv_sim_weight_block
    buf = (ctypes.c_double * 8)()
    parts = (ctypes.c_void_p * 4)(*[ctypes.addressof(buf)] * 4)
    hole = (ctypes.c_void_p * 2)(ctypes.addressof(buf), None)
    assert fn(None, 0, 1, 0, 1, 1, parts, buf, 0, buf) == 1
    assert b"null handle" in L.fv_last_error()
    assert fn(None, 0, 1, 0, 1, 4, parts, None, 0, buf) == 1  # weights may be null: the handle is what is missing
    assert b"null handle" in L.fv_last_error()
    for nparts in (0, 5):
        assert fn(None, 0, 1, 0, 1, nparts, parts, None, 0, buf) == 1
        assert b"nparts must be 1 .. 4" in L.fv_last_error()
    assert fn(None, 0, 1, 0, 1, 1, None, None, 0, buf) == 1
    assert fn(None, 0, 1, 0, 1, 2, hole, None, 0, buf) == 1
    assert b"null part" in L.fv_last_error()
    assert fn(None, 0, 1, 0, 1, 1, parts, None, 0, None) == 1
    assert b"null q_ft" in L.fv_last_error()
    for flag in (2, -1):
        assert fn(None, 0, 1, 0, 1, 1, parts, buf, flag, buf) == 1
        assert b"on_device" in L.fv_last_error()
