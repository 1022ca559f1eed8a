"""CPU tests of the Gauss-Newton product with per-antenna gains (``simulate_vis_gain_gauss_newton``, ``fv_gain_weight_rows``,
``fv_sim_gain_weight_block``): the numpy reference against the stencil of the gained forward and against the already-pinned
``gain_refs.chi2_gains``, the C surface, and the argument errors raised before any engine exists or any device is
touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import gain_gauss_newton_refs as ggr
from tests import gain_refs
from tests.test_derivative_api_host import _cfg
from tests.test_gains_host import _case, _shapes


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _gn_case(polarized, seed=0, nparts=2):
    """``test_gains_host._case`` with tangent parts and a gain direction; NaN parts and V under the flags."""
    V, _, w, g, a1, a2 = _case(polarized, seed)
    rng = np.random.default_rng(seed + 100)

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    parts = [c(V.shape) for _ in range(nparts)]
    dg = c(g.shape)
    return parts, V, w, g, dg, a1, a2


@pytest.mark.parametrize("polarized", [False, True])
def test_reference_tangent_is_the_stencil_of_the_gained_forward(polarized):
    parts, V, w, g, dg, a1, a2 = _gn_case(polarized)
    U = parts[0] + parts[1]
    Up = ggr.tangent(parts, V, g, dg, a1, a2)
    # eps -> apply_gains(V + eps U, g + eps dg) is a cubic in eps: the five-point stencil is exact up to rounding
    fd = gain_refs.five_point(lambda h: gain_refs.apply_gains(V + h * U, g + h * dg, a1, a2), 0.25)
    worst = float(np.abs(fd - Up).max() / np.abs(Up).max())
    print("gain Gauss-Newton reference: stencil against U'", worst)
    assert worst <= 1e-12  # (test_gains_host's stencil tolerance)
    # without a gain direction dm = 0, and without parts U = 0
    assert np.allclose(ggr.tangent(parts, V, g, None, a1, a2), gain_refs.apply_gains(U, g, a1, a2), rtol=1e-15)
    assert np.allclose(ggr.tangent([], V, g, dg, a1, a2), Up - gain_refs.apply_gains(U, g, a1, a2), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("nparts,direction", [(2, True), (1, False), (0, True)])
@pytest.mark.parametrize("polarized", [False, True])
def test_reference_is_the_gain_objective_reference_with_this_residual(polarized, nparts, direction):
    """chi2_gains(V, d, ...) with d = m V - U' has V' - d = U': its rows, G', G and ggains are this reference's."""
    parts, V, w, g, dg, a1, a2 = _gn_case(polarized, seed=4, nparts=nparts)
    dg = dg if direction else None
    used = w != 0
    Up = ggr.tangent(parts, V, g, dg, a1, a2)
    d = gain_refs.apply_gains(V, g, a1, a2) - Up
    Vn = np.where(used, V, np.nan)
    pn = [np.where(used, p, np.nan) for p in parts]
    rows, Gp, G, hg = ggr.gain_gauss_newton(pn, Vn, w, g, dg, a1, a2)
    rows0, Gp0, G0, hg0 = gain_refs.chi2_gains(V, d, w, g, a1, a2)
    assert np.isfinite(G).all() and np.isfinite(hg).all() and np.all(G[~used] == 0) and np.all(hg[..., -1] == 0)
    scale = np.abs(Gp0).max()
    for got, exp in ((rows, rows0), (Gp, Gp0), (G, G0), (hg, hg0)):
        assert got.shape == exp.shape and np.abs(got - exp).max() <= 1e-13 * max(scale, np.abs(exp).max())
    # <p, H p> = 2 quad on the reference: p's sky part pairs with G through U (J p = U), the gains' with hgains
    U = sum(parts) if parts else np.zeros_like(V)
    sky = float(np.sum((np.conj(np.where(used, U, 0)) * G).real))
    gains = ggr.inner_gains(dg, hg) if direction else 0.0
    assert abs(sky + gains - 2 * rows.sum()) <= 1e-12 * 2 * rows.sum()


_NEW = {"fv_gain_weight_rows": 16, "fv_sim_gain_weight_block": 17}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_gain_weight_rows\(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, "
                     r"const int \*ant1,\s+const int \*ant2, const void \*gains, const void \*d_gains, int nparts, "
                     r"const void \*const \*parts, void \*vis,\s+const void \*weights, double \*q_rows, void \*hgains\);",
                     header, re.M)
    assert re.search(r"^int fv_sim_gain_weight_block\(fv_sim \*h, int t0, int t1, int f0, int f1, int nparts, "
                     r"void \*const \*parts_dev, void \*vis_dev,\s+const void \*weights, int weights_on_device, "
                     r"const void \*gains, int gains_on_device,\s+const void \*d_gains, int d_gains_on_device, double \*q_ft, "
                     r"void \*hgains, int hgains_on_device\);", header, re.M)
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.gain_weight_block)
    flat = " ".join(header.split()).replace(" * ", " ")
    for stated in ("m = conj(g1) g2 dm = conj(h1) g2 + conj(g1) h2 (dm = 0 without a gain direction)",
                   "U' = m U + dm V (the tangent of V' along p = (sky directions, dg))",
                   "G' = 2 (w U') quad row += w |U'|^2 (terms formed and added in fp64)",
                   "stored G = conj(m) G' (what the public sky adjoints read: their result on it is H p for their block)",
                   "hgains[a, f] = sum_{k: a1=a, p=f} conj(G') g2 V + sum_{k: a2=a, q=f} G' g1 conj(V)"):
        assert stated in flat, stated


def test_exported_with_the_plain_signature_plus_two_keywords():
    plain = inspect.signature(adjoint.simulate_vis_gauss_newton).parameters
    own = inspect.signature(adjoint.simulate_vis_gain_gauss_newton).parameters
    names = list(plain)
    at = names.index("d_beam_coefs") + 1
    assert list(own) == names[:8] + ["gains"] + names[8:at] + ["d_gains"] + names[at:]
    assert all(own[n].kind == plain[n].kind and own[n].default == plain[n].default for n in plain)
    assert own["gains"].kind.name == "KEYWORD_ONLY" and own["gains"].default is inspect.Parameter.empty
    assert own["d_gains"].kind.name == "KEYWORD_ONLY" and own["d_gains"].default is None
    assert "gains" not in plain and "d_gains" not in plain
    assert fftvis_amd.simulate_vis_gain_gauss_newton is adjoint.simulate_vis_gain_gauss_newton
    doc = " ".join(adjoint.simulate_vis_gain_gauss_newton.__doc__.split())
    for word in ("``U' = m U + dm V``", "``G = conj(m) 2 w U'``", "NOT", "every call reruns the forward",
                 "several directions per call", "the gradient in the same call", "leakage", "sharding", "hvp"):
        assert word in doc, word
    assert "simulate_vis_gain_gauss_newton" in adjoint.simulate_vis_gain_chi2.__doc__
    assert "simulate_vis_gain_gauss_newton" in adjoint.simulate_vis_gauss_newton.__doc__


def _call(basis=False, **changes):
    cfg = _cfg(basis)
    if not any(k.startswith("d_") for k in changes):
        changes["d_fluxes"] = np.ones_like(cfg["fluxes"])
    return adjoint.simulate_vis_gain_gauss_newton(**dict(cfg, **changes))


def test_the_plain_call_rejects_the_gains_name_up_front():
    """(the parent ran the whole engine and ended in a KeyError)"""
    cfg = _cfg()
    for wrt in ("gains", ("fluxes", "gains")):
        with pytest.raises(ValueError, match="^wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and "
                                             "'beam_coefs', got "):
            adjoint.simulate_vis_gauss_newton(**dict(cfg, d_fluxes=np.ones_like(cfg["fluxes"]), wrt=wrt))
    with pytest.raises(TypeError, match="gains"):
        adjoint.simulate_vis_gauss_newton(**dict(cfg, d_fluxes=np.ones_like(cfg["fluxes"]), gains=np.ones(_shapes(cfg)[0], complex)))


@pytest.mark.parametrize("basis", [False, True])
def test_bad_gains_and_directions(basis):
    cfg = _cfg(basis)
    const, per_time = _shapes(cfg)
    ones = np.ones(const, complex)
    with _raises(ValueError, f"gains must have shape {const} or {per_time}, got {const[:-1]}"):
        _call(basis, gains=np.ones(const[:-1], complex))
    with _raises(ValueError, "gains must be complex (one gain per antenna, feed and channel)"):
        _call(basis, gains=np.ones(const))
    with _raises(ValueError, "gains must be finite"):
        _call(basis, gains=ones * np.nan)
    # d_gains: gains' own shape (time-constant or per time as gains is), complex, finite
    for bad in (per_time, const[:-1], (const[0] + 1,) + const[1:]):
        with _raises(ValueError, f"d_gains must have gains' shape {const}, got {bad}"):
            _call(basis, gains=ones, d_gains=np.ones(bad, complex))
    with _raises(ValueError, f"d_gains must have gains' shape {per_time}, got {const}"):
        _call(basis, gains=np.ones(per_time, complex), d_gains=ones)
    with _raises(ValueError, "d_gains must be complex, like gains"):
        _call(basis, gains=ones, d_gains=np.ones(const))
    for value in (np.nan, complex(1, np.inf)):
        dg = ones.copy()
        dg[(0,) * dg.ndim] = value
        with _raises(ValueError, "d_gains must be finite"):
            _call(basis, gains=ones, d_gains=dg)
    # the gains' names without gains
    for wrt in ("gains", ("fluxes", "gains")):
        with _raises(ValueError, "wrt='gains' needs gains="):
            _call(basis, gains=None, wrt=wrt)
    with _raises(ValueError, "d_gains needs gains="):
        _call(basis, gains=None, d_gains=ones)
    with _raises(ValueError, "d_gains needs gains="):
        adjoint.simulate_vis_gain_gauss_newton(**dict(cfg, gains=None, d_gains=ones))
    with _raises(ValueError, "simulate_vis_gain_gauss_newton needs a direction: d_fluxes, d_ants, d_baselines, d_radec, d_topo, "
                             "d_beam_coefs or d_gains"):
        adjoint.simulate_vis_gain_gauss_newton(**dict(cfg, gains=ones))
    with _raises(ValueError, "wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and 'gains', "
                             "got 'antennas'"):
        _call(basis, gains=ones, wrt="antennas")
    with pytest.raises(ValueError, match="^wrt must name "):
        _call(basis, gains=ones, wrt=("gains", "gains"))
    with pytest.raises(TypeError, match="gains"):
        adjoint.simulate_vis_gain_gauss_newton(**dict(cfg, d_fluxes=np.ones_like(cfg["fluxes"])))  # gains is required


def test_d_gains_alone_passes_the_argument_checks(monkeypatch):
    """``d_gains`` alone is a valid call: it reaches the engine."""
    cfg = _cfg()
    ones = np.ones(_shapes(cfg)[0], complex)

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)
    with pytest.raises(Reached):
        adjoint.simulate_vis_gain_gauss_newton(**dict(cfg, gains=ones, d_gains=ones))


def test_fv_gain_weight_rows_argument_checks():
    L = _lib.lib()
    fn = L.fv_gain_weight_rows
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    parts = (ctypes.c_void_p * 4)(*[ctypes.addressof(buf)] * 4)
    hole = (ctypes.c_void_p * 4)(ctypes.addressof(buf), None, None, None)

    def call(precision=2, nrows=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, g=buf, dg=None, nparts=1, p=parts, v=None, q=buf, hg=None):
        return fn(0, precision, nrows, nbls, tpol, nant, a1, a2, g, dg, nparts, p, v, None, q, hg)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and b"fv_gain_weight_rows: tpol must be 1 or 4" in L.fv_last_error()
    for kw in (dict(nrows=-1), dict(nbls=-1)):
        assert call(**kw) == 1 and b"fv_gain_weight_rows: negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and b"fv_gain_weight_rows: nant must be positive" in L.fv_last_error()
    assert call(g=None) == 1 and b"fv_gain_weight_rows: null gains" in L.fv_last_error()
    for kw in (dict(nparts=-1), dict(nparts=5), dict(p=None)):
        assert call(**kw) == 1 and b"fv_gain_weight_rows: nparts must be 0 .. 4" in L.fv_last_error()
    assert call(nparts=0, v=buf) == 1 and b"fv_gain_weight_rows: nparts == 0 needs d_gains" in L.fv_last_error()
    assert call(nparts=2, p=hole) == 1 and b"fv_gain_weight_rows: null part" in L.fv_last_error()
    for kw in (dict(dg=buf), dict(hg=buf), dict(nparts=0, dg=buf)):
        assert call(**kw) == 1 and b"fv_gain_weight_rows: d_gains and hgains need vis" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(q=None)):
        assert call(**kw) == 1 and b"fv_gain_weight_rows: null pairs or q_rows" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2, tpol=4) == 1 and b"fv_gain_weight_rows: antenna index outside [0, nant)" in L.fv_last_error()


def test_fv_sim_gain_weight_block_argument_checks():
    L = _lib.lib()
    fn = L.fv_sim_gain_weight_block
    buf = (ctypes.c_double * 8)()
    parts = (ctypes.c_void_p * 4)(*[ctypes.addressof(buf)] * 4)
    hole = (ctypes.c_void_p * 4)(ctypes.addressof(buf), None, None, None)

    def call(nparts=1, p=parts, v=buf, g=buf, dg=None, q=buf, hg=None, flags=(0, 0, 0, 0)):
        return fn(None, 0, 1, 0, 1, nparts, p, v, None, flags[0], g, flags[1], dg, flags[2], q, hg, flags[3])

    assert call() == 1 and b"null handle" in L.fv_last_error()
    assert call(nparts=0, dg=buf) == 1 and b"null handle" in L.fv_last_error()  # (a valid gains-only call)
    for kw in (dict(nparts=-1), dict(nparts=5), dict(p=None)):
        assert call(**kw) == 1 and b"nparts must be 0 .. 4" in L.fv_last_error()
    assert call(nparts=0) == 1 and b"nparts == 0 needs d_gains" in L.fv_last_error()
    assert call(nparts=2, p=hole) == 1 and b"null part" in L.fv_last_error()
    for kw in (dict(g=None), dict(q=None)):
        assert call(**kw) == 1 and b"null gains or q_ft" in L.fv_last_error()
    for kw in (dict(v=None, dg=buf), dict(v=None, hg=buf)):
        assert call(**kw) == 1 and b"d_gains and hgains need vis" in L.fv_last_error()
    for flags in [(2, 0, 0, 0), (0, -1, 0, 0), (0, 0, 3, 0), (0, 0, 0, 2)]:
        assert call(dg=buf, hg=buf, flags=flags) == 1 and b"on_device flags must be 0 or 1" in L.fv_last_error()
