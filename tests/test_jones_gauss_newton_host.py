"""CPU tests of the Gauss-Newton product with 2 x 2 Jones gains (``simulate_vis_jones_gauss_newton``, ``fv_jones_weight_rows``,
``fv_sim_jones_weight_block``): the numpy reference against the stencil of the Jones forward, against the already-pinned
``jones_refs.chi2_jones`` and against the diagonal gains' reference, the C surface, and the argument errors raised before
any engine exists or any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, adjoint, wrapper
from tests import gain_gauss_newton_refs as ggr
from tests import jones_gauss_newton_refs as jgr
from tests import jones_refs
from tests.test_derivative_api_host import _cfg
from tests.test_jones_host import _case, _shapes


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    def reached(*a, **k):
        pytest.fail("an engine was created: the argument checks come first")

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)


def _raises(exc, message):
    return pytest.raises(exc, match="^" + re.escape(message) + "$")


def _gn_case(seed=0, nparts=2):
    """``test_jones_host._case`` (an auto-correlation, an antenna without a baseline, 20 % flags, baseline 3 flagged in all
    four samples) with tangent parts and a Jones direction of the matrices' size."""
    V, _, w, J, a1, a2 = _case(seed)
    rng = np.random.default_rng(seed + 100)

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    parts = [c(V.shape) for _ in range(nparts)]
    dJ = 0.4 * c(J.shape)
    return parts, V, w, J, dJ, a1, a2


def test_reference_tangent_is_the_stencil_of_the_jones_forward():
    parts, V, w, J, dJ, a1, a2 = _gn_case()
    U = parts[0] + parts[1]
    Up = jgr.tangent(parts, V, J, dJ, a1, a2)
    # eps -> apply_jones(V + eps U, J + eps dJ) is a cubic in eps: the five-point stencil is exact up to rounding
    fd = jones_refs.five_point(lambda h: jones_refs.apply_jones(V + h * U, J + h * dJ, a1, a2), 0.25)
    worst = float(np.abs(fd - Up).max() / np.abs(Up).max())
    print("jones Gauss-Newton reference: stencil against U'", worst)
    assert worst <= 1e-12  # (test_jones_host's stencil tolerance)
    # without a direction the sky term alone, and without parts U = 0
    assert np.allclose(jgr.tangent(parts, V, J, None, a1, a2), jones_refs.apply_jones(U, J, a1, a2), rtol=1e-15)
    assert np.allclose(jgr.tangent([], V, J, dJ, a1, a2), Up - jones_refs.apply_jones(U, J, a1, a2), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("nparts,direction", [(2, True), (1, False), (0, True)])
def test_reference_is_the_jones_objective_reference_with_this_residual(nparts, direction):
    """chi2_jones(V, d, ...) with d = V' - U' has V' - d = U': its rows, G', G and gjones are this reference's."""
    parts, V, w, J, dJ, a1, a2 = _gn_case(seed=4, nparts=nparts)
    dJ = dJ if direction else None
    used = w != 0
    live = used.any(axis=(-3, -2), keepdims=True)
    Up = jgr.tangent(parts, V, J, dJ, a1, a2)
    d = jones_refs.apply_jones(V, J, a1, a2) - Up
    Vn = np.where(live, V, np.nan)  # (a baseline flagged in all four samples uses neither its parts nor V)
    pn = [np.where(live, p, np.nan) for p in parts]
    rows, Gp, G, hj, S, A = jgr.jones_gauss_newton(pn, Vn, w, J, dJ, a1, a2, with_abs=True)
    rows0, Gp0, G0, gj0 = jones_refs.chi2_jones(V, d, w, J, a1, a2)
    assert np.isfinite(G).all() and np.isfinite(hj).all() and np.all(Gp[~used] == 0) and np.all(G[..., 3] == 0)
    assert np.all(hj[..., -1] == 0)
    scale = np.abs(Gp0).max()
    for got, exp in ((rows, rows0), (Gp, Gp0), (G, G0), (hj, gj0)):
        assert got.shape == exp.shape and np.abs(got - exp).max() <= 1e-13 * max(scale, np.abs(exp).max())
    # the majorants bound what they stand for
    assert np.all(S[used] >= np.abs(Up[used]) * (1 - 1e-15)) and np.all(A >= np.abs(hj)) and np.all(A[..., -1] == 0)
    # <p, H p> = 2 quad on the reference: p's sky part pairs with G through U (J p = U), the matrices' with hjones
    U = sum(parts) if parts else np.zeros_like(V)
    sky = float(np.sum((np.conj(np.where(live, U, 0)) * G).real))
    mat = jgr.inner_jones(dJ, hj) if direction else 0.0
    assert abs(sky + mat - 2 * rows.sum()) <= 1e-12 * 2 * rows.sum()


@pytest.mark.parametrize("nparts,direction", [(2, True), (1, False), (0, True)])
def test_diagonal_matrices_and_direction_are_the_gain_reference(nparts, direction):
    parts, V, w, J, _, a1, a2 = _gn_case(seed=5, nparts=nparts)
    rng = np.random.default_rng(6)
    shape = J.shape[:2] + (2, J.shape[-1])
    g = 1 + 0.3 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    dg = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) if direction else None
    # (the gain reference flags sample by sample: no NaN here, where the two rules differ only in what they read)
    rows, Gp, G, hj = jgr.jones_gauss_newton(parts, V, w, jones_refs.diagonal(g), None if dg is None else jones_refs.diagonal(dg),
                                             a1, a2)
    rows_g, Gp_g, G_g, hg = ggr.gain_gauss_newton(parts, V, w, g, dg, a1, a2)

    def close(a, b):
        return np.abs(a - b).max() <= 1e-13 * np.abs(b).max()

    assert close(rows, rows_g) and close(Gp, Gp_g) and close(G, G_g)
    assert close(hj[..., 0, 0, :], hg[..., 0, :]) and close(hj[..., 1, 1, :], hg[..., 1, :])
    assert np.abs(hj[..., 0, 1, :]).max() > 0.1  # (the leakage entries have a product of their own at diagonal matrices)


_NEW = {"fv_jones_weight_rows": 15, "fv_sim_jones_weight_block": 17}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    assert re.search(r"^int fv_jones_weight_rows\(int device, int precision, int64_t nrows, int64_t nbls, int nant, "
                     r"const int \*ant1,\s+const int \*ant2,\s+const void \*jones, const void \*d_jones, int nparts, "
                     r"const void \*const \*parts, void \*vis,\s+const void \*weights, double \*q_rows, void \*hjones\);",
                     header, re.M)
    assert re.search(r"^int fv_sim_jones_weight_block\(fv_sim \*h, int t0, int t1, int f0, int f1, int nparts, "
                     r"void \*const \*parts_dev, void \*vis_dev,\s+const void \*weights, int weights_on_device, "
                     r"const void \*jones, int jones_on_device,\s+const void \*d_jones, int d_jones_on_device, double \*q_ft, "
                     r"void \*hjones, int hjones_on_device\);", header, re.M)
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    # fv_gain_weight_rows without tpol, and fv_sim_gain_weight_block argument for argument
    gain = _lib.SYMBOLS["fv_gain_weight_rows"][1]
    assert _lib.SYMBOLS["fv_jones_weight_rows"][1] == gain[:4] + gain[5:]
    assert _lib.SYMBOLS["fv_sim_jones_weight_block"] == _lib.SYMBOLS["fv_sim_gain_weight_block"]
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.jones_weight_block)
    flat = " ".join(header.split()).replace(" * ", " ")
    for stated in ("U' = (S(U; G1, G2) + S(V; H1, G2)) + S(V; G1, H2)",
                   "G'[x, y] = 2 (w[x, y] U'[x, y]) quad row += w |U'|^2 (terms formed and added in fp64)",
                   "stored G[x', y'] = sum_{x, y} conj(G2[x', x]) G'[x, y] G1[y', y]",
                   "hjones[a, y', y] += sum_x conj(G'[x, y]) (G2^T V)[x, y'] for every k with a1[k] = a",
                   "hjones[a, x', x] += sum_y G'[x, y] conj((V conj G1)[x', y]) for every k with a2[k] = a"):
        assert stated in flat, stated


def test_exported_with_the_gain_signature_and_the_two_keywords_swapped():
    gain = inspect.signature(adjoint.simulate_vis_gain_gauss_newton).parameters
    own = inspect.signature(adjoint.simulate_vis_jones_gauss_newton).parameters
    swap = {"gains": "jones", "d_gains": "d_jones"}
    assert list(own) == [swap.get(n, n) for n in gain]
    assert all(own[swap.get(n, n)].kind == gain[n].kind and own[swap.get(n, n)].default == gain[n].default for n in gain)
    assert own["jones"].default is inspect.Parameter.empty and own["d_jones"].default is None
    assert "gains" not in own and "d_gains" not in own
    assert fftvis_amd.simulate_vis_jones_gauss_newton is adjoint.simulate_vis_jones_gauss_newton
    doc = " ".join(adjoint.simulate_vis_jones_gauss_newton.__doc__.split())
    for word in ("``U' = S(U; J[a1], J[a2]) + S(V; dJ[a1], J[a2]) + S(V; J[a1], dJ[a2])``", "polarized=True", "NOT",
                 "several directions per call", "the gradient in the same call", "sharding", "hvp", "``model=``"):
        assert word in doc, word
    for fn in (adjoint.simulate_vis_jones_chi2, adjoint.simulate_vis_gain_gauss_newton, adjoint.simulate_vis_jones_solve):
        assert "simulate_vis_jones_gauss_newton" in fn.__doc__, fn.__name__
        assert "Jones matrices in the Gauss-Newton product" not in " ".join(fn.__doc__.split()), fn.__name__


def _call(**changes):
    cfg = dict(_cfg(), polarized=True)
    if not any(k.startswith("d_") for k in changes):
        changes["d_fluxes"] = np.ones_like(cfg["fluxes"])
    return adjoint.simulate_vis_jones_gauss_newton(**dict(cfg, **changes))


def test_bad_jones_and_directions():
    cfg = _cfg()
    const, per_time = _shapes(cfg)
    nant, nf = const[0], const[-1]
    ones = np.ones(const, complex)
    for bad in ((nant, 2, nf), const[:-1], (2, 2, nant, nf)):
        with _raises(ValueError, f"jones must have shape {const} or {per_time}, got {bad}"):
            _call(jones=np.ones(bad, complex))
    with _raises(ValueError, "jones must be complex (one 2 x 2 matrix per antenna and channel)"):
        _call(jones=np.ones(const))
    with _raises(ValueError, "jones must be finite"):
        _call(jones=ones * np.nan)
    # d_jones: jones' own shape (time-constant or per time as jones is), complex, finite
    for bad in (per_time, const[:-1], (nant + 1,) + const[1:]):
        with _raises(ValueError, f"d_jones must have jones' shape {const}, got {bad}"):
            _call(jones=ones, d_jones=np.ones(bad, complex))
    with _raises(ValueError, f"d_jones must have jones' shape {per_time}, got {const}"):
        _call(jones=np.ones(per_time, complex), d_jones=ones)
    with _raises(ValueError, "d_jones must be complex, like jones"):
        _call(jones=ones, d_jones=np.ones(const))
    for value in (np.nan, complex(1, np.inf)):
        dj = ones.copy()
        dj[(0,) * dj.ndim] = value
        with _raises(ValueError, "d_jones must be finite"):
            _call(jones=ones, d_jones=dj)
    # refused up front: an unpolarized run, the direction or the name without the matrices, gains= next to jones=
    with _raises(ValueError, "jones needs polarized=True: a 2 x 2 matrix per antenna mixes the two feeds"):
        _call(jones=ones, polarized=False)
    with _raises(ValueError, "d_jones needs jones="):
        _call(jones=None, d_jones=ones)
    for wrt in ("jones", ("fluxes", "jones")):
        with _raises(ValueError, "wrt='jones' needs jones="):
            _call(jones=None, wrt=wrt)
    with pytest.raises(TypeError, match="gains"):
        _call(jones=ones, gains=np.ones((nant, 2, nf), complex))
    with pytest.raises(TypeError, match="d_gains"):
        _call(jones=ones, d_gains=np.ones((nant, 2, nf), complex))
    with pytest.raises(TypeError, match="jones"):
        adjoint.simulate_vis_gain_gauss_newton(**dict(cfg, polarized=True, d_fluxes=np.ones_like(cfg["fluxes"]),
                                                      gains=np.ones((nant, 2, nf), complex), jones=ones))
    with _raises(ValueError, "simulate_vis_jones_gauss_newton needs a direction: d_fluxes, d_ants, d_baselines, d_radec, d_topo, "
                             "d_beam_coefs or d_jones"):
        adjoint.simulate_vis_jones_gauss_newton(**dict(cfg, polarized=True, jones=ones))
    for wrt in ("antennas", "gains"):  # (the gains are simulate_vis_gain_gauss_newton's)
        with _raises(ValueError, "wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and 'jones', "
                                 f"got '{wrt}'"):
            _call(jones=ones, wrt=wrt)
    with pytest.raises(ValueError, match="^wrt must name "):
        _call(jones=ones, wrt=("jones", "jones"))
    pol = dict(cfg, polarized=True, d_fluxes=np.ones_like(cfg["fluxes"]))
    for wrt in ("jones", ("fluxes", "jones")):  # the other two functions do not know the name
        with pytest.raises(ValueError, match="^wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec' and 'beam_coefs', got"):
            adjoint.simulate_vis_gauss_newton(**dict(pol, wrt=wrt))
        with pytest.raises(ValueError, match="^wrt must name some of 'fluxes', 'ants', 'baselines', 'topo', 'radec', 'beam_coefs' and "
                                             "'gains', got"):
            adjoint.simulate_vis_gain_gauss_newton(**dict(pol, wrt=wrt, gains=np.ones((nant, 2, nf), complex)))
    with pytest.raises(TypeError, match="jones"):
        adjoint.simulate_vis_jones_gauss_newton(**pol)  # jones is required


def test_d_jones_alone_passes_the_argument_checks(monkeypatch):
    """``d_jones`` alone is a valid call: it reaches the engine."""
    cfg = dict(_cfg(), polarized=True)
    ones = np.ones(_shapes(cfg)[0], complex)

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached

    monkeypatch.setattr(wrapper, "create_simulation_engine", reached)
    with pytest.raises(Reached):
        adjoint.simulate_vis_jones_gauss_newton(**dict(cfg, jones=ones, d_jones=ones))


def test_gauss_newton_of_takes_the_matrices_in_a_form_of_their_own():
    from fftvis_amd.gpu import gpu_simulate as gs

    blk = np.ones((2, 2, 2, 2, 7), complex)
    tagged = ("jones", (blk, None))
    d = {"d_fluxes": np.ones((3, 2))}
    gs._check_gauss_newton((d, None, {"gjones": blk}, tagged), False)
    gs._check_gauss_newton(({}, None, {}, ("jones", (blk, blk))), False)  # (a Jones direction counts as a direction)
    assert gs._gauss_newton_holds_v({"gjones": blk}, tagged) and gs._gauss_newton_holds_v({}, ("jones", (blk, blk)))
    assert not gs._gauss_newton_holds_v({}, tagged) and not gs._gauss_newton_holds_v({"gjones": None}, tagged)
    with _raises(ValueError, "gauss_newton_of: no direction given"):
        gs._check_gauss_newton(({}, None, {}, tagged), False)
    with _raises(ValueError, "gauss_newton_of: gjones needs the matrices (a fourth element ('jones', (jones, d_jones)))"):
        gs._check_gauss_newton((d, None, {"gjones": blk}, (blk[:, :, 0], None)), False)
    with _raises(ValueError, "gauss_newton_of: ggains needs the gains (a fourth element)"):
        gs._check_gauss_newton((d, None, {"ggains": blk}, tagged), False)
    with pytest.raises(ValueError, match=r"^gauss_newton_of: the fourth element is \(gains, d_gains\), d_gains or None"):
        gs._check_gauss_newton((d, None, {}, ("jones", (None, blk))), False)


def test_fv_jones_weight_rows_argument_checks():
    L = _lib.lib()
    fn = L.fv_jones_weight_rows
    buf = (ctypes.c_double * 256)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    parts = (ctypes.c_void_p * 4)(*[ctypes.addressof(buf)] * 4)
    hole = (ctypes.c_void_p * 4)(ctypes.addressof(buf), None, None, None)

    def call(precision=2, nrows=1, nbls=3, nant=3, a1=a, a2=a, j=buf, dj=None, nparts=1, p=parts, v=None, q=buf, hj=None):
        return fn(0, precision, nrows, nbls, nant, a1, a2, j, dj, nparts, p, v, None, q, hj)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for kw in (dict(nrows=-1), dict(nbls=-1)):
        assert call(**kw) == 1 and b"fv_jones_weight_rows: negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and b"fv_jones_weight_rows: nant must be positive" in L.fv_last_error()
    assert call(j=None) == 1 and b"fv_jones_weight_rows: null jones" in L.fv_last_error()
    for kw in (dict(nparts=-1), dict(nparts=5), dict(p=None)):
        assert call(**kw) == 1 and b"fv_jones_weight_rows: nparts must be 0 .. 4" in L.fv_last_error()
    assert call(nparts=0, v=buf) == 1 and b"fv_jones_weight_rows: nparts == 0 needs d_jones" in L.fv_last_error()
    assert call(nparts=2, p=hole) == 1 and b"fv_jones_weight_rows: null part" in L.fv_last_error()
    for kw in (dict(dj=buf), dict(hj=buf), dict(nparts=0, dj=buf)):
        assert call(**kw) == 1 and b"fv_jones_weight_rows: d_jones and hjones need vis" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(q=None)):
        assert call(**kw) == 1 and b"fv_jones_weight_rows: null pairs or q_rows" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2) == 1 and b"fv_jones_weight_rows: antenna index outside [0, nant)" in L.fv_last_error()
    # no rows and no baselines need no device: nothing, and zeros
    assert call(nrows=0, j=None, q=None) == 0
    rows, hj = (ctypes.c_double * 2)(7.0, 7.0), (ctypes.c_double * 48)(*([7.0] * 48))
    assert call(nrows=2, nbls=0, a1=None, a2=None, q=rows, hj=hj, v=buf) == 0
    assert list(rows) == [0.0, 0.0] and not any(hj)


def test_fv_sim_jones_weight_block_argument_checks():
    L = _lib.lib()
    fn = L.fv_sim_jones_weight_block
    buf = (ctypes.c_double * 8)()
    parts = (ctypes.c_void_p * 4)(*[ctypes.addressof(buf)] * 4)
    hole = (ctypes.c_void_p * 4)(ctypes.addressof(buf), None, None, None)

    def call(nparts=1, p=parts, v=buf, j=buf, dj=None, q=buf, hj=None, flags=(0, 0, 0, 0)):
        return fn(None, 0, 1, 0, 1, nparts, p, v, None, flags[0], j, flags[1], dj, flags[2], q, hj, flags[3])

    assert call() == 1 and b"null handle" in L.fv_last_error()
    assert call(nparts=0, dj=buf) == 1 and b"null handle" in L.fv_last_error()  # (a valid matrices-only call)
    for kw in (dict(nparts=-1), dict(nparts=5), dict(p=None)):
        assert call(**kw) == 1 and b"nparts must be 0 .. 4" in L.fv_last_error()
    assert call(nparts=0) == 1 and b"nparts == 0 needs d_jones" in L.fv_last_error()
    assert call(nparts=2, p=hole) == 1 and b"null part" in L.fv_last_error()
    for kw in (dict(j=None), dict(q=None)):
        assert call(**kw) == 1 and b"null jones or q_ft" in L.fv_last_error()
    for kw in (dict(v=None, dj=buf), dict(v=None, hj=buf)):
        assert call(**kw) == 1 and b"d_jones and hjones need vis" in L.fv_last_error()
    for flags in [(2, 0, 0, 0), (0, -1, 0, 0), (0, 0, 3, 0), (0, 0, 0, 2)]:
        assert call(dj=buf, hj=buf, flags=flags) == 1 and b"on_device flags must be 0 or 1" in L.fv_last_error()
