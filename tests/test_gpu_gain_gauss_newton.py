"""GPU tests of the Gauss-Newton product with per-antenna gains (``simulate_vis_gain_gauss_newton``,
``fv_sim_gain_weight_block`` and the kernel pair alone through ``fv_gain_weight_rows``).

The kernel pair is held to bounds derived from its arithmetic, as ``test_gpu_gains`` derives its own.  u = eps_T / 2 is the
unit roundoff of the run's precision T; a complex product has a modulus error within 3 u |a| |b|, a component-wise sum
within u times its result.  S = sum_j |P_j| and D = |h1| |g2| + |g1| |h2| are the sums of moduli behind U and dm.  The
in-place kernel forms, in T and in this order, U (NP - 1 <= 3 adds: 3 u S), m (3 u |m|), m U (3 u |m| |U| of its own, 3 u
from m, 3 u |m| S from U: 9 u |m| S, as |U| <= S), dm (two products and a sum: 4 u D), dm V (3 u + 4 u: 7 u D |V|),
U' = m U + dm V (u |U'| more), G' = 2 (w U') (one rounding, an exact doubling) and the stored G = conj(m) G' (3 u |G| from
m, 3 u |G| of its own).  With A = |m| S + D |V|, to first order
    |G - G_ref| <= u (18 w |m| A + 8 |G_ref|)  <=  eps_T (18 w |m| A + 8 |G_ref|),
the bound asserted, against the fp64 reference of the same T-typed inputs.  The element function's arithmetic in T is compiled
without floating-point contraction, so numpy reproduces its T-typed U' bit for bit, operation by operation; the rows' sums
add the fp64 terms w (ur^2 + ui^2) of that U' (at most four roundings each: c = 4) in some order: ``(L + 4) 2^-52`` relative
to ``math.fsum``, L = tpol nbls.  The gather adds, per antenna, n_a signed fp64 terms conj(G') g V with G' = 2 w U' formed in
fp64.  The inputs are constructed, and asserted, to keep S <= 1.5 |U| (the parts lie in a cone of half-angle pi / 4),
D <= 1.5 |dm| (so does dg / g) and |m U| + |dm V| <= 4 |U'| (U is negated where it would not hold) at every unflagged
sample.  Then U carries 3 u S <= 4.5 u |U|, m U (6 + 4.5) u |m U|, dm V (3 + 4 * 1.5) u |dm V| = 9 u |dm V|, and
U' u |U'| + 10.5 u (|m U| + |dm V|) <= 43 u |U'|; the weight adds u, the other factor g V 3 u and the last product 3 u:
50 u = 25 * 2^-52 per term on the device and as much in the numpy reference, and the two summation orders n_a u each:
    |hgains - ref| <= (n_a + 50) 2^-52 sum |terms|.
Through the engine G, the rows and the gain block are held to ``test_gpu_objective``'s BOUND against the composition
``simulate_vis`` -> public jvp -> the numpy reference, on directions chosen so that ||U'|| >= 0.1 (||m U|| + ||dm V||)."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from tests import basis_source_refs as bsr
from tests import gain_gauss_newton_refs as ggr
from tests import gain_refs
from tests import gauss_newton_refs as gnr
from tests.helpers import rel_l2
from tests.objective_refs import row_major_sum, row_sums_exact
from tests.source_adjoint_refs import source_config
from tests.tangent_refs import edge_config, hex19_config
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_gains import _ant_rows, _block_layout, _blocked, _from_block, _gains, _pairs
from tests.test_gpu_gauss_newton import CELLS, _composition, _directions, _gn, _weights
from tests.test_gpu_lattice_adjoint import _handle
from tests.test_gpu_objective import BOUND, CDT, RDT, _public
from tests.test_gpu_position_adjoint import K32
from tests.test_gpu_sky_adjoint import _same_flux
from tests.test_gpu_source_adjoint import _edge_cfg, _sid

pytestmark = pytest.mark.gpu

NANT = 7


# ---- 1. the kernel pair alone --------------------------------------------------------------------------------------------
def _cone(rng, shape):
    """r exp(i phi), r in U(0.5, 1.5), |phi| <= pi / 4: sums of such factors do not cancel."""
    return rng.uniform(0.5, 1.5, size=shape) * np.exp(1j * rng.uniform(-np.pi / 4, np.pi / 4, size=shape))


def _elements(g, a1, a2, tpol, ncol):
    """(g1, g2) of every element of a row: ``g[:, p, a1[k]]`` and ``g[:, q, a2[k]]``, pol = 2 q + p."""
    nbls = len(a1)
    pol = np.arange(ncol) // nbls
    k = np.arange(ncol) % nbls
    p, q = (pol & 1, pol >> 1) if tpol == 4 else (0 * pol, 0 * pol)
    return g[:, p, a1[k]], g[:, q, a2[k]]


def _kernel_inputs(nrows, nbls, tpol, nparts, direction, precision, weights, seed=0, pairs=None, nant=NANT):
    rng = np.random.default_rng(seed + 10 * nbls + tpol + 100 * nparts + (1000 if direction else 0))
    shape = (nrows, tpol * nbls)
    nfeed = 2 if tpol == 4 else 1
    cdt = CDT[precision]

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    a1, a2 = _pairs(nbls, rng, nant) if pairs is None else pairs
    V = c(shape).astype(cdt)
    P0 = c(shape)
    parts = [P0.astype(cdt)] + [(P0 * _cone(rng, shape)).astype(cdt) for _ in range(nparts - 1)]
    parts = parts[:nparts]
    g = (1 + 0.3 * c((nrows, nfeed, nant))).astype(cdt)
    dg = (g * 0.5 * _cone(rng, g.shape)).astype(cdt) if direction else None
    if direction and nparts:  # (keeps the cancellation in m U + dm V bounded: the module docstring)
        g1, g2 = _elements(g.astype(np.complex128), a1, a2, tpol, shape[1])
        h1, h2 = _elements(dg.astype(np.complex128), a1, a2, tpol, shape[1])
        mU = np.conj(g1) * g2 * sum(p.astype(np.complex128) for p in parts)
        dmV = (np.conj(h1) * g2 + np.conj(g1) * h2) * V
        near = np.abs(mU) + np.abs(dmV) > 3.5 * np.abs(mU + dmV)
        for p in parts:
            p[near] = -p[near]
    w = None
    if weights != "none":
        w = rng.uniform(0.5, 2.0, size=shape).astype(RDT[precision])
    if weights == "flags":
        flagged = rng.random(shape) < 0.3
        flagged[0, 0] = True
        w[flagged] = 0
        for x in parts + [V]:
            x[flagged] = np.where(rng.random(int(flagged.sum())) < 0.5, complex(np.nan, 0.0), complex(np.inf, -np.inf))
    return parts, V, w, g, dg, a1, a2


def _run(parts, V, w, g, dg, a1, a2, tpol, precision, want_hg=True, give_v=True):
    own = [p.copy() for p in parts]
    vis = V.copy() if give_v else None
    q = np.full(V.shape[0], -1.0)
    hg = np.full(g.shape, 7.0, dtype=np.complex128) if want_hg else None
    ptrs = (ctypes.c_void_p * max(len(own), 1))(*[p.ctypes.data for p in own])
    status = _lib.lib().fv_gain_weight_rows(0, precision, V.shape[0], len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                            _lib.ptr(g), _lib.ptr(dg), len(own), ptrs, _lib.ptr(vis), _lib.ptr(w), _lib.ptr(q),
                                            _lib.ptr(hg))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(own[1:], parts[1:]))  # read only
    if own and give_v:
        assert np.array_equal(vis, V, equal_nan=True)
    return status, (own[0] if own else vis), q, hg


def _uprime_as_the_kernel_forms_it(parts, V, g, dg, a1, a2, tpol):
    """U, m, m U, dm, dm V and U' operation by operation in T (no contraction), as the element function."""
    g1, g2 = _elements(g, a1, a2, tpol, V.shape[1])
    mr = g1.real * g2.real + g1.imag * g2.imag
    mi = g1.real * g2.imag - g1.imag * g2.real
    ur = ui = None
    if parts:
        re, im = parts[0].real.copy(), parts[0].imag.copy()
        for p in parts[1:]:
            re, im = re + p.real, im + p.imag
        ur, ui = mr * re - mi * im, mr * im + mi * re
    if dg is not None:
        h1, h2 = _elements(dg, a1, a2, tpol, V.shape[1])
        dmr = (h1.real * g2.real + h1.imag * g2.imag) + (g1.real * h2.real + g1.imag * h2.imag)
        dmi = (h1.real * g2.imag - h1.imag * g2.real) + (g1.real * h2.imag - g1.imag * h2.real)
        tr, ti = dmr * V.real - dmi * V.imag, dmr * V.imag + dmi * V.real
        ur, ui = (ur + tr, ui + ti) if parts else (tr, ti)
    assert ur.dtype == V.real.dtype
    return ur, ui


def _check_kernel_pair(label, parts, V, w, g, dg, a1, a2, tpol, precision):
    L = V.shape[1]
    status, G, q, hg = _run(parts, V, w, g, dg, a1, a2, tpol, precision)
    assert status == 0, _lib.lib().fv_last_error()
    used = np.ones(V.shape, bool) if w is None else w != 0
    w64 = np.ones(V.shape) if w is None else w.astype(np.float64)
    z = lambda x: np.where(used, x, 0).astype(x.dtype)  # noqa: E731  (what lies under a flag is not used)
    pz, Vz = [z(p) for p in parts], z(V)
    pb, Vb, wb = [_blocked(p, tpol) for p in pz], _blocked(Vz, tpol), _blocked(w64, tpol)
    rows_ref, Gp_ref, G_ref, hg_ref, hg_abs = ggr.gain_gauss_newton(pb, Vb, wb, g, dg, a1, a2, with_abs=True)
    G_ref = G_ref.reshape(V.shape)
    # the data conditions of the bounds
    g1, g2 = _elements(g.astype(np.complex128), a1, a2, tpol, L)
    m = np.conj(g1) * g2
    S = sum(np.abs(p.astype(np.complex128)) for p in pz) if parts else np.zeros(V.shape)
    U = sum(p.astype(np.complex128) for p in pz) if parts else np.zeros(V.shape, complex)
    D, dm = np.zeros(V.shape), np.zeros(V.shape, complex)
    if dg is not None:
        h1, h2 = _elements(dg.astype(np.complex128), a1, a2, tpol, L)
        D = np.abs(h1) * np.abs(g2) + np.abs(g1) * np.abs(h2)
        dm = np.conj(h1) * g2 + np.conj(g1) * h2
    Up = m * U + dm * Vz.astype(np.complex128)
    assert np.all(S[used] <= 1.5 * np.abs(U)[used]) and np.all(D <= 1.5 * np.abs(dm))
    assert np.all((np.abs(m * U) + np.abs(dm * Vz) <= 4 * np.abs(Up))[used])
    eps_t = float(np.finfo(RDT[precision]).eps)
    err = np.abs(G.astype(np.complex128) - G_ref)
    bound = eps_t * (18 * w64 * np.abs(m) * (np.abs(m) * S + D * np.abs(Vz)) + 8 * np.abs(G_ref))
    print("gain weight kernels G", label, float((err[used] / bound[used]).max(initial=0.0)))
    assert np.all(err <= bound)
    assert np.all(G[~used] == 0) and np.isfinite(G).all()
    ur, ui = _uprime_as_the_kernel_forms_it(pz, Vz, g, dg, a1, a2, tpol)
    terms = np.where(used, w64 * (ur.astype(np.float64) ** 2 + ui.astype(np.float64) ** 2), 0.0)
    exact = row_sums_exact(terms)
    print("gain weight kernels rows", label, float((np.abs(q - exact) / np.maximum(exact, 1e-300)).max() / 2.0**-52))
    assert np.all(np.abs(q - exact) <= (L + 4) * 2.0**-52 * exact)
    assert np.all(np.abs(exact - rows_ref.ravel()) <= 64 * eps_t * rows_ref.ravel())  # (the T-typed U' is the reference's)
    nfeed = g.shape[1]
    n_a = nfeed * (np.bincount(a1, minlength=g.shape[-1]) + np.bincount(a2, minlength=g.shape[-1]))
    herr = np.abs(hg - hg_ref)
    hbound = (n_a + 50) * 2.0**-52 * hg_abs
    print("gain weight kernels hgains", label, float((herr / np.maximum(hbound, 1e-300)).max()), int(n_a.max()))
    assert np.all(herr <= hbound)
    assert np.all(hg[..., n_a == 0] == 0) and (n_a == 0).any()
    assert np.all(hg[..., n_a > 0] != 0) or w is not None
    status, G2, q2, hg2 = _run(parts, V, w, g, dg, a1, a2, tpol, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(G2, G) and np.array_equal(q2, q) and np.array_equal(hg2, hg)
    status, G3, q3, _ = _run(parts, V, w, g, dg, a1, a2, tpol, precision, want_hg=False)  # ... with or without the gather
    assert status == 0 and np.array_equal(G3, G) and np.array_equal(q3, q)
    if parts and dg is None:  # ... and without V, which only the gather reads then
        status, G4, q4, _ = _run(parts, V, w, g, dg, a1, a2, tpol, precision, want_hg=False, give_v=False)
        assert status == 0 and np.array_equal(G4, G) and np.array_equal(q4, q)
    return n_a


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nparts,direction", [(0, True), (1, False), (1, True), (2, False), (2, True), (4, False), (4, True)])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_kernel_pair(gpu, nbls, tpol, nrows, nparts, direction, precision, weights):
    parts, V, w, g, dg, a1, a2 = _kernel_inputs(nrows, nbls, tpol, nparts, direction, precision, weights)
    n_a = _check_kernel_pair(f"{nbls} {tpol} {nrows} {nparts} {direction} {precision} {weights}", parts, V, w, g, dg, a1, a2,
                             tpol, precision)
    both = set(a1[a1 != a2]) | set(a2[a1 != a2])
    if nbls > 8:
        assert (a1 == a2).sum() > 1 and NANT - 2 not in both and n_a[NANT - 2] > 0  # autos; an antenna in autos only
    if nbls >= 257:
        assert n_a[0] > 64 * (2 if tpol == 4 else 1)


def _weight_rows(parts, w, precision):
    own = [p.copy() for p in parts]
    q = np.full(parts[0].shape[0], -1.0)
    ptrs = (ctypes.c_void_p * len(own))(*[p.ctypes.data for p in own])
    assert _lib.lib().fv_weight_rows(0, precision, parts[0].shape[0], parts[0].shape[1], len(own), ptrs, _lib.ptr(w),
                                     _lib.ptr(q)) == 0
    return own[0], q


@pytest.mark.parametrize("nrows,nbls,tpol", [(3, 257, 4), (400, 1, 1), (400, 1, 4), (7, 75, 1)])
@pytest.mark.parametrize("nparts", [1, 2, 3, 4])
def test_unit_gains_are_the_weight_kernel_bit_for_bit(gpu, nparts, nrows, nbls, tpol):
    """Every instance of the kernel on both of its paths: rows of one value go element by element, rows of four are one or
    two whole vectors (sums of one to four terms show a last bit that a long row's rounding would hide), rows of 75 mix
    the two, and rows of 1 028 span blocks."""
    for precision in (2, 1):
        parts, V, w, g, _, a1, a2 = _kernel_inputs(nrows, nbls, tpol, nparts, False, precision, "flags")
        G0, q0 = _weight_rows(parts, w, precision)
        status, G, q, _ = _run(parts, V, w, np.ones_like(g), None, a1, a2, tpol, precision, want_hg=False)
        assert status == 0 and np.array_equal(G, G0) and np.array_equal(q, q0)
        status, G, q, hg = _run(parts, V, w, np.ones_like(g), np.zeros_like(g), a1, a2, tpol, precision)  # a zero direction
        assert status == 0 and np.array_equal(G, G0) and np.array_equal(q, q0) and np.isfinite(hg).all()


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what", ["negative weight", "nan weight"])
def test_bad_weight_fails_the_call_and_the_next_good_call_reproduces_its_bits(gpu, what, precision):
    parts, V, w, g, dg, a1, a2 = _kernel_inputs(3, 75, 4, 2, True, precision, "positive")
    good = _run(parts, V, w, g, dg, a1, a2, 4, precision)
    assert good[0] == 0
    bw = w.copy()
    if what == "negative weight":
        bw[1, 257] = -1.0
    else:
        bw[2, 7] = np.nan
    status = _run(parts, V, bw, g, dg, a1, a2, 4, precision)[0]
    assert status == 1 and b"1 weights are negative or not finite" in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    again = _run(parts, V, w, g, dg, a1, a2, 4, precision)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))


def test_one_hera350_row(gpu):
    """350 antennas, every cross pair: nbls = 61 075, tpol = 4, one row of 244 300 values over 120 blocks, 349 incidences
    per antenna (698 terms per feed); 351 antennas' gains and direction, 2 * 702 complex128, fit the LDS budget."""
    i, j = np.triu_indices(350, 1)
    assert len(i) == 61_075
    parts, V, w, g, dg, a1, a2 = _kernel_inputs(1, 61_075, 4, 2, True, 2, "flags", pairs=(i.astype(np.int32), j.astype(np.int32)),
                                                nant=351)
    n_a = _check_kernel_pair("hera350", parts, V, w, g, dg, a1, a2, 4, 2)
    assert n_a.max() == 2 * 349 and n_a[350] == 0


def test_gains_beyond_the_lds_budget_are_read_from_global_memory(gpu):
    """1 100 antennas, polarized, with a direction: 2 * 2 200 complex128 = 70 400 bytes > GAIN_LDS_BYTES; without one the
    35 200 bytes of the gains alone do not fit either, and in fp32 with a direction exactly 35 200 do not; fp32 without one
    (17 600) does: the same bounds on every path."""
    rng = np.random.default_rng(3)
    nant, nbls = 1100, 300
    a1, a2 = rng.integers(0, nant - 1, nbls).astype(np.int32), rng.integers(0, nant - 1, nbls).astype(np.int32)
    for precision, direction in ((2, True), (2, False), (1, True), (1, False)):
        parts, V, w, g, dg, _, _ = _kernel_inputs(2, nbls, 4, 2, direction, precision, "flags", pairs=(a1, a2), nant=nant)
        _check_kernel_pair(f"global gains {precision} {direction}", parts, V, w, g, dg, a1, a2, 4, precision)


# ---- 2. through the engine -----------------------------------------------------------------------------------------------
def _ggn(cfg, **kw):
    return fftvis_amd.simulate_vis_gain_gauss_newton(**cfg, **kw)


def _d_gains(cfg, g, seed=13, scale=0.3):
    rng = np.random.default_rng(seed)
    return (scale * (rng.normal(size=g.shape) + 1j * rng.normal(size=g.shape))).astype(g.dtype)


def _reference(cfg, dirs, w, g, dg, basis=False):
    """(rows, G, the gain block in g's shape, U', m U, dm V) from ``simulate_vis`` -> the public jvp -> the numpy reference."""
    V = fftvis_amd.simulate_vis(**cfg).astype(np.complex128)
    parts = _composition(cfg, dirs, basis) if dirs else []
    a1, a2 = _ant_rows(cfg)
    gb = _block_layout(cfg, g)
    dgb = None if dg is None else _block_layout(cfg, dg)
    rows, Gp, G, hg = ggr.gain_gauss_newton(parts, V, w, gb, dgb, a1, a2)
    mU = ggr.tangent(parts, V, gb, None, a1, a2)
    Up = ggr.tangent(parts, V, gb, dgb, a1, a2)
    return rows, G, _from_block(cfg, hg, g.shape), Up, mU, Up - mU


def _assert_value(label, cfg, dirs, w, g, dg, basis=False, **kw):
    p = cfg.get("precision", 2)
    quad_ft, hg, G = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, wrt="gains", quad_per="freq_time", return_gvis=True, **kw)
    rows, G_ref, hg_ref, Up, mU, dmV = _reference(cfg, dirs, w, g, dg, basis)
    cond = np.linalg.norm(Up) / (np.linalg.norm(mU) + np.linalg.norm(dmV))
    print("gain gauss-newton value", label, rel_l2(G, G_ref), float((np.abs(quad_ft - rows) / rows).max()), rel_l2(hg, hg_ref),
          cond)
    assert cond >= 0.1  # nothing rides on cancellation
    assert G.shape == G_ref.shape and G.dtype == CDT[p] and rel_l2(G, G_ref) <= BOUND[p]
    assert quad_ft.shape == rows.shape and np.all(rows > 0) and np.all(np.abs(quad_ft - rows) <= BOUND[p] * rows)
    assert hg.shape == g.shape and hg.dtype == np.complex128 and rel_l2(hg, hg_ref) <= BOUND[p]
    return quad_ft, hg, G


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_value(gpu, precision, sky, beams):
    """G, the rows and the gain block: a joint direction, fixed gains, the gain direction alone."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    label = f"{precision} {sky} {beams}"
    _assert_value(label + " joint", cfg, dirs, w, g, dg)
    _assert_value(label + " fixed gains", cfg, dirs, w, g, None)
    _assert_value(label + " gains alone", cfg, {}, w, g, dg)
    one = {"d_fluxes": dirs["d_fluxes"]}
    _assert_value(label + " fluxes, no weights", cfg, one, None, g, dg)
    # the total is the rows' sums added in row-major order
    quad_ft, _ = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, wrt=(), quad_per="freq_time")
    total, prods = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, wrt=())
    assert isinstance(total, float) and prods == () and total == row_major_sum(quad_ft) and total > 0


@pytest.mark.parametrize("precision", [2, 1])
def test_basis_beams(gpu, monkeypatch, precision):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    dirs, w, g = _directions(cfg, basis=True), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    _assert_value(f"basis {precision}", cfg, dirs, w, g, dg, basis=True)
    _assert_products(f"basis {precision}", cfg, dirs, w, g, dg, ("fluxes", "beam_coefs", "ants", "radec", "gains"), basis=True)


def _assert_products(label, cfg, dirs, w, g, dg, names, basis=False):
    """Every product but the gains' is its public pass on the returned G, bit for bit (the fluxes under ``_same_flux``)."""
    quad, prods, G = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, wrt=names, return_gvis=True)
    assert isinstance(prods, tuple) and len(prods) == len(names) and quad > 0
    sky_names = tuple(n for n in names if n != "gains")
    want = _public(cfg, G, sky_names, basis)
    for n, got in zip(names, prods):
        if n == "gains":
            assert got.shape == g.shape and got.dtype == np.complex128 and np.count_nonzero(got) > 0
            continue
        assert got.shape == want[n].shape and got.dtype == want[n].dtype and np.count_nonzero(want[n]) > 0, (label, n)
        if n == "fluxes":
            assert _same_flux(got, want[n]), (label, names)
            assert np.abs(got - want[n]).max() <= 1e-12 * np.abs(want[n]).max()
        else:
            assert np.array_equal(got, want[n]), (label, names, n)


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_products_are_the_public_passes_on_gvis(gpu, monkeypatch, precision, sky, beams):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    for names in (("fluxes",), ("fluxes", "gains"), ("topo", "baselines", "gains"), ("fluxes", "ants", "radec", "gains")):
        _assert_products(f"{precision} {sky} {beams}", cfg, dirs, w, g, dg, names)
    _assert_products(f"{precision} {sky} {beams} fixed gains", cfg, dirs, w, g, None, ("fluxes", "ants"))


_ORDER = ("d_ants", "d_baselines", "d_radec", "d_topo", "d_fluxes", "d_beam_coefs")


def _inner(dirs, dg, prods):
    """<p, prods> over the blocks in ``wrt=None``'s order, the gains last."""
    order = [k for k in _ORDER if k in dirs]
    return sum(gnr.inner(dirs[k], x) for k, x in zip(order, prods)) + ggr.inner_gains(dg, prods[-1])


def _norms(dirs, dg, prods):
    order = [k for k in _ORDER if k in dirs]
    return sum(np.linalg.norm(dirs[k]) * np.linalg.norm(x) for k, x in zip(order, prods)) + \
        np.linalg.norm(dg) * np.linalg.norm(prods[-1])


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_quadratic_form_and_symmetry(gpu, precision, sky, beams):
    """<p, H p> = 2 quad for a joint direction, and <p1, H p2> = <p2, H p1>.  Each side is a chain of passes held to k base
    times the norms it is rounded in (``test_gpu_gauss_newton._quadratic_form``): the products' pairings, and 2 quad itself
    for the rows."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    w, g = _weights(cfg), _gains(cfg)
    p1, p2 = _directions(cfg, seed=11), _directions(cfg, seed=12)
    dg1, dg2 = _d_gains(cfg, g, seed=13), _d_gains(cfg, g, seed=14)
    k = (10.0 if precision == 2 else K32) * _forward_base(cfg)
    quad, H1 = _ggn(cfg, **p1, gains=g, d_gains=dg1, weights=w)
    _, H2 = _ggn(cfg, **p2, gains=g, d_gains=dg2, weights=w)
    assert len(H1) == len(p1) + 1 and H1[-1].shape == g.shape  # (wrt=None: the directions' names, then "gains")
    lhs, bound = _inner(p1, dg1, H1), k * (2 * quad + _norms(p1, dg1, H1))
    print("gain gauss-newton quadratic form", precision, sky, beams, lhs, 2 * quad, abs(lhs - 2 * quad) / bound)
    assert quad > 0 and abs(lhs - 2 * quad) <= bound
    a, b = _inner(p1, dg1, H2), _inner(p2, dg2, H1)
    bound = k * (_norms(p1, dg1, H2) + _norms(p2, dg2, H1))
    print("gain gauss-newton symmetry", precision, sky, beams, a, b, abs(a - b) / bound)
    assert abs(a - b) <= bound and abs(a) > 0


def test_small_hessian(gpu):
    """8 sources, 1 channel, 1 time, 6 baselines, Stokes-I fluxes, fp64 at eps 1e-12: H over (8 fluxes, Re and Im of the
    gains of antennas 0 .. 3) assembled column by column is symmetric and equals 2 Re(J^H W J), J's flux columns from
    ``simulate_vis`` on unit fluxes times m and its gain columns dm V, the gain product's exact linearisation."""
    cfg = edge_config(nsrc=8, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)],
               coord_method="SiderealRotation")
    cfg["fluxes"] = np.ascontiguousarray(synth.catalog(8, cfg["freqs"], 0, polarized_sky=True)[2][..., 0])
    w, g = _weights(cfg), _gains(cfg)
    a1, a2 = _ant_rows(cfg)
    gb = _block_layout(cfg, g)
    pol = bool(cfg["polarized"])
    unit = np.eye(8)[:, :, None]
    gdirs = []
    for a in range(4):
        for f in range(g.shape[1] if pol else 1):
            for c in (1.0, 1j):
                e = np.zeros(g.shape, dtype=g.dtype)
                e[(a, f, 0) if pol else (a, 0)] = c
                gdirs.append(e)

    def column(prods):  # (fluxes, Re hgains, Im hgains): d = Re conj(hgains) dg is the gradient in (Re g, Im g)
        return np.concatenate([prods[0][:, 0]] + [[np.sum(np.conj(e) * prods[1]).real] for e in gdirs])

    cols = [column(_ggn(cfg, d_fluxes=unit[j], gains=g, weights=w, wrt=("fluxes", "gains"))[1]) for j in range(8)]
    cols += [column(_ggn(cfg, d_gains=e, gains=g, weights=w, wrt=("fluxes", "gains"))[1]) for e in gdirs]
    H = np.stack(cols, axis=1)
    V = fftvis_amd.simulate_vis(**cfg).astype(np.complex128)
    m = gain_refs.gain_product(gb, a1, a2, pol)
    J = [(m * fftvis_amd.simulate_vis(**dict(cfg, fluxes=unit[j]))).ravel() for j in range(8)]
    J += [ggr.tangent([], V, gb, _block_layout(cfg, e), a1, a2).ravel() for e in gdirs]
    J = np.stack(J, axis=1)
    H_ref = 2 * (J.conj().T @ (w.ravel()[:, None] * J)).real
    norm = np.linalg.norm(H_ref)
    print("gain gauss-newton small hessian", H.shape, np.linalg.norm(H - H.T) / norm, np.linalg.norm(H - H_ref) / norm)
    assert H.shape == (8 + len(gdirs),) * 2 and len(gdirs) >= 8
    assert np.linalg.norm(H - H.T) <= 10 * BOUND[2] * norm  # (test_gpu_gauss_newton.test_small_hessian's tolerance)
    assert np.linalg.norm(H - H_ref) <= 10 * BOUND[2] * norm
    assert np.all(np.diag(H) >= 0) and np.trace(H) > 0


@pytest.mark.parametrize("sky,beams", CELLS[1:])
@pytest.mark.parametrize("precision", [2, 1])
def test_stencil_of_the_gradient_at_zero_residual(gpu, precision, sky, beams):
    """With data = V' the residual is 0 and the Hessian of chi2 is the Gauss-Newton one: the five-point stencil of
    ``simulate_vis_gain_chi2``'s ("fluxes", "gains") gradient along p is H p.  The gradient along p is a quintic in the step:
    p is a 1e-2 relative change, so the stencil's truncation, O((h 1e-2)^4) of H p, is far below its rounding, which
    ``test_gpu_gains`` sets to 1.5 BOUND times the size of the stencilled values over h.  The values here are gradients
    J^H 2 w (V' - d) whose two terms cancel to O(h p): their rounding is BOUND times the gradient of the uncancelled term,
    the gradient at data = 0."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    w, g = _weights(cfg), _gains(cfg)
    rng = np.random.default_rng(21)
    F = np.asarray(cfg["fluxes"])
    dF = F * 1e-2 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1))
    dg = (g * 1e-2 * (rng.normal(size=g.shape) + 1j * rng.normal(size=g.shape))).astype(g.dtype)
    a1, a2 = _ant_rows(cfg)
    d = gain_refs.apply_gains(fftvis_amd.simulate_vis(**cfg), _block_layout(cfg, g), a1, a2).astype(CDT[precision])
    _, (hf, hg) = _ggn(cfg, d_fluxes=dF, gains=g, d_gains=dg, weights=w, wrt=("fluxes", "gains"))
    h = 0.25

    def grad(s, data=d):
        at = dict(cfg, fluxes=F + s * h * dF)
        return fftvis_amd.simulate_vis_gain_chi2(data, **at, gains=g + g.dtype.type(s * h) * dg, weights=w,
                                                 wrt=("fluxes", "gains"))[1]

    vals = {s: grad(s) for s in (-2, -1, 1, 2)}
    scale = grad(0, np.zeros_like(d))
    for i, (an, name) in enumerate(((hf, "fluxes"), (hg, "gains"))):
        fd = (vals[-2][i] - 8 * vals[-1][i] + 8 * vals[1][i] - vals[2][i]) / (12 * h)
        tol = 1.5 * BOUND[precision] * np.linalg.norm(scale[i]) / h
        print("gain gauss-newton stencil", precision, sky, beams, name, np.linalg.norm(fd - an), tol, np.linalg.norm(an))
        assert np.linalg.norm(an) > 0 and np.linalg.norm(fd - an) <= tol


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_unit_gains_reproduce_the_call_without_gains(gpu, monkeypatch, precision, sky, beams):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w = _directions(cfg), _weights(cfg)
    names = ("fluxes", "baselines", "topo")
    plain = _gn(cfg, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    unit = _ggn(cfg, **dirs, gains=np.ones_like(_gains(cfg)), weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    assert np.array_equal(unit[0], plain[0]) and np.array_equal(unit[2], plain[2])
    assert _same_flux(unit[1][0], plain[1][0]) and all(np.array_equal(a, b) for a, b in zip(unit[1][1:], plain[1][1:]))


def test_a_gain_direction_alone_runs_no_tangent_pass(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _edge_cfg()
    w, g = _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    ran, forwards = [], []
    for name in dir(gs.SimHandle):
        if name.startswith("run_") and name.endswith("tangent"):
            monkeypatch.setattr(gs.SimHandle, name, lambda self, *a, _n=name, **k: ran.append(_n))
    real = gs.SimHandle.run_device
    monkeypatch.setattr(gs.SimHandle, "run_device", lambda self, *a, **k: forwards.append(a[:2]) or real(self, *a, **k))
    quad, prods = _ggn(cfg, gains=g, d_gains=dg, weights=w)
    assert ran == [] and forwards == [(0, len(cfg["times"]))]  # one forward at the real fluxes, nothing else
    assert isinstance(prods, tuple) and len(prods) == 1 and prods[0].shape == g.shape and quad > 0
    monkeypatch.undo()
    rows, _, hg_ref, _, _, _ = _reference(cfg, {}, w, g, dg)
    assert rel_l2(prods[0], hg_ref) <= BOUND[2] and abs(quad - rows.sum()) <= BOUND[2] * quad
    assert abs(ggr.inner_gains(dg, prods[0]) - 2 * quad) <= BOUND[2] * 2 * quad


def test_time_handling(gpu, monkeypatch):
    """Constant gains are per-time gains repeated; one ``gain_weight_block`` per time block and no ``weight_block``."""
    from fftvis_amd.gpu import gpu_simulate

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg(ntimes=3)
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    rep, drep = np.repeat(g[..., None], 3, axis=-1), np.repeat(dg[..., None], 3, axis=-1)
    names = ("fluxes", "gains")
    kw = dict(weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    one = _ggn(cfg, **dirs, gains=g, d_gains=dg, **kw)
    per = _ggn(cfg, **dirs, gains=rep, d_gains=drep, **kw)
    assert np.array_equal(per[0], one[0]) and np.array_equal(per[2], one[2]) and per[1][1].shape == rep.shape
    assert np.abs(per[1][1].sum(axis=-1) - one[1][1]).max() <= 1e-14 * np.abs(one[1][1]).max()
    calls, plain = [], []
    real = gpu_simulate.SimHandle.gain_weight_block
    monkeypatch.setattr(gpu_simulate.SimHandle, "gain_weight_block",
                        lambda self, *a, **k: calls.append((a[0], a[1], len(a[4]), a[5] is not None, tuple(a[7].shape)))
                        or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate.SimHandle, "weight_block", lambda self, *a, **k: plain.append(a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    blk = _ggn(cfg, **dirs, gains=rep, d_gains=drep, **kw)
    nant, nf = len(cfg["ants"]), len(cfg["freqs"])
    assert calls == [(t, t + 1, 2, True, (nf, 1, 2, nant)) for t in range(3)] and plain == [], (calls, plain)
    assert np.all(np.abs(blk[0] - per[0]) <= 1e-12 * per[0]) and rel_l2(blk[2], per[2]) <= 1e-12
    assert rel_l2(blk[1][1], per[1][1]) <= 1e-12 and np.abs(blk[1][0] - per[1][0]).max() <= 1e-12 * np.abs(per[1][0]).max()


def test_time_blocks_are_sized_for_the_forward_block_too(gpu, monkeypatch):
    """``_time_block`` sees the parts, half a block of weights and, only when V is held, one block more."""
    from fftvis_amd.gpu import gpu_simulate

    cfg = _edge_cfg()
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    nf = len(cfg["freqs"])
    seen = []
    real = gpu_simulate._time_block
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: seen.append(a[2]) or real(*a, **k))
    _ggn(cfg, **dirs, gains=g, weights=w, wrt=())                 # two parts and weights, fixed gains: 2.5 blocks
    _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, wrt=())     # ... and V: 3.5
    _ggn(cfg, **dirs, gains=g, weights=w, wrt="gains")            # ... V for the gain block alone: 3.5
    _ggn(cfg, gains=g, d_gains=dg, wrt=())                        # V alone
    assert seen == [int(np.ceil(2.5 * nf)), int(np.ceil(3.5 * nf)), int(np.ceil(3.5 * nf)), nf], seen


@pytest.mark.parametrize("path,took", [("type3", 3), ("type2", 2)])
def test_lattice_forward_is_type1_for_the_fluxes_and_the_gains(gpu, monkeypatch, path, took):
    """Gains alone do not force the type-3 transform: the handle stays a lattice handle, which alone takes the type-2
    adjoint."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = hex19_config()
    dirs, w, g = {"d_fluxes": _directions(cfg)["d_fluxes"]}, _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    quad, (gf, hg), G = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, wrt=("fluxes", "gains"), return_gvis=True,
                             adjoint_path=path)
    assert _handle().last_adjoint_path() == took
    rows, G_ref, hg_ref, _, _, _ = _reference(cfg, dirs, w, g, dg)
    assert rel_l2(G, G_ref) <= BOUND[2] and rel_l2(hg, hg_ref) <= BOUND[2] and abs(quad - rows.sum()) <= BOUND[2] * quad
    no_flux = {k: v for k, v in cfg.items() if k != "fluxes"}
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **no_flux, adjoint_path=path))
    with pytest.raises(ValueError, match="adjoint_path='type2' needs the lattice path"):
        _ggn(cfg, **dirs, gains=g, d_gains=dg, wrt=("fluxes", "ants"), adjoint_path="type2")


def test_device_tensors(gpu):
    import torch

    cfg = _edge_cfg()
    d, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    rng = np.random.default_rng(8)
    dirs = dict(d_fluxes=d["d_fluxes"], d_baselines=1e-2 * rng.normal(size=(len(cfg["baselines"]), 3)))
    names = ("fluxes", "ants", "gains")
    kw = dict(wrt=names, quad_per="freq_time", return_gvis=True)
    quad_ft, prods, G = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=w, **kw)
    D = {k: torch.from_numpy(v).cuda() for k, v in dirs.items()}
    W = torch.from_numpy(w).cuda()
    dq, dp, dG = _ggn(cfg, **D, gains=torch.from_numpy(g).cuda(), d_gains=torch.from_numpy(dg).cuda(), weights=W, **kw)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dq, dG) + tuple(dp))
    assert dp[2].dtype == torch.complex128 and tuple(dp[2].shape) == g.shape
    assert np.all(np.abs(dq.cpu().numpy() - quad_ft) <= BOUND[2] * quad_ft) and rel_l2(dG.cpu().numpy(), G) <= BOUND[2]
    assert all(rel_l2(a.cpu().numpy(), b) <= BOUND[2] for a, b in zip(dp, prods))
    hq, hp, hG = _ggn(cfg, gains=g, d_gains=torch.from_numpy(dg), weights=torch.from_numpy(w), **dict(kw, wrt="gains"))
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cpu" for x in (hq, hp, hG))


def test_staged_buffers_are_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the forward."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _ggn(cfg, **dirs, gains=g, d_gains=_d_gains(cfg, g), weights=w)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    # (the pairs and their incidence lists stay with the handle: 16 bytes per baseline)
    assert held.value - before < 16 * len(cfg["baselines"]) + 4096, (before, held.value)


def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu, monkeypatch):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg()
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    V = fftvis_amd.simulate_vis(**cfg)
    first = _ggn(cfg, **dirs, gains=g, d_gains=_d_gains(cfg, g), weights=w, quad_per="freq_time", return_gvis=True)
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), V)
    again = _ggn(cfg, **dirs, gains=g, d_gains=_d_gains(cfg, g), weights=w, quad_per="freq_time", return_gvis=True)
    # (the pairs are set again with the same values: nothing is rebuilt, and the bits are the first call's)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[2], first[2])
    assert np.array_equal(again[1][-1], first[1][-1])


def test_flagged_samples_and_a_bad_weight(gpu):
    cfg = _edge_cfg()
    dirs, w, g = _directions(cfg), _weights(cfg), _gains(cfg)
    dg = _d_gains(cfg, g)
    flagged = np.random.default_rng(2).random(w.shape) < 0.3
    wf = w.copy()
    wf[flagged] = 0
    quad_ft, hg, G = _assert_value("flags", cfg, dirs, wf, g, dg)
    assert np.all(G[flagged] == 0) and np.all(G[~flagged] != 0)
    with pytest.raises(_lib.FftvisHipError, match="weights are negative or not finite"):
        _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=-w, wrt=())
    again = _ggn(cfg, **dirs, gains=g, d_gains=dg, weights=wf, wrt=(), quad_per="freq_time")[0]  # the handle stays usable
    assert np.array_equal(again, quad_ft)


def test_the_handle_call_needs_the_pairs(gpu):
    """``fv_sim_gain_weight_block`` on a handle a call without gains configured: ``run_residual_gains``' message."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _edge_cfg()
    nf, nt, nant = len(cfg["freqs"]), len(cfg["times"]), len(cfg["ants"])
    gs.release_handles()
    fftvis_amd.simulate_vis(**cfg)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run, without pairs
    try:
        part = torch.zeros(h.out_shape(nt, nf), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(_lib.FftvisHipError, match="fv_sim_gain_weight_block: fv_sim_set_gain_pairs first"):
            h.gain_weight_block(0, nt, 0, nf, [part], None, None, np.ones((nf, nt, 2, nant), dtype=np.complex128))
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
