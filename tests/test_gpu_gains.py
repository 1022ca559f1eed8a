"""GPU tests of the per-antenna gains in the fused objective (``simulate_vis_gain_chi2``, ``torch_simulate_vis_chi2``,
``fv_sim_run_residual_gains`` and the kernel pair alone through ``fv_gain_residual_chi2``).

The kernel pair is held to bounds derived from its arithmetic.  u = eps_T / 2 is the unit roundoff of the run's precision T.
A complex product fl(a b) has per component two products and one sum, each component within 2 u |a| |b|, the modulus within
2 sqrt(2) u |a| |b| <= 3 u |a| |b| (fused multiply-adds only lower this).  The in-place kernel forms, in T and in this order,
m = conj(g1) g2 (3 u |m|), V' = m V (3 u |m| |V| of its own plus 3 u from m: 6 u |m| |V|), delta = V' - d (component-wise:
u |delta| more), G' = 2 (w delta) (one rounding and an exact doubling: 12 u w |m| |V| + 2 u |G'| so far) and the stored
G = conj(m) G' (|m| times that, plus 3 u |G| from m, plus 3 u |G| of its own): to first order
    |G - G_ref| <= u (12 w |m|^2 |V| + 8 |G_ref|)  <=  eps_T (12 w |m|^2 |V| + 8 |G_ref|),
the bound asserted, against the fp64 reference of the same T-typed inputs.  The element function's arithmetic in T is compiled
without floating-point contraction, so numpy reproduces its T-typed delta bit for bit, operation by operation; the rows' sums
add the fp64 terms w (dr^2 + di^2) of that delta (at most four roundings each, fused or not: c = 4) in some order: ``(L + 4) 2^-52`` relative to ``math.fsum``,
L = tpol nbls, as for ``fv_residual_chi2``.  The gain gradient adds, per antenna, n_a signed fp64 terms (n_a = nfeed times the
antenna's incidences); a term is conj(G') g V with G' = 2 w (m V - d) formed in fp64.  The test's data keep
|m V| + |d| <= 4 |m V - d| at every unflagged sample (asserted), so the rounding of V' (6 u |V'|) reaches delta as at most
(6 * 4 + 1) u |delta|, the weight adds u, the other factor g V 3 u and the last product 3 u: 32 u = 16 * 2^-52 per term on the
device and as much in the numpy reference, and the two summation orders n_a u each:
    |ggains - ref| <= (n_a + 32) 2^-52 sum |terms|.
Through the engine the value is held to ``test_gpu_objective``'s BOUND, ten times the project's bound for two runs of one
forward, the data being chosen so that ||G|| >= 0.1 ||2 w V'||."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import basis_source_refs as bsr
from tests import gain_refs
from tests.helpers import rel_l2
from tests.objective_refs import row_sums_exact
from tests.source_adjoint_refs import source_config
from tests.test_gpu_sky_adjoint import _same_flux
from tests.test_gpu_source_adjoint import _edge_cfg, _sid

pytestmark = pytest.mark.gpu

BOUND = {2: 1e-11, 1: 1e-4}  # test_gpu_objective's
CDT = {1: np.complex64, 2: np.complex128}
RDT = {1: np.float32, 2: np.float64}
NANT = 7


# ---- 1. the kernel pair alone --------------------------------------------------------------------------------------------
def _pairs(nbls, rng, nant=NANT):
    """Random pairs over antennas 0 .. nant - 3 with autos; antenna nant - 2 appears in autos only, antenna nant - 1 in no
    baseline, and antenna 0 in every second baseline (more than 64 from nbls = 257 on)."""
    a1, a2 = rng.integers(0, nant - 2, nbls), rng.integers(0, nant - 2, nbls)
    a1[2::2] = 0
    a2[::7] = a1[::7]
    if nbls > 1:
        a1[1] = a2[1] = nant - 2
    if nbls > 8:
        a1[8] = a2[8] = nant - 2
    return a1.astype(np.int32), a2.astype(np.int32)


def _kernel_inputs(nrows, nbls, tpol, precision, weights, seed=0, pairs=None, nant=NANT):
    rng = np.random.default_rng(seed + 10 * nbls + tpol)
    shape = (nrows, tpol * nbls)
    nfeed = 2 if tpol == 4 else 1

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    a1, a2 = _pairs(nbls, rng, nant) if pairs is None else pairs
    V, d = c(shape).astype(CDT[precision]), c(shape).astype(CDT[precision])
    g = (1 + 0.3 * c((nrows, nfeed, nant))).astype(CDT[precision])
    Vp = gain_refs.apply_gains(_blocked(V, tpol), g, a1, a2).reshape(shape)
    near = np.abs(Vp) + np.abs(d) > 3.5 * np.abs(Vp - d)  # (keeps the cancellation in V' - d bounded: the module docstring)
    d[near] = -d[near]
    w = None
    if weights != "none":
        w = rng.uniform(0.5, 2.0, size=shape).astype(RDT[precision])
    if weights == "flags":
        flagged = rng.random(shape) < 0.3
        flagged[0, 0] = True
        w[flagged] = 0
        d[flagged] = np.where(rng.random(int(flagged.sum())) < 0.5, complex(np.nan, 0.0), complex(np.inf, -np.inf))
    return V, d, w, g, a1, a2


def _blocked(x, tpol):
    return x.reshape(x.shape[0], 2, 2, -1) if tpol == 4 else x


def _run(V, d, w, g, a1, a2, tpol, precision, want_gg=True):
    G, chi2 = V.copy(), np.full(V.shape[0], -1.0)
    gg = np.full(g.shape, 7.0, dtype=np.complex128) if want_gg else None
    status = _lib.lib().fv_gain_residual_chi2(0, precision, V.shape[0], len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                              _lib.ptr(g), _lib.ptr(G), _lib.ptr(d), _lib.ptr(w), _lib.ptr(chi2), _lib.ptr(gg))
    return status, G, chi2, gg


def _delta_as_the_kernel_forms_it(V, d, g, a1, a2, tpol):
    """m = conj(g1) g2, V' = m V and delta = V' - d operation by operation in T (no contraction), as the element function."""
    nbls = len(a1)
    pol = np.arange(V.shape[1]) // nbls
    k = np.arange(V.shape[1]) % nbls
    p, q = (pol & 1, pol >> 1) if tpol == 4 else (0 * pol, 0 * pol)
    g1, g2 = g[:, p, a1[k]], g[:, q, a2[k]]
    mr = g1.real * g2.real + g1.imag * g2.imag
    mi = g1.real * g2.imag - g1.imag * g2.real
    return (mr * V.real - mi * V.imag) - d.real, (mr * V.imag + mi * V.real) - d.imag


def _check_kernel_pair(label, V, d, w, g, a1, a2, tpol, precision):
    nbls, L = len(a1), V.shape[1]
    status, G, chi2, gg = _run(V, d, w, g, a1, a2, tpol, precision)
    assert status == 0, _lib.lib().fv_last_error()
    used = np.ones(V.shape, bool) if w is None else w != 0
    w64 = np.ones(V.shape) if w is None else w.astype(np.float64)
    Vb, db, wb = _blocked(V, tpol), _blocked(d, tpol), _blocked(w64, tpol)
    rows_ref, Gp_ref, G_ref, gg_ref, gg_abs = gain_refs.chi2_gains(Vb, db, wb, g, a1, a2, with_abs=True)
    G_ref = G_ref.reshape(V.shape)
    m = gain_refs.gain_product(g, a1, a2, tpol == 4).reshape(V.shape)
    Vp = m * V.astype(np.complex128)
    dz = np.where(used, d, 0).astype(np.complex128)
    assert np.all((np.abs(Vp) + np.abs(dz) <= 4 * np.abs(Vp - dz))[used])  # the data condition of the gradient's bound
    eps_t = float(np.finfo(RDT[precision]).eps)
    err = np.abs(G.astype(np.complex128) - G_ref)
    bound = eps_t * (12 * w64 * np.abs(m) ** 2 * np.abs(V) + 8 * np.abs(G_ref))
    print("gain kernels G", label, float((err[used] / bound[used]).max(initial=0.0)))
    assert np.all(err <= bound)
    assert np.all(G[~used] == 0)
    dr, di = _delta_as_the_kernel_forms_it(V, np.where(used, d, 0).astype(V.dtype), g, a1, a2, tpol)
    terms = np.where(used, w64 * (dr.astype(np.float64) ** 2 + di.astype(np.float64) ** 2), 0.0)
    exact = row_sums_exact(terms)
    print("gain kernels chi2", label, float((np.abs(chi2 - exact) / np.maximum(exact, 1e-300)).max() / 2.0**-52))
    assert np.all(np.abs(chi2 - exact) <= (L + 4) * 2.0**-52 * exact)
    nfeed = g.shape[1]
    n_a = nfeed * (np.bincount(a1, minlength=g.shape[-1]) + np.bincount(a2, minlength=g.shape[-1]))
    gerr = np.abs(gg - gg_ref)
    gbound = (n_a + 32) * 2.0**-52 * gg_abs
    print("gain kernels ggains", label, float((gerr / np.maximum(gbound, 1e-300)).max()), int(n_a.max()))
    assert np.all(gerr <= gbound)
    assert np.all(gg[..., n_a == 0] == 0) and (n_a == 0).any()
    assert np.all(gg[..., n_a > 0] != 0) or w is not None
    status, G2, chi2_2, gg2 = _run(V, d, w, g, a1, a2, tpol, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(G2, G) and np.array_equal(chi2_2, chi2) and np.array_equal(gg2, gg)
    status, G3, chi2_3, _ = _run(V, d, w, g, a1, a2, tpol, precision, want_gg=False)  # ... with or without the gather
    assert status == 0 and np.array_equal(G3, G) and np.array_equal(chi2_3, chi2)
    return n_a


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_kernel_pair(gpu, nbls, tpol, nrows, precision, weights):
    V, d, w, g, a1, a2 = _kernel_inputs(nrows, nbls, tpol, precision, weights)
    n_a = _check_kernel_pair(f"{nbls} {tpol} {nrows} {precision} {weights}", V, d, w, g, a1, a2, tpol, precision)
    both = set(a1[a1 != a2]) | set(a2[a1 != a2])
    if nbls > 8:
        assert (a1 == a2).sum() > 1 and NANT - 2 not in both and n_a[NANT - 2] > 0  # autos; an antenna in autos only
    if nbls >= 257:
        assert n_a[0] > 64 * (2 if tpol == 4 else 1)


def test_unit_gains_are_the_residual_kernel_bit_for_bit(gpu):
    for precision in (2, 1):
        V, d, w, g, a1, a2 = _kernel_inputs(3, 257, 4, precision, "flags")
        status, G, chi2, _ = _run(V, d, w, np.ones_like(g), a1, a2, 4, precision)
        G0, chi2_0 = V.copy(), np.zeros(3)
        assert _lib.lib().fv_residual_chi2(0, precision, 3, V.shape[1], _lib.ptr(G0), _lib.ptr(d), _lib.ptr(w), _lib.ptr(chi2_0)) == 0
        assert status == 0 and np.array_equal(G, G0) and np.array_equal(chi2, chi2_0)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what,message", [("negative weight", b"1 weights are negative or not finite"),
                                          ("nan weight", b"1 weights are negative or not finite"),
                                          ("nan datum", b"1 entries of data are not finite where the weight is positive")])
def test_bad_input_fails_the_call_and_the_next_good_call_succeeds(gpu, what, message, precision):
    V, d, w, g, a1, a2 = _kernel_inputs(3, 75, 4, precision, "positive")
    good = _run(V, d, w, g, a1, a2, 4, precision)
    assert good[0] == 0
    bw, bd = w.copy(), d.copy()
    if what == "negative weight":
        bw[1, 257] = -1.0
    elif what == "nan weight":
        bw[2, 7] = np.nan
    else:
        bd[0, 299] = complex(1.0, np.nan)
    status = _run(V, bd, bw, g, a1, a2, 4, precision)[0]
    assert status == 1 and message in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    again = _run(V, d, w, g, a1, a2, 4, precision)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))
    if what == "nan datum":  # under a zero weight the same datum is not an error
        bw[0, 299] = 0
        status, G, chi2, gg = _run(V, bd, bw, g, a1, a2, 4, precision)
        assert status == 0 and G[0, 299] == 0 and np.isfinite(chi2).all() and np.isfinite(gg).all()


def test_one_hera350_row(gpu):
    """350 antennas, every cross pair: nbls = 61 075, tpol = 4, one row of 244 300 values over 120 blocks, 349 incidences
    per antenna (698 terms per feed), the gains of a row beyond one block's threads."""
    i, j = np.triu_indices(350, 1)
    assert len(i) == 61_075
    V, d, w, g, a1, a2 = _kernel_inputs(1, 61_075, 4, 2, "flags", pairs=(i.astype(np.int32), j.astype(np.int32)), nant=351)
    n_a = _check_kernel_pair("hera350", V, d, w, g, a1, a2, 4, 2)
    assert n_a.max() == 2 * 349 and n_a[350] == 0


# ---- 2. through the engine -----------------------------------------------------------------------------------------------
def _chi2(cfg, data, **kw):
    """``simulate_vis_gain_chi2`` when gains are given, ``simulate_vis_chi2`` otherwise."""
    return (fftvis_amd.simulate_vis_gain_chi2 if "gains" in kw else fftvis_amd.simulate_vis_chi2)(data, **cfg, **kw)


def _ant_rows(cfg):
    nums = list(cfg["ants"])
    return (np.array([nums.index(b[0]) for b in cfg["baselines"]]), np.array([nums.index(b[1]) for b in cfg["baselines"]]))


def _gains(cfg, seed=11, per_time=False, feed_independent=False):
    """1 + 0.3 N(0, 1) complex, in ``simulate_vis_gain_chi2``'s shape."""
    rng = np.random.default_rng(seed)
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    shape = ((nant, 2) if cfg.get("polarized", False) else (nant,)) + (nf,) + ((nt,) if per_time else ())
    g = 1 + 0.3 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    if feed_independent:
        g[:, 1] = g[:, 0]
    return g.astype(CDT[cfg.get("precision", 2)])


def _block_layout(cfg, g):
    """The gains as the references take them: (nf, nt, nfeed, nant)."""
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    g4 = np.broadcast_to(g.reshape(nant, 2 if cfg.get("polarized", False) else 1, nf, -1), (nant, 2 if cfg.get("polarized", False) else 1, nf, nt))
    return np.ascontiguousarray(g4.transpose(2, 3, 1, 0))


def _from_block(cfg, gg, shape):
    g = gg.transpose(3, 2, 0, 1)
    per_time = len(shape) == (4 if cfg.get("polarized", False) else 3)
    return (g if per_time else g.sum(axis=-1)).reshape(shape)


def _data(cfg, g, seed=5):
    """(d, w): the gained forward of fluxes scaled source by source by 1 + 0.3 N(0, 1), plus noise of half its rms; weights
    U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    p = cfg.get("precision", 2)
    F = np.asarray(cfg["fluxes"])
    V0 = fftvis_amd.simulate_vis(**dict(cfg, fluxes=F * (1 + 0.3 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1)))))
    V0 = gain_refs.apply_gains(V0, _block_layout(cfg, g), *_ant_rows(cfg))
    rms = np.sqrt(np.mean(np.abs(V0) ** 2))
    d = V0 + 0.5 * rms * (rng.normal(size=V0.shape) + 1j * rng.normal(size=V0.shape)) / np.sqrt(2)
    return d.astype(CDT[p]), rng.uniform(0.5, 2.0, size=V0.shape).astype(RDT[p])


def _reference(cfg, d, w, g):
    V = fftvis_amd.simulate_vis(**cfg)
    a1, a2 = _ant_rows(cfg)
    rows, Gp, G, gg = gain_refs.chi2_gains(V, d, w, _block_layout(cfg, g), a1, a2)
    return V, rows, Gp, G, _from_block(cfg, gg, g.shape)


CELLS = [("unpol", "airy"), ("I", "two"), ("full", "complex")]


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_value_and_gradient(gpu, precision, sky, beams):
    """2a and 2d: G, chi2 per (f, t) and ggains against ``simulate_vis`` -> ``gain_refs``; ggains against the five-point
    stencil of the device's own chi2."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    g = _gains(cfg)
    d, w = _data(cfg, g)
    chi2_ft, gg, G = _chi2(cfg, d, weights=w, gains=g, wrt="gains", chi2_per="freq_time", return_gvis=True)
    V, rows, Gp, G_ref, gg_ref = _reference(cfg, d, w, g)
    two_wv = 2 * w.astype(np.float64) * gain_refs.apply_gains(V, _block_layout(cfg, g), *_ant_rows(cfg))
    print("gains value", precision, sky, beams, rel_l2(G, G_ref), float((np.abs(chi2_ft - rows) / rows).max()),
          rel_l2(gg, gg_ref), np.linalg.norm(Gp) / np.linalg.norm(two_wv))
    assert np.linalg.norm(Gp) >= 0.1 * np.linalg.norm(two_wv)
    assert G.shape == V.shape and G.dtype == CDT[precision] and rel_l2(G, G_ref) <= BOUND[precision]
    assert chi2_ft.shape == V.shape[:2] and np.all(np.abs(chi2_ft - rows) <= BOUND[precision] * rows)
    assert gg.shape == g.shape and gg.dtype == np.complex128 and rel_l2(gg, gg_ref) <= BOUND[precision]
    rng = np.random.default_rng(9)
    h = 0.25
    for _ in range(2):
        dg = rng.normal(size=g.shape) + 1j * rng.normal(size=g.shape)
        dg = (dg / np.linalg.norm(dg)).astype(g.dtype)
        vals = {s: _chi2(cfg, d, weights=w, gains=g + g.dtype.type(s * h) * dg, wrt=())[0] for s in (-2, -1, 1, 2)}
        fd = (vals[-2] - 8 * vals[-1] + 8 * vals[1] - vals[2]) / (12 * h)
        an = float(np.sum(np.conj(gg) * dg.astype(np.complex128)).real)
        tol = 1.5 * BOUND[precision] * max(vals.values()) / h
        print("gains stencil", precision, sky, beams, abs(fd - an), tol)
        assert abs(fd - an) <= tol


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_unit_gains_reproduce_the_call_without_gains(gpu, monkeypatch, precision, sky, beams):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    d, w = _data(cfg, np.ones_like(_gains(cfg)))
    names = ("fluxes", "baselines", "topo")
    plain = _chi2(cfg, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True)
    unit = _chi2(cfg, d, weights=w, gains=np.ones_like(_gains(cfg)), wrt=names, chi2_per="freq_time", return_gvis=True)
    assert np.array_equal(unit[0], plain[0]) and np.array_equal(unit[2], plain[2])
    assert _same_flux(unit[1][0], plain[1][0]) and all(np.array_equal(a, b) for a, b in zip(unit[1][1:], plain[1][1:]))


@pytest.mark.parametrize("precision", [2, 1])
def test_feed_axes_are_those_of_jones_matrices_scaled_by_the_gains(gpu, precision):
    """2c: scaling feed column p of antenna a's E-field table by g[a, p] IS the gain product on the output."""
    cfg = _sid(source_config("cm", "full", "complex", False, precision))
    ants = cfg["ants"]
    nant, nf = len(ants), len(cfg["freqs"])
    nums = list(ants)
    bls = [(nums[i], nums[j]) for i, j in [(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2), (4, 4), (5, 3), (0, 0)]]
    rng = np.random.default_rng(0)
    g = np.exp(2j * np.pi * rng.random((nant, 2, nf)))  # a phase of its own per antenna, feed and channel
    g[:, 1] *= 1.6
    assert np.all(np.abs(g[:, 0] - g[:, 1]) >= 0.3 * np.maximum(np.abs(g[:, 0]), np.abs(g[:, 1])))
    base = cfg["beam"]
    tab0 = np.array(base.data, dtype=complex)
    tab0 = np.repeat(tab0, nf, axis=0) if tab0.shape[0] == 1 else tab0
    scaled = [fftvis_amd.TabulatedBeam(tab0 * g[a].T[:, None, :, None, None], cfg["freqs"], base.za_max) for a in range(nant)]
    same = [fftvis_amd.TabulatedBeam(tab0.copy(), cfg["freqs"], base.za_max) for a in range(nant)]
    kw = dict(cfg, beam_idx=np.arange(nant), baselines=bls, reference_compat=False)
    V1 = fftvis_amd.simulate_vis(**dict(kw, beam=scaled))
    V0 = fftvis_amd.simulate_vis(**dict(kw, beam=same))
    a1, a2 = _ant_rows(kw)
    gb = _block_layout(kw, g)
    right = rel_l2(gain_refs.apply_gains(V0, gb, a1, a2), V1)
    m = gain_refs.gain_product(gb, a1, a2, True)
    wrong = [rel_l2(np.swapaxes(m, 2, 3) * V0, V1), rel_l2(np.conj(m) * V0, V1), rel_l2(np.conj(np.swapaxes(m, 2, 3)) * V0, V1)]
    print("gains feed axes", precision, right, wrong)
    assert right <= 100 * cfg["eps"] and min(wrong) >= 0.1
    # ... and the device applies that same product: chi2 of (scaled tables) == chi2 of (base tables, gains)
    d, w = _data(dict(kw, beam=same), g.astype(CDT[precision]))
    c1 = _chi2(dict(kw, beam=scaled), d, weights=w, wrt=(), chi2_per="freq_time")[0]
    c0 = _chi2(dict(kw, beam=same), d, weights=w, gains=g.astype(CDT[precision]), wrt=(), chi2_per="freq_time")[0]
    assert np.all(np.abs(c1 - c0) <= max(BOUND[precision], 100 * cfg["eps"]) * c0)


@pytest.mark.parametrize("precision", [2, 1])
def test_basis_beams_absorb_feed_independent_gains(gpu, monkeypatch, precision):
    """2c and 2e with basis beams: (C, g) is (C g[:, None, :]); the other gradients are the public passes' on G."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    g = _gains(cfg, feed_independent=True)
    d, w = _data(cfg, g)
    C = np.asarray(cfg["beam_coefs"])
    names = ("fluxes", "beam_coefs", "gains")
    chi2, (gf, gc, gg), G = _chi2(cfg, d, weights=w, gains=g, wrt=names, return_gvis=True)
    scaled = dict(cfg, beam_coefs=(C * g[:, 0][:, None, :]).astype(C.dtype))
    chi2_s, gc_s = _chi2(scaled, d, weights=w, wrt="beam_coefs")
    print("gains basis", precision, abs(chi2 - chi2_s) / chi2_s)
    assert abs(chi2 - chi2_s) <= BOUND[precision] * chi2_s
    lhs, rhs = gg.sum(axis=1), (np.conj(C) * gc_s).sum(axis=1)
    assert np.linalg.norm(lhs - rhs) <= BOUND[precision] * np.linalg.norm(rhs)
    rest = {k: v for k, v in cfg.items()}
    wf, wc = fftvis_amd.simulate_vis_basis_adjoint(G, **rest, wrt=("fluxes", "beam_coefs"))
    assert _same_flux(gf, wf) and np.array_equal(gc, wc) and np.count_nonzero(wc) > 0
    assert np.array_equal(_chi2(cfg, d, weights=w, gains=g, wrt="gains")[1], gg)


@pytest.mark.parametrize("precision", [2, 1])
def test_other_gradients_are_the_public_passes_on_gvis(gpu, monkeypatch, precision):
    """2e: with gains every non-gain gradient is its public pass applied to the returned G."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", "full", "two", False, precision))
    g = _gains(cfg)
    d, w = _data(cfg, g)
    names = ("fluxes", "baselines", "topo", "gains")
    chi2, (gf, gb, gt, gg), G = _chi2(cfg, d, weights=w, gains=g, wrt=names, return_gvis=True)
    wf, wt = fftvis_amd.simulate_vis_sky_adjoint(G, **cfg, wrt=("fluxes", "topo"))
    wb = fftvis_amd.simulate_vis_position_adjoint(G, **cfg, wrt="baselines")
    assert _same_flux(gf, wf) and np.array_equal(gt, wt) and np.array_equal(gb, wb)
    assert np.count_nonzero(wt) > 0 and np.count_nonzero(wb) > 0
    assert np.array_equal(_chi2(cfg, d, weights=w, gains=g, wrt="gains")[1], gg)


def test_time_handling(gpu, monkeypatch):
    """2f: constant gains are per-time gains repeated; one ``run_gain_residual`` per time block and no ``run_residual``."""
    from fftvis_amd.gpu import gpu_simulate

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg(ntimes=3)
    g = _gains(cfg)
    d, w = _data(cfg, g)
    rep = np.repeat(g[..., None], 3, axis=-1)
    one = _chi2(cfg, d, weights=w, gains=g, wrt="gains", chi2_per="freq_time", return_gvis=True)
    per = _chi2(cfg, d, weights=w, gains=rep, wrt="gains", chi2_per="freq_time", return_gvis=True)
    assert np.array_equal(per[0], one[0]) and np.array_equal(per[2], one[2]) and per[1].shape == rep.shape
    assert np.abs(per[1].sum(axis=-1) - one[1]).max() <= 1e-14 * np.abs(one[1]).max()
    calls, plain = [], []
    real = gpu_simulate.SimHandle.run_gain_residual
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_gain_residual",
                        lambda self, *a, **k: calls.append((a[0], a[1], tuple(a[6].shape))) or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_residual", lambda self, *a, **k: plain.append(a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    blk = _chi2(cfg, d, weights=w, gains=rep, wrt="gains", chi2_per="freq_time", return_gvis=True)
    nant, nf = len(cfg["ants"]), len(cfg["freqs"])
    assert calls == [(t, t + 1, (nf, 1, 2, nant)) for t in range(3)] and plain == [], (calls, plain)
    assert np.all(np.abs(blk[0] - per[0]) <= 1e-12 * per[0])
    assert rel_l2(blk[1], per[1]) <= 1e-12 and rel_l2(blk[2], per[2]) <= 1e-12


def test_device_tensors_and_torch(gpu, monkeypatch):
    """2g: resident data, weights and gains; the autograd entry point, complex128 and complex64 leaves, a host leaf."""
    import torch

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg()
    g = _gains(cfg)
    d, w = _data(cfg, g)
    names = ("fluxes", "gains")
    chi2_ft, (gf, gg), G = _chi2(cfg, d, weights=w, gains=g, wrt=names, chi2_per="freq_time", return_gvis=True)
    D, W, Gn = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(g).cuda()
    dc, (df, dgg), dG = _chi2(cfg, D, weights=W, gains=Gn, wrt=names, chi2_per="freq_time", return_gvis=True)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dc, df, dgg, dG))
    assert dgg.dtype == torch.complex128 and rel_l2(dgg.cpu().numpy(), gg) <= BOUND[2] and rel_l2(dG.cpu().numpy(), G) <= BOUND[2]
    assert np.all(np.abs(dc.cpu().numpy() - chi2_ft) <= BOUND[2] * chi2_ft) and rel_l2(df.cpu().numpy(), gf) <= BOUND[2]
    hg = _chi2(cfg, torch.from_numpy(d), weights=torch.from_numpy(w), gains=Gn, wrt="gains")[1]  # gains elsewhere: copied
    assert isinstance(hg, torch.Tensor) and hg.device.type == "cpu" and rel_l2(hg.numpy(), gg) <= BOUND[2]
    total = _chi2(cfg, d, weights=w, gains=g, wrt=())[0]
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    F = torch.tensor(np.asarray(cfg["fluxes"]), dtype=torch.float64, device="cuda")
    for dtype, leaf_device in ((torch.complex128, "cuda"), (torch.complex64, "cuda"), (torch.complex128, "cpu")):
        leaf = torch.from_numpy(g).to(device=leaf_device, dtype=dtype).requires_grad_(True)
        want_c, want = _chi2(cfg, D, weights=W, gains=leaf.detach(), wrt="gains")
        loss = fftvis_amd.torch_simulate_vis_chi2(D, F, weights=W, gains=leaf, **kw)
        assert loss.dtype == torch.float64 and loss.item() == want_c
        loss.backward()
        assert leaf.grad.dtype == dtype and leaf.grad.device.type == leaf_device
        assert torch.equal(leaf.grad, want.to(device=leaf_device, dtype=dtype))
    assert abs(want_c - total) <= BOUND[2] * total
    leaf, Fl = Gn.clone().requires_grad_(True), F.clone().requires_grad_(True)
    want_c, (wf, wg) = _chi2(cfg, D, weights=W, gains=Gn, wrt=names)
    fftvis_amd.torch_simulate_vis_chi2(D, Fl, weights=W, gains=leaf, **kw).backward()
    assert torch.equal(leaf.grad, wg) and torch.equal(Fl.grad, wf.to(Fl.grad.dtype))
    const = fftvis_amd.torch_simulate_vis_chi2(D, Fl, weights=W, gains=g, **kw)  # a constant array is passed through
    assert const.item() == want_c


def test_raw_c_abi(gpu, monkeypatch):
    """2h: ``fv_sim_run_residual_gains`` on the cached handle the last Python call configured: host and device buffers,
    ggains NULL, a sub-block of times and channels."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")

    L = _lib.lib()
    fn = L.fv_sim_run_residual_gains
    cfg = _edge_cfg()
    g = _gains(cfg, per_time=True)
    d, w = _data(cfg, g)
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    gs.release_handles()
    V = fftvis_amd.simulate_vis(**cfg)
    chi2_ft, gg, G = _chi2(cfg, d, weights=w, gains=g, wrt="gains", chi2_per="freq_time", return_gvis=True)
    gb = _block_layout(cfg, g)
    gg_b = np.ascontiguousarray(gg.transpose(2, 3, 1, 0))
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run, the pairs included
    try:
        hG, hc, hgg = np.full(d.shape, 7.0, dtype=np.complex128), np.full((nf, nt), -1.0), np.full(gb.shape, 7.0, dtype=np.complex128)
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(w), 0, hp(gb), 0, hp(hG), 0, hp(hc), hp(hgg), 0) == 0, L.fv_last_error()
        assert rel_l2(hG, G) <= BOUND[2] and np.all(np.abs(hc - chi2_ft) <= BOUND[2] * chi2_ft) and rel_l2(hgg, gg_b) <= BOUND[2]
        dD, dW, dGn = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(gb).cuda()
        dG = torch.full(d.shape, 7.0, dtype=torch.complex128, device="cuda")
        dgg = torch.full(gb.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        dc = np.full((nf, nt), -1.0)
        assert fn(h._h, 0, nt, 0, nf, p(dD), 1, p(dW), 1, p(dGn), 1, p(dG), 1, hp(dc), p(dgg), 1) == 0, L.fv_last_error()
        assert rel_l2(dG.cpu().numpy(), G) <= BOUND[2] and rel_l2(dgg.cpu().numpy(), gg_b) <= BOUND[2]
        assert np.all(np.abs(dc - chi2_ft) <= BOUND[2] * chi2_ft)
        nG, nc = np.full(d.shape, 7.0, dtype=np.complex128), np.full((nf, nt), -1.0)  # ggains NULL: the same G and rows
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(w), 0, hp(gb), 0, hp(nG), 0, hp(nc), None, 0) == 0, L.fv_last_error()
        assert np.array_equal(nG, hG) and np.array_equal(nc, hc)
        # one channel, the second time step, no weights
        blk, gblk = np.ascontiguousarray(d[1:2, 1:2]), np.ascontiguousarray(gb[1:2, 1:2])
        bG, bc, bgg = np.zeros_like(blk), np.full((1, 1), -1.0), np.zeros(gblk.shape, dtype=np.complex128)
        assert fn(h._h, 1, 2, 1, 2, hp(blk), 0, None, 0, hp(gblk), 0, hp(bG), 0, hp(bc), hp(bgg), 0) == 0, L.fv_last_error()
        a1, a2 = _ant_rows(cfg)
        rows, _, ref_G, ref_gg = gain_refs.chi2_gains(V[1:2, 1:2], blk, None, gblk, a1, a2)
        # (a run of one channel plans its own grid: the transform's tolerance, as in test_gpu_objective.test_raw_c_abi)
        assert rel_l2(bG, ref_G) <= 10 * cfg["eps"] and abs(bc[0, 0] - rows[0, 0]) <= 10 * cfg["eps"] * rows[0, 0]
        assert rel_l2(bgg, ref_gg) <= 10 * cfg["eps"]
        for t0, t1, f0, f1 in [(1, 1, 0, nf), (0, nt, 2, 2)]:
            assert fn(h._h, t0, t1, f0, f1, hp(d), 0, None, 0, hp(gb), 0, hp(hG), 0, hp(hc), None, 0) == 1
            assert b"empty range" in L.fv_last_error()
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # a fresh handle has no pairs
    try:
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, None, 0, hp(gb), 0, hp(hG), 0, hp(hc), None, 0) == 1
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
