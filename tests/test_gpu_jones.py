"""GPU tests of the Jones gains in the fused objective (``simulate_vis_jones_chi2``, ``torch_simulate_vis_chi2(jones=)``,
``fv_sim_run_residual_jones`` and the kernels alone through ``fv_jones_residual_chi2``), section by section as
``test_gpu_gains.py`` tests the diagonal gains.

The kernels are held to bounds derived from their arithmetic.  u = eps_T / 2 is the unit roundoff of the run's precision T; a
complex product fl(a b) is within 3 u |a| |b| of a b and a complex sum within u of its value.  The in-place kernel forms, in
T, B = V conj(G1) (a sum of two products: 4 u of its majorant), V' = G2^T B (4 u from B, 3 u and u of its own: 8 u S, with
S[x, y] = sum |G1[y', y]| |G2[x', x]| |V[x', y']|; 9 u S covers either product order, the sixteen triple products too),
delta = V' - d (u |delta| more), G' = 2 (w delta) (one rounding and an exact doubling): |G' - G'_ref| <= 18 u w S + 2 u |G'|
with 9 u S for V'.  The stored G is two
more 2 x 2 products of G': 8 u T of their own, T[x', y'] = sum |G2[x', x]| |G'_ref[x, y]| |G1[y', y]|, plus the error of G'
carried through, sum |G2| |G1| (18 u w S + 2 u |G'|) = u (18 P + 2 T) with P[x', y'] = sum |G2[x', x]| |G1[y', y]| w[x, y]
S[x, y]: to first order |G - G_ref| <= u (18 P + 10 T) <= u (18 P + 11 T), and
    |G - G_ref| <= eps_T (18 P + 11 T)
is asserted element by element, twice the first-order bound, against the fp64 reference of the same T-typed inputs.  A
row's chi2 adds the fp64 terms w |delta|^2 of the T-typed delta, |delta - delta_ref| <= e = eps_T (9 S + |delta_ref|), in
the row walk's order: |chi2 - fsum_ref| <= sum w (2 |delta_ref| e + e^2) + (4 nbls + 4) 2^-52 ref.  The gradient adds, per
antenna and entry, n_a signed fp64 terms (n_a = 2 x the antenna's incidences: two products per incidence), each a chain of
products and sums formed in fp64 on the device and in numpy from the same inputs; with A the reference's formula with every
factor replaced by its modulus and delta by S + |d| over the unflagged samples, a term is within 19 * 2^-53 of its
majorant on each side, and the two summation orders add n_a 2^-53 each:
    |gjones - ref| <= (n_a + 40) 2^-52 A.
Through the engine every result is held to ``test_gpu_objective``'s BOUND, ten times the project's bound for two runs of
one forward, the data being chosen so that ||G'|| >= 0.1 ||2 w V'||."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import gain_refs, jones_refs
from tests.helpers import rel_l2
from tests.objective_refs import row_sums_exact
from tests.source_adjoint_refs import source_config
from tests.test_gpu_gains import BOUND, CDT, NANT, RDT, _ant_rows, _pairs
from tests.test_gpu_sky_adjoint import _same_flux
from tests.test_gpu_source_adjoint import _edge_cfg, _sid

pytestmark = pytest.mark.gpu

TRIPLE = "...ack,...cdk,...bdk->...abk"  # out[x', y'] = sum_{x, y} G2[x', x] M[x, y] G1[y', y]


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------
def _matrices(shape, rng, dtype):
    """Identity plus 0.3 N(0, 1) complex in every entry: gains and leakage of the same size."""
    J = 0.3 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    J[..., 0, 0, :] += 1
    J[..., 1, 1, :] += 1
    return J.astype(dtype)


def _kernel_inputs(nrows, nbls, precision, weights, seed=0, pairs=None, nant=NANT, J=None):
    rng = np.random.default_rng(seed + 10 * nbls + 4)
    shape = (nrows, 4 * nbls)

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    a1, a2 = _pairs(nbls, rng, nant) if pairs is None else pairs
    V, d = c(shape).astype(CDT[precision]), c(shape).astype(CDT[precision])
    J = _matrices((nrows, 2, 2, nant), rng, CDT[precision]) if J is None else J(rng).astype(CDT[precision])
    Vp = jones_refs.apply_jones(_blocked(V), J, a1, a2).reshape(shape)
    near = np.abs(Vp) + np.abs(d) > 3.5 * np.abs(Vp - d)  # (bounded cancellation in V' - d: the gain kernels' data condition)
    d[near] = -d[near]
    w = None
    if weights != "none":
        w = rng.uniform(0.5, 2.0, size=shape).astype(RDT[precision])
    if weights in ("flags", "baselines"):
        flagged = rng.random(shape) < 0.3
        flagged[0, 0] = True
        if weights == "baselines":  # every sample of every third baseline
            whole = np.zeros((nrows, 4, nbls), bool)
            whole[:, :, ::3] = True
            flagged |= whole.reshape(shape)
        w[flagged] = 0
        d[flagged] = np.where(rng.random(int(flagged.sum())) < 0.5, complex(np.nan, 0.0), complex(np.inf, -np.inf))
    return V, d, w, J, a1, a2


def _blocked(x):
    return x.reshape(x.shape[0], 2, 2, -1)


def _run(V, d, w, J, a1, a2, precision, want_gj=True):
    G, chi2 = V.copy(), np.full(V.shape[0], -1.0)
    gj = np.full(J.shape, 7.0, dtype=np.complex128) if want_gj else None
    status = _lib.lib().fv_jones_residual_chi2(0, precision, V.shape[0], len(a1), J.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                               _lib.ptr(J), _lib.ptr(G), _lib.ptr(d), _lib.ptr(w), _lib.ptr(chi2), _lib.ptr(gj))
    return status, G, chi2, gj


def _bounds(V, d, w, J, a1, a2, precision):
    """The fp64 reference of the T-typed inputs and the module docstring's bounds: (used, rows_ref, G_ref, gj_ref, the
    bound of G, of the rows, of gjones, n_a)."""
    used = np.ones(V.shape, bool) if w is None else w != 0
    w64 = np.ones(V.shape) if w is None else w.astype(np.float64)
    Vb, db, wb, ub = _blocked(V), _blocked(d), _blocked(w64), _blocked(used)
    rows_ref, Gp_ref, G_ref, gj_ref, A = jones_refs.chi2_jones(Vb, db, wb, J, a1, a2, with_abs=True)
    eps_t = float(np.finfo(RDT[precision]).eps)
    absJ = np.abs(J.astype(np.complex128))
    G1, G2 = absJ[..., a1], absJ[..., a2]
    S = jones_refs.apply_jones(np.abs(Vb), absJ, a1, a2).real
    T = np.einsum(TRIPLE, G2, np.abs(Gp_ref), G1)
    P = np.einsum(TRIPLE, G2, wb * S, G1)
    g_bound = eps_t * (18 * P + 11 * T)
    delta = np.where(ub, jones_refs.apply_jones(Vb, J, a1, a2) - np.where(ub, db, 0), 0)
    e = eps_t * (9 * S + np.abs(delta))
    exact = row_sums_exact((wb * np.abs(delta) ** 2).reshape(V.shape))
    r_bound = (wb * (2 * np.abs(delta) * e + e**2)).reshape(V.shape).sum(axis=1) + (V.shape[1] + 4) * 2.0**-52 * exact
    n_a = 2 * (np.bincount(a1, minlength=J.shape[-1]) + np.bincount(a2, minlength=J.shape[-1]))
    return used, exact, G_ref.reshape(V.shape), gj_ref, g_bound.reshape(V.shape), r_bound, (n_a + 40) * 2.0**-52 * A, n_a


def _check_kernels(label, V, d, w, J, a1, a2, precision):
    status, G, chi2, gj = _run(V, d, w, J, a1, a2, precision)
    assert status == 0, _lib.lib().fv_last_error()
    used, exact, G_ref, gj_ref, g_bound, r_bound, j_bound, n_a = _bounds(V, d, w, J, a1, a2, precision)
    err = np.abs(G.astype(np.complex128) - G_ref)
    print("jones kernels G", label, float((err[g_bound > 0] / g_bound[g_bound > 0]).max(initial=0.0)))
    assert np.all(err <= g_bound)
    none_used = ~_blocked(used).any(axis=(1, 2))  # (nrows, nbls): every sample of the baseline flagged
    assert np.all(_blocked(G).transpose(0, 3, 1, 2)[none_used] == 0)
    print("jones kernels chi2", label, float((np.abs(chi2 - exact) / np.maximum(r_bound, 1e-300)).max()))
    assert np.all(np.abs(chi2 - exact) <= r_bound)
    jerr = np.abs(gj - gj_ref)
    print("jones kernels gjones", label, float((jerr / np.maximum(j_bound, 1e-300)).max()), int(n_a.max()))
    assert np.all(jerr <= j_bound)
    assert np.all(gj[..., n_a == 0] == 0) and (n_a == 0).any()
    assert np.all(gj[..., n_a > 0] != 0) or w is not None
    status, G2, chi2_2, gj2 = _run(V, d, w, J, a1, a2, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(G2, G) and np.array_equal(chi2_2, chi2) and np.array_equal(gj2, gj)
    status, G3, chi2_3, _ = _run(V, d, w, J, a1, a2, precision, want_gj=False)  # ... with or without the gather
    assert status == 0 and np.array_equal(G3, G) and np.array_equal(chi2_3, chi2)
    return n_a, none_used


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_kernels(gpu, nbls, nrows, precision, weights):
    V, d, w, J, a1, a2 = _kernel_inputs(nrows, nbls, precision, weights)
    n_a, _ = _check_kernels(f"{nbls} {nrows} {precision} {weights}", V, d, w, J, a1, a2, precision)
    both = set(a1[a1 != a2]) | set(a2[a1 != a2])
    if nbls > 8:
        assert (a1 == a2).sum() > 1 and NANT - 2 not in both and n_a[NANT - 2] > 0  # autos; an antenna in autos only
    if nbls >= 257:
        assert n_a[0] > 2 * 64  # more than one entry per lane


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nbls", [64, 257])
def test_baselines_with_every_sample_flagged(gpu, nbls, precision):
    V, d, w, J, a1, a2 = _kernel_inputs(7, nbls, precision, "baselines")
    _, none_used = _check_kernels(f"whole baselines {nbls} {precision}", V, d, w, J, a1, a2, precision)
    assert none_used[:, ::3].all() and not none_used.all()


def test_identity_matrices_are_the_residual_kernel_bit_for_bit(gpu):
    for precision in (2, 1):
        for nbls in (257, 256):  # misaligned planes, and the vector path
            V, d, w, J, a1, a2 = _kernel_inputs(3, nbls, precision, "flags")
            eye = jones_refs.diagonal(np.ones((3, 2, NANT), dtype=CDT[precision]))
            status, G, chi2, _ = _run(V, d, w, eye, a1, a2, precision)
            G0, chi2_0 = V.copy(), np.zeros(3)
            assert _lib.lib().fv_residual_chi2(0, precision, 3, V.shape[1], _lib.ptr(G0), _lib.ptr(d), _lib.ptr(w),
                                               _lib.ptr(chi2_0)) == 0
            assert status == 0 and np.array_equal(G, G0) and np.array_equal(chi2, chi2_0)


@pytest.mark.parametrize("precision", [2, 1])
def test_diagonal_matrices_agree_with_the_gain_kernels(gpu, precision):
    """Within the sum of the two kernel pairs' bounds: this module's and ``test_gpu_gains``' (G: eps_T (12 w |m|^2 |V| +
    8 |G_ref|); rows: delta within eps_T (6 |m V| + |delta_ref|), twice its first-order error; ggains: (n_a + 32) 2^-52 of
    the sum of the moduli of its terms)."""
    nant, nbls = NANT, 257
    g = {}

    def diag(rng):
        g["g"] = (1 + 0.3 * (rng.normal(size=(5, 2, nant)) + 1j * rng.normal(size=(5, 2, nant)))).astype(CDT[precision])
        return jones_refs.diagonal(g["g"])

    V, d, w, J, a1, a2 = _kernel_inputs(5, nbls, precision, "flags", J=diag)
    g = g["g"]
    status, G, chi2, gj = _run(V, d, w, J, a1, a2, precision)
    assert status == 0, _lib.lib().fv_last_error()
    Gg, chi2_g, gg = V.copy(), np.zeros(5), np.zeros(g.shape, dtype=np.complex128)
    assert _lib.lib().fv_gain_residual_chi2(0, precision, 5, nbls, 4, nant, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(g), _lib.ptr(Gg),
                                            _lib.ptr(d), _lib.ptr(w), _lib.ptr(chi2_g), _lib.ptr(gg)) == 0
    used, exact, G_ref, gj_ref, g_bound, r_bound, j_bound, n_a = _bounds(V, d, w, J, a1, a2, precision)
    eps_t = float(np.finfo(RDT[precision]).eps)
    w64 = w.astype(np.float64)
    m = gain_refs.gain_product(g, a1, a2, True).reshape(V.shape)
    gg_abs = gain_refs.chi2_gains(_blocked(V), _blocked(d), _blocked(w64), g, a1, a2, with_abs=True)[4]
    assert np.all(np.abs(G.astype(np.complex128) - Gg)
                  <= g_bound + eps_t * (12 * w64 * np.abs(m) ** 2 * np.abs(V) + 8 * np.abs(G_ref)))
    delta = np.where(used, m * V.astype(np.complex128) - np.where(used, d, 0), 0)
    e = eps_t * (6 * np.abs(m * V) + np.abs(delta))
    rows_g = (w64 * (2 * np.abs(delta) * e + e**2)).sum(axis=1) + (V.shape[1] + 4) * 2.0**-52 * exact
    assert np.all(np.abs(chi2 - chi2_g) <= r_bound + rows_g)
    for f in range(2):
        assert np.all(np.abs(gj[:, f, f] - gg[:, f]) <= j_bound[:, f, f] + (n_a + 32) * 2.0**-52 * gg_abs[:, f])
    assert np.abs(gj[:, 0, 1]).max() > 0  # (the leakage entries' gradient does not vanish at diagonal matrices)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what,message", [("negative weight", b"1 weights are negative or not finite"),
                                          ("nan weight", b"1 weights are negative or not finite"),
                                          ("nan datum", b"1 entries of data are not finite where the weight is positive")])
def test_bad_input_fails_the_call_and_the_next_good_call_succeeds(gpu, what, message, precision):
    V, d, w, J, a1, a2 = _kernel_inputs(3, 75, precision, "positive")
    good = _run(V, d, w, J, a1, a2, precision)
    assert good[0] == 0
    bw, bd = w.copy(), d.copy()
    if what == "negative weight":
        bw[1, 257] = -1.0
    elif what == "nan weight":
        bw[2, 7] = np.nan
    else:
        bd[0, 299] = complex(1.0, np.nan)
    status = _run(V, bd, bw, J, a1, a2, precision)[0]
    assert status == 1 and message in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    again = _run(V, d, w, J, a1, a2, precision)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))
    if what == "nan datum":  # under a zero weight the same datum is not an error
        bw[0, 299] = 0
        status, G, chi2, gj = _run(V, bd, bw, J, a1, a2, precision)
        assert status == 0 and np.isfinite(G).all() and np.isfinite(chi2).all() and np.isfinite(gj).all()


def test_one_hera350_row(gpu):
    """350 antennas, every cross pair: nbls = 61 075 (odd: the four planes of the row are not aligned alike), one row of
    244 300 values, 349 incidences per antenna, the row's matrices (351 x 4 complex128, 22 KB) staged in LDS."""
    i, j = np.triu_indices(350, 1)
    assert len(i) == 61_075
    V, d, w, J, a1, a2 = _kernel_inputs(1, 61_075, 2, "flags", pairs=(i.astype(np.int32), j.astype(np.int32)), nant=351)
    n_a, _ = _check_kernels("hera350", V, d, w, J, a1, a2, 2)
    assert n_a.max() == 2 * 349 and n_a[350] == 0


# ---- 2. through the engine -----------------------------------------------------------------------------------------------
def _chi2(cfg, data, **kw):
    """``simulate_vis_jones_chi2`` when matrices are given, ``simulate_vis_gain_chi2`` for gains, else ``simulate_vis_chi2``."""
    fn = (fftvis_amd.simulate_vis_jones_chi2 if "jones" in kw else
          fftvis_amd.simulate_vis_gain_chi2 if "gains" in kw else fftvis_amd.simulate_vis_chi2)
    return fn(data, **cfg, **kw)


def _jones(cfg, seed=11, per_time=False):
    """Identity plus 0.3 N(0, 1) complex in every entry, in ``simulate_vis_jones_chi2``'s shape."""
    rng = np.random.default_rng(seed)
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    shape = (nant, 2, 2, nf) + ((nt,) if per_time else ())
    J = 0.3 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    J[:, 0, 0] += 1
    J[:, 1, 1] += 1
    return J.astype(CDT[cfg.get("precision", 2)])


def _identity(cfg):
    J = np.zeros((len(cfg["ants"]), 2, 2, len(cfg["freqs"])), dtype=CDT[cfg.get("precision", 2)])
    J[:, 0, 0] = J[:, 1, 1] = 1
    return J


def _block_layout(cfg, J):
    """The matrices as the references take them: (nf, nt, 2, 2, nant)."""
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    J5 = np.broadcast_to(J.reshape(nant, 2, 2, nf, -1), (nant, 2, 2, nf, nt))
    return np.ascontiguousarray(J5.transpose(3, 4, 1, 2, 0))


def _from_block(gj, shape):
    g = gj.transpose(4, 2, 3, 0, 1)
    return g if len(shape) == 5 else g.sum(axis=-1)


def _data(cfg, J, seed=5):
    """(d, w): the forward of fluxes scaled source by source by 1 + 0.3 N(0, 1) through the matrices, plus noise of half its
    rms; weights U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    p = cfg.get("precision", 2)
    F = np.asarray(cfg["fluxes"])
    V0 = fftvis_amd.simulate_vis(**dict(cfg, fluxes=F * (1 + 0.3 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1)))))
    V0 = jones_refs.apply_jones(V0, _block_layout(cfg, J), *_ant_rows(cfg))
    rms = np.sqrt(np.mean(np.abs(V0) ** 2))
    d = V0 + 0.5 * rms * (rng.normal(size=V0.shape) + 1j * rng.normal(size=V0.shape)) / np.sqrt(2)
    return d.astype(CDT[p]), rng.uniform(0.5, 2.0, size=V0.shape).astype(RDT[p])


def _reference(cfg, d, w, J):
    V = fftvis_amd.simulate_vis(**cfg)
    a1, a2 = _ant_rows(cfg)
    rows, Gp, G, gj = jones_refs.chi2_jones(V, d, w, _block_layout(cfg, J), a1, a2)
    return V, rows, Gp, G, _from_block(gj, J.shape)


CELLS = [("I", "two"), ("full", "complex")]  # (the polarized cells of test_gpu_gains)


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_value_and_gradient(gpu, precision, sky, beams):
    """2a: G, chi2 per (f, t) and gjones against ``simulate_vis`` -> ``jones_refs``; gjones against the five-point stencil of
    the device's own chi2."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    J = _jones(cfg)
    d, w = _data(cfg, J)
    chi2_ft, gj, G = _chi2(cfg, d, weights=w, jones=J, wrt="jones", chi2_per="freq_time", return_gvis=True)
    V, rows, Gp, G_ref, gj_ref = _reference(cfg, d, w, J)
    two_wv = 2 * w.astype(np.float64) * jones_refs.apply_jones(V, _block_layout(cfg, J), *_ant_rows(cfg))
    print("jones value", precision, sky, beams, rel_l2(G, G_ref), float((np.abs(chi2_ft - rows) / rows).max()),
          rel_l2(gj, gj_ref), np.linalg.norm(Gp) / np.linalg.norm(two_wv))
    assert np.linalg.norm(Gp) >= 0.1 * np.linalg.norm(two_wv)
    assert G.shape == V.shape and G.dtype == CDT[precision] and rel_l2(G, G_ref) <= BOUND[precision]
    assert chi2_ft.shape == V.shape[:2] and np.all(np.abs(chi2_ft - rows) <= BOUND[precision] * rows)
    assert gj.shape == J.shape and gj.dtype == np.complex128 and rel_l2(gj, gj_ref) <= BOUND[precision]
    rng = np.random.default_rng(9)
    h = 0.25
    for _ in range(2):
        dJ = rng.normal(size=J.shape) + 1j * rng.normal(size=J.shape)
        dJ = (dJ / np.linalg.norm(dJ)).astype(J.dtype)
        vals = {s: _chi2(cfg, d, weights=w, jones=J + J.dtype.type(s * h) * dJ, wrt=())[0] for s in (-2, -1, 1, 2)}
        fd = (vals[-2] - 8 * vals[-1] + 8 * vals[1] - vals[2]) / (12 * h)
        an = float(np.sum(np.conj(gj) * dJ.astype(np.complex128)).real)
        tol = 1.5 * BOUND[precision] * max(vals.values()) / h
        print("jones stencil", precision, sky, beams, abs(fd - an), tol)
        assert abs(fd - an) <= tol


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_identity_matrices_reproduce_the_call_without_them(gpu, monkeypatch, precision, sky, beams):
    """2b: value, G and the other gradients, bit for bit."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    d, w = _data(cfg, _identity(cfg))
    names = ("fluxes", "baselines", "topo")
    plain = _chi2(cfg, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True)
    unit = _chi2(cfg, d, weights=w, jones=_identity(cfg), wrt=names, chi2_per="freq_time", return_gvis=True)
    assert np.array_equal(unit[0], plain[0]) and np.array_equal(unit[2], plain[2])
    assert _same_flux(unit[1][0], plain[1][0]) and all(np.array_equal(a, b) for a, b in zip(unit[1][1:], plain[1][1:]))


@pytest.mark.parametrize("precision", [2, 1])
def test_diagonal_matrices_reproduce_the_gain_call(gpu, precision):
    """2c: ``jones[a] = diag(gains[a])`` is ``simulate_vis_gain_chi2`` within BOUND: value, G, and the diagonal of gjones."""
    cfg = _sid(source_config("cm", "full", "two", False, precision))
    rng = np.random.default_rng(3)
    nant, nf = len(cfg["ants"]), len(cfg["freqs"])
    g = (1 + 0.3 * (rng.normal(size=(nant, 2, nf)) + 1j * rng.normal(size=(nant, 2, nf)))).astype(CDT[precision])
    J = np.zeros((nant, 2, 2, nf), dtype=g.dtype)
    J[:, 0, 0], J[:, 1, 1] = g[:, 0], g[:, 1]
    d, w = _data(cfg, J)
    cj, gj, Gj = _chi2(cfg, d, weights=w, jones=J, wrt="jones", chi2_per="freq_time", return_gvis=True)
    cg, gg, Gg = _chi2(cfg, d, weights=w, gains=g, wrt="gains", chi2_per="freq_time", return_gvis=True)
    assert np.all(np.abs(cj - cg) <= BOUND[precision] * cg) and rel_l2(Gj, Gg) <= BOUND[precision]
    assert rel_l2(np.stack([gj[:, 0, 0], gj[:, 1, 1]], axis=1), gg) <= BOUND[precision]


@pytest.mark.parametrize("precision", [2, 1])
def test_matrices_mix_the_feed_columns_of_the_jones_matrices(gpu, precision):
    """2d, the convention: mixing the feed columns of antenna a's E-field table by Gamma_a, new[f, ax, j] = sum_i tab[f, ax, i]
    Gamma[a, i, j, f], IS ``apply_jones`` on the output; its transposed, conjugated and antenna-swapped variants are not."""
    cfg = _sid(source_config("cm", "full", "complex", False, precision))
    ants = cfg["ants"]
    nant, nf = len(ants), len(cfg["freqs"])
    nums = list(ants)
    bls = [(nums[i], nums[j]) for i, j in [(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2), (4, 4), (5, 3), (0, 0)]]
    rng = np.random.default_rng(0)
    J = 0.5 * (rng.normal(size=(nant, 2, 2, nf)) + 1j * rng.normal(size=(nant, 2, 2, nf)))
    J[:, 0, 0] += 1
    J[:, 1, 1] += 1.6
    base = cfg["beam"]
    tab0 = np.array(base.data, dtype=complex)
    tab0 = np.repeat(tab0, nf, axis=0) if tab0.shape[0] == 1 else tab0
    mixed = [fftvis_amd.TabulatedBeam(np.einsum("faizn,ijf->fajzn", tab0, J[a]), cfg["freqs"], base.za_max) for a in range(nant)]
    same = [fftvis_amd.TabulatedBeam(tab0.copy(), cfg["freqs"], base.za_max) for a in range(nant)]
    kw = dict(cfg, beam_idx=np.arange(nant), baselines=bls, reference_compat=False)
    V1 = fftvis_amd.simulate_vis(**dict(kw, beam=mixed))
    V0 = fftvis_amd.simulate_vis(**dict(kw, beam=same))
    a1, a2 = _ant_rows(kw)
    Jb = _block_layout(kw, J)
    right = rel_l2(jones_refs.apply_jones(V0, Jb, a1, a2), V1)
    wrong = [rel_l2(jones_refs.apply_jones(V0, np.swapaxes(Jb, 2, 3), a1, a2), V1),
             rel_l2(jones_refs.apply_jones(V0, np.conj(Jb), a1, a2), V1),
             rel_l2(jones_refs.apply_jones(V0, Jb, a2, a1), V1)]
    print("jones feed axes", precision, right, wrong)
    assert right <= 100 * cfg["eps"] and min(wrong) >= 0.1
    # ... and the device applies that same product: chi2 of (mixed tables) == chi2 of (base tables, jones)
    Jt = J.astype(CDT[precision])
    d, w = _data(dict(kw, beam=same), Jt)
    c1 = _chi2(dict(kw, beam=mixed), d, weights=w, wrt=(), chi2_per="freq_time")[0]
    c0 = _chi2(dict(kw, beam=same), d, weights=w, jones=Jt, wrt=(), chi2_per="freq_time")[0]
    assert np.all(np.abs(c1 - c0) <= max(BOUND[precision], 100 * cfg["eps"]) * c0)


@pytest.mark.parametrize("precision", [2, 1])
def test_other_gradients_are_the_public_passes_on_gvis(gpu, monkeypatch, precision):
    """2e: with matrices every other gradient is its public pass applied to the returned G."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", "full", "two", False, precision))
    J = _jones(cfg)
    d, w = _data(cfg, J)
    names = ("fluxes", "baselines", "topo", "jones")
    chi2, (gf, gb, gt, gj), G = _chi2(cfg, d, weights=w, jones=J, wrt=names, return_gvis=True)
    wf, wt = fftvis_amd.simulate_vis_sky_adjoint(G, **cfg, wrt=("fluxes", "topo"))
    wb = fftvis_amd.simulate_vis_position_adjoint(G, **cfg, wrt="baselines")
    assert _same_flux(gf, wf) and np.array_equal(gt, wt) and np.array_equal(gb, wb)
    assert np.count_nonzero(wt) > 0 and np.count_nonzero(wb) > 0
    assert np.array_equal(_chi2(cfg, d, weights=w, jones=J, wrt="jones")[1], gj)


def test_time_handling(gpu, monkeypatch):
    """2f: constant matrices are per-time matrices repeated; one ``run_jones_residual`` per time block, and neither
    ``run_residual`` nor ``run_gain_residual``."""
    from fftvis_amd.gpu import gpu_simulate

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg(ntimes=3)
    J = _jones(cfg)
    d, w = _data(cfg, J)
    rep = np.repeat(J[..., None], 3, axis=-1)
    one = _chi2(cfg, d, weights=w, jones=J, wrt="jones", chi2_per="freq_time", return_gvis=True)
    per = _chi2(cfg, d, weights=w, jones=rep, wrt="jones", chi2_per="freq_time", return_gvis=True)
    assert np.array_equal(per[0], one[0]) and np.array_equal(per[2], one[2]) and per[1].shape == rep.shape
    assert np.abs(per[1].sum(axis=-1) - one[1]).max() <= 1e-14 * np.abs(one[1]).max()
    calls, others = [], []
    real = gpu_simulate.SimHandle.run_jones_residual
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_jones_residual",
                        lambda self, *a, **k: calls.append((a[0], a[1], tuple(a[6].shape))) or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_residual", lambda self, *a, **k: others.append(a))
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_gain_residual", lambda self, *a, **k: others.append(a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    blk = _chi2(cfg, d, weights=w, jones=rep, wrt="jones", chi2_per="freq_time", return_gvis=True)
    nant, nf = len(cfg["ants"]), len(cfg["freqs"])
    assert calls == [(t, t + 1, (nf, 1, 2, 2, nant)) for t in range(3)] and others == [], (calls, others)
    assert np.all(np.abs(blk[0] - per[0]) <= 1e-12 * per[0])
    assert rel_l2(blk[1], per[1]) <= 1e-12 and rel_l2(blk[2], per[2]) <= 1e-12


def test_device_tensors_and_torch(gpu, monkeypatch):
    """2g: resident data, weights and matrices; the autograd entry point, complex128 and complex64 leaves, a host leaf."""
    import torch

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg()
    J = _jones(cfg)
    d, w = _data(cfg, J)
    names = ("fluxes", "jones")
    chi2_ft, (gf, gj), G = _chi2(cfg, d, weights=w, jones=J, wrt=names, chi2_per="freq_time", return_gvis=True)
    D, W, Jn = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(J).cuda()
    dc, (df, dgj), dG = _chi2(cfg, D, weights=W, jones=Jn, wrt=names, chi2_per="freq_time", return_gvis=True)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dc, df, dgj, dG))
    assert dgj.dtype == torch.complex128 and rel_l2(dgj.cpu().numpy(), gj) <= BOUND[2] and rel_l2(dG.cpu().numpy(), G) <= BOUND[2]
    assert np.all(np.abs(dc.cpu().numpy() - chi2_ft) <= BOUND[2] * chi2_ft) and rel_l2(df.cpu().numpy(), gf) <= BOUND[2]
    hj = _chi2(cfg, torch.from_numpy(d), weights=torch.from_numpy(w), jones=Jn, wrt="jones")[1]  # matrices elsewhere: copied
    assert isinstance(hj, torch.Tensor) and hj.device.type == "cpu" and rel_l2(hj.numpy(), gj) <= BOUND[2]
    total = _chi2(cfg, d, weights=w, jones=J, wrt=())[0]
    kw = {k: v for k, v in cfg.items() if k != "fluxes"}
    F = torch.tensor(np.asarray(cfg["fluxes"]), dtype=torch.float64, device="cuda")
    for dtype, leaf_device in ((torch.complex128, "cuda"), (torch.complex64, "cuda"), (torch.complex128, "cpu")):
        leaf = torch.from_numpy(J).to(device=leaf_device, dtype=dtype).requires_grad_(True)
        want_c, want = _chi2(cfg, D, weights=W, jones=leaf.detach(), wrt="jones")
        loss = fftvis_amd.torch_simulate_vis_chi2(D, F, weights=W, jones=leaf, **kw)
        assert loss.dtype == torch.float64 and loss.item() == want_c
        loss.backward()
        assert leaf.grad.dtype == dtype and leaf.grad.device.type == leaf_device
        assert torch.equal(leaf.grad, want.to(device=leaf_device, dtype=dtype))
    assert abs(want_c - total) <= BOUND[2] * total
    leaf, Fl = Jn.clone().requires_grad_(True), F.clone().requires_grad_(True)
    want_c, (wf, wj) = _chi2(cfg, D, weights=W, jones=Jn, wrt=names)
    fftvis_amd.torch_simulate_vis_chi2(D, Fl, weights=W, jones=leaf, **kw).backward()
    assert torch.equal(leaf.grad, wj) and torch.equal(Fl.grad, wf.to(Fl.grad.dtype))
    const = fftvis_amd.torch_simulate_vis_chi2(D, Fl, weights=W, jones=J, **kw)  # a constant array is passed through
    assert const.item() == want_c


def test_raw_c_abi(gpu, monkeypatch):
    """2h: ``fv_sim_run_residual_jones`` on the cached handle the last Python call configured: host and device buffers,
    gjones NULL, a sub-block of times and channels, empty ranges, a handle without pairs, a handle that is not polarized."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")

    L = _lib.lib()
    fn = L.fv_sim_run_residual_jones
    cfg = _edge_cfg()
    J = _jones(cfg, per_time=True)
    d, w = _data(cfg, J)
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    gs.release_handles()
    V = fftvis_amd.simulate_vis(**cfg)
    chi2_ft, gj, G = _chi2(cfg, d, weights=w, jones=J, wrt="jones", chi2_per="freq_time", return_gvis=True)
    Jb = _block_layout(cfg, J)
    gj_b = np.ascontiguousarray(gj.transpose(3, 4, 1, 2, 0))
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run, the pairs included
    try:
        hG, hc, hgj = np.full(d.shape, 7.0, dtype=np.complex128), np.full((nf, nt), -1.0), np.full(Jb.shape, 7.0, dtype=np.complex128)
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(w), 0, hp(Jb), 0, hp(hG), 0, hp(hc), hp(hgj), 0) == 0, L.fv_last_error()
        assert rel_l2(hG, G) <= BOUND[2] and np.all(np.abs(hc - chi2_ft) <= BOUND[2] * chi2_ft) and rel_l2(hgj, gj_b) <= BOUND[2]
        dD, dW, dJ = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(Jb).cuda()
        dG = torch.full(d.shape, 7.0, dtype=torch.complex128, device="cuda")
        dgj = torch.full(Jb.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        dc = np.full((nf, nt), -1.0)
        assert fn(h._h, 0, nt, 0, nf, p(dD), 1, p(dW), 1, p(dJ), 1, p(dG), 1, hp(dc), p(dgj), 1) == 0, L.fv_last_error()
        assert rel_l2(dG.cpu().numpy(), G) <= BOUND[2] and rel_l2(dgj.cpu().numpy(), gj_b) <= BOUND[2]
        assert np.all(np.abs(dc - chi2_ft) <= BOUND[2] * chi2_ft)
        nG, nc = np.full(d.shape, 7.0, dtype=np.complex128), np.full((nf, nt), -1.0)  # gjones NULL: the same G and rows
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(w), 0, hp(Jb), 0, hp(nG), 0, hp(nc), None, 0) == 0, L.fv_last_error()
        assert np.array_equal(nG, hG) and np.array_equal(nc, hc)
        # one channel, the second time step, no weights
        blk, jblk = np.ascontiguousarray(d[1:2, 1:2]), np.ascontiguousarray(Jb[1:2, 1:2])
        bG, bc, bgj = np.zeros_like(blk), np.full((1, 1), -1.0), np.zeros(jblk.shape, dtype=np.complex128)
        assert fn(h._h, 1, 2, 1, 2, hp(blk), 0, None, 0, hp(jblk), 0, hp(bG), 0, hp(bc), hp(bgj), 0) == 0, L.fv_last_error()
        a1, a2 = _ant_rows(cfg)
        rows, _, ref_G, ref_gj = jones_refs.chi2_jones(V[1:2, 1:2], blk, None, jblk, a1, a2)
        # (a run of one channel plans its own grid: the transform's tolerance, as in test_gpu_objective.test_raw_c_abi)
        assert rel_l2(bG, ref_G) <= 10 * cfg["eps"] and abs(bc[0, 0] - rows[0, 0]) <= 10 * cfg["eps"] * rows[0, 0]
        assert rel_l2(bgj, ref_gj) <= 10 * cfg["eps"]
        for t0, t1, f0, f1 in [(1, 1, 0, nf), (0, nt, 2, 2)]:
            assert fn(h._h, t0, t1, f0, f1, hp(d), 0, None, 0, hp(Jb), 0, hp(hG), 0, hp(hc), None, 0) == 1
            assert b"empty range" in L.fv_last_error()
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # a fresh handle has no pairs
    try:
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, None, 0, hp(Jb), 0, hp(hG), 0, hp(hc), None, 0) == 1
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
    unpol = _sid(source_config("cm", "unpol", "airy", False, 2))
    fftvis_amd.simulate_vis(**unpol)
    key, h = gs._acquire_handle(0, 2, unpol["eps"], 2, False)  # configured, and not polarized
    try:
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, None, 0, hp(Jb), 0, hp(hG), 0, hp(hc), None, 0) == 1
        assert b"polarized" in L.fv_last_error()
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
