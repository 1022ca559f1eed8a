"""GPU tests of the Gauss-Newton product with 2 x 2 Jones gains (``simulate_vis_jones_gauss_newton``,
``fv_sim_jones_weight_block`` and the kernel pair alone through ``fv_jones_weight_rows``), section by section as
``test_gpu_gain_gauss_newton.py`` tests the diagonal gains.

The kernel pair is held to bounds derived from its arithmetic, as ``test_gpu_jones`` derives its own.  u = eps_T / 2 is the
unit roundoff of the run's precision T; a complex product fl(a b) is within 3 u |a| |b| of a b and a component-wise sum within
u of its value.  With S(X; A, B)[x, y] = sum conj(A[y', y]) B[x', x] X[x', y'] the in-place kernel forms, in T and in this
order,
    U = ((P_0 + P_1) + P_2) + P_3                        (NP - 1 <= 3 adds: 3 u Z, Z = sum_j |P_j| >= |U|),
    S(U; G1, G2) as jones_residual_baseline forms V'     (B = U conj(G1), a sum of two products: 4 u of its majorant; G2^T B:
                                                          4 u from B, 3 u and u of its own: 8 u, 9 u covers either product
                                                          order; 3 u more from U: 12 u M_0, M_0 = sum |G1| |G2| Z),
    S(V; H1, G2) and S(V; G1, H2), the same way          (V is an input: 9 u M_1 and 9 u M_2, M_1 = sum |H1| |G2| |V|,
                                                          M_2 = sum |G1| |H2| |V|),
    U' = (S(U) + S(V; H1, G2)) + S(V; G1, H2)            (u (M_0 + M_1) for the first sum, u S_tot for the second,
                                                          S_tot = M_0 + M_1 + M_2):
|U' - U'_ref| <= u (14 M_0 + 11 M_1 + 10 M_2) <= 14 u S_tot.  G' = 2 (w U') is one rounding and an exact doubling:
|G' - G'_ref| <= 28 u w S_tot + u |G'|.  The stored G is two more 2 x 2 products of G' (jones_stored_g, the Jones objective's
back half): 8 u T of their own, T[x', y'] = sum |G2[x', x]| |G'_ref[x, y]| |G1[y', y]|, plus the error of G' carried through,
sum |G2| |G1| (28 u w S_tot + u |G'|) = u (28 P + T) with P[x', y'] = sum |G2[x', x]| |G1[y', y]| w[x, y] S_tot[x, y]: to
first order |G - G_ref| <= u (28 P + 9 T), and
    |G - G_ref| <= eps_T (28 P + 9 T)
is asserted element by element, twice the first-order bound, against the fp64 reference of the same T-typed inputs.  The
kernel's arithmetic in T is compiled without floating-point contraction, so numpy reproduces its T-typed U' and G operation
by operation (``_as_the_kernel_forms_it``): before anything runs on the device that reproduction is checked to lie inside
the bound for the very inputs of the test, and the rows' sums -- the fp64 terms w (ur^2 + ui^2) of that U' (at most four
roundings each) added in the row walk's order -- are held to ``(4 nbls + 4) 2^-52`` relative to ``math.fsum`` of the
reproduction's terms, which in turn lie within sum w (2 |U'_ref| e + e^2), e = 14 eps_T S_tot (twice the first-order error of
U'), of the reference's.  The gather adds, per antenna and entry, n_a signed fp64 terms (n_a = 2 x the antenna's incidences:
two products per incidence), each a chain formed in fp64 on the device and in numpy from the same inputs: U' within 14 of its
majorant S_tot (in units of 2^-53), G' = 2 w U' one more (15), M = G2^T V or V conj(G1) 4, the product conj(G') M 3 and the
sum of the two products 1: 23 * 2^-53 on each side, and the two summation orders add n_a 2^-53 each.  With A the reference's
formula with every factor replaced by its modulus and G' by 2 w S_tot over the unflagged samples,
    |hjones - ref| <= (n_a + 46) 2^-52 A
is asserted, twice the first-order chain as in ``test_gpu_jones``.  Through the engine every result is held to
``test_gpu_objective``'s BOUND against the composition ``simulate_vis`` -> public jvp -> the numpy reference, on directions
chosen so that ||U'|| >= 0.1 (||S(U)|| + ||the direction's terms||)."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from tests import gain_gauss_newton_refs as ggr
from tests import gauss_newton_refs as gnr
from tests import jones_gauss_newton_refs as jgr
from tests import jones_refs
from tests.helpers import rel_l2
from tests.objective_refs import row_major_sum, row_sums_exact
from tests.source_adjoint_refs import source_config
from tests.tangent_refs import edge_config, hex19_config
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_gain_gauss_newton import _kernel_inputs as _gain_kernel_inputs
from tests.test_gpu_gains import NANT, _ant_rows, _pairs
from tests.test_gpu_gauss_newton import _composition, _directions, _gn, _weights
from tests.test_gpu_jones import CELLS, TRIPLE, _block_layout, _blocked, _from_block, _identity, _jones, _matrices
from tests.test_gpu_lattice_adjoint import _handle
from tests.test_gpu_objective import BOUND, CDT, RDT, _public
from tests.test_gpu_position_adjoint import K32
from tests.test_gpu_sky_adjoint import _same_flux
from tests.test_gpu_source_adjoint import _edge_cfg, _sid

pytestmark = pytest.mark.gpu


# ---- 1. the kernel pair alone --------------------------------------------------------------------------------------------
def _kernel_inputs(nrows, nbls, nparts, direction, precision, weights, seed=0, pairs=None, nant=NANT, J=None):
    """Parts, V, weights, ``test_gpu_jones._matrices`` and a direction of the same size.  ``weights``: "none", "positive",
    "flags" (30 % of the samples, whose parts and V stay finite: the baseline's other samples use them) or "baselines"
    (also every third baseline whole, with NaN and Inf in its parts and V)."""
    rng = np.random.default_rng(seed + 10 * nbls + 100 * nparts + (1000 if direction else 0) + 4)
    shape = (nrows, 4 * nbls)
    cdt = CDT[precision]

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    a1, a2 = _pairs(nbls, rng, nant) if pairs is None else pairs
    V = c(shape).astype(cdt)
    parts = [c(shape).astype(cdt) for _ in range(nparts)]
    J = _matrices((nrows, 2, 2, nant), rng, cdt) if J is None else J.astype(cdt)
    dJ = (0.3 * c((nrows, 2, 2, nant))).astype(cdt) if direction else None
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
            whole = whole.reshape(shape)
            for x in parts + [V]:
                x[whole] = np.where(rng.random(int(whole.sum())) < 0.5, complex(np.nan, 0.0), complex(np.inf, -np.inf))
        w[flagged] = 0
    return parts, V, w, J, dJ, a1, a2


def _run(parts, V, w, J, dJ, a1, a2, precision, want_hj=True, give_v=True):
    own = [p.copy() for p in parts]
    vis = V.copy() if give_v else None
    q = np.full(V.shape[0], -1.0)
    hj = np.full(J.shape, 7.0, dtype=np.complex128) if want_hj else None
    ptrs = (ctypes.c_void_p * max(len(own), 1))(*[p.ctypes.data for p in own])
    status = _lib.lib().fv_jones_weight_rows(0, precision, V.shape[0], len(a1), J.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                             _lib.ptr(J), _lib.ptr(dJ), len(own), ptrs, _lib.ptr(vis), _lib.ptr(w), _lib.ptr(q),
                                             _lib.ptr(hj))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(own[1:], parts[1:]))  # read only
    if own and give_v:
        assert np.array_equal(vis, V, equal_nan=True)
    return status, (own[0] if own else vis), q, hj


class _C:
    """A complex array as two real arrays of the run's precision, with the kernel's products: every operation rounds on
    its own (numpy does not contract)."""

    def __init__(self, re, im):
        self.re, self.im = re, im

    @classmethod
    def of(cls, z):
        return cls(z.real.copy(), z.imag.copy())

    def mul(self, b):  # jones_mul: a b
        return _C(self.re * b.re - self.im * b.im, self.re * b.im + self.im * b.re)

    def mulc(self, b):  # jones_mulc: a conj(b)
        return _C(self.re * b.re + self.im * b.im, self.im * b.re - self.re * b.im)

    def add(self, b):
        return _C(self.re + b.re, self.im + b.im)


def _entries(X, a):
    """``[X[:, i, j, a[k]] for 2 i + j]`` of matrices (nrows, 2, 2, nant): (nrows, nbls) each."""
    return [_C.of(X[:, i, j][:, a]) for i in range(2) for j in range(2)]


def _sandwich(x, ga, gb):
    """jones_sandwich: B[x', y] = X[x', 0] conj(A[0, y]) + X[x', 1] conj(A[1, y]), S[x, y] = B[0, x] B'[0, y] + B[1, x] B'[1, y]."""
    b = [x[2 * xs].mulc(ga[y]).add(x[2 * xs + 1].mulc(ga[2 + y])) for xs in range(2) for y in range(2)]
    return [gb[xx].mul(b[y]).add(gb[2 + xx].mul(b[2 + y])) for xx in range(2) for y in range(2)]


def _as_the_kernel_forms_it(parts, V, w, J, dJ, a1, a2):
    """(U' real, U' imaginary, G) operation by operation in T, as k_jones_weight_rows: inputs (nrows, 4 nbls) with what lies
    in a wholly flagged baseline zeroed by the caller; U' and G in the inputs' layout, G' = 0 where flagged."""
    nrows, nbls = V.shape[0], len(a1)
    rdt = V.real.dtype
    planes = lambda z: [_C.of(z.reshape(nrows, 4, nbls)[:, p]) for p in range(4)]  # noqa: E731
    g1, g2 = _entries(J, a1), _entries(J, a2)
    up = None
    if parts:
        u = planes(parts[0])
        for p in parts[1:]:
            u = [a.add(b) for a, b in zip(u, planes(p))]
        up = _sandwich(u, g1, g2)
    if dJ is not None:
        v = planes(V)
        d = _sandwich(v, _entries(dJ, a1), g2)
        up = [a.add(b) for a, b in zip(up, d)] if parts else d
        d = _sandwich(v, g1, _entries(dJ, a2))
        up = [a.add(b) for a, b in zip(up, d)]
    wp = [np.ones((nrows, nbls), dtype=rdt) if w is None else w.reshape(nrows, 4, nbls)[:, p] for p in range(4)]
    two = rdt.type(2)
    with np.errstate(invalid="ignore"):
        gp = [_C(np.where(wp[s] > 0, two * (wp[s] * up[s].re), rdt.type(0)), np.where(wp[s] > 0, two * (wp[s] * up[s].im), rdt.type(0)))
              for s in range(4)]
    G = []
    for xs in range(2):  # jones_stored_g
        c0 = gp[0].mulc(g2[2 * xs]).add(gp[2].mulc(g2[2 * xs + 1]))
        c1 = gp[1].mulc(g2[2 * xs]).add(gp[3].mulc(g2[2 * xs + 1]))
        for ys in range(2):
            G.append(c0.mul(g1[2 * ys]).add(c1.mul(g1[2 * ys + 1])))
    assert up[0].re.dtype == rdt and G[0].re.dtype == rdt
    flat = lambda xs: np.stack(xs, axis=1).reshape(nrows, 4 * nbls)  # noqa: E731
    return flat([x.re for x in up]), flat([x.im for x in up]), flat([x.re for x in G]) + 1j * flat([x.im for x in G])


def _bounds(parts, V, w, J, dJ, a1, a2, precision):
    """The fp64 reference of the T-typed inputs and the module docstring's bounds."""
    used = np.ones(V.shape, bool) if w is None else w != 0
    w64 = np.ones(V.shape) if w is None else w.astype(np.float64)
    wb, ub = _blocked(w64), _blocked(used)
    pb, Vb = [_blocked(p) for p in parts], _blocked(V)
    rows_ref, Gp_ref, G_ref, hj_ref, S, A = jgr.jones_gauss_newton(pb, Vb, wb, J, dJ, a1, a2, with_abs=True)
    eps_t = float(np.finfo(RDT[precision]).eps)
    absJ = np.abs(J.astype(np.complex128))
    G1, G2 = absJ[..., a1], absJ[..., a2]
    T = np.einsum(TRIPLE, G2, np.abs(Gp_ref), G1)
    P = np.einsum(TRIPLE, G2, np.where(ub, wb * S, 0), G1)
    g_bound = (eps_t * (28 * P + 9 * T)).reshape(V.shape)
    Up_ref = np.where(ub, jgr.tangent([np.where(ub.any(axis=(1, 2), keepdims=True), p, 0) for p in pb],
                                      np.where(ub.any(axis=(1, 2), keepdims=True), Vb, 0), J, dJ, a1, a2), 0)
    e = np.where(ub, 14 * eps_t * S, 0)
    r_slack = (wb * (2 * np.abs(Up_ref) * e + e**2)).reshape(V.shape).sum(axis=1)
    n_a = 2 * (np.bincount(a1, minlength=J.shape[-1]) + np.bincount(a2, minlength=J.shape[-1]))
    return used, rows_ref, G_ref.reshape(V.shape), hj_ref, g_bound, r_slack, (n_a + 46) * 2.0**-52 * A, n_a


def _check_kernel_pair(label, parts, V, w, J, dJ, a1, a2, precision):
    L = V.shape[1]
    used, rows_ref, G_ref, hj_ref, g_bound, r_slack, h_bound, n_a = _bounds(parts, V, w, J, dJ, a1, a2, precision)
    live = np.repeat(_blocked(used).any(axis=(1, 2))[:, None, :], 4, axis=1).reshape(V.shape)  # baselines with a sample that counts
    z = lambda x: np.where(live, x, 0).astype(x.dtype)  # noqa: E731  (what lies in a wholly flagged baseline is not used)
    w64 = np.ones(V.shape) if w is None else w.astype(np.float64)
    # on the host first: the kernel's own order of operations, reproduced in T, lies inside the bounds for these inputs
    ur, ui, G_t = _as_the_kernel_forms_it([z(p) for p in parts], z(V), w, J, dJ, a1, a2)
    G_t = np.where(live, G_t, 0)
    err_t = np.abs(G_t.astype(np.complex128) - G_ref)
    assert np.all(err_t <= g_bound), (label, float((err_t[g_bound > 0] / g_bound[g_bound > 0]).max()))
    terms = np.where(used, w64 * (ur.astype(np.float64) ** 2 + ui.astype(np.float64) ** 2), 0.0)
    exact = row_sums_exact(terms)
    assert np.all(np.abs(exact - rows_ref.ravel()) <= r_slack + 2.0**-50 * rows_ref.ravel()), label
    # then the device
    status, G, q, hj = _run(parts, V, w, J, dJ, a1, a2, precision)
    assert status == 0, _lib.lib().fv_last_error()
    err = np.abs(G.astype(np.complex128) - G_ref)
    print("jones weight kernels G", label, float((err[g_bound > 0] / g_bound[g_bound > 0]).max(initial=0.0)),
          "the host's reproduction bit for bit:", bool(np.array_equal(G, G_t.astype(G.dtype))))
    assert np.isfinite(G).all() and np.all(err <= g_bound)
    assert np.all(G[~live] == 0)  # fully flagged baselines store exactly 0
    print("jones weight kernels rows", label, float((np.abs(q - exact) / np.maximum(exact, 1e-300)).max() / 2.0**-52))
    assert np.all(np.abs(q - exact) <= (L + 4) * 2.0**-52 * exact)
    herr = np.abs(hj - hj_ref)
    print("jones weight kernels hjones", label, float((herr / np.maximum(h_bound, 1e-300)).max()), int(n_a.max()))
    assert np.all(herr <= h_bound)
    assert np.all(hj[..., n_a == 0] == 0) and (n_a == 0).any()  # an antenna without a baseline gets exactly 0
    assert np.all(hj[..., n_a > 0] != 0) or w is not None
    status, G2, q2, hj2 = _run(parts, V, w, J, dJ, a1, a2, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(G2, G) and np.array_equal(q2, q) and np.array_equal(hj2, hj)
    status, G3, q3, _ = _run(parts, V, w, J, dJ, a1, a2, precision, want_hj=False)  # ... with or without the gather
    assert status == 0 and np.array_equal(G3, G) and np.array_equal(q3, q)
    if parts and dJ is None:  # ... and without V, which only the gather reads then
        status, G4, q4, _ = _run(parts, V, w, J, dJ, a1, a2, precision, want_hj=False, give_v=False)
        assert status == 0 and np.array_equal(G4, G) and np.array_equal(q4, q)
    return n_a, live


@pytest.mark.parametrize("weights", ["none", "positive", "flags", "baselines"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nparts,direction", [(0, True), (1, False), (1, True), (2, True), (4, False), (4, True)])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_kernel_pair(gpu, nbls, nrows, nparts, direction, precision, weights):
    parts, V, w, J, dJ, a1, a2 = _kernel_inputs(nrows, nbls, nparts, direction, precision, weights)
    n_a, live = _check_kernel_pair(f"{nbls} {nrows} {nparts} {direction} {precision} {weights}", parts, V, w, J, dJ, a1, a2,
                                   precision)
    both = set(a1[a1 != a2]) | set(a2[a1 != a2])
    if nbls > 8:
        assert (a1 == a2).sum() > 1 and NANT - 2 not in both and n_a[NANT - 2] > 0  # autos; an antenna in autos only
    if nbls >= 257:
        assert n_a[0] > 2 * 64  # more than one entry per lane
    if weights == "baselines":
        assert not live.reshape(nrows, 4, nbls)[:, :, ::3].any() and (live.any() or nbls == 1)


# ---- 2. identity matrices, no direction: fv_weight_rows' bits ----------------------------------------------------------------
def _weight_rows(parts, w, precision):
    own = [p.copy() for p in parts]
    q = np.full(parts[0].shape[0], -1.0)
    ptrs = (ctypes.c_void_p * len(own))(*[p.ctypes.data for p in own])
    assert _lib.lib().fv_weight_rows(0, precision, parts[0].shape[0], parts[0].shape[1], len(own), ptrs, _lib.ptr(w),
                                     _lib.ptr(q)) == 0
    return own[0], q


@pytest.mark.parametrize("nrows,nbls", [(3, 257), (400, 1), (7, 75)])
@pytest.mark.parametrize("nparts", [1, 2, 3, 4])
def test_identity_matrices_are_the_weight_kernel_bit_for_bit(gpu, nparts, nrows, nbls):
    """Every instance of the kernel: rows of four values (one baseline) whose sums of one to four terms show a last bit that
    a long row's rounding would hide, rows of 300 and of 1 028 values that span the clipped runs and, in fp32, the vector
    path's misaligned planes."""
    for precision in (2, 1):
        parts, V, w, J, _, a1, a2 = _kernel_inputs(nrows, nbls, nparts, False, precision, "flags")
        eye = jones_refs.diagonal(np.ones((nrows, 2, J.shape[-1]), dtype=CDT[precision]))
        G0, q0 = _weight_rows(parts, w, precision)
        status, G, q, _ = _run(parts, V, w, eye, None, a1, a2, precision, want_hj=False)
        assert status == 0 and np.array_equal(G, G0) and np.array_equal(q, q0)
        status, G, q, hj = _run(parts, V, w, eye, np.zeros_like(eye), a1, a2, precision)  # a zero direction
        assert status == 0 and np.array_equal(G, G0) and np.array_equal(q, q0) and np.isfinite(hj).all()


# ---- 3. diagonal matrices and a diagonal direction: fv_gain_weight_rows ------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
def test_diagonal_matrices_agree_with_the_gain_kernels(gpu, precision):
    """Within the sum of the two kernel pairs' bounds: this module's and ``test_gpu_gain_gauss_newton``'s, on its inputs
    (whose data conditions its hgains bound needs) -- G: eps_T (18 w |m| (|m| Z + D |V|) + 8 |G_ref|); rows: U' within
    eps_T (9 |m| Z + 7 D |V| + |U'|), twice its first-order error; hgains: (n_a + 50) 2^-52 of the sum of the moduli of
    its terms.  The flags here leave finite values under them: a flagged sample's parts and V are still read for the
    baseline's other samples, and 0 * NaN is NaN."""
    nant, nbls, nrows = NANT, 257, 5
    parts, V, w, g, dg, a1, a2 = _gain_kernel_inputs(nrows, nbls, 4, 2, True, precision, "positive")
    flagged = np.random.default_rng(17).random(V.shape) < 0.3
    w[flagged] = 0
    J, dJ = jones_refs.diagonal(g), jones_refs.diagonal(dg)
    status, G, q, hj = _run(parts, V, w, J, dJ, a1, a2, precision)
    assert status == 0, _lib.lib().fv_last_error()
    own = [p.copy() for p in parts]
    qg, hg = np.zeros(nrows), np.zeros(g.shape, dtype=np.complex128)
    ptrs = (ctypes.c_void_p * 2)(*[p.ctypes.data for p in own])
    assert _lib.lib().fv_gain_weight_rows(0, precision, nrows, nbls, 4, nant, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(g), _lib.ptr(dg),
                                          2, ptrs, _lib.ptr(V.copy()), _lib.ptr(w), _lib.ptr(qg), _lib.ptr(hg)) == 0
    Gg = own[0]
    used, rows_ref, G_ref, hj_ref, g_bound, r_slack, h_bound, n_a = _bounds(parts, V, w, J, dJ, a1, a2, precision)
    eps_t = float(np.finfo(RDT[precision]).eps)
    w64 = w.astype(np.float64)
    g64, dg64 = g.astype(np.complex128), dg.astype(np.complex128)
    pol = np.arange(4 * nbls) // nbls
    k = np.arange(4 * nbls) % nbls
    g1, g2 = g64[:, pol & 1, a1[k]], g64[:, pol >> 1, a2[k]]
    h1, h2 = dg64[:, pol & 1, a1[k]], dg64[:, pol >> 1, a2[k]]
    m, D = np.conj(g1) * g2, np.abs(h1) * np.abs(g2) + np.abs(g1) * np.abs(h2)
    Z = sum(np.abs(p.astype(np.complex128)) for p in parts)
    absV = np.abs(V.astype(np.complex128))
    gain_g = eps_t * (18 * w64 * np.abs(m) * (np.abs(m) * Z + D * absV) + 8 * np.abs(G_ref))
    assert np.all(np.abs(G.astype(np.complex128) - Gg) <= g_bound + gain_g)
    Up = np.where(used, jgr.tangent([_blocked(p) for p in parts], _blocked(V), J, dJ, a1, a2).reshape(V.shape), 0)
    e = np.where(used, eps_t * (9 * np.abs(m) * Z + 7 * D * absV + np.abs(Up)), 0)
    rows_g = (w64 * (2 * np.abs(Up) * e + e**2)).sum(axis=1) + (V.shape[1] + 4) * 2.0**-52 * rows_ref.ravel()
    assert np.all(np.abs(q - qg) <= r_slack + (V.shape[1] + 4) * 2.0**-52 * rows_ref.ravel() + rows_g)
    hg_abs = ggr.gain_gauss_newton([_blocked(p) for p in parts], _blocked(V), _blocked(w64), g, dg, a1, a2, with_abs=True)[4]
    for f in range(2):
        assert np.all(np.abs(hj[:, f, f] - hg[:, f]) <= h_bound[:, f, f] + (n_a + 50) * 2.0**-52 * hg_abs[:, f])
    assert np.abs(hj[:, 0, 1]).max() > 0 and np.abs(hj[:, 1, 0]).max() > 0  # (cross-hand V: the leakage entries' product)


# ---- 4. a bad weight ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what", ["negative weight", "nan weight"])
def test_bad_weight_fails_the_call_and_the_next_good_call_reproduces_its_bits(gpu, what, precision):
    parts, V, w, J, dJ, a1, a2 = _kernel_inputs(3, 75, 2, True, precision, "positive")
    good = _run(parts, V, w, J, dJ, a1, a2, precision)
    assert good[0] == 0
    bw = w.copy()
    if what == "negative weight":
        bw[1, 257] = -1.0
    else:
        bw[2, 7] = np.nan
    status = _run(parts, V, bw, J, dJ, a1, a2, precision)[0]
    assert status == 1 and b"1 weights are negative or not finite" in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    again = _run(parts, V, w, J, dJ, a1, a2, precision)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))


# ---- 5. one HERA-350 row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
def test_one_hera350_row(gpu, precision):
    """350 antennas, every cross pair: nbls = 61 075 (odd: the four planes of the row are not aligned alike), one row of
    244 300 values over several blocks, 349 incidences per antenna.  The row's matrices, 351 x 4 values, are staged in LDS; in
    fp64 (22 464 bytes) the direction does not fit next to them and is read from global memory, in fp32 both are staged."""
    i, j = np.triu_indices(350, 1)
    assert len(i) == 61_075 and 2 * 351 * 4 * 16 > 32768 >= 351 * 4 * 16 and 2 * 351 * 4 * 8 <= 32768
    parts, V, w, J, dJ, a1, a2 = _kernel_inputs(1, 61_075, 2, True, precision, "flags", pairs=(i.astype(np.int32), j.astype(np.int32)),
                                                nant=351)
    n_a, _ = _check_kernel_pair(f"hera350 {precision}", parts, V, w, J, dJ, a1, a2, precision)
    assert n_a.max() == 2 * 349 and n_a[350] == 0


# ---- 6. matrices beyond the LDS budget ---------------------------------------------------------------------------------------
def test_matrices_beyond_the_lds_budget_are_read_from_global_memory(gpu):
    """1 100 antennas: 4 400 complex128 = 70 400 bytes > GAIN_LDS_BYTES, and 35 200 in fp32: neither the matrices nor the
    direction is staged, in either precision, with and without a direction: the same bounds on every path."""
    rng = np.random.default_rng(3)
    nant, nbls = 1100, 300
    a1, a2 = rng.integers(0, nant - 1, nbls).astype(np.int32), rng.integers(0, nant - 1, nbls).astype(np.int32)
    for precision, direction in ((2, True), (2, False), (1, True), (1, False)):
        parts, V, w, J, dJ, _, _ = _kernel_inputs(2, nbls, 2, direction, precision, "flags", pairs=(a1, a2), nant=nant)
        _check_kernel_pair(f"global matrices {precision} {direction}", parts, V, w, J, dJ, a1, a2, precision)


# ---- 7. through the engine ---------------------------------------------------------------------------------------------------
def _jgn(cfg, **kw):
    return fftvis_amd.simulate_vis_jones_gauss_newton(**cfg, **kw)


def _d_jones(cfg, J, seed=13, scale=0.3):
    rng = np.random.default_rng(seed)
    return (scale * (rng.normal(size=J.shape) + 1j * rng.normal(size=J.shape))).astype(J.dtype)


def _reference(cfg, dirs, w, J, dJ):
    """(rows, G, the matrices' block in J's shape, U', S(U), the direction's terms) from ``simulate_vis`` -> the public jvp ->
    the numpy reference."""
    V = fftvis_amd.simulate_vis(**cfg).astype(np.complex128)
    parts = _composition(cfg, dirs) if dirs else []
    a1, a2 = _ant_rows(cfg)
    Jb = _block_layout(cfg, J)
    dJb = None if dJ is None else _block_layout(cfg, dJ)
    rows, Gp, G, hj = jgr.jones_gauss_newton(parts, V, w, Jb, dJb, a1, a2)
    sky = jgr.tangent(parts, V, Jb, None, a1, a2)
    Up = jgr.tangent(parts, V, Jb, dJb, a1, a2)
    return rows, G, _from_block(hj, J.shape), Up, sky, Up - sky


def _assert_value(label, cfg, dirs, w, J, dJ, **kw):
    p = cfg.get("precision", 2)
    quad_ft, hj, G = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, wrt="jones", quad_per="freq_time", return_gvis=True, **kw)
    rows, G_ref, hj_ref, Up, sky, rest = _reference(cfg, dirs, w, J, dJ)
    cond = np.linalg.norm(Up) / (np.linalg.norm(sky) + np.linalg.norm(rest))
    print("jones gauss-newton value", label, rel_l2(G, G_ref), float((np.abs(quad_ft - rows) / rows).max()), rel_l2(hj, hj_ref),
          cond)
    assert cond >= 0.1  # nothing rides on cancellation
    assert G.shape == G_ref.shape and G.dtype == CDT[p] and rel_l2(G, G_ref) <= BOUND[p]
    assert quad_ft.shape == rows.shape and np.all(rows > 0) and np.all(np.abs(quad_ft - rows) <= BOUND[p] * rows)
    assert hj.shape == J.shape and hj.dtype == np.complex128 and rel_l2(hj, hj_ref) <= BOUND[p]
    return quad_ft, hj, G


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_value(gpu, precision, sky, beams):
    """G, the rows and the matrices' block: a joint direction, fixed matrices, the Jones direction alone."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    label = f"{precision} {sky} {beams}"
    _assert_value(label + " joint", cfg, dirs, w, J, dJ)
    _assert_value(label + " fixed matrices", cfg, dirs, w, J, None)
    _assert_value(label + " matrices alone", cfg, {}, w, J, dJ)
    one = {"d_fluxes": dirs["d_fluxes"]}
    _assert_value(label + " fluxes, no weights", cfg, one, None, J, dJ)
    # the total is the rows' sums added in row-major order
    quad_ft, _ = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, wrt=(), quad_per="freq_time")
    total, prods = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, wrt=())
    assert isinstance(total, float) and prods == () and total == row_major_sum(quad_ft) and total > 0


def _assert_products(label, cfg, dirs, w, J, dJ, names):
    """Every product but the matrices' is its public pass on the returned G, bit for bit (the fluxes under ``_same_flux``)."""
    quad, prods, G = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, wrt=names, return_gvis=True)
    assert isinstance(prods, tuple) and len(prods) == len(names) and quad > 0
    want = _public(cfg, G, tuple(n for n in names if n != "jones"), False)
    for n, got in zip(names, prods):
        if n == "jones":
            assert got.shape == J.shape and got.dtype == np.complex128 and np.count_nonzero(got) > 0
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
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    for names in (("fluxes", "jones"), ("topo", "baselines", "jones"), ("fluxes", "ants", "radec", "jones")):
        _assert_products(f"{precision} {sky} {beams}", cfg, dirs, w, J, dJ, names)
    _assert_products(f"{precision} {sky} {beams} fixed matrices", cfg, dirs, w, J, None, ("fluxes", "ants"))


_ORDER = ("d_ants", "d_baselines", "d_radec", "d_topo", "d_fluxes", "d_beam_coefs")


def _inner(dirs, dJ, prods):
    """<p, prods> over the blocks in ``wrt=None``'s order, the matrices last."""
    order = [k for k in _ORDER if k in dirs]
    return sum(gnr.inner(dirs[k], x) for k, x in zip(order, prods)) + jgr.inner_jones(dJ, prods[-1])


def _norms(dirs, dJ, prods):
    order = [k for k in _ORDER if k in dirs]
    return sum(np.linalg.norm(dirs[k]) * np.linalg.norm(x) for k, x in zip(order, prods)) + \
        np.linalg.norm(dJ) * np.linalg.norm(prods[-1])


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_quadratic_form_and_symmetry(gpu, precision, sky, beams):
    """<p, H p> = 2 quad for a joint direction, and <p1, H p2> = <p2, H p1>.  Each side is a chain of passes held to k base
    times the norms it is rounded in (``test_gpu_gauss_newton._quadratic_form``): the products' pairings, and 2 quad itself
    for the rows."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    w, J = _weights(cfg), _jones(cfg)
    p1, p2 = _directions(cfg, seed=11), _directions(cfg, seed=12)
    dJ1, dJ2 = _d_jones(cfg, J, seed=13), _d_jones(cfg, J, seed=14)
    k = (10.0 if precision == 2 else K32) * _forward_base(cfg)
    quad, H1 = _jgn(cfg, **p1, jones=J, d_jones=dJ1, weights=w)
    _, H2 = _jgn(cfg, **p2, jones=J, d_jones=dJ2, weights=w)
    assert len(H1) == len(p1) + 1 and H1[-1].shape == J.shape  # (wrt=None: the directions' names, then "jones")
    lhs, bound = _inner(p1, dJ1, H1), k * (2 * quad + _norms(p1, dJ1, H1))
    print("jones gauss-newton quadratic form", precision, sky, beams, lhs, 2 * quad, abs(lhs - 2 * quad) / bound)
    assert quad > 0 and abs(lhs - 2 * quad) <= bound
    a, b = _inner(p1, dJ1, H2), _inner(p2, dJ2, H1)
    bound = k * (_norms(p1, dJ1, H2) + _norms(p2, dJ2, H1))
    print("jones gauss-newton symmetry", precision, sky, beams, a, b, abs(a - b) / bound)
    assert abs(a - b) <= bound and abs(a) > 0


def test_small_hessian(gpu):
    """8 sources, 1 channel, 1 time, 6 baselines, Stokes-I fluxes, fp64 at eps 1e-12: H over (8 fluxes, Re and Im of the four
    entries of the matrices of antennas 0 and 1) assembled column by column is symmetric, positive semi-definite and equals
    2 Re(J^H W J), J's flux columns the Jones product of ``simulate_vis`` on unit fluxes and its matrix columns the
    reference tangent, the product's exact linearisation."""
    cfg = edge_config(nsrc=8, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)],
               coord_method="SiderealRotation")
    cfg["fluxes"] = np.ascontiguousarray(synth.catalog(8, cfg["freqs"], 0, polarized_sky=True)[2][..., 0])
    w, Jm = _weights(cfg), _jones(cfg)
    a1, a2 = _ant_rows(cfg)
    Jb = _block_layout(cfg, Jm)
    unit = np.eye(8)[:, :, None]
    jdirs = []
    for a in range(2):
        for i in range(2):
            for j in range(2):
                for c in (1.0, 1j):
                    e = np.zeros(Jm.shape, dtype=Jm.dtype)
                    e[a, i, j, 0] = c
                    jdirs.append(e)

    def column(prods):  # (fluxes, Re hjones, Im hjones): Re conj(hjones) dJ is the gradient in (Re J, Im J)
        return np.concatenate([prods[0][:, 0]] + [[np.sum(np.conj(e) * prods[1]).real] for e in jdirs])

    cols = [column(_jgn(cfg, d_fluxes=unit[j], jones=Jm, weights=w, wrt=("fluxes", "jones"))[1]) for j in range(8)]
    cols += [column(_jgn(cfg, d_jones=e, jones=Jm, weights=w, wrt=("fluxes", "jones"))[1]) for e in jdirs]
    H = np.stack(cols, axis=1)
    V = fftvis_amd.simulate_vis(**cfg).astype(np.complex128)
    Jac = [jones_refs.apply_jones(fftvis_amd.simulate_vis(**dict(cfg, fluxes=unit[j])), Jb, a1, a2).ravel() for j in range(8)]
    Jac += [jgr.tangent([], V, Jb, _block_layout(cfg, e), a1, a2).ravel() for e in jdirs]
    Jac = np.stack(Jac, axis=1)
    H_ref = 2 * (Jac.conj().T @ (w.ravel()[:, None] * Jac)).real
    norm = np.linalg.norm(H_ref)
    low = float(np.linalg.eigvalsh((H + H.T) / 2).min())
    print("jones gauss-newton small hessian", H.shape, np.linalg.norm(H - H.T) / norm, np.linalg.norm(H - H_ref) / norm, low / norm)
    assert H.shape == (8 + len(jdirs),) * 2 and len(jdirs) == 16
    assert np.linalg.norm(H - H.T) <= 10 * BOUND[2] * norm  # (test_gpu_gauss_newton.test_small_hessian's tolerance)
    assert np.linalg.norm(H - H_ref) <= 10 * BOUND[2] * norm
    assert np.all(np.diag(H) >= 0) and np.trace(H) > 0 and low >= -10 * BOUND[2] * norm


@pytest.mark.parametrize("sky,beams", CELLS[1:])
@pytest.mark.parametrize("precision", [2, 1])
def test_stencil_of_the_gradient_at_zero_residual(gpu, precision, sky, beams):
    """With data = V' the residual is 0 and the Hessian of chi2 is the Gauss-Newton one: the five-point stencil of
    ``simulate_vis_jones_chi2``'s ("fluxes", "jones") gradient along p is H p.  The tolerances are
    ``test_gpu_gain_gauss_newton``'s: p is a 1e-2 relative change, so the stencil's truncation is far below its rounding,
    1.5 BOUND times the gradient at data = 0 (the uncancelled term) over h."""
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    w, J = _weights(cfg), _jones(cfg)
    rng = np.random.default_rng(21)
    F = np.asarray(cfg["fluxes"])
    dF = F * 1e-2 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1))
    dJ = (1e-2 * (rng.normal(size=J.shape) + 1j * rng.normal(size=J.shape))).astype(J.dtype)
    a1, a2 = _ant_rows(cfg)
    d = jones_refs.apply_jones(fftvis_amd.simulate_vis(**cfg), _block_layout(cfg, J), a1, a2).astype(CDT[precision])
    _, (hf, hj) = _jgn(cfg, d_fluxes=dF, jones=J, d_jones=dJ, weights=w, wrt=("fluxes", "jones"))
    h = 0.25

    def grad(s, data=d):
        at = dict(cfg, fluxes=F + s * h * dF)
        return fftvis_amd.simulate_vis_jones_chi2(data, **at, jones=J + J.dtype.type(s * h) * dJ, weights=w,
                                                  wrt=("fluxes", "jones"))[1]

    vals = {s: grad(s) for s in (-2, -1, 1, 2)}
    scale = grad(0, np.zeros_like(d))
    for i, (an, name) in enumerate(((hf, "fluxes"), (hj, "jones"))):
        fd = (vals[-2][i] - 8 * vals[-1][i] + 8 * vals[1][i] - vals[2][i]) / (12 * h)
        tol = 1.5 * BOUND[precision] * np.linalg.norm(scale[i]) / h
        print("jones gauss-newton stencil", precision, sky, beams, name, np.linalg.norm(fd - an), tol, np.linalg.norm(an))
        assert np.linalg.norm(an) > 0 and np.linalg.norm(fd - an) <= tol


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_identity_matrices_reproduce_the_call_without_them(gpu, monkeypatch, precision, sky, beams):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w = _directions(cfg), _weights(cfg)
    names = ("fluxes", "baselines", "topo")
    plain = _gn(cfg, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    unit = _jgn(cfg, **dirs, jones=_identity(cfg), weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    assert np.array_equal(unit[0], plain[0]) and np.array_equal(unit[2], plain[2])
    assert _same_flux(unit[1][0], plain[1][0]) and all(np.array_equal(a, b) for a, b in zip(unit[1][1:], plain[1][1:]))


@pytest.mark.parametrize("precision", [2, 1])
def test_diagonal_matrices_reproduce_the_gain_call(gpu, precision):
    """``jones[a] = diag(gains[a])``, ``d_jones[a] = diag(d_gains[a])`` is ``simulate_vis_gain_gauss_newton`` within BOUND:
    the rows, G, the flux product and the diagonal of the matrices' block."""
    cfg = _sid(source_config("cm", "full", "two", False, precision))
    dirs, w = _directions(cfg), _weights(cfg)
    rng = np.random.default_rng(3)
    nant, nf = len(cfg["ants"]), len(cfg["freqs"])

    def c(scale):
        return scale * (rng.normal(size=(nant, 2, nf)) + 1j * rng.normal(size=(nant, 2, nf)))

    g, dg = (1 + c(0.3)).astype(CDT[precision]), c(0.3).astype(CDT[precision])
    J, dJ = (np.zeros((nant, 2, 2, nf), dtype=g.dtype) for _ in range(2))
    J[:, 0, 0], J[:, 1, 1], dJ[:, 0, 0], dJ[:, 1, 1] = g[:, 0], g[:, 1], dg[:, 0], dg[:, 1]
    kw = dict(weights=w, quad_per="freq_time", return_gvis=True)
    qj, (fj, hj), Gj = _jgn(cfg, **dirs, jones=J, d_jones=dJ, wrt=("fluxes", "jones"), **kw)
    qg, (fg, hg), Gg = fftvis_amd.simulate_vis_gain_gauss_newton(**cfg, **dirs, gains=g, d_gains=dg, wrt=("fluxes", "gains"), **kw)
    assert np.all(np.abs(qj - qg) <= BOUND[precision] * qg) and rel_l2(Gj, Gg) <= BOUND[precision]
    assert rel_l2(fj, fg) <= BOUND[precision]
    assert rel_l2(np.stack([hj[:, 0, 0], hj[:, 1, 1]], axis=1), hg) <= BOUND[precision]
    assert np.abs(hj[:, 0, 1]).max() > 0


def test_a_jones_direction_alone_runs_no_tangent_pass(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _edge_cfg()
    w, J = _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    ran, forwards = [], []
    for name in dir(gs.SimHandle):
        if name.startswith("run_") and name.endswith("tangent"):
            monkeypatch.setattr(gs.SimHandle, name, lambda self, *a, _n=name, **k: ran.append(_n))
    real = gs.SimHandle.run_device
    monkeypatch.setattr(gs.SimHandle, "run_device", lambda self, *a, **k: forwards.append(a[:2]) or real(self, *a, **k))
    quad, prods = _jgn(cfg, jones=J, d_jones=dJ, weights=w)
    assert ran == [] and forwards == [(0, len(cfg["times"]))]  # one forward at the real fluxes, nothing else
    assert isinstance(prods, tuple) and len(prods) == 1 and prods[0].shape == J.shape and quad > 0
    monkeypatch.undo()
    rows, _, hj_ref, _, _, _ = _reference(cfg, {}, w, J, dJ)
    assert rel_l2(prods[0], hj_ref) <= BOUND[2] and abs(quad - rows.sum()) <= BOUND[2] * quad
    assert abs(jgr.inner_jones(dJ, prods[0]) - 2 * quad) <= BOUND[2] * 2 * quad


def test_time_handling(gpu, monkeypatch):
    """Constant matrices are per-time matrices repeated; one ``jones_weight_block`` per time block and neither
    ``weight_block`` nor ``gain_weight_block``."""
    from fftvis_amd.gpu import gpu_simulate

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg(ntimes=3)
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    rep, drep = np.repeat(J[..., None], 3, axis=-1), np.repeat(dJ[..., None], 3, axis=-1)
    names = ("fluxes", "jones")
    kw = dict(weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    one = _jgn(cfg, **dirs, jones=J, d_jones=dJ, **kw)
    per = _jgn(cfg, **dirs, jones=rep, d_jones=drep, **kw)
    assert np.array_equal(per[0], one[0]) and np.array_equal(per[2], one[2]) and per[1][1].shape == rep.shape
    assert np.abs(per[1][1].sum(axis=-1) - one[1][1]).max() <= 1e-14 * np.abs(one[1][1]).max()
    calls, others = [], []
    real = gpu_simulate.SimHandle.jones_weight_block
    monkeypatch.setattr(gpu_simulate.SimHandle, "jones_weight_block",
                        lambda self, *a, **k: calls.append((a[0], a[1], len(a[4]), a[5] is not None, tuple(a[7].shape)))
                        or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate.SimHandle, "weight_block", lambda self, *a, **k: others.append(a))
    monkeypatch.setattr(gpu_simulate.SimHandle, "gain_weight_block", lambda self, *a, **k: others.append(a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    blk = _jgn(cfg, **dirs, jones=rep, d_jones=drep, **kw)
    nant, nf = len(cfg["ants"]), len(cfg["freqs"])
    assert calls == [(t, t + 1, 2, True, (nf, 1, 2, 2, nant)) for t in range(3)] and others == [], (calls, others)
    assert np.all(np.abs(blk[0] - per[0]) <= 1e-12 * per[0]) and rel_l2(blk[2], per[2]) <= 1e-12
    assert rel_l2(blk[1][1], per[1][1]) <= 1e-12 and np.abs(blk[1][0] - per[1][0]).max() <= 1e-12 * np.abs(per[1][0]).max()


def test_time_blocks_are_sized_for_the_forward_block_and_the_terms(gpu, monkeypatch):
    """``_time_block`` sees the parts, half a block of weights, the rows' fp64 terms (half a block in fp64) and, only when V
    is held, one block more."""
    from fftvis_amd.gpu import gpu_simulate

    cfg = _edge_cfg()
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    nf = len(cfg["freqs"])
    seen = []
    real = gpu_simulate._time_block
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: seen.append(a[2]) or real(*a, **k))
    _jgn(cfg, **dirs, jones=J, weights=w, wrt=())                 # two parts, weights and the terms, fixed matrices: 3 blocks
    _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, wrt=())     # ... and V: 4
    _jgn(cfg, **dirs, jones=J, weights=w, wrt="jones")            # ... V for the matrices' block alone: 4
    _jgn(cfg, jones=J, d_jones=dJ, wrt=())                        # V and the terms
    assert seen == [3 * nf, 4 * nf, 4 * nf, int(np.ceil(1.5 * nf))], seen


@pytest.mark.parametrize("path,took", [("type3", 3), ("type2", 2)])
def test_lattice_forward_is_type1_for_the_fluxes_and_the_matrices(gpu, monkeypatch, path, took):
    """Jones matrices alone do not force the type-3 transform: the handle stays a lattice handle, which alone takes the
    type-2 adjoint."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = hex19_config()
    dirs, w, J = {"d_fluxes": _directions(cfg)["d_fluxes"]}, _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    quad, (gf, hj), G = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, wrt=("fluxes", "jones"), return_gvis=True,
                             adjoint_path=path)
    assert _handle().last_adjoint_path() == took
    rows, G_ref, hj_ref, _, _, _ = _reference(cfg, dirs, w, J, dJ)
    assert rel_l2(G, G_ref) <= BOUND[2] and rel_l2(hj, hj_ref) <= BOUND[2] and abs(quad - rows.sum()) <= BOUND[2] * quad
    no_flux = {k: v for k, v in cfg.items() if k != "fluxes"}
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **no_flux, adjoint_path=path))
    with pytest.raises(ValueError, match="adjoint_path='type2' needs the lattice path"):
        _jgn(cfg, **dirs, jones=J, d_jones=dJ, wrt=("fluxes", "ants"), adjoint_path="type2")


def test_device_tensors(gpu):
    import torch

    cfg = _edge_cfg()
    d, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    rng = np.random.default_rng(8)
    dirs = dict(d_fluxes=d["d_fluxes"], d_baselines=1e-2 * rng.normal(size=(len(cfg["baselines"]), 3)))
    names = ("fluxes", "ants", "jones")
    kw = dict(wrt=names, quad_per="freq_time", return_gvis=True)
    quad_ft, prods, G = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=w, **kw)
    D = {k: torch.from_numpy(v).cuda() for k, v in dirs.items()}
    W = torch.from_numpy(w).cuda()
    dq, dp, dG = _jgn(cfg, **D, jones=torch.from_numpy(J).cuda(), d_jones=torch.from_numpy(dJ).cuda(), weights=W, **kw)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dq, dG) + tuple(dp))
    assert dp[2].dtype == torch.complex128 and tuple(dp[2].shape) == J.shape
    assert np.all(np.abs(dq.cpu().numpy() - quad_ft) <= BOUND[2] * quad_ft) and rel_l2(dG.cpu().numpy(), G) <= BOUND[2]
    assert all(rel_l2(a.cpu().numpy(), b) <= BOUND[2] for a, b in zip(dp, prods))
    hq, hp, hG = _jgn(cfg, jones=J, d_jones=torch.from_numpy(dJ), weights=torch.from_numpy(w), **dict(kw, wrt="jones"))
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cpu" for x in (hq, hp, hG))


def test_staged_buffers_are_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the forward."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _jgn(cfg, **dirs, jones=J, d_jones=_d_jones(cfg, J), weights=w)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    # (the pairs and their incidence lists stay with the handle: 16 bytes per baseline)
    assert held.value - before < 16 * len(cfg["baselines"]) + 4096, (before, held.value)


def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu, monkeypatch):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg()
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    V = fftvis_amd.simulate_vis(**cfg)
    first = _jgn(cfg, **dirs, jones=J, d_jones=_d_jones(cfg, J), weights=w, quad_per="freq_time", return_gvis=True)
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), V)
    again = _jgn(cfg, **dirs, jones=J, d_jones=_d_jones(cfg, J), weights=w, quad_per="freq_time", return_gvis=True)
    # (the pairs are set again with the same values: nothing is rebuilt, and the bits are the first call's)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[2], first[2])
    assert np.array_equal(again[1][-1], first[1][-1])


def test_flagged_samples_and_a_bad_weight(gpu):
    cfg = _edge_cfg()
    dirs, w, J = _directions(cfg), _weights(cfg), _jones(cfg)
    dJ = _d_jones(cfg, J)
    flagged = np.random.default_rng(2).random(w.shape) < 0.3
    flagged[..., 3] = True  # one baseline with every sample flagged
    wf = w.copy()
    wf[flagged] = 0
    quad_ft, hj, G = _assert_value("flags", cfg, dirs, wf, J, dJ)
    # (the stored G of a flagged sample is not 0: the transposed product mixes the baseline's other samples into it)
    assert np.all(G[..., 3] == 0) and np.count_nonzero(G[..., :3]) == G[..., :3].size
    with pytest.raises(_lib.FftvisHipError, match="weights are negative or not finite"):
        _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=-w, wrt=())
    again = _jgn(cfg, **dirs, jones=J, d_jones=dJ, weights=wf, wrt=(), quad_per="freq_time")[0]  # the handle stays usable
    assert np.array_equal(again, quad_ft)


def test_the_handle_call_needs_the_pairs_and_a_polarized_handle(gpu):
    """``fv_sim_jones_weight_block`` on a handle a call without matrices configured, and on one that is not polarized."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _edge_cfg()
    nf, nt, nant = len(cfg["freqs"]), len(cfg["times"]), len(cfg["ants"])
    J = np.ones((nf, nt, 2, 2, nant), dtype=np.complex128)
    gs.release_handles()
    fftvis_amd.simulate_vis(**cfg)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run, without pairs
    try:
        part = torch.zeros(h.out_shape(nt, nf), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(_lib.FftvisHipError, match="fv_sim_jones_weight_block: fv_sim_set_gain_pairs first"):
            h.jones_weight_block(0, nt, 0, nf, [part], None, None, J)
        with pytest.raises(_lib.FftvisHipError, match="fv_sim_jones_weight_block: empty range"):
            h.jones_weight_block(1, 1, 0, nf, [part], None, None, J)
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
    unpol = _sid(source_config("cm", "unpol", "airy", False, 2))
    fftvis_amd.simulate_vis(**unpol)
    key, h = gs._acquire_handle(0, 2, unpol["eps"], 2, False)  # configured, and not polarized
    try:
        part = torch.zeros(h.out_shape(nt, nf), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(_lib.FftvisHipError, match="polarized"):
            h.jones_weight_block(0, nt, 0, nf, [part], None, None, J)
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
