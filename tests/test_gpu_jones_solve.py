"""GPU tests of the Jones solve on a resident model (``simulate_vis_jones_solve``, ``fv_jones_solve`` and its gather alone
through ``fv_jones_normal_rows``), section by section as ``test_gpu_gain_solve.py`` tests the diagonal solve.

The gather's bound is counted from its arithmetic, with u = 2^-53.  Everything is fp64 formed from the same T-typed inputs
on the device and in the numpy reference.  A complex product is within 3 u of the product of the moduli, a complex sum
within u.  Per used sample the kernel forms u_o[i], a sum of two complex products: 3 u + u = 4 u of its majorant
U_i = sum |Go| |X|.  A term of A01 is w u_0 conj(u_1): 4 u + 4 u carried, 3 u for the product, u for the weight: 12 u of
w U_0 U_1.  A term of A00 or A11 is w (re^2 + im^2): 8 u carried, 2 u, u: 11 u.  A term of b is w u_i t with an exact t:
4 u + 3 u + u = 8 u.  So a term is within 12 u of its majorant on the device, and as much in numpy, whose einsum forms
the same products in another order: 24 u = 12 * 2^-52 together; the two summation orders of n_a terms (n_a = 2 x the
antenna's incidences: two samples per incidence and column) add n_a u each.  With 4 * 2^-52 on top for the second-order
terms,
    |A - ref| <= (n_a + 16) 2^-52 A_abs,      |b - ref| <= (n_a + 16) 2^-52 b_abs,
``A_abs``, ``b_abs`` the reference's sums with every factor replaced by its modulus.  The loop is held to
``test_gpu_gains``' BOUND against the numpy reference on the same rounded inputs: all of its arithmetic is fp64 whatever
the run's precision, and the test asserts that the reference's systems are far from the rank rule's threshold
(det >= 0.1 A00 A11, so that the closed-form solve amplifies errors by at most 10).  The reported chi2 is held to
``(L + 4) 2^-52`` relative, L = 4 nbls, where the data are unrelated to the model; at a fitted minimum the bound carries
the cancellation in ``V' - d`` (``_chi2_bound``)."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import basis_source_refs as bsr
from tests import jones_refs
from tests import jones_solve_refs as jsr
from tests.gain_solve_refs import used_weights
from tests.helpers import rel_l2
from tests.source_adjoint_refs import source_config
from tests.test_gpu_gains import BOUND, CDT, NANT, RDT, _ant_rows, _pairs
from tests.test_gpu_jones import _blocked, _kernel_inputs, _matrices
from tests.test_gpu_source_adjoint import _sid
from tests.test_jones_solve_host import jones_case, per_row

pytestmark = pytest.mark.gpu


def _start(shape, seed):
    """Identity plus 0.3 N(0, 1) complex in every entry, complex128."""
    return _matrices(shape, np.random.default_rng(seed), np.complex128)


def _incidences(a1, a2, nant):
    return 2 * (np.bincount(a1, minlength=nant) + np.bincount(a2, minlength=nant))


def _no_autos(V, w, a1, a2):
    """``w`` (None: ones) as an array of ``V``'s real dtype with the auto-correlations' weights zeroed."""
    w0 = np.ones(V.shape, dtype=V.real.dtype) if w is None else w.copy()
    w0.reshape(V.shape[0], 4, -1)[:, :, a1 == a2] = 0
    return w0


# ---- 1. the gather alone -------------------------------------------------------------------------------------------------
def _normal(V, d, w, J, a1, a2, precision):
    nrows, nant = V.shape[0], J.shape[-1]
    A, b = np.full((nrows, 4, 2, nant), 7.0), np.full((nrows, 2, 2, nant), 7.0, dtype=np.complex128)
    status = _lib.lib().fv_jones_normal_rows(0, precision, nrows, len(a1), nant, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(J),
                                             _lib.ptr(V), _lib.ptr(d), _lib.ptr(w), _lib.ptr(A), _lib.ptr(b))
    return status, A, b


def _check_normal(label, V, d, w, J, a1, a2, precision):
    status, A, b = _normal(V, d, w, J, a1, a2, precision)
    assert status == 0, _lib.lib().fv_last_error()
    nant = J.shape[-1]
    w64 = None if w is None else _blocked(w.astype(np.float64))
    A_ref, b_ref, A_abs, b_abs = jsr.normal_sums(_blocked(V), _blocked(d), w64, J, a1, a2, with_abs=True)
    n_a = _incidences(a1, a2, nant)
    bound = (n_a + 16) * 2.0**-52
    print("jones normal systems", label, float((np.abs(A - A_ref) / np.maximum(bound * A_abs, 1e-300)).max()),
          float((np.abs(b - b_ref) / np.maximum(bound * b_abs, 1e-300)).max()), int(n_a.max()))
    assert np.all(np.abs(A - A_ref) <= bound * A_abs) and np.all(np.abs(b - b_ref) <= bound * b_abs)
    crossed = np.zeros(nant, bool)
    crossed[a1[a1 != a2]] = crossed[a2[a1 != a2]] = True
    assert np.all(A[..., ~crossed] == 0) and np.all(b[..., ~crossed] == 0) and not crossed.all()
    if w is None:
        assert np.all(A[:, :2][..., crossed] > 0)
    assert np.isfinite(A).all() and np.isfinite(b).all()
    status, A2, b2 = _normal(V, d, w, J, a1, a2, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(A2, A) and np.array_equal(b2, b)
    return A, b, A_abs, b_abs, n_a


@pytest.mark.parametrize("weights", ["none", "positive", "flags", "baselines"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_normal_systems(gpu, nbls, nrows, precision, weights):
    V, d, w, J32, a1, a2 = _kernel_inputs(nrows, nbls, precision, weights)
    # complex128 whatever the run's precision, of values that the objective's kernels can take in theirs
    J = _start(J32.shape, nbls + 4).astype(CDT[precision]).astype(np.complex128)
    A, b, A_abs, b_abs, n_a = _check_normal(f"{nbls} {nrows} {precision} {weights}", V, d, w, J, a1, a2, precision)
    crossed = set(a1[a1 != a2]) | set(a2[a1 != a2])
    assert NANT - 2 not in crossed and NANT - 1 not in crossed  # an antenna in autos only (nbls > 1), one in no baseline
    if nbls > 8:
        assert (a1 == a2).sum() > 1 and n_a[NANT - 2] > 0
    if nbls >= 257:
        assert n_a[0] > 2 * 64  # more than one entry per lane
    if weights in ("flags", "baselines"):
        assert not np.isfinite(d).all()
    # 2 (A Gamma - b) is fv_jones_residual_chi2's gjones with the autos' weights zeroed, within the sum of the two kernels'
    # bounds: this module's carried through the 2 x 2 product (A01's two parts are bounded one by one: sqrt 2 for its
    # modulus) and test_gpu_jones' (n_a + 40) 2^-52 of its majorant.  The product itself is formed in extended precision.
    w0 = _no_autos(V, w, a1, a2)
    gj, G, chi2 = np.full(J.shape, 7.0, dtype=np.complex128), V.copy(), np.zeros(nrows)
    J_t = J.astype(CDT[precision])
    assert _lib.lib().fv_jones_residual_chi2(0, precision, nrows, nbls, NANT, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(J_t), _lib.ptr(G),
                                             _lib.ptr(d), _lib.ptr(w0), _lib.ptr(chi2), _lib.ptr(gj)) == 0
    gj_abs = jones_refs.chi2_jones(_blocked(V), _blocked(d), _blocked(w0.astype(np.float64)), J, a1, a2, with_abs=True)[4]
    wide = jsr.gradient(A.astype(np.longdouble), b.astype(np.clongdouble), J.astype(np.clongdouble))
    Ja, r2 = np.abs(J), np.sqrt(2.0)
    carried = np.stack([A_abs[:, 0] * Ja[:, 0] + r2 * A_abs[:, 2] * Ja[:, 1] + b_abs[:, 0],
                        r2 * A_abs[:, 2] * Ja[:, 0] + A_abs[:, 1] * Ja[:, 1] + b_abs[:, 1]], axis=1)
    bound = 2 * (n_a + 16) * 2.0**-52 * carried + (n_a + 40) * 2.0**-52 * gj_abs
    err = np.abs((wide - gj).astype(np.complex128))
    print("jones normal systems against gjones", nbls, nrows, precision, weights, float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


# ---- 2. three iterations, fixed ------------------------------------------------------------------------------------------
def _solve(V, d, w, J0, a1, a2, precision, per_time, max_iter, tol, on_device=False):
    """``fv_jones_solve`` on (nfreqs, ntimes, 4 nbls) blocks: (status, matrices, niter, change, chi2, solved)."""
    nf, nt = V.shape[:2]
    J = np.ascontiguousarray(J0, dtype=np.complex128).copy()
    niter = np.full(1, -1, dtype=np.int32)
    change, chi2 = np.full(J.shape[:2], -1.0), np.full((nf, nt), -1.0)
    solved = np.full(J.shape[:2] + (2, J.shape[-1]), 7, dtype=np.int32)
    bufs = [np.ascontiguousarray(V), np.ascontiguousarray(d), None if w is None else np.ascontiguousarray(w)]
    if on_device:
        import torch

        bufs = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
        ptrs = [None if b is None else ctypes.c_void_p(b.data_ptr()) for b in bufs]
    else:
        ptrs = [_lib.ptr(b) for b in bufs]
    flag = int(on_device)
    status = _lib.lib().fv_jones_solve(0, precision, nf, nt, len(a1), J.shape[-1], _lib.ptr(a1), _lib.ptr(a2), int(per_time),
                                       ptrs[0], flag, ptrs[1], flag, ptrs[2], flag, _lib.ptr(J), max_iter, tol, _lib.ptr(niter),
                                       _lib.ptr(change), _lib.ptr(chi2), _lib.ptr(solved))
    return status, J, int(niter[0]), change, chi2, solved != 0


def _as_block(x, nf, nt):
    return x.reshape(nf, nt, 2, 2, -1)


def _det_ratio(A, which=None):
    """det / (A00 A11) of every non-empty column of the packed systems, or of those that the mask ``which`` selects."""
    a00, a11 = A[..., 0, :, :], A[..., 1, :, :]
    full = (a00 > 0) | (a11 > 0)
    return ((a00 * a11 - A[..., 2, :, :] ** 2 - A[..., 3, :, :] ** 2) / np.where(full, a00 * a11, 1.0))[full if which is None else full & which]


def _three_iterations(label, nant, nbls, precision, per_time, nf=2, nt=3, floor=0.1):
    """``floor``: what det / (A00 A11) of every solved column of the reference must reach at all three iterations, so that
    the closed-form solve amplifies errors by at most 1 / floor; a non-empty column that is not solved must be rank one to
    rounding, (n + 32) 2^-52 < 2^-40.  Either way no column is anywhere near the rule's threshold of 2^-30."""
    V, d, w, J32, a1, a2 = _kernel_inputs(nf * nt, nbls, precision, "flags", nant=nant)
    J0 = _start((nf, nt if per_time else 1, 2, 2, nant), nbls)
    rows = [x.reshape(nf, nt, -1) for x in (V, d, w)]
    status, J, niter, change, chi2, solved = _solve(*rows, J0, a1, a2, precision, per_time, 3, 0.0)
    assert status == 0, _lib.lib().fv_last_error()
    Vb, db, wb = (_as_block(x, nf, nt) for x in (V, d, w.astype(np.float64)))
    ratios, noise = [], []
    for n in (1, 2, 3):
        _, _, _, ok, (A, _) = jsr.solve(Vb, db, wb, J0, a1, a2, per_time, n, 0.0)
        ratios.append(float(_det_ratio(A, ok).min()))
        noise.append(float(np.abs(_det_ratio(A, ~ok)).max(initial=0.0)))
    J_ref, changes, _, solved_ref, _ = jsr.solve(Vb, db, wb, J0, a1, a2, per_time, 3, 0.0)
    print("jones solve, three iterations", label, rel_l2(J, J_ref), float(np.abs(change - changes[-1]).max()), ratios, noise)
    assert min(ratios) >= floor and max(noise) <= 2.0**-40
    assert niter == 3 and len(changes) == 3
    assert J.shape == J0.shape and rel_l2(J, J_ref) <= BOUND[precision]
    assert np.all(np.abs(change - changes[-1]) <= BOUND[precision] * np.maximum(changes[-1], 1.0))
    assert np.array_equal(solved, solved_ref) and solved.any() and not solved.all()
    keep = ~np.broadcast_to(solved[:, :, None], J.shape)
    assert np.array_equal(J[keep], J0[keep])  # (an unsolved column keeps its start bits)
    chi2_ref = jsr.chi2_rows(Vb, db, wb, per_row(J, nt) if not per_time else J, a1, a2)  # at the returned matrices
    L = 4 * nbls
    print("jones solve, chi2", label, float((np.abs(chi2 - chi2_ref) / chi2_ref).max() / 2.0**-52), L + 4)
    assert chi2.shape == (nf, nt) and np.all(np.abs(chi2 - chi2_ref) <= (L + 4) * 2.0**-52 * chi2_ref)
    return rows, J0, a1, a2, (J, niter, change, chi2, solved)


@pytest.mark.parametrize("per_time", [False, True])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nbls", [65, 257])
def test_three_iterations(gpu, nbls, precision, per_time):
    rows, J0, a1, a2, first = _three_iterations(f"{nbls} {precision} {per_time}", NANT, nbls, precision, per_time)
    assert not first[4][..., NANT - 2:].any() and first[4][..., :NANT - 2].all()  # (every non-empty column is solved)
    again = _solve(*rows, J0, a1, a2, precision, per_time, 3, 0.0)  # the same input gives the same bits
    resident = _solve(*rows, J0, a1, a2, precision, per_time, 3, 0.0, on_device=True)  # ... host or device blocks
    for other in (again, resident):
        assert other[0] == 0 and other[2] == 3
        assert all(np.array_equal(x, y) for x, y in zip(other[1:], first))


# ---- 3. the rank rule on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
def test_a_column_with_one_used_sample_is_not_solved(gpu, precision):
    """Antenna NANT - 1's only baseline is (0, NANT - 1): it is a2 there, its measured feed is x, and of column x = 1 the
    sample (x, y) = (1, 0) is flagged: that column has one used sample per unit and rank one, column 0 has two."""
    nbls, nf, nt = 65, 1, 2
    rng = np.random.default_rng(5)
    a1, a2 = _pairs(nbls, rng)
    k = 5
    a1[k], a2[k] = 0, NANT - 1
    V, d, w, _, a1, a2 = _kernel_inputs(nf * nt, nbls, precision, "positive", pairs=(a1, a2))
    wb = w.reshape(nf * nt, 2, 2, nbls)
    wb[:, :, :, k] = 1
    wb[:, 1, 0, k] = 0
    J0 = _start((nf, nt, 2, 2, NANT), 6)
    rows = [x.reshape(nf, nt, -1) for x in (V, d, w)]
    status, J, niter, change, chi2, solved = _solve(*rows, J0, a1, a2, precision, True, 3, 0.0)
    assert status == 0 and niter == 3, _lib.lib().fv_last_error()
    Vb, db, wb = (_as_block(x, nf, nt) for x in (V, d, w.astype(np.float64)))
    J_ref, _, _, solved_ref, (A, _) = jsr.solve(Vb, db, wb, J0, a1, a2, True, 3, 0.0)
    assert np.all(A[..., 0, 1, NANT - 1] > 0) and np.all(A[..., 1, 1, NANT - 1] > 0)
    assert np.array_equal(solved, solved_ref) and solved[..., 0, NANT - 1].all() and not solved[..., 1, NANT - 1].any()
    assert np.array_equal(J[..., :, 1, NANT - 1], J0[..., :, 1, NANT - 1])
    assert not np.array_equal(J[..., :, 0, NANT - 1], J0[..., :, 0, NANT - 1]) and rel_l2(J, J_ref) <= BOUND[precision]


# ---- 4. matrices beyond the LDS budget -----------------------------------------------------------------------------------
def test_matrices_beyond_the_lds_budget(gpu):
    """600 antennas: 38.4 KB of complex128 matrices per unit, read from global memory instead of LDS.  Most antennas have
    one baseline here, so some columns have a single used sample and are not solved, and a solved column may rest on two
    samples: det >= 1e-3 A00 A11 is asked of those, which keeps the gather's error, some 1e-15, a factor 10 under BOUND."""
    nant, nbls = 600, 257
    assert 64 * nant > 32768
    V, d, w, J32, a1, a2 = _kernel_inputs(6, nbls, 2, "flags", nant=nant)
    _check_normal("600 antennas", V, d, w, _start(J32.shape, 3), a1, a2, 2)
    _three_iterations("600 antennas", nant, nbls, 2, False, floor=1e-3)


# ---- 5. recovery ---------------------------------------------------------------------------------------------------------
def _rounded_case(noise, leakage, precision, seed=0):
    """``jones_case`` with inputs of the run's precision: the data are formed from the rounded model."""
    V, _, w, J, a1, a2 = jones_case(0.0, leakage, seed)
    rng = np.random.default_rng(seed + 50)
    V = V.astype(CDT[precision])
    d = jones_refs.apply_jones(V, per_row(J, V.shape[1]), a1, a2)
    d = (d + noise * (rng.normal(size=d.shape) + 1j * rng.normal(size=d.shape)) / np.sqrt(2)).astype(CDT[precision])
    return V, d, w.astype(RDT[precision]), J, a1, a2


def _flat(x):
    return np.ascontiguousarray(x.reshape(x.shape[:2] + (-1,)))


def _chi2_bound(V, w, J, a1, a2, chi2):
    """The relative bound of a reported chi2 against the numpy reference, per (f, t).  Both form V' in fp64 from the same
    inputs, a sum of four products of three factors: within 9 u S of its value on either side, S = sum |G1| |G2| |V| (the
    figure of ``test_gpu_jones``), the subtraction adds u |delta|.  A term w |delta|^2 is then off by at most
    2 w |delta| (9 u S + u |delta|) on either side; over both sides and by Cauchy-Schwarz the row is off by
    36 u sqrt(sum w S^2 / chi2) + 4 u relative, and the two summation orders add ``(L + 4) 2^-52``."""
    wu = used_weights(V, w, a1, a2)
    S = jones_refs.apply_jones(np.abs(V), np.abs(J), a1, a2).real
    power = (wu * S**2).reshape(chi2.shape + (-1,)).sum(axis=-1)
    L = int(np.prod(V.shape[2:]))
    return (L + 6) * 2.0**-52 + 36 * 2.0**-53 * np.sqrt(power / chi2)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("leakage", [0.05, 0.3])
def test_recovery(gpu, leakage, precision):
    V, d, w, J_true, a1, a2 = _rounded_case(0.0, leakage, precision)
    nt = V.shape[1]
    J0 = jones_refs.diagonal(np.ones((2, 1, 2, 8), complex))
    status, J, niter, change, chi2, solved = _solve(_flat(V), _flat(d), _flat(w), J0, a1, a2, precision, False, 200, 1e-10)
    assert status == 0, _lib.lib().fv_last_error()
    _, changes, _, _, _ = jsr.solve(V, d, w, J0, a1, a2, False, 200, 1e-10)
    used = used_weights(V, w, a1, a2) > 0
    worst = float(np.abs(jones_refs.apply_jones(V, per_row(J, nt), a1, a2) - d)[used].max())
    print("jones solve recovery", leakage, precision, niter, len(changes), float(change.max()), worst)
    assert niter < 200 and np.all(change < 1e-10) and solved.all() and abs(niter - len(changes)) <= 2
    assert worst <= (1e-8 if precision == 2 else BOUND[1])
    # noisy data: chi2 falls, and is the reference's at the returned matrices
    V, d, w, _, a1, a2 = _rounded_case(0.05, leakage, precision, seed=1)
    status, J, niter, change, chi2, solved = _solve(_flat(V), _flat(d), _flat(w), J0, a1, a2, precision, False, 200, 1e-10)
    assert status == 0 and niter < 200
    start = jsr.chi2_rows(V, d, w, per_row(J0, nt), a1, a2)
    ref = jsr.chi2_rows(V, d, w, per_row(J, nt), a1, a2)
    bound = _chi2_bound(V, w, per_row(J, nt), a1, a2, ref)
    print("jones solve noisy", leakage, precision, niter, start.sum(), chi2.sum(), float((np.abs(chi2 - ref) / ref / bound).max()))
    assert chi2.sum() < 0.1 * start.sum() and np.all(np.abs(chi2 - ref) <= bound * ref)


# ---- 6. bad input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what,message", [("negative weight", b"1 weights are negative or not finite"),
                                          ("nan datum", b"1 entries of data are not finite where the weight is positive"),
                                          ("inf model", b"1 values of the model are not finite")])
def test_bad_input_fails_the_call_and_the_next_good_call_succeeds(gpu, what, message, precision):
    V, d, w, J, a1, a2 = _rounded_case(0.05, 0.05, precision)
    V, d, w = _flat(V), _flat(d), _flat(w)
    J0 = jones_refs.diagonal(np.ones((2, 1, 2, 8), complex))
    good = _solve(V, d, w, J0, a1, a2, precision, False, 4, 0.0)
    assert good[0] == 0
    cross = int(np.flatnonzero(a1 != a2)[0]) + 2 * len(a1)  # plane 2 of a cross-correlation
    auto = int(np.flatnonzero(a1 == a2)[1])
    bV, bd, bw = V.copy(), d.copy(), w.copy()
    if what == "negative weight":
        bw[1, 0, auto] = -1.0  # (an auto-correlation's weight is checked like any other)
    elif what == "nan datum":
        bd[1, 1, cross] = complex(1.0, np.nan)
    else:
        bV[0, 0, cross] = complex(np.inf, 0.0)
    status, J_bad = _solve(bV, bd, bw, J0, a1, a2, precision, False, 4, 0.0)[:2]
    assert status == 1 and message in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    assert np.array_equal(J_bad, J0)  # (the start is untouched)
    again = _solve(V, d, w, J0, a1, a2, precision, False, 4, 0.0)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))
    if what == "nan datum":  # under a zero weight, or on an auto-correlation, the same datum is not an error
        bw[1, 1, cross] = 0
        bd[0, 0, auto] = complex(np.nan, np.inf)
        status, J_ok, _, _, chi2, _ = _solve(V, bd, bw, J0, a1, a2, precision, False, 4, 0.0)
        assert status == 0 and np.isfinite(J_ok).all() and np.isfinite(chi2).all()


# ---- 7. the public function ----------------------------------------------------------------------------------------------
def _solve_public(cfg, data, **kw):
    return fftvis_amd.simulate_vis_jones_solve(data, **cfg, **kw)


def _true_matrices(cfg, seed=11, leakage=0.1):
    rng = np.random.default_rng(seed)
    shape = (len(cfg["ants"]), 2, 2, len(cfg["freqs"]))
    J = leakage * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    for f in range(2):
        J[:, f, f] = 1 + 0.3 * (rng.normal(size=shape[:1] + shape[3:]) + 1j * rng.normal(size=shape[:1] + shape[3:]))
    return J


def _block(cfg, J):
    """The matrices as the references take them: (nf, nt, 2, 2, nant)."""
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    return np.ascontiguousarray(np.broadcast_to(J.reshape(nant, 2, 2, nf, -1), (nant, 2, 2, nf, nt)).transpose(3, 4, 1, 2, 0))


def _noisy(cfg, V, precision, seed):
    rng = np.random.default_rng(seed)
    a1, a2 = _ant_rows(cfg)
    d = jones_refs.apply_jones(V, _block(cfg, _true_matrices(cfg)), a1, a2)
    noise = 0.05 * np.abs(V).mean() * (rng.normal(size=V.shape) + 1j * rng.normal(size=V.shape))
    w = rng.uniform(0.5, 2.0, size=V.shape).astype(RDT[precision])
    w[0, 0, 1, 0, 3] = 0
    return (d + noise).astype(CDT[precision]), w


@pytest.mark.parametrize("precision", [2, 1])
def test_public_function_and_the_resident_model(gpu, monkeypatch, precision):
    import torch

    from fftvis_amd.gpu import gpu_simulate

    cfg = _sid(source_config("cm", "full", "complex", False, precision))
    a1, a2 = _ant_rows(cfg)
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    V = fftvis_amd.simulate_vis(**cfg)
    d, w = _noisy(cfg, V, precision, 4)
    J, info, model = _solve_public(cfg, d, weights=w, max_iter=6, tol=0.0, return_model=True)
    assert J.shape == (nant, 2, 2, nf) and J.dtype == np.complex128 and info["solved"].shape == J.shape
    assert info["solved"].dtype == bool and np.array_equal(info["solved"][:, 0], info["solved"][:, 1])
    assert info["niter"] == 6 and not info["converged"] and info["chi2"].shape == (nf, nt) and info["change"].shape == (nf,)
    assert isinstance(model, torch.Tensor) and model.device.type == "cuda" and tuple(model.shape) == V.shape
    assert rel_l2(model.cpu().numpy(), V) <= BOUND[precision] / 10  # (two runs of one forward)
    M = model.cpu().numpy()
    eye = jones_refs.diagonal(np.ones((nf, 1, 2, nant), complex))
    ref, _, chi2_ref, solved_ref, (A, _) = jsr.solve(M, d, w, eye, a1, a2, False, 6, 0.0)
    print("jones solve public", precision, rel_l2(_block(cfg, J)[:, :1], ref), float(_det_ratio(A).min()))
    assert _det_ratio(A).min() >= 0.1 and rel_l2(_block(cfg, J)[:, :1], ref) <= BOUND[precision]
    assert np.all(np.abs(info["chi2"] - chi2_ref) <= BOUND[precision] * chi2_ref) and solved_ref.all() and info["solved"].all()

    # the resident model serves the next call: no forward, fluxes not needed, the same bits
    def forward(*a, **k):
        raise AssertionError("the forward ran")

    with monkeypatch.context() as mp:
        mp.setattr(gpu_simulate.SimHandle, "run_device", forward)
        mp.setattr(gpu_simulate.SimHandle, "run", forward)
        J2, info2 = _solve_public(dict(cfg, fluxes=None), d, weights=w, model=model, max_iter=6, tol=0.0)
        J3, _ = _solve_public(dict(cfg, fluxes=None), d, weights=w, model=M, max_iter=6, tol=0.0)  # uploaded once
    assert np.array_equal(J2, J) and np.array_equal(J3, J) and np.array_equal(info2["chi2"], info["chi2"])
    # resident data and weights, per-time matrices: the bits of the host-array call, on the device
    host = _solve_public(cfg, d, weights=w, model=model, max_iter=4, tol=0.0, per_time=True)
    D, W = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()
    dev = _solve_public(cfg, D, weights=W, model=model, max_iter=4, tol=0.0, per_time=True)
    assert host[0].shape == J.shape + (nt,) and host[1]["niter"] == 4 and host[1]["change"].shape == (nf, nt)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dev[0], dev[1]["chi2"], dev[1]["solved"], dev[1]["change"]))
    assert np.array_equal(dev[0].cpu().numpy(), host[0]) and np.array_equal(dev[1]["chi2"].cpu().numpy(), host[1]["chi2"])
    assert dev[1]["solved"].dtype == torch.bool and np.array_equal(dev[1]["solved"].cpu().numpy(), host[1]["solved"])
    ref_t = jsr.solve(M, d, w, jones_refs.diagonal(np.ones((nf, nt, 2, nant), complex)), a1, a2, True, 4, 0.0)[0]
    assert rel_l2(_block(cfg, host[0]), ref_t) <= BOUND[precision]
    # per-time start matrices keep their shape; time-constant ones with per_time=True are refused
    start = np.repeat(_true_matrices(cfg)[..., None], nt, axis=-1)
    kept = _solve_public(cfg, d, weights=w, model=model, jones=start, max_iter=2, tol=0.0)
    assert kept[0].shape == start.shape and kept[1]["solved"].shape == start.shape and kept[1]["change"].shape == (nf, nt)
    with pytest.raises(ValueError, match="per_time=True needs per-time jones"):
        _solve_public(cfg, d, model=model, jones=_true_matrices(cfg), per_time=True)
    # the reference antenna: chi2 unchanged, jones[ref][0, 0] real and positive, V' the same up to rounding
    nums = list(cfg["ants"])
    plain = _solve_public(cfg, d, weights=w, model=model, jones=_true_matrices(cfg), max_iter=4, tol=0.0)
    fixed = _solve_public(cfg, d, weights=w, model=model, jones=_true_matrices(cfg), max_iter=4, tol=0.0, ref_ant=nums[2])
    assert np.array_equal(fixed[1]["chi2"], plain[1]["chi2"]) and not np.array_equal(fixed[0], plain[0])
    assert np.all(fixed[0][2, 0, 0].real > 0) and np.all(np.abs(fixed[0][2, 0, 0].imag) <= 1e-15 * np.abs(fixed[0][2, 0, 0]))
    p_fixed, p_plain = (jones_refs.apply_jones(M, _block(cfg, x[0]), a1, a2) for x in (fixed, plain))
    S = jones_refs.apply_jones(np.abs(M), np.abs(_block(cfg, plain[0])), a1, a2).real
    assert np.all(np.abs(p_fixed - p_plain) <= 32 * 2.0**-52 * S)  # (a unit-modulus factor per matrix, four products deep)
    # info["chi2"] is simulate_vis_jones_chi2's at the returned matrices, with the autos' weights zeroed
    w0 = w.copy()
    w0[..., a1 == a2] = 0
    chi2, _ = fftvis_amd.simulate_vis_jones_chi2(d, **cfg, jones=J, weights=w0, wrt="jones", chi2_per="freq_time")
    print("jones solve public chi2", precision, float((np.abs(info["chi2"] - chi2) / chi2).max()))
    assert np.all(np.abs(info["chi2"] - chi2) <= BOUND[precision] * chi2)
    # bad weights fail the call, and the next good call succeeds
    bw = w.copy()
    bw[1, 1, 0, 0, 5] = -1.0
    with pytest.raises(_lib.FftvisHipError, match="1 weights are negative or not finite"):
        _solve_public(cfg, d, weights=bw, model=model, max_iter=6, tol=0.0)
    again = _solve_public(cfg, d, weights=w, model=model, max_iter=6, tol=0.0)
    assert np.array_equal(again[0], J)


@pytest.mark.parametrize("precision", [2, 1])
def test_basis_beams(gpu, precision):
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    a1, a2 = _ant_rows(cfg)
    nant, nf, nt = len(cfg["ants"]), len(cfg["freqs"]), len(cfg["times"])
    V = fftvis_amd.simulate_vis(**cfg)
    d, w = _noisy(cfg, V, precision, 9)
    J, info = _solve_public(cfg, d, weights=w, max_iter=5, tol=0.0, per_time=True)
    J0 = jones_refs.diagonal(np.ones((nf, nt, 2, nant), complex))
    ref, _, chi2_ref, _, (A, _) = jsr.solve(V, d, w, J0, a1, a2, True, 5, 0.0)
    print("jones solve basis beams", precision, rel_l2(_block(cfg, J), ref), float(_det_ratio(A).min()))
    assert _det_ratio(A).min() >= 0.1 and rel_l2(_block(cfg, J), ref) <= BOUND[precision]
    assert np.all(np.abs(info["chi2"] - chi2_ref) <= BOUND[precision] * chi2_ref) and info["niter"] == 5
