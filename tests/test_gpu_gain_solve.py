"""GPU tests of the gain solve on a resident model (``simulate_vis_gain_solve``, ``fv_gain_solve`` and its gather alone
through ``fv_gain_normal_rows``).

The gather is held to the bound of the gain gradient's test (``test_gpu_gains``): per antenna it adds n_a signed fp64 terms
(n_a = nfeed times the antenna's incidences), each a product of three complex factors and the weight formed in fp64 -- at most
16 * 2^-52 per term on the device and as much in the numpy reference, no subtraction anywhere -- and the two summation
orders differ by n_a u each:  |num - ref| <= (n_a + 32) 2^-52 sum |terms|,  and the same for den, whose terms are their own
moduli.  The loop is held to ``test_gpu_objective``'s BOUND against the numpy reference run on the same rounded inputs: all
of its arithmetic is fp64 whatever the run's precision.  The reported chi2 is held to ``(L + 4) 2^-52`` relative,
``L = tpol nbls``, as ``fv_residual_chi2``'s rows are, where the data are unrelated to the model; at a fitted minimum
``delta = V' - d`` is a small difference of large numbers and the bound says so (``_chi2_bound``)."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import basis_source_refs as bsr
from tests import gain_refs
from tests import gain_solve_refs as gsr
from tests.helpers import rel_l2
from tests.source_adjoint_refs import source_config
from tests.tangent_refs import hex19_config
from tests.test_gain_solve_host import solve_case
from tests.test_gpu_gains import BOUND, CDT, NANT, RDT, _ant_rows, _block_layout, _blocked, _gains, _kernel_inputs
from tests.test_gpu_source_adjoint import _sid

pytestmark = pytest.mark.gpu


def _start(shape, seed):
    rng = np.random.default_rng(seed)
    return 1 + 0.3 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))


def _incidences(a1, a2, nant, nfeed):
    return nfeed * (np.bincount(a1, minlength=nant) + np.bincount(a2, minlength=nant))


# ---- 1. the gather alone -------------------------------------------------------------------------------------------------
def _normal(V, d, w, g, a1, a2, tpol, precision):
    num, den = np.full(g.shape, 7.0, dtype=np.complex128), np.full(g.shape, 7.0)
    status = _lib.lib().fv_gain_normal_rows(0, precision, V.shape[0], len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                            _lib.ptr(g), _lib.ptr(V), _lib.ptr(d), _lib.ptr(w), _lib.ptr(num), _lib.ptr(den))
    return status, num, den


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_normal_sums(gpu, nbls, tpol, nrows, precision, weights):
    V, d, w, g32, a1, a2 = _kernel_inputs(nrows, nbls, tpol, precision, weights)
    g = _start(g32.shape, nbls + tpol)  # complex128 whatever the run's precision
    status, num, den = _normal(V, d, w, g, a1, a2, tpol, precision)
    assert status == 0, _lib.lib().fv_last_error()
    w64 = None if w is None else _blocked(w.astype(np.float64), tpol)
    num_ref, den_ref, num_abs = gsr.normal_sums(_blocked(V, tpol), _blocked(d, tpol), w64, g, a1, a2, with_abs=True)
    n_a = _incidences(a1, a2, NANT, g.shape[1])
    bound = (n_a + 32) * 2.0**-52
    print("gain normal sums", nbls, tpol, nrows, precision, weights,
          float((np.abs(num - num_ref) / np.maximum(bound * num_abs, 1e-300)).max()),
          float((np.abs(den - den_ref) / np.maximum(bound * den_ref, 1e-300)).max()), int(n_a.max()))
    assert np.all(np.abs(num - num_ref) <= bound * num_abs) and np.all(np.abs(den - den_ref) <= bound * den_ref)
    crossed = np.zeros(NANT, bool)
    crossed[a1[a1 != a2]] = crossed[a2[a1 != a2]] = True
    assert not crossed[NANT - 2] and not crossed[NANT - 1]  # an antenna in autos only (nbls > 1), one in no baseline
    assert np.all(num[..., ~crossed] == 0) and np.all(den[..., ~crossed] == 0)
    if w is None:
        assert np.all(den[..., crossed] > 0)
    if nbls > 8:
        assert (a1 == a2).sum() > 1 and n_a[NANT - 2] > 0
    if nbls >= 257:
        assert n_a[0] > 64 * g.shape[1]
    if weights == "flags":
        assert not np.isfinite(d).all() and np.isfinite(num).all()
    status, num2, den2 = _normal(V, d, w, g, a1, a2, tpol, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(num2, num) and np.array_equal(den2, den)


# ---- 2. three iterations, fixed ------------------------------------------------------------------------------------------
def _solve(V, d, w, g0, a1, a2, tpol, precision, per_time, max_iter, tol, on_device=False):
    """``fv_gain_solve`` on (nfreqs, ntimes, tpol nbls) blocks: (status, gains, niter, change, chi2, solved)."""
    nf, nt = V.shape[:2]
    g = np.ascontiguousarray(g0, dtype=np.complex128).copy()
    niter = np.full(1, -1, dtype=np.int32)
    change, chi2, solved = np.full(g.shape[:2], -1.0), np.full((nf, nt), -1.0), np.full(g.shape, 7, dtype=np.int32)
    bufs = [np.ascontiguousarray(V), np.ascontiguousarray(d), None if w is None else np.ascontiguousarray(w)]
    if on_device:
        import torch

        bufs = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
        ptrs = [None if b is None else ctypes.c_void_p(b.data_ptr()) for b in bufs]
    else:
        ptrs = [_lib.ptr(b) for b in bufs]
    flag = int(on_device)
    status = _lib.lib().fv_gain_solve(0, precision, nf, nt, len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2), int(per_time),
                                      ptrs[0], flag, ptrs[1], flag, ptrs[2], flag, _lib.ptr(g), max_iter, tol, _lib.ptr(niter),
                                      _lib.ptr(change), _lib.ptr(chi2), _lib.ptr(solved))
    return status, g, int(niter[0]), change, chi2, solved != 0


def _as_block(x, nf, nt, tpol):
    """(nf nt, tpol nbls) rows as the references take them: (nf, nt, [2, 2,] nbls)."""
    return x.reshape((nf, nt, 2, 2, -1) if tpol == 4 else (nf, nt, -1))


def _per_row(g, nt):
    return np.broadcast_to(g, (g.shape[0], nt) + g.shape[2:])


@pytest.mark.parametrize("per_time", [False, True])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [65, 257])
def test_three_iterations(gpu, nbls, tpol, precision, per_time):
    nf, nt = 2, 3
    V, d, w, g32, a1, a2 = _kernel_inputs(nf * nt, nbls, tpol, precision, "flags")
    g0 = _start((nf, nt if per_time else 1) + g32.shape[1:], nbls)
    rows = [x.reshape(nf, nt, -1) for x in (V, d, w)]
    status, g, niter, change, chi2, solved = _solve(*rows, g0, a1, a2, tpol, precision, per_time, 3, 0.0)
    assert status == 0, _lib.lib().fv_last_error()
    Vb, db, wb = (_as_block(x, nf, nt, tpol) for x in (V, d, w.astype(np.float64)))
    g_ref, changes, _, solved_ref = gsr.solve(Vb, db, wb, g0, a1, a2, per_time, 3, 0.0)
    print("gain solve, three iterations", nbls, tpol, precision, per_time, rel_l2(g, g_ref),
          float(np.abs(change - changes[-1]).max()))
    assert niter == 3 and len(changes) == 3
    assert g.shape == g0.shape and rel_l2(g, g_ref) <= BOUND[precision]
    assert np.all(np.abs(change - changes[-1]) <= BOUND[precision] * np.maximum(changes[-1], 1.0))
    assert np.array_equal(solved, solved_ref) and not solved[..., NANT - 2:].any() and solved[..., :NANT - 2].all()
    assert np.array_equal(g[..., NANT - 2:], g0[..., NANT - 2:])  # (an antenna without a used sample keeps its value)
    chi2_ref = gsr.chi2_rows(Vb, db, wb, _per_row(g, nt), a1, a2)  # at the returned gains
    L = tpol * nbls
    print("gain solve, chi2", float((np.abs(chi2 - chi2_ref) / chi2_ref).max() / 2.0**-52), L + 4)
    assert chi2.shape == (nf, nt) and np.all(np.abs(chi2 - chi2_ref) <= (L + 4) * 2.0**-52 * chi2_ref)
    again = _solve(*rows, g0, a1, a2, tpol, precision, per_time, 3, 0.0)  # the same input gives the same bits
    resident = _solve(*rows, g0, a1, a2, tpol, precision, per_time, 3, 0.0, on_device=True)  # ... host or device blocks
    for other in (again, resident):
        assert other[0] == 0 and other[2] == 3
        assert all(np.array_equal(x, y) for x, y in zip(other[1:], (g, niter, change, chi2, solved)))


def test_gains_beyond_the_lds_budget(gpu):
    """1 100 antennas, two feeds: 35.2 KB of complex128 gains per unit, read from global memory instead of LDS."""
    nant, nbls, nf, nt = 1100, 257, 2, 3
    V, d, w, g32, a1, a2 = _kernel_inputs(nf * nt, nbls, 4, 2, "flags", nant=nant)
    assert 16 * 2 * nant > 32768
    g = _start(g32.shape, 3)
    status, num, den = _normal(V, d, w, g, a1, a2, 4, 2)
    assert status == 0, _lib.lib().fv_last_error()
    num_ref, den_ref, num_abs = gsr.normal_sums(_blocked(V, 4), _blocked(d, 4), _blocked(w, 4), g, a1, a2, with_abs=True)
    bound = (_incidences(a1, a2, nant, 2) + 32) * 2.0**-52
    assert np.all(np.abs(num - num_ref) <= bound * num_abs) and np.all(np.abs(den - den_ref) <= bound * den_ref)
    assert (den > 0).any() and (den == 0).any()
    g0 = _start((nf, 1, 2, nant), 4)
    rows = [x.reshape(nf, nt, -1) for x in (V, d, w)]
    status, got, niter, change, chi2, solved = _solve(*rows, g0, a1, a2, 4, 2, False, 3, 0.0)
    assert status == 0 and niter == 3, _lib.lib().fv_last_error()
    Vb, db, wb = (_as_block(x, nf, nt, 4) for x in (V, d, w))
    g_ref, _, chi2_ref, solved_ref = gsr.solve(Vb, db, wb, g0, a1, a2, False, 3, 0.0)
    assert rel_l2(got, g_ref) <= BOUND[2] and np.array_equal(solved, solved_ref) and solved.any() and not solved.all()
    assert np.all(np.abs(chi2 - chi2_ref) <= BOUND[2] * chi2_ref)


# ---- 3. recovery ---------------------------------------------------------------------------------------------------------
def _rounded_case(polarized, noise, precision, seed=0):
    """``solve_case`` with inputs of the run's precision: the data are formed from the rounded model."""
    V, _, w, g, a1, a2 = solve_case(polarized, 0.0, seed)
    rng = np.random.default_rng(seed + 50)
    V = V.astype(CDT[precision])
    d = gain_refs.apply_gains(V, _per_row(g, V.shape[1]), a1, a2)
    d = (d + noise * (rng.normal(size=d.shape) + 1j * rng.normal(size=d.shape)) / np.sqrt(2)).astype(CDT[precision])
    return V, d, w.astype(RDT[precision]), g, a1, a2


def _flat(x):
    return np.ascontiguousarray(x.reshape(x.shape[:2] + (-1,)))


def _chi2_bound(V, w, g, a1, a2, chi2):
    """The relative bound of a reported chi2 against the numpy reference, per (f, t).  Both form delta = m V - d in fp64 from
    the same inputs: m V carries at most 6 u |V'| (two complex products), the subtraction u |delta|, so a term w |delta|^2 is
    off by at most 2 w |delta| 7 u |V'| on either side, and by Cauchy-Schwarz the row by 28 u sqrt(sum w |V'|^2 / chi2)
    relative; the two summation orders add ``(L + 4) 2^-52``."""
    wu = gsr.used_weights(V, w, a1, a2)
    Vp = gain_refs.apply_gains(V, g, a1, a2)
    lead = chi2.shape
    power = (wu * np.abs(Vp) ** 2).reshape(lead + (-1,)).sum(axis=-1)
    L = int(np.prod(V.shape[2:]))
    return (L + 4) * 2.0**-52 + 28 * 2.0**-53 * np.sqrt(power / chi2)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("polarized", [False, True])
def test_recovery(gpu, polarized, precision):
    tpol = 4 if polarized else 1
    V, d, w, g_true, a1, a2 = _rounded_case(polarized, 0.0, precision)
    g0 = np.ones_like(g_true)
    status, g, niter, change, chi2, solved = _solve(_flat(V), _flat(d), _flat(w), g0, a1, a2, tpol, precision, False, 200, 1e-10)
    assert status == 0, _lib.lib().fv_last_error()
    _, changes, _, _ = gsr.solve(V, d, w, g0, a1, a2, False, 200, 1e-10)
    used = gsr.used_weights(V, w, a1, a2) > 0
    m = gain_refs.gain_product(_per_row(g, V.shape[1]), a1, a2, polarized)
    m_true = gain_refs.gain_product(_per_row(g_true, V.shape[1]), a1, a2, polarized)
    worst = float(np.abs(m - m_true)[used].max())
    print("gain solve recovery", polarized, precision, niter, len(changes), float(change.max()), worst)
    assert niter < 200 and np.all(change < 1e-10) and solved.all() and abs(niter - len(changes)) <= 2
    assert worst <= (1e-8 if precision == 2 else BOUND[1])
    # noisy data: chi2 falls, and is the objective's with the auto weights zeroed
    V, d, w, _, a1, a2 = _rounded_case(polarized, 0.05, precision, seed=1)
    status, g, niter, change, chi2, solved = _solve(_flat(V), _flat(d), _flat(w), g0, a1, a2, tpol, precision, False, 200, 1e-10)
    assert status == 0 and niter < 200
    start = gsr.chi2_rows(V, d, w, _per_row(g0, V.shape[1]), a1, a2)
    ref = gsr.chi2_rows(V, d, w, _per_row(g, V.shape[1]), a1, a2)
    bound = _chi2_bound(V, w, _per_row(g, V.shape[1]), a1, a2, ref)
    print("gain solve noisy", polarized, precision, niter, start.sum(), chi2.sum(), float((np.abs(chi2 - ref) / ref / bound).max()))
    assert chi2.sum() < 0.1 * start.sum() and np.all(np.abs(chi2 - ref) <= bound * ref)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what,message", [("negative weight", b"1 weights are negative or not finite"),
                                          ("nan weight", b"1 weights are negative or not finite"),
                                          ("nan datum", b"1 entries of data are not finite where the weight is positive"),
                                          ("inf model", b"1 values of the model are not finite")])
def test_bad_input_fails_the_call_and_the_next_good_call_succeeds(gpu, what, message, precision):
    V, d, w, g, a1, a2 = _rounded_case(True, 0.05, precision)
    V, d, w = _flat(V), _flat(d), np.ones_like(_flat(w))
    g0 = np.ones_like(g)
    good = _solve(V, d, w, g0, a1, a2, 4, precision, False, 4, 0.0)
    assert good[0] == 0
    cross = int(np.flatnonzero(a1 != a2)[0]) + 2 * len(a1)  # pol 2 of a cross-correlation
    auto = int(np.flatnonzero(a1 == a2)[1])
    bV, bd, bw = V.copy(), d.copy(), w.copy()
    if what == "negative weight":
        bw[1, 0, auto] = -1.0  # (an auto-correlation's weight is checked like any other)
    elif what == "nan weight":
        bw[0, 1, cross] = np.nan
    elif what == "nan datum":
        bd[1, 1, cross] = complex(1.0, np.nan)
    else:
        bV[0, 0, cross] = complex(np.inf, 0.0)
    status, g_bad = _solve(bV, bd, bw, g0, a1, a2, 4, precision, False, 4, 0.0)[:2]
    assert status == 1 and message in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    assert np.array_equal(g_bad, g0)  # (the start is untouched)
    again = _solve(V, d, w, g0, a1, a2, 4, precision, False, 4, 0.0)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))
    if what == "nan datum":  # under a zero weight, or on an auto-correlation, the same datum is not an error
        bw[1, 1, cross] = 0
        bd[0, 0, auto] = complex(np.nan, np.inf)
        status, g_ok, _, _, chi2, _ = _solve(V, bd, bw, g0, a1, a2, 4, precision, False, 4, 0.0)
        assert status == 0 and np.isfinite(g_ok).all() and np.isfinite(chi2).all()


# ---- 4. the public function ----------------------------------------------------------------------------------------------
def _solve_public(cfg, data, **kw):
    return fftvis_amd.simulate_vis_gain_solve(data, **cfg, **kw)


def _cross_flags(cfg, shape):
    w = np.ones(shape, dtype=RDT[cfg.get("precision", 2)])
    if cfg.get("polarized", False):
        w[:, :, 0, 1] = 0
        w[:, :, 1, 0] = 0
    return w


def _products(cfg, g):
    a1, a2 = _ant_rows(cfg)
    return gain_refs.gain_product(_block_layout(cfg, g), a1, a2, cfg.get("polarized", False))


@pytest.mark.parametrize("precision", [2, 1])
def test_public_recovery_and_the_resident_model(gpu, monkeypatch, precision):
    import torch

    from fftvis_amd.gpu import gpu_simulate

    cfg = _sid(source_config("cm", "unpol", "airy", False, precision))
    a1, a2 = _ant_rows(cfg)
    g_true = _gains(cfg).astype(np.complex128)
    V = fftvis_amd.simulate_vis(**cfg)
    d = gain_refs.apply_gains(V, _block_layout(cfg, g_true), a1, a2).astype(CDT[precision])
    g, info, model = _solve_public(cfg, d, tol=1e-10, max_iter=200, return_model=True)
    used = gsr.used_weights(V, None, a1, a2) > 0
    worst = float(np.abs(_products(cfg, g) - _products(cfg, g_true))[used].max())
    print("gain solve public recovery", precision, info["niter"], worst)
    assert info["converged"] and info["niter"] < 200 and np.all(info["change"] < 1e-10) and info["solved"].all()
    assert g.shape == g_true.shape and g.dtype == np.complex128 and info["solved"].shape == g.shape
    assert info["chi2"].shape == V.shape[:2] and info["change"].shape == (len(cfg["freqs"]),)
    assert worst <= (1e-8 if precision == 2 else BOUND[1])
    assert isinstance(model, torch.Tensor) and model.device.type == "cuda" and tuple(model.shape) == V.shape
    assert rel_l2(model.cpu().numpy(), V) <= BOUND[precision] / 10  # (two runs of one forward)

    # the resident model serves the next call: no forward, fluxes not needed, the same bits
    def forward(*a, **k):
        raise AssertionError("the forward ran")

    with monkeypatch.context() as mp:
        mp.setattr(gpu_simulate.SimHandle, "run_device", forward)
        mp.setattr(gpu_simulate.SimHandle, "run", forward)
        g2, info2 = _solve_public(dict(cfg, fluxes=None), d, model=model, tol=1e-10, max_iter=200)
        g3, _ = _solve_public(dict(cfg, fluxes=None), d, model=model.cpu().numpy(), tol=1e-10, max_iter=200)  # uploaded once
    assert np.array_equal(g2, g) and np.array_equal(g3, g) and info2["niter"] == info["niter"]
    assert np.array_equal(info2["chi2"], info["chi2"])
    # resident data and weights: the bits of the host-array call, on the device
    w = np.random.default_rng(3).uniform(0.5, 2.0, size=V.shape).astype(RDT[precision])
    w[0, 0, 3] = 0
    noisy = (d + 0.05 * _start(d.shape, 4)).astype(CDT[precision])
    host = _solve_public(cfg, noisy, weights=w, model=model, max_iter=6, tol=0.0, per_time=True)
    D, W = torch.from_numpy(noisy).cuda(), torch.from_numpy(w).cuda()
    dev = _solve_public(cfg, D, weights=W, model=model, max_iter=6, tol=0.0, per_time=True)
    assert host[0].shape == g.shape + (len(cfg["times"]),) and host[1]["niter"] == 6 and not host[1]["converged"]
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dev[0], dev[1]["chi2"], dev[1]["solved"], dev[1]["change"]))
    assert np.array_equal(dev[0].cpu().numpy(), host[0]) and np.array_equal(dev[1]["chi2"].cpu().numpy(), host[1]["chi2"])
    assert dev[1]["solved"].dtype == torch.bool and np.array_equal(dev[1]["solved"].cpu().numpy(), host[1]["solved"])
    ref, _, chi2_ref, _ = gsr.solve(model.cpu().numpy(), noisy, w, np.ones((V.shape[0], V.shape[1], 1, len(cfg["ants"])), complex),
                                    a1, a2, True, 6, 0.0)
    assert rel_l2(_block_layout(cfg, host[0]), ref) <= BOUND[precision] and np.all(np.abs(host[1]["chi2"] - chi2_ref) <= BOUND[precision] * chi2_ref)
    # start gains, and the reference antenna: chi2 unchanged, g[ref, feed 0] real and positive
    nums = list(cfg["ants"])
    plain = _solve_public(cfg, noisy, weights=w, model=model, gains=g_true, max_iter=6, tol=0.0)
    fixed = _solve_public(cfg, noisy, weights=w, model=model, gains=g_true, max_iter=6, tol=0.0, ref_ant=nums[2])
    assert np.array_equal(fixed[1]["chi2"], plain[1]["chi2"])
    assert np.all(fixed[0][2].real > 0) and np.all(np.abs(fixed[0][2].imag) <= 1e-15 * np.abs(fixed[0][2]))
    # (a unit-modulus factor per antenna: the products are the same up to the roundings of four complex products)
    p_fixed, p_plain = _products(cfg, fixed[0]), _products(cfg, plain[0])
    assert np.all(np.abs(p_fixed - p_plain) <= 16 * 2.0**-52 * np.abs(p_plain)) and not np.array_equal(fixed[0], plain[0])
    with pytest.raises(ValueError, match="model lives on cuda:0, the run is on cuda:1"):
        _solve_public(dict(cfg, device=1), d, model=model)
    # bad weights fail the call, and the next good call succeeds
    bw = w.copy()
    bw[1, 1, 5] = -1.0
    with pytest.raises(_lib.FftvisHipError, match="1 weights are negative or not finite"):
        _solve_public(cfg, noisy, weights=bw, model=model, max_iter=6, tol=0.0, per_time=True)
    again = _solve_public(cfg, noisy, weights=w, model=model, max_iter=6, tol=0.0, per_time=True)
    assert np.array_equal(again[0], host[0])
    # the raw C ABI on a handle-less block
    nf, nt = V.shape[:2]
    raw = _solve(model.cpu().numpy().reshape(nf, nt, -1), noisy.reshape(nf, nt, -1), w.reshape(nf, nt, -1),
                 np.ones((nf, nt, 1, len(nums)), complex), a1.astype(np.int32), a2.astype(np.int32), 1, precision, True, 6, 0.0)
    assert raw[0] == 0 and np.array_equal(raw[1], _block_layout(cfg, host[0])) and np.array_equal(raw[4], host[1]["chi2"])


@pytest.mark.parametrize("precision", [2, 1])
def test_polarized_full_stokes_with_flagged_cross_hands(gpu, precision):
    cfg = _sid(source_config("cm", "full", "two", False, precision))
    a1, a2 = _ant_rows(cfg)
    g_true = _gains(cfg).astype(np.complex128)
    V = fftvis_amd.simulate_vis(**cfg)
    d = gain_refs.apply_gains(V, _block_layout(cfg, g_true), a1, a2).astype(CDT[precision])
    w = _cross_flags(cfg, V.shape)
    g, info = _solve_public(cfg, d, weights=w, tol=1e-10, max_iter=200)
    used = gsr.used_weights(V, w, a1, a2) > 0
    worst = float(np.abs(_products(cfg, g) - _products(cfg, g_true))[used].max())
    print("gain solve public polarized", precision, info["niter"], worst)
    assert info["converged"] and g.shape == g_true.shape and info["solved"].all()
    assert worst <= (1e-8 if precision == 2 else BOUND[1])


def test_the_model_is_filled_time_block_by_time_block(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    cfg = _sid(source_config("cm", "full", "two", False, 2))
    V = fftvis_amd.simulate_vis(**cfg)
    calls = []
    real = gpu_simulate.SimHandle.run_device
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_device", lambda self, *a: calls.append(a[:2]) or real(self, *a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    _, info, model = _solve_public(cfg, V, weights=_cross_flags(cfg, V.shape), max_iter=1, tol=0.0, return_model=True)
    assert calls == [(t, t + 1) for t in range(V.shape[1])] and info["niter"] == 1
    assert model.is_contiguous() and rel_l2(model.cpu().numpy(), V) <= BOUND[2] / 10  # (two runs of one forward)


def test_lattice_array_takes_its_type1_forward(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    cfg = hex19_config()
    a1, a2 = _ant_rows(cfg)
    V = fftvis_amd.simulate_vis(**cfg)
    d = (gain_refs.apply_gains(V, _block_layout(cfg, _gains(cfg)), a1, a2) + 0.05 * np.abs(V).mean() * _start(V.shape, 8))
    w = _cross_flags(cfg, V.shape)
    seen = []
    real1, real3 = gpu_simulate.SimHandle.set_array_type1, gpu_simulate.SimHandle.set_array
    monkeypatch.setattr(gpu_simulate.SimHandle, "set_array_type1", lambda self, *a: seen.append(1) or real1(self, *a))
    monkeypatch.setattr(gpu_simulate.SimHandle, "set_array", lambda self, *a: seen.append(3) or real3(self, *a))
    g, info = _solve_public(cfg, d, weights=w, max_iter=5, tol=0.0)
    assert seen == [1]
    g0 = np.ones((V.shape[0], 1, 2, len(cfg["ants"])), complex)
    ref, _, chi2_ref, _ = gsr.solve(V, d, w, g0, a1, a2, False, 5, 0.0)
    print("gain solve lattice", rel_l2(_block_layout(cfg, g)[:, :1], ref))
    assert rel_l2(_block_layout(cfg, g)[:, :1], ref) <= BOUND[2] and np.all(np.abs(info["chi2"] - chi2_ref) <= BOUND[2] * chi2_ref)
    _solve_public(dict(cfg, force_use_type3=True), d, weights=w, max_iter=1, tol=0.0)  # (and the other one when asked)
    assert seen == [1, 3]


@pytest.mark.parametrize("precision", [2, 1])
def test_basis_beams(gpu, precision):
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    a1, a2 = _ant_rows(cfg)
    V = fftvis_amd.simulate_vis(**cfg)
    d = (gain_refs.apply_gains(V, _block_layout(cfg, _gains(cfg)), a1, a2) + 0.05 * np.abs(V).mean() * _start(V.shape, 9)).astype(CDT[precision])
    w = _cross_flags(cfg, V.shape)
    g, info = _solve_public(cfg, d, weights=w, max_iter=5, tol=0.0, per_time=True)
    g0 = np.ones((V.shape[0], V.shape[1], 2, len(cfg["ants"])), complex)
    ref, _, chi2_ref, _ = gsr.solve(V, d, w, g0, a1, a2, True, 5, 0.0)
    print("gain solve basis beams", precision, rel_l2(_block_layout(cfg, g), ref))
    assert rel_l2(_block_layout(cfg, g), ref) <= BOUND[precision]
    assert np.all(np.abs(info["chi2"] - chi2_ref) <= BOUND[precision] * chi2_ref) and info["niter"] == 5
