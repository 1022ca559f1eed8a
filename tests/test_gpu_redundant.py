"""GPU tests of redundant calibration (``redundant_gain_solve``, ``redundant_average``; ``fv_redundant_solve`` and its two
halves alone through ``fv_redundant_vis_rows`` and ``fv_redundant_normal_rows``).

The U-step adds, per (row, pol, group), n_r signed fp64 terms w conj(m) d, m = conj(g[a1]) g[a2] (n_r: the group's members):
each a product of three complex factors and the weight formed in fp64 -- at most 16 * 2^-52 per term on the device and as
much in the numpy reference, as for the gather (``test_gpu_gain_solve``) -- and the two summation orders differ by n_r u
each.  With b = (n_r + 32) 2^-52:  |num - num_ref| <= b sum |terms| = b num_abs,  and  |den - den_ref| <= b den_ref,  whose
terms w |m|^2 are their own moduli and take fewer roundings.  U = num / den component by component, one rounding each on
either side (2 * 2^-53 |U| together), so to first order
    |U - U_ref| <= |num - num_ref| / den_ref + |U_ref| |den - den_ref| / den_ref + 2^-52 |U_ref|
                <= b (num_abs / den_ref + |U_ref|) + 4 * 2^-52 |U_ref|,
the last term with room for the second order.  The gather with the groups' visibilities as its model is held to
``test_gpu_gain_solve``'s (n_a + 32) 2^-52 sum |terms|: the model is read from another array, nothing else differs.  The
loop is held to ``test_gpu_objective``'s BOUND against the numpy reference on the same rounded inputs -- all of its
arithmetic is fp64 whatever the run's precision -- and its chi2 to the gain solve's ``_chi2_bound``."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import gain_refs
from tests import gain_solve_refs as gsr
from tests import redundant_refs as rr
from tests.helpers import rel_l2
from tests.tangent_refs import hex19_config
from tests.test_gpu_gain_solve import _as_block, _chi2_bound, _cross_flags, _flat, _incidences, _per_row, _start
from tests.test_gpu_gains import BOUND, CDT, NANT, RDT, _ant_rows, _block_layout, _blocked, _kernel_inputs
from tests.test_redundant_host import red_case

pytestmark = pytest.mark.gpu

NGROUPS = 9


def _groups(nbls, seed=0):
    """Nine groups: group 0 takes every second baseline (more than 64 members from nbls = 257 on), group 7 is a singleton
    (nbls > 3), group 8 has no member, the others share the rest at random."""
    group = np.random.default_rng(seed + nbls).integers(1, 7, nbls).astype(np.int32)
    group[::2] = 0
    if nbls > 3:
        group[3] = 7
    return group


def _inputs(nrows, nbls, tpol, precision, weights, nant=NANT):
    """``test_gpu_gains``' inputs without the model, with groups; under "flags" group 6 is flagged altogether."""
    _, d, w, g32, a1, a2 = _kernel_inputs(nrows, nbls, tpol, precision, weights, nant=nant)
    group = _groups(nbls)
    if weights == "flags":
        for pol in range(tpol):
            w[:, pol * nbls + np.flatnonzero(group == 6)] = 0
            d[:, pol * nbls + np.flatnonzero(group == 6)] = complex(np.nan, np.inf)
    g = _start(g32.shape, nbls + tpol)  # complex128 whatever the run's precision
    return d, w, g, a1, a2, group


def _u_shape(nrows, tpol):
    return (nrows, 2, 2, NGROUPS) if tpol == 4 else (nrows, NGROUPS)


def _w64(w, tpol):
    return None if w is None else _blocked(w.astype(np.float64), tpol)


# ---- 1. the U-step alone -------------------------------------------------------------------------------------------------
def _vis_rows(d, w, g, a1, a2, group, tpol, precision, U0):
    U, den = np.ascontiguousarray(U0, dtype=np.complex128).copy(), np.full(U0.shape, 7.0)
    status = _lib.lib().fv_redundant_vis_rows(0, precision, d.shape[0], len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                              NGROUPS, _lib.ptr(group), _lib.ptr(g), _lib.ptr(d), _lib.ptr(w), _lib.ptr(U),
                                              _lib.ptr(den))
    return status, U, den


def _check_vis_step(label, d, w, g, a1, a2, group, tpol, precision):
    nrows = d.shape[0]
    U0 = np.full(_u_shape(nrows, tpol), 3 - 2j)
    status, U, den = _vis_rows(d, w, g, a1, a2, group, tpol, precision, U0)
    assert status == 0, _lib.lib().fv_last_error()
    U_ref, den_ref, num_abs = rr.vis_step(_blocked(d, tpol), _w64(w, tpol), g, a1, a2, group, NGROUPS, U0, with_abs=True)
    n_r = np.bincount(group, minlength=NGROUPS)
    b = (n_r + 32) * 2.0**-52
    ok = den_ref > 0
    safe = np.where(ok, den_ref, 1.0)
    bound = b * (num_abs / safe + np.abs(U_ref)) + 4 * 2.0**-52 * np.abs(U_ref)
    print(label, float((np.abs(den - den_ref) / np.maximum(b * den_ref, 1e-300)).max()),
          float((np.abs(U - U_ref)[ok] / bound[ok]).max()) if ok.any() else 0.0, int(n_r.max()))
    assert np.all(np.abs(den - den_ref) <= b * den_ref) and np.array_equal(den > 0, ok)
    assert np.all(np.abs(U - U_ref)[ok] <= bound[ok]) and np.isfinite(U).all()
    assert np.all(U[~ok] == 3 - 2j)  # an empty or fully flagged group keeps the value passed in
    assert not ok[..., 8].any()
    status, U2, den2 = _vis_rows(d, w, g, a1, a2, group, tpol, precision, U0)  # the same input gives the same bits
    assert status == 0 and np.array_equal(U2, U) and np.array_equal(den2, den)
    return ok


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_vis_step(gpu, nbls, tpol, nrows, precision, weights):
    d, w, g, a1, a2, group = _inputs(nrows, nbls, tpol, precision, weights)
    ok = _check_vis_step(f"redundant U-step {nbls} {tpol} {nrows} {precision} {weights}", d, w, g, a1, a2, group, tpol, precision)
    n_r = np.bincount(group, minlength=NGROUPS)
    assert n_r[8] == 0 and n_r[7] == (nbls > 3) and n_r[0] == (nbls + 1) // 2
    if nbls >= 257:
        assert n_r[0] > 64
    if nbls >= 63:
        assert ok[..., 0].all() and n_r[6] > 0
        if weights == "flags":
            assert not ok[..., 6].any() and not np.isfinite(d).all()
        if weights == "none":
            assert ok[..., 7].all() == (a1[3] != a2[3])


# ---- 2. the gather with the groups' visibilities as its model ------------------------------------------------------------
def _normal_rows(U, d, w, g, a1, a2, group, tpol, precision):
    num, den = np.full(g.shape, 7.0, dtype=np.complex128), np.full(g.shape, 7.0)
    status = _lib.lib().fv_redundant_normal_rows(0, precision, d.shape[0], len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2),
                                                 NGROUPS, _lib.ptr(group), _lib.ptr(g), _lib.ptr(U), _lib.ptr(d), _lib.ptr(w),
                                                 _lib.ptr(num), _lib.ptr(den))
    return status, num, den


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [1, 63, 64, 65, 257, 1023])
def test_normal_sums_with_group_visibilities(gpu, nbls, tpol, nrows, precision, weights):
    d, w, g, a1, a2, group = _inputs(nrows, nbls, tpol, precision, weights)
    U = np.ascontiguousarray(_start(_u_shape(nrows, tpol), nbls + 3))
    status, num, den = _normal_rows(U, d, w, g, a1, a2, group, tpol, precision)
    assert status == 0, _lib.lib().fv_last_error()
    num_ref, den_ref, num_abs = rr.normal_sums(U, _blocked(d, tpol), _w64(w, tpol), g, a1, a2, group, with_abs=True)
    n_a = _incidences(a1, a2, NANT, g.shape[1])
    bound = (n_a + 32) * 2.0**-52
    print("redundant normal sums", nbls, tpol, nrows, precision, weights,
          float((np.abs(num - num_ref) / np.maximum(bound * num_abs, 1e-300)).max()),
          float((np.abs(den - den_ref) / np.maximum(bound * den_ref, 1e-300)).max()), int(n_a.max()))
    assert np.all(np.abs(num - num_ref) <= bound * num_abs) and np.all(np.abs(den - den_ref) <= bound * den_ref)
    assert np.all(num[..., NANT - 2:] == 0) and np.all(den[..., NANT - 2:] == 0)  # autos only, and no baseline
    if nbls >= 63:
        assert (den[..., :NANT - 2] > 0).all() and np.isfinite(num).all()
    status, num2, den2 = _normal_rows(U, d, w, g, a1, a2, group, tpol, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(num2, num) and np.array_equal(den2, den)


# ---- 3. three iterations, fixed ------------------------------------------------------------------------------------------
def _solve(d, w, g0, a1, a2, group, ngroups, tpol, precision, per_time, max_iter, tol, on_device=False):
    """``fv_redundant_solve`` on (nfreqs, ntimes, tpol nbls) blocks: (status, gains, U, niter, change, chi2, solved, vis_solved)."""
    nf, nt = d.shape[:2]
    g = np.ascontiguousarray(g0, dtype=np.complex128).copy()
    niter = np.full(1, -1, dtype=np.int32)
    change, chi2, solved = np.full(g.shape[:2], -1.0), np.full((nf, nt), -1.0), np.full(g.shape, 7, dtype=np.int32)
    U = np.full((nf, nt, tpol, ngroups), 7.0, dtype=np.complex128)
    vis_solved = np.full(U.shape, 7, dtype=np.int32)
    bufs = [np.ascontiguousarray(d), None if w is None else np.ascontiguousarray(w)]
    if on_device:
        import torch

        bufs = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
        ptrs = [None if b is None else ctypes.c_void_p(b.data_ptr()) for b in bufs]
    else:
        ptrs = [_lib.ptr(b) for b in bufs]
    flag = int(on_device)
    group = np.ascontiguousarray(group, dtype=np.int32)
    status = _lib.lib().fv_redundant_solve(0, precision, nf, nt, len(a1), tpol, g.shape[-1], _lib.ptr(a1), _lib.ptr(a2), ngroups,
                                           _lib.ptr(group), int(per_time), ptrs[0], flag, ptrs[1], flag, _lib.ptr(g), _lib.ptr(U),
                                           max_iter, tol, _lib.ptr(niter), _lib.ptr(change), _lib.ptr(chi2), _lib.ptr(solved),
                                           _lib.ptr(vis_solved))
    U = U.reshape((nf, nt, 2, 2, ngroups) if tpol == 4 else (nf, nt, ngroups))
    return status, g, U, int(niter[0]), change, chi2, solved != 0, (vis_solved != 0).reshape(U.shape)


def _check_three_iterations(label, d, w, g0, a1, a2, group, tpol, precision, per_time, nf, nt, nant):
    rows = [x.reshape(nf, nt, -1) for x in (d, w)]
    status, g, U, niter, change, chi2, solved, vis_solved = _solve(*rows, g0, a1, a2, group, NGROUPS, tpol, precision, per_time, 3, 0.0)
    assert status == 0, _lib.lib().fv_last_error()
    db, wb = (_as_block(x, nf, nt, tpol) for x in (d, w.astype(np.float64)))
    g_ref, U_ref, changes, _, solved_ref, vis_solved_ref = rr.solve(db, wb, g0, a1, a2, group, NGROUPS, per_time, 3, 0.0)
    print(label, rel_l2(g, g_ref), rel_l2(U, U_ref), float(np.abs(change - changes[-1]).max()))
    assert niter == 3 and len(changes) == 3
    assert g.shape == g0.shape and rel_l2(g, g_ref) <= BOUND[precision] and rel_l2(U, U_ref) <= BOUND[precision]
    assert np.all(np.abs(change - changes[-1]) <= BOUND[precision] * np.maximum(changes[-1], 1.0))
    assert np.array_equal(solved, solved_ref) and not solved[..., nant - 2:].any() and solved[..., :nant - 2].all()
    assert np.array_equal(g[..., nant - 2:], g0[..., nant - 2:])  # (an antenna without a used sample keeps its value)
    assert np.array_equal(vis_solved, vis_solved_ref) and not vis_solved[..., 6:9:2].any() and vis_solved[..., 0].all()
    assert np.all(U[~vis_solved] == 0)
    chi2_ref = rr.chi2_rows(U, db, wb, _per_row(g, nt), a1, a2, group)  # at the returned gains and visibilities
    bound = _chi2_bound(rr.model(U, group), wb, _per_row(g, nt), a1, a2, chi2_ref)
    print(label, "chi2", float((np.abs(chi2 - chi2_ref) / chi2_ref / bound).max()))
    assert chi2.shape == (nf, nt) and np.all(np.abs(chi2 - chi2_ref) <= bound * chi2_ref)
    return rows, (g, U, niter, change, chi2, solved, vis_solved)


@pytest.mark.parametrize("per_time", [False, True])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("tpol", [1, 4])
@pytest.mark.parametrize("nbls", [65, 257])
def test_three_iterations(gpu, nbls, tpol, precision, per_time):
    nf, nt = 2, 3
    d, w, g1, a1, a2, group = _inputs(nf * nt, nbls, tpol, precision, "flags")
    g0 = _start((nf, nt if per_time else 1) + g1.shape[1:], nbls)
    rows, first = _check_three_iterations(f"redundant solve, three iterations {nbls} {tpol} {precision} {per_time}", d, w, g0, a1, a2,
                                          group, tpol, precision, per_time, nf, nt, NANT)
    again = _solve(*rows, g0, a1, a2, group, NGROUPS, tpol, precision, per_time, 3, 0.0)  # the same input gives the same bits
    resident = _solve(*rows, g0, a1, a2, group, NGROUPS, tpol, precision, per_time, 3, 0.0, on_device=True)  # host or device blocks
    for other in (again, resident):
        assert other[0] == 0 and all(np.array_equal(x, y) for x, y in zip(other[1:], first))


# ---- 4. recovery ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("polarized,cross", [(False, None), (True, "strong"), (True, "flagged")])
def test_recovery(gpu, polarized, cross, precision):
    tpol = 4 if polarized else 1
    _, w, g_true, U_true, a1, a2, group, ngroups, _ = red_case(polarized, 0.0, cross=cross)
    nt = w.shape[1]
    U_true = U_true.astype(CDT[precision])  # the data are formed from the rounded inputs
    clean = gain_refs.apply_gains(rr.model(U_true, group), _per_row(g_true, nt), a1, a2)
    d, w = clean.astype(CDT[precision]), w.astype(RDT[precision])
    g0 = np.ones_like(g_true)
    status, g, U, niter, change, chi2, solved, vis_solved = _solve(_flat(d), _flat(w), g0, a1, a2, group, ngroups, tpol, precision,
                                                                   False, 400, 1e-10)
    assert status == 0, _lib.lib().fv_last_error()
    _, _, changes, _, _, _ = rr.solve(d, w.astype(np.float64), g0, a1, a2, group, ngroups, False, 400, 1e-10)
    used = gsr.used_weights(d, w, a1, a2) > 0
    fit = gain_refs.apply_gains(rr.model(U, group), _per_row(g, nt), a1, a2)
    worst = float(np.abs(fit - clean)[used].max())
    print("redundant solve recovery", polarized, cross, precision, niter, len(changes), float(change.max()), worst)
    assert niter < 400 and abs(niter - len(changes)) <= 2 and np.all(change < 1e-10) and solved.all()
    assert np.array_equal(vis_solved, rr._group_sums(w.astype(np.float64), group, ngroups) > 0)
    assert worst <= (1e-8 if precision == 2 else BOUND[1])


# ---- 5. bad input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what,message", [("negative weight", b"1 weights are negative or not finite"),
                                          ("nan weight", b"1 weights are negative or not finite"),
                                          ("nan datum", b"1 entries of data are not finite where the weight is positive")])
def test_bad_input_fails_the_call_and_the_next_good_call_succeeds(gpu, what, message, precision):
    nf, nt, nbls = 2, 2, 65
    d, w, g1, a1, a2, group = _inputs(nf * nt, nbls, 4, precision, "positive")
    d, w = d.reshape(nf, nt, -1), w.reshape(nf, nt, -1)
    g0 = _start((nf, 1) + g1.shape[1:], 2)
    args = (a1, a2, group, NGROUPS, 4, precision, False, 4, 0.0)
    good = _solve(d, w, g0, *args)
    assert good[0] == 0
    cross = int(np.flatnonzero(a1 != a2)[0]) + 2 * nbls  # pol 2 of a cross-correlation
    auto = int(np.flatnonzero(a1 == a2)[1])
    bd, bw = d.copy(), w.copy()
    if what == "negative weight":
        bw[1, 0, auto] = -1.0  # (an auto-correlation's weight is checked like any other)
    elif what == "nan weight":
        bw[0, 1, cross] = np.nan
    else:
        bd[1, 1, cross] = complex(1.0, np.nan)
    status, g_bad = _solve(bd, bw, g0, *args)[:2]
    assert status == 1 and message in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    assert np.array_equal(g_bad, g0)  # (the start is untouched)
    again = _solve(d, w, g0, *args)
    assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(again[1:], good[1:]))
    if what == "nan datum":  # under a zero weight, or on an auto-correlation, the same datum is not an error
        bw[1, 1, cross] = 0
        bd[0, 0, auto] = complex(np.nan, np.inf)
        status, g_ok, U_ok, _, _, chi2, _, _ = _solve(bd, bw, g0, *args)
        assert status == 0 and np.isfinite(g_ok).all() and np.isfinite(U_ok).all() and np.isfinite(chi2).all()


# ---- 6. gains beyond the LDS budget --------------------------------------------------------------------------------------
def test_gains_beyond_the_lds_budget(gpu):
    """1 100 antennas, two feeds: 35.2 KB of complex128 gains per unit, read from global memory instead of LDS."""
    nant, nbls, nf, nt = 1100, 257, 2, 3
    d, w, g, a1, a2, group = _inputs(nf * nt, nbls, 4, 2, "flags", nant=nant)
    assert 16 * 2 * nant > 32768
    _check_vis_step("redundant U-step beyond LDS", d, w, g, a1, a2, group, 4, 2)
    g0 = _start((nf, 1, 2, nant), 4)
    rows = [x.reshape(nf, nt, -1) for x in (d, w)]
    status, got, U, niter, change, chi2, solved, vis_solved = _solve(*rows, g0, a1, a2, group, NGROUPS, 4, 2, False, 3, 0.0)
    assert status == 0 and niter == 3, _lib.lib().fv_last_error()
    db, wb = (_as_block(x, nf, nt, 4) for x in (d, w))
    g_ref, U_ref, _, chi2_ref, solved_ref, vis_solved_ref = rr.solve(db, wb, g0, a1, a2, group, NGROUPS, False, 3, 0.0)
    assert rel_l2(got, g_ref) <= BOUND[2] and rel_l2(U, U_ref) <= BOUND[2]
    assert np.array_equal(solved, solved_ref) and solved.any() and not solved.all() and np.array_equal(vis_solved, vis_solved_ref)
    assert np.all(np.abs(chi2 - chi2_ref) <= BOUND[2] * chi2_ref)


# ---- 7. the public functions with the simulator --------------------------------------------------------------------------
def _public_case():
    cfg = hex19_config()
    reds, bls, group = fftvis_amd.redundant_groups(cfg["ants"])
    cfg = dict(cfg, baselines=bls)
    rng = np.random.default_rng(21)
    shape = (len(cfg["ants"]), 2, len(cfg["freqs"]))
    g_true = 1 + 0.1 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    return cfg, reds, bls, group, g_true


def test_public_path_with_the_simulator(gpu):
    import torch

    cfg, reds, bls, group, g_true = _public_case()
    ants = cfg["ants"]
    a1, a2 = _ant_rows(cfg)
    V = fftvis_amd.simulate_vis(**cfg)
    d = gain_refs.apply_gains(V, _block_layout(cfg, g_true), a1, a2)
    w = _cross_flags(cfg, V.shape)  # (an unpolarized sky: the cross-hands are weak, flag them)
    kw = dict(baselines=bls, weights=w, polarized=True, tol=1e-10, max_iter=400)
    g, vis, info = fftvis_amd.redundant_gain_solve(d, ants, **kw)
    assert info["converged"] and info["niter"] < 400 and np.all(info["change"] < 1e-10) and info["solved"].all()
    assert g.shape == g_true.shape and g.dtype == np.complex128 and info["solved"].shape == g.shape
    assert vis.shape == V.shape[:-1] + (len(reds),) and vis.dtype == np.complex128 and info["vis_solved"].shape == vis.shape
    assert info["chi2"].shape == V.shape[:2] and info["change"].shape == (len(cfg["freqs"]),)
    assert info["reds"] == reds and info["baselines"] == bls
    assert info["vis_solved"][:, :, 0, 0].all() and not info["vis_solved"][:, :, 0, 1].any()
    fixed = fftvis_amd.fix_redundant_degeneracies(g, ants, ref_gains=g_true, solved=info["solved"])
    avg, den = fftvis_amd.redundant_average(d, ants, fixed, baselines=bls, weights=w, polarized=True)
    first = fftvis_amd.simulate_vis(**dict(cfg, baselines=[red[0] for red in reds]))
    par = (slice(None), slice(None), [0, 1], [0, 1])  # the parallel hands
    res_g, res_v = float(np.abs(fixed - g_true).max()), float(np.abs(avg - first)[par].max() / np.abs(first[par]).max())
    # the same comparison with the numpy reference solve on the same d: what the forward's own eps leaves of redundancy
    g0 = np.ones((V.shape[0], 1, 2, len(ants)), complex)
    g_ref, _, changes, _, solved_ref, _ = rr.solve(d, w, g0, a1, a2, group, len(reds), False, 400, 1e-10)
    pub = np.ascontiguousarray(g_ref.transpose(3, 2, 0, 1)).reshape(g_true.shape)
    fixed_ref = fftvis_amd.fix_redundant_degeneracies(pub, ants, ref_gains=g_true)
    rows = _per_row(np.ascontiguousarray(fixed_ref.reshape(len(ants), 2, -1, 1).transpose(2, 3, 1, 0)), V.shape[1])
    avg_ref, _ = rr.vis_step(d, w, rows, a1, a2, group, len(reds))
    ref_g, ref_v = float(np.abs(fixed_ref - g_true).max()), float(np.abs(avg_ref - first)[par].max() / np.abs(first[par]).max())
    print("redundant public path: gains", res_g, "reference", ref_g, "visibilities", res_v, "reference", ref_v, "iterations",
          info["niter"], len(changes))
    assert abs(info["niter"] - len(changes)) <= 2
    assert res_g <= 10 * ref_g and res_v <= 10 * ref_v
    assert np.array_equal(den > 0, info["vis_solved"]) and np.all(avg[den == 0] == 0)
    # tensors on the device: the host call's bits, on the device
    D, W = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()
    short = dict(kw, max_iter=6, tol=0.0, per_time=True, ref_ant=list(ants)[2])
    host = fftvis_amd.redundant_gain_solve(d, ants, **short)
    dev = fftvis_amd.redundant_gain_solve(D, ants, **dict(short, weights=W))
    assert host[0].shape == g.shape + (len(cfg["times"]),) and host[2]["niter"] == 6 and not host[2]["converged"]
    assert np.all(np.abs(host[0][2, 0].imag) <= 1e-15 * np.abs(host[0][2, 0])) and np.all(host[0][2, 0].real > 0)
    for x, y in [(dev[0], host[0]), (dev[1], host[1])] + [(dev[2][k], host[2][k]) for k in ("change", "chi2", "solved", "vis_solved")]:
        assert isinstance(x, torch.Tensor) and x.device.type == "cuda" and np.array_equal(x.cpu().numpy(), y)
    avg_dev, den_dev = fftvis_amd.redundant_average(D, ants, torch.from_numpy(fixed).cuda(), baselines=bls, weights=W, polarized=True)
    assert avg_dev.device.type == "cuda" and np.array_equal(avg_dev.cpu().numpy(), avg) and np.array_equal(den_dev.cpu().numpy(), den)
    with pytest.raises(_lib.FftvisHipError, match="1 weights are negative or not finite"):
        bw = w.copy()
        bw[1, 1, 0, 0, 5] = -1.0
        fftvis_amd.redundant_gain_solve(d, ants, **dict(kw, weights=bw))
