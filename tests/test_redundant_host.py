"""CPU tests of redundant calibration (``redundant_gain_solve``, ``redundant_average``, ``redundant_groups``,
``fix_redundant_degeneracies``; ``fv_redundant_solve``, ``fv_redundant_vis_rows``, ``fv_redundant_normal_rows``): the numpy
reference against the properties of the iteration, the grouping, the degeneracies, the C surface and the argument errors
raised before any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, redundant
from tests import gain_refs
from tests import redundant_refs as rr
from tests.position_adjoint_refs import hex_positions


def hex19():
    xy = 14.6 * hex_positions(2)
    return {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(len(xy))}


def _per_row(g, nt):
    return np.broadcast_to(g, (g.shape[0], nt) + g.shape[2:])


def red_case(polarized, noise, seed=0, lead=(2, 2), cross="strong", sigma=0.1, per_time=False):
    """hex-19, every baseline in group order, data from true gains ``1 + sigma N`` (time-constant unless ``per_time``), random
    group visibilities and noise of standard deviation ``noise``; polarized: cross-hands as strong as the parallel hands
    (``cross="strong"``) or flagged (``"flagged"``).  Returns (d, w, true gains, true U, a1, a2, group, ngroups, ants)."""
    rng = np.random.default_rng(seed)
    ants = hex19()
    reds, bls, group = fftvis_amd.redundant_groups(ants)
    a1 = np.array([bl[0] for bl in bls], dtype=np.int32)
    a2 = np.array([bl[1] for bl in bls], dtype=np.int32)
    pol = (2, 2) if polarized else ()

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    U = c(lead + pol + (len(reds),))
    g = 1 + sigma * c((lead[0], lead[1] if per_time else 1, 2 if polarized else 1, len(ants)))
    shape = lead + pol + (len(bls),)
    d = gain_refs.apply_gains(rr.model(U, group), _per_row(g, lead[1]), a1, a2) + noise * c(shape) / np.sqrt(2)
    w = np.ones(shape)
    if polarized and cross == "flagged":
        w[..., 0, 1, :] = 0
        w[..., 1, 0, :] = 0
    return d, w, g, U, a1, a2, group, len(reds), ants


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polarized,cross", [(False, None), (True, "strong"), (True, "flagged")])
def test_reference_converges_on_hex19(polarized, cross):
    d, w, g, U, a1, a2, group, ngroups, _ = red_case(polarized, 0.0, cross=cross)
    got, Ugot, changes, chi2, solved, vis_solved = rr.solve(d, w, np.ones_like(g), a1, a2, group, ngroups, False, 400, 1e-10)
    power = float((w * np.abs(d) ** 2).sum())
    print("redundant reference: iterations, chi2 / sum w |d|^2", polarized, cross, len(changes), float(chi2.sum()) / power)
    assert len(changes) < 400 and changes[-1].max() < 1e-10
    assert chi2.sum() <= 1e-16 * power
    assert solved.all() and got.shape == g.shape and Ugot.shape == U.shape and chi2.shape == d.shape[:2]
    assert np.array_equal(vis_solved, rr._group_sums(w, group, ngroups) > 0) and vis_solved.all() == (cross != "flagged")
    # the degeneracy-free product matches the data
    fit = gain_refs.apply_gains(rr.model(Ugot, group), _per_row(got, d.shape[1]), a1, a2)
    assert np.abs(fit - d)[w > 0].max() <= 1e-8


def test_reference_chi2_reaches_the_noise_floor():
    noise = 0.01
    d, w, g, U, a1, a2, group, ngroups, ants = red_case(False, noise, seed=3, per_time=True)
    g0 = np.ones_like(g)
    _, _, changes, chi2, _, _ = rr.solve(d, w, g0, a1, a2, group, ngroups, True, 400, 1e-10)
    expected = noise**2 * (len(a1) - ngroups - len(ants) + 2)
    print("redundant reference: chi2 / (noise^2 dof)", len(changes), (chi2 / expected).ravel())
    assert len(changes) < 400
    assert np.all(chi2 >= 0.5 * expected) and np.all(chi2 <= 1.5 * expected)


def test_reference_per_time_units_are_independent_solves():
    d, w, g, U, a1, a2, group, ngroups, _ = red_case(True, 0.05, seed=2)
    g0 = np.ones(d.shape[:2] + g.shape[2:], dtype=complex)
    got, Ugot, changes, chi2, solved, _ = rr.solve(d, w, g0, a1, a2, group, ngroups, True, 7, 0.0)
    assert len(changes) == 7 and changes[0].shape == d.shape[:2] and solved.all()
    one = rr.solve(d[1:, :1], w[1:, :1], g0[1:, :1], a1, a2, group, ngroups, True, 7, 0.0)
    assert np.array_equal(one[0], got[1:, :1]) and np.array_equal(one[1], Ugot[1:, :1]) and np.array_equal(one[3], chi2[1:, :1])


def test_a_group_without_a_used_sample_keeps_zero():
    d, w, g, U, a1, a2, group, ngroups, _ = red_case(False, 0.0, seed=4)
    w[0, 1, group == 5] = 0
    d[0, 1, group == 5] = np.nan
    _, Ugot, _, chi2, solved, vis_solved = rr.solve(d, w, np.ones_like(g), a1, a2, group, ngroups, False, 5, 0.0)
    assert not vis_solved[0, 1, 5] and vis_solved.sum() == vis_solved.size - 1 and Ugot[0, 1, 5] == 0
    assert np.isfinite(Ugot).all() and np.isfinite(chi2).all() and solved.all()
    # the U-step alone keeps the value passed in
    U0 = np.full(Ugot.shape, 3 - 2j)
    U1, den = rr.vis_step(d, w, _per_row(g, 2), a1, a2, group, ngroups, U0)
    assert U1[0, 1, 5] == 3 - 2j and den[0, 1, 5] == 0 and (den > 0).sum() == den.size - 1
    assert np.abs(U1 - U)[den > 0].max() <= 1e-13  # (at the true gains the average is the true visibility)


# ---- the groups ------------------------------------------------------------------------------------------------------------
def test_redundant_groups():
    ants = hex19()
    reds, bls, group = fftvis_amd.redundant_groups(ants)
    assert reds == fftvis_amd.core.utils.get_pos_reds(ants, include_autos=False)
    assert bls == [bl for red in reds for bl in red] and len(bls) == 171 and len(reds) == 30
    assert group.dtype == np.int32 and np.array_equal(group, [r for r, red in enumerate(reds) for _ in red])
    # a list is taken as it stands
    some = [reds[3][1], reds[0][0], reds[3][0]]
    reds2, bls2, group2 = fftvis_amd.redundant_groups(ants, some)
    assert reds2 == reds and bls2 == some and group2.tolist() == [3, 0, 3]
    # a reversed baseline raises, and says what to do
    i, j = reds[2][1]
    with pytest.raises(ValueError, match=re.escape(f"baseline {(j, i)} is in its redundant group as {(i, j)}: swap the pair and "
                                                   "conjugate the datum (transposing [x, y] when polarized)")):
        fftvis_amd.redundant_groups(ants, [reds[0][0], (j, i)])
    with pytest.raises(ValueError, match="names an antenna that is not a key of ants"):
        fftvis_amd.redundant_groups(ants, [(0, 99)])
    # an auto gets a group of its own
    reds3, bls3, group3 = fftvis_amd.redundant_groups(ants, [reds[1][0], (4, 4), (7, 7), (4, 4)])
    assert group3.tolist() == [1, 30, 31, 30] and reds3[:30] == reds and reds3[30:] == [[(4, 4)], [(7, 7)]]


# ---- the degeneracies ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tilt", ["per_feed", "shared"])
def test_degeneracies_are_fixed_against_the_originals(tilt):
    rng = np.random.default_rng(7)
    ants = hex19()
    pos = np.array(list(ants.values()))
    nant, nf, nt = len(ants), 3, 2
    g = 1 + 0.2 * (rng.normal(size=(nant, 2, nf, nt)) + 1j * rng.normal(size=(nant, 2, nf, nt)))
    amp = rng.uniform(0.5, 2.0, size=(2, nf, nt))
    psi = rng.uniform(-1.0, 1.0, size=(2, nf, nt))
    reach = np.abs(pos - pos.mean(axis=0)).sum(axis=1).max()
    Phi = rng.uniform(-1.0, 1.0, size=(3, 1 if tilt == "shared" else 2, nf, nt)) * 0.9 / reach  # |Phi . x| < 1 rad
    x = pos - pos.mean(axis=0)
    moved = g * amp * np.exp(1j * (psi + np.einsum("ai,ifnt->afnt", x, np.broadcast_to(Phi, (3, 2, nf, nt)))))
    assert np.abs(np.einsum("ai,ifnt->afnt", x, np.broadcast_to(Phi, (3, 2, nf, nt)))).max() < 1 and np.abs(moved - g).max() > 0.1
    fixed = fftvis_amd.fix_redundant_degeneracies(moved, ants, ref_gains=g, tilt=tilt)
    print("degeneracies fixed", tilt, float(np.abs(fixed - g).max()))
    assert fixed.shape == g.shape and fixed.dtype == np.complex128 and np.abs(fixed - g).max() <= 1e-12
    # antennas that were not solved stay as they are and do not enter the fits
    solved = np.ones(g.shape, dtype=bool)
    solved[3] = False
    moved[3] = 5.0
    fixed = fftvis_amd.fix_redundant_degeneracies(moved, ants, ref_gains=g, solved=solved, tilt=tilt)
    assert np.all(fixed[3] == 5.0) and np.abs(fixed - g)[solved].max() <= 1e-12
    # time-constant unpolarized gains, and ones as the reference
    flat = fftvis_amd.fix_redundant_degeneracies(moved[:, 0, :, 0] / g[:, 0, :, 0], ants, solved=solved[:, 0, :, 0])
    assert np.abs(flat - 1)[solved[:, 0, :, 0]].max() <= 1e-12
    with pytest.raises(ValueError, match='tilt must be "per_feed" or "shared"'):
        fftvis_amd.fix_redundant_degeneracies(g, ants, tilt="both")
    with pytest.raises(ValueError, match="one row per antenna"):
        fftvis_amd.fix_redundant_degeneracies(g[1:], ants)


@pytest.mark.parametrize("polarized", [False, True])
def test_fixing_the_degeneracies_leaves_chi2_where_it_was(polarized):
    """On parallel hands: the four numbers are free, so chi2 at (fixed gains, the U-step at them) is the chi2 before."""
    d, w, g, U, a1, a2, group, ngroups, ants = red_case(polarized, 0.05, seed=5, cross="flagged")
    got, Ugot, _, chi2, _, _ = rr.solve(d, w, np.ones_like(g), a1, a2, group, ngroups, False, 30, 0.0)
    public = np.ascontiguousarray(got.transpose(3, 2, 0, 1)).reshape((len(ants), 2, 2) if polarized else (len(ants), 2))
    truth = np.ascontiguousarray(g.transpose(3, 2, 0, 1)).reshape(public.shape)
    fixed = fftvis_amd.fix_redundant_degeneracies(public, ants, ref_gains=truth)
    assert np.abs(fixed - public).max() > 1e-3
    block = fixed.reshape(len(ants), -1, 2, 1).transpose(2, 3, 1, 0)
    rows = _per_row(block, d.shape[1])
    U2, _ = rr.vis_step(d, w, rows, a1, a2, group, ngroups)
    after = rr.chi2_rows(U2, d, w, rows, a1, a2, group)
    print("chi2 after fixing the degeneracies", polarized, float(np.abs(after - chi2).max() / chi2.max()))
    assert np.all(np.abs(after - chi2) <= 1e-12 * chi2)


# ---- the C surface ---------------------------------------------------------------------------------------------------------
_NEW = {"fv_redundant_vis_rows": 15, "fv_redundant_normal_rows": 16, "fv_redundant_solve": 25}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    flat = " ".join(header.split())
    for declared in ("int fv_redundant_vis_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, "
                     "const int *ant1, const int *ant2, int ngroups, const int *group, const void *gains, const void *data, "
                     "const void *weights, void *uvis, double *den);",
                     "int fv_redundant_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, "
                     "const int *ant1, const int *ant2, int ngroups, const int *group, const void *gains, const void *uvis, "
                     "const void *data, const void *weights, void *num, double *den);",
                     "int fv_redundant_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, "
                     "const int *ant1, const int *ant2, int ngroups, const int *group, int per_time, const void *data, "
                     "int data_on_device, const void *weights, int weights_on_device, void *gains, void *uvis_out, int max_iter, "
                     "double tol, int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, "
                     "int *vis_solved_out);"):
        assert declared in flat, declared
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    flat = flat.replace(" * ", " ")
    for stated in ("V'[row, pol, k] = conj(g[p, ant1]) g[q, ant2] U[row, pol, group[k]]",
                   "num = sum w conj(m) d den = sum w |m|^2 U = num / den where den > 0, else U keeps its value",
                   "V = U[row, pol, group[k]]", "g <- g^ for odd i and (g^ + g) / 2 for even i", "starts from 0",
                   "one more U-step at the returned gains"):
        assert stated in flat, stated


def test_public_signatures():
    own = inspect.signature(redundant.redundant_gain_solve).parameters
    assert list(own) == ["data", "ants", "reds", "baselines", "gains", "per_time", "weights", "max_iter", "tol", "ref_ant",
                         "polarized", "precision", "device"]
    defaults = dict(reds=None, baselines=None, gains=None, per_time=False, weights=None, max_iter=200, tol=1e-8, ref_ant=None,
                    polarized=False, precision=2, device=0)
    assert all(own[n].kind.name == "KEYWORD_ONLY" and own[n].default == v for n, v in defaults.items())
    avg = inspect.signature(redundant.redundant_average).parameters
    assert list(avg) == ["data", "ants", "gains", "reds", "baselines", "weights", "polarized", "precision", "device"]
    assert all(avg[n].kind.name == "KEYWORD_ONLY" for n in list(avg)[3:])
    fix = inspect.signature(redundant.fix_redundant_degeneracies).parameters
    assert list(fix) == ["gains", "ants", "ref_gains", "solved", "tilt"] and fix["tilt"].default == "per_feed"
    assert list(inspect.signature(redundant.redundant_groups).parameters) == ["ants", "baselines", "decimals"]
    for name in ("redundant_groups", "redundant_gain_solve", "redundant_average", "fix_redundant_degeneracies"):
        assert getattr(fftvis_amd, name) is getattr(redundant, name)
    doc = " ".join(redundant.redundant_gain_solve.__doc__.split())
    for word in ("simulate_vis(..., baselines=[red[0] for red in reds])", "firstcal", "Jones matrices", "near-redundancy",
                 "a joint sky and redundant solve", "sharding", "flag them"):
        assert word in doc, word
    assert "(-pi, pi)" in redundant.fix_redundant_degeneracies.__doc__ and "no unwrapping" in redundant.fix_redundant_degeneracies.__doc__


def test_python_argument_errors_come_before_the_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ants = hex19()
    d = np.zeros((2, 2, 171), complex)
    call = fftvis_amd.redundant_gain_solve
    with pytest.raises(ValueError, match=re.escape("data must have shape (nfreqs, ntimes, nbls), got (2, 171)")):
        call(d[0], ants)
    with pytest.raises(ValueError, match=re.escape("data must have shape (nfreqs, ntimes, 2, 2, nbls), got (2, 2, 171)")):
        call(d, ants, polarized=True)
    with pytest.raises(ValueError, match="data holds 170 baselines, baselines lists 171"):
        call(d[..., :170], ants)
    with pytest.raises(ValueError, match=re.escape("weights must have data's shape (2, 2, 171), got (2, 171)")):
        call(d, ants, weights=np.ones((2, 171)))
    with pytest.raises(ValueError, match="weights must be real"):
        call(d, ants, weights=np.ones(d.shape, complex))
    with pytest.raises(ValueError, match=re.escape("gains must have shape (19, 2) or (19, 2, 2), got (19,)")):
        call(d, ants, gains=np.ones(19, complex))
    with pytest.raises(ValueError, match="per_time=True needs per-time gains"):
        call(d, ants, gains=np.ones((19, 2), complex), per_time=True)
    with pytest.raises(ValueError, match="ref_ant must be a key of ants, got 1000"):
        call(d, ants, ref_ant=1000)
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match="max_iter must be a positive integer"):
            call(d, ants, max_iter=bad)
    with pytest.raises(ValueError, match="tol must be non-negative"):
        call(d, ants, tol=-1.0)
    with pytest.raises(ValueError, match="precision must be 1 or 2"):
        call(d, ants, precision=3)
    with pytest.raises(ValueError, match="gains must be complex"):
        fftvis_amd.redundant_average(d, ants, np.ones((19, 2)))


def _check_shared(L, call, name):
    a = (ctypes.c_int * 3)(0, 1, 2)
    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and name + b": tpol must be 1 or 4" in L.fv_last_error()
    assert call(nbls=-1) == 1 and name + b": negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and name + b": nant must be positive" in L.fv_last_error()
    for bad in (0, -2):
        assert call(ngroups=bad) == 1 and name + b": ngroups must be positive" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, low), (high, a), (a, high)]:
        assert call(a1=a1, a2=a2, tpol=4) == 1 and name + b": antenna index outside [0, nant)" in L.fv_last_error()
    for grp in (low, high):
        assert call(group=grp) == 1 and name + b": group index outside [0, ngroups)" in L.fv_last_error()


def test_fv_redundant_rows_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)

    def vis(precision=2, nrows=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, ngroups=3, group=a, g=buf, d=buf, u=buf, den=buf):
        return L.fv_redundant_vis_rows(0, precision, nrows, nbls, tpol, nant, a1, a2, ngroups, group, g, d, None, u, den)

    def normal(precision=2, nrows=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, ngroups=3, group=a, g=buf, u=buf, d=buf, num=buf, den=buf):
        return L.fv_redundant_normal_rows(0, precision, nrows, nbls, tpol, nant, a1, a2, ngroups, group, g, u, d, None, num, den)

    _check_shared(L, vis, b"fv_redundant_vis_rows")
    _check_shared(L, normal, b"fv_redundant_normal_rows")
    assert vis(nrows=-1) == 1 and b"fv_redundant_vis_rows: negative shape" in L.fv_last_error()
    assert normal(nrows=-1) == 1 and b"fv_redundant_normal_rows: negative shape" in L.fv_last_error()
    for kw in (dict(g=None), dict(u=None), dict(den=None)):
        assert vis(**kw) == 1 and b"fv_redundant_vis_rows: null gains, uvis or den" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(group=None), dict(d=None)):
        assert vis(**kw) == 1 and b"fv_redundant_vis_rows: null pairs, group or data" in L.fv_last_error()
    for kw in (dict(g=None), dict(num=None), dict(den=None)):
        assert normal(**kw) == 1 and b"fv_redundant_normal_rows: null gains, num or den" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(group=None), dict(u=None), dict(d=None)):
        assert normal(**kw) == 1 and b"fv_redundant_normal_rows: null pairs, group, uvis or data" in L.fv_last_error()
    # no baseline: den 0 and U as passed in; zeros -- without a device
    u, den = np.full((2, 1, 3), 3 - 2j), np.full((2, 1, 3), 7.0)
    assert L.fv_redundant_vis_rows(0, 2, 2, 0, 1, 3, None, None, 3, None, buf, None, None, _lib.ptr(u), _lib.ptr(den)) == 0
    assert np.all(u == 3 - 2j) and np.all(den == 0)
    num, den = np.full((2, 1, 3), 7.0, dtype=complex), np.full((2, 1, 3), 7.0)
    assert L.fv_redundant_normal_rows(0, 2, 2, 0, 1, 3, None, None, 3, None, buf, None, None, None, _lib.ptr(num), _lib.ptr(den)) == 0
    assert np.all(num == 0) and np.all(den == 0)


def test_fv_redundant_solve_argument_checks():
    L = _lib.lib()
    fn = L.fv_redundant_solve
    name = b"fv_redundant_solve"
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    niter = (ctypes.c_int * 1)(-1)

    def call(precision=2, nfreqs=1, ntimes=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, ngroups=3, group=a, per_time=0, d=buf, flags=(0, 0),
             g=buf, u=buf, max_iter=5, tol=1e-8, n=niter, change=buf, chi2=buf, solved=buf, vis_solved=buf):
        return fn(0, precision, nfreqs, ntimes, nbls, tpol, nant, a1, a2, ngroups, group, per_time, d, flags[0], None, flags[1], g, u,
                  max_iter, tol, n, change, chi2, solved, vis_solved)

    _check_shared(L, call, name)
    for kw in (dict(nfreqs=-1), dict(ntimes=-1)):
        assert call(**kw) == 1 and name + b": negative shape" in L.fv_last_error()
    for bad in (0, -1):
        assert call(max_iter=bad) == 1 and name + b": max_iter must be positive" in L.fv_last_error()
    for bad in (-1e-9, float("nan")):
        assert call(tol=bad) == 1 and name + b": tol must be non-negative" in L.fv_last_error()
    for kw in (dict(per_time=2), dict(flags=(2, 0)), dict(flags=(0, -1))):
        assert call(**kw) == 1 and name + b": per_time and the on_device flags must be 0 or 1" in L.fv_last_error()
    assert call(n=None) == 1 and name + b": null niter_out" in L.fv_last_error()
    for kw in (dict(g=None), dict(u=None), dict(change=None), dict(chi2=None), dict(solved=None), dict(vis_solved=None)):
        assert call(**kw) == 1 and name + b": null gains, uvis_out, change_out, chi2_ft_out, solved_out or vis_solved_out" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(group=None), dict(d=None)):
        assert call(**kw) == 1 and name + b": null pairs, group or data" in L.fv_last_error()
    assert niter[0] == -1  # (nothing ran)
    # no baseline: the start gains, U = 0, chi2 0, nothing solved, without a device
    g = np.arange(2 * 3 * 2 * 3, dtype=complex).reshape(2, 3, 2, 3) + 1j
    start = g.copy()
    change, chi2, solved = np.full((2, 3), 7.0), np.full((2, 3), 7.0), np.full(g.shape, 7, dtype=np.int32)
    u, vis_solved = np.full((2, 3, 4, 5), 7.0, dtype=complex), np.full((2, 3, 4, 5), 7, dtype=np.int32)
    assert fn(0, 1, 2, 3, 0, 4, 3, None, None, 5, None, 1, None, 0, None, 0, _lib.ptr(g), _lib.ptr(u), 5, 0.0, niter, _lib.ptr(change),
              _lib.ptr(chi2), _lib.ptr(solved), _lib.ptr(vis_solved)) == 0, L.fv_last_error()
    assert niter[0] == 0 and np.array_equal(g, start) and not change.any() and not chi2.any() and not solved.any()
    assert not u.any() and not vis_solved.any()
