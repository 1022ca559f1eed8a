"""GPU tests of abscal (``redundant_abscal``; ``fv_abscal_slopes`` and ``fv_abscal_evaluate`` alone).

The device is held to the numpy reference on the same inputs (``abscal_refs``, whose docstring derives the bounds, each for
one implementation: two differ by at most twice as much).  The six sums of an evaluation agree within twice their bounds.
The coarse peak must be a grid point whose reference value is the largest within 2 e, e the bound of one grid value -- the
reference's own peak, or a point that ties with it.  The refined slope must agree, within the reference's ``slope_bound``,
with the reference's refinement FROM THE DEVICE'S PEAK.  Re S at the result: twice the bound of f, plus what the slope's bound
may move it by, ``|g| B + |H| B^2 / 2``; eta = Re S / N adds N's relative error; N and P, sums of nt ngroups non-negative terms
of three products each, agree to ``(nt + ngroups + 8) 2^-52`` of themselves.  chi2 is compared at the device's own
parameters, within ``abscal_refs.chi2_bound``.  A complex64 model is rounded before either side sees it."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import abscal_refs as ar
from tests import gain_refs
from tests import redundant_refs as rr
from tests.helpers import rel_l2
from tests.test_abscal_host import array, group_baselines
from tests.test_gpu_gains import CDT

pytestmark = pytest.mark.gpu

EPS = 2.0**-52
LDS_GROUPS = 32768 // 80  # the largest ngroups whose rows k_abscal_refine stages in LDS


def _rows(x, tpol):
    """A block (nf, nt, [2, 2,] ngroups) as the library reads it: (nf, nt, tpol, ngroups)."""
    return None if x is None else np.ascontiguousarray(x.reshape(x.shape[:2] + (tpol, x.shape[-1])))


def _device(bufs):
    import torch

    tensors = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
    torch.cuda.synchronize()
    return tensors, [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in tensors]


def _slopes(U, M, W, X, n, h, refine, per_time, precision, on_device=False, expect=0):
    """One ``fv_abscal_slopes`` call: a dict of the outputs, ``(nfreqs, ntu, nfeed, ...)`` and ``chi2`` ``(nfreqs, ntimes)``."""
    tpol = 4 if U.ndim == 5 else 1
    u, m = _rows(U.astype(np.complex128), tpol), _rows(M.astype(CDT[precision]), tpol)
    w = None if W is None else _rows(np.asarray(W, dtype=np.float64), tpol)
    nf, nt, ng = u.shape[0], u.shape[1], u.shape[-1]
    units = (nf, nt if per_time else 1, 2 if tpol == 4 else 1)
    outs = dict(peak=np.full(units + (2,), 7, dtype=np.int32), slopes=np.full(units + (2,), 7.0), amp=np.full(units, 7.0),
                power=np.full(units, 7.0), unorm=np.full(units, 7.0), mnorm=np.full(units, 7.0), used=np.full(units, 7, dtype=np.int32),
                chi2=np.full((nf, nt), 7.0))
    before = [None if b is None else b.copy() for b in (u, m, w)]
    keep, ptrs = _device([u, m, w]) if on_device else (None, [_lib.ptr(u), _lib.ptr(m), _lib.ptr(w)])
    coords = np.ascontiguousarray(X, dtype=np.float64)
    status = _lib.lib().fv_abscal_slopes(0, precision, nf, nt, tpol, ng, int(per_time), ptrs[0], int(on_device), ptrs[1], int(on_device),
                                         ptrs[2], int(on_device), _lib.ptr(coords), X.shape[1], n[0], n[1], float(h[0]), float(h[1]), refine,
                                         *[_lib.ptr(outs[k]) for k in ("peak", "slopes", "amp", "power", "unorm", "mnorm", "used", "chi2")])
    assert status == expect, _lib.lib().fv_last_error()
    if on_device:
        for t, b in zip(keep, before):  # the caller's blocks are unchanged
            assert t is None or np.array_equal(t.cpu().numpy(), b, equal_nan=True)
    for a, b in zip((u, m, w), before):
        assert a is None or np.array_equal(a, b, equal_nan=True)
    outs["error"] = _lib.lib().fv_last_error() if status else b""
    return outs


def _check_fit(label, U, M, W, X, n, h, refine, per_time, precision, got):
    """``fv_abscal_slopes``' outputs against the reference, by the module's docstring.  Returns the number of rows whose peak
    differs from the reference's."""
    Mr = M.astype(CDT[precision]).astype(np.complex128)
    ref = ar.abscal(U, Mr, W, X, n, h, refine, per_time, peak=got["peak"])
    used = got["used"] != 0
    assert np.array_equal(used, ref["used"]), label
    nt_u, ng = 1 if per_time else U.shape[1], U.shape[-1]
    # the coarse peak
    i1, i2 = got["peak"][..., 0] + (n[0] - 1) // 2, got["peak"][..., 1] + (n[1] - 1) // 2
    assert np.all((i1 >= 0) & (i1 < n[0]) & (i2 >= 0) & (i2 < n[1])), label
    y = ref["y"].reshape(ref["y"].shape[:-2] + (-1,))
    at = np.take_along_axis(y, (i1 * n[1] + i2)[..., None], axis=-1)[..., 0]
    with np.errstate(all="ignore"):
        short = np.where(used, (y.max(axis=-1) - at) / ref["e"], 0.0)
    differs = int((used & (got["peak"] != ref["j"]).any(axis=-1)).sum())
    # the refinement
    dphi = np.abs(got["slopes"] - ref["phi"]).max(axis=-1)
    s = ref["sums"].astype(np.float64)
    fb = ar.evaluate(ref["prod"]["c"], X, ref["phi"], a=ref["prod"]["a"], extra=nt_u + 4)[1][..., 0]
    B = np.where(np.isfinite(ref["slope_bound"]), ref["slope_bound"], 0.0)
    moved = (np.abs(s[..., 1]) + np.abs(s[..., 2])) * B + 0.5 * (np.abs(s[..., 3]) + 2 * np.abs(s[..., 4]) + np.abs(s[..., 5])) * B**2
    power_tol = 2 * fb + moved
    sum_tol = (nt_u + ng + 8) * EPS
    amp_tol = np.where(used, got["amp"] * (power_tol / np.where(used, s[..., 0], 1) + sum_tol), 0.0)
    chi2, power, t_max = ar.chi2_rows(U, Mr, W, X, got["amp"], got["slopes"], per_time)
    chi2_tol = ar.chi2_bound(chi2, power, t_max, (2 if U.ndim == 5 else 1) * ng)
    with np.errstate(all="ignore"):
        ratio = np.where(ref["slope_bound"] > 0, dphi / ref["slope_bound"], 0.0)
    print(f"abscal {label}: rows {used.size}, used {int(used.sum())}, peaks that differ from the reference's {differs}, worst shortfall / e "
          f"{float(short.max()):.3g}, |dphi| / bound {float(ratio.max()):.3g}, largest "
          f"finite bound {float(B.max()):.3g}, rows with an infinite bound {int((~np.isfinite(ref['slope_bound'])).sum())}, |dpower| / tol "
          f"{float(np.max(np.abs(got['power'] - ref['power']) / np.where(used, power_tol, 1))):.3g}, |dchi2| / tol "
          f"{float(np.max(np.abs(got['chi2'] - chi2) / np.where(chi2_tol > 0, chi2_tol, 1))):.3g}")
    assert np.all(short <= 2.0), label
    assert np.all(dphi <= ref["slope_bound"]), label
    assert np.all(np.abs(got["power"] - ref["power"]) <= np.where(used, power_tol, 0.0)), label
    assert np.all(np.abs(got["amp"] - ref["amp"]) <= amp_tol), label
    assert np.all(np.abs(got["unorm"] - ref["N"]) <= sum_tol * ref["N"]) and np.all(np.abs(got["mnorm"] - ref["P"]) <= sum_tol * ref["P"]), label
    assert np.all(np.abs(got["chi2"] - chi2) <= chi2_tol), label
    # rows that are not used are exactly neutral
    off = ~used
    assert np.all(got["amp"][off] == 1.0) and not got["slopes"][off].any() and not got["peak"][off].any() and not got["power"][off].any()
    return differs, ref


def _coords(rng, ng, ndim):
    """Random in-plane baselines of 14 .. 300 m, with two equal and two opposite ones where there is room."""
    X = rng.uniform(-300, 300, (ng, ndim))
    X[np.abs(X).sum(axis=1) < 14] += 14
    if ng >= 4:
        X[1], X[3] = X[0], -X[2]
    return X


def _cn(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


# ---- 1. the evaluation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [1, 2])
@pytest.mark.parametrize("ng", [1, 2, 63, 64, 65, 257, LDS_GROUPS, LDS_GROUPS + 1, 1000])
def test_evaluate(ng, ndim):
    rng = np.random.default_rng(100 * ng + ndim)
    X = _coords(rng, ng, ndim)
    nrows = 7  # two blocks of four waves, the second one short
    truth = rng.uniform(-0.01, 0.01, (nrows, 2))
    x1, x2 = ar._xy(X, np.float64)
    c = rng.uniform(0.5, 1.5, (nrows, ng)) * np.exp(-1j * (truth[:, :1] * x1 + truth[:, 1:] * x2))
    c[3] = _cn(rng, ng)
    phi = rng.uniform(-0.02, 0.02, (nrows, 2))
    phi[0], phi[1], phi[2] = 0.0, truth[1], truth[2]
    out = np.full((nrows, 6), 7.0)
    before = c.copy()
    assert _lib.lib().fv_abscal_evaluate(0, nrows, ng, _lib.ptr(c), _lib.ptr(X), ndim, _lib.ptr(phi), _lib.ptr(out)) == 0, _lib.lib().fv_last_error()
    ref, bound = ar.evaluate(c, X, phi if ndim == 2 else phi * [1, 0])
    worst = np.abs(out - ref) / np.where(bound > 0, 2 * bound, 1)
    print(f"abscal evaluate ng {ng} ndim {ndim}: worst |d| / (2 bound) per sum {np.round(worst.max(axis=0), 3).tolist()}")
    assert np.array_equal(c, before) and np.all(np.abs(out - ref) <= 2 * bound)
    assert np.all(ref[1:3, 0] >= 0.999 * np.abs(c[1:3]).sum(axis=-1))  # (at the truth every term is in phase)
    if ndim == 1:
        assert not out[:, [2, 4, 5]].any()


# ---- 2. the search ------------------------------------------------------------------------------------------------------------
def _planted_case(rng, X, n, h, nt, polarized, noise=0.0):
    """Four frequencies: the truth exactly on a grid point, half-way between two, at the box's edge, and random inside the
    box; eta in 0.5 .. 2; random positive weights."""
    ng, ndim = X.shape
    half = [(n[i] - 1) // 2 for i in range(2)]
    spot = np.array([[min(2, half[0]), -min(1, half[1])], [min(1, half[0]) - 0.5 * (half[0] > 0), 0.0], [half[0], -half[1]], [0.0, 0.0]])
    spot[3] = [rng.uniform(-half[0], half[0]), rng.uniform(-half[1], half[1])]
    phi = spot * np.array(h)
    if ndim == 1:
        phi[:, 1] = 0
    x1, x2 = ar._xy(X, np.float64)
    theta = phi[:, :1] * x1 + phi[:, 1:] * x2  # (4, ng)
    pol = (2, 2) if polarized else ()
    shape = (4, nt) + pol + (ng,)
    M = _cn(rng, shape)
    eta = rng.uniform(0.5, 2.0, 4)
    lead = (4,) + (1,) * (len(shape) - 2)
    U = M * np.exp(1j * theta).reshape(lead + (ng,)) / eta.reshape(lead + (1,)) + noise * _cn(rng, shape)
    return U, M, rng.uniform(0.5, 1.5, shape), phi, eta


GRIDS = [((1, 1), 2), ((3, 1), 1), ((19, 1), 1), ((19, 1), 2), ((15, 9), 2), ((55, 51), 2), ((301, 9), 2)]


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("n,ndim", GRIDS)
def test_search(n, ndim, precision):
    """(301, 9) has 602 runs, three tiles of 256, the last one short; ngroups lies on both sides of the staging chunk (512)
    and of a wave (64).  ``refine=0`` returns the grid point itself."""
    differs = 0
    for ng, polarized in ((63, False), (65, True), (511, False), (513, n != (55, 51))):
        rng = np.random.default_rng(n[0] * 1000 + n[1] + ng)
        X = _coords(rng, ng, ndim)
        extent = np.ptp(X, axis=0)
        h = [2 * np.pi / (4 * extent[0]), 2 * np.pi / (4 * extent[1]) if ndim == 2 else 1.0]
        U, M, W, phi, eta = _planted_case(rng, X, n, h, 2, polarized)
        got = _slopes(U, M, W, X, n, h, 0, False, precision)
        d, ref = _check_fit(f"search {n} ng {ng} polarized {polarized} precision {precision}", U, M, W, X, n, h, 0, False, precision, got)
        differs += d
        assert np.all(got["used"] == 1)
        assert np.array_equal(got["slopes"][..., 0], got["peak"][..., 0] * h[0])
        assert np.array_equal(got["slopes"][..., 1], got["peak"][..., 1] * h[1] if ndim == 2 else np.zeros(got["slopes"].shape[:-1]))
        want = np.round(phi / np.array(h)).astype(int)
        for f in (0, 2):  # on a grid point, and at the box's edge: that point (or one that ties with it within 2 e)
            if np.array_equal(ref["j"][f, 0, 0], want[f] * [1, ndim == 2]):
                assert np.array_equal(got["peak"][f], ref["j"][f])
    print(f"abscal search {n} precision {precision}: peaks that differ from the reference's {differs}")


# ---- 3. the refinement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("polarized", [False, True])
@pytest.mark.parametrize("ng,ndim,n", [(30, 2, (29, 25)), (LDS_GROUPS + 1, 2, (15, 9)), (5, 1, (17, 1)), (513, 1, (19, 1))])
def test_refinement(ng, ndim, n, polarized, precision):
    rng = np.random.default_rng(7 * ng + ndim)
    X = _coords(rng, ng, ndim)
    extent = np.ptp(X, axis=0)
    h = [2 * np.pi / (4 * extent[0]), 2 * np.pi / (4 * extent[1]) if ndim == 2 else 1.0]
    U, M, W, phi, eta = _planted_case(rng, X, n, h, 2, polarized, noise=0.02)
    got = _slopes(U, M, W, X, n, h, 6, False, precision)
    _, ref = _check_fit(f"refine ng {ng} ndim {ndim} polarized {polarized} precision {precision}", U, M, W, X, n, h, 6, False, precision, got)
    inside = [0, 1, 3]  # (the truth at the box's edge may be refined across it, where the lobe need not be concave)
    assert np.isfinite(ref["slope_bound"][inside]).all() and ref["slope_bound"][inside].max() < 1e-10
    assert np.all(np.abs(got["slopes"][inside, 0, :, :] - phi[inside, None, :]) <= 0.2 * np.array(h))
    assert np.all(np.abs(got["amp"][inside, 0] - eta[inside, None]) <= 0.05 * eta[inside, None])


# ---- 4. flags -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("polarized", [False, True])
def test_flags(polarized, precision):
    rng = np.random.default_rng(9)
    ng, n = 40, (15, 9)
    X = _coords(rng, ng, 2)
    X[5] = 0.0  # an auto-correlation's own group: never used, never read
    extent = np.ptp(X, axis=0)
    h = [2 * np.pi / (4 * extent[0]), 2 * np.pi / (4 * extent[1])]
    U, M, W, phi, eta = _planted_case(rng, X, n, h, 2, polarized)
    bad = complex(np.nan, np.inf)
    U[..., 5] = M[..., 5] = bad
    W[0, :, ..., 7:11] = 0  # flagged samples hold NaN and are not read
    U[0, :, ..., 7:11] = M[0, :, ..., 7:11] = bad
    W[0, 1, ..., 20] = 0
    M[0, 1, ..., 20] = bad
    W[1] = 0  # a unit with no used group
    U[1] = bad
    W[2, ..., :3], W[2, ..., 4:] = 0, 0  # a unit with a single group, its model minus its data
    M[2, ..., 3] = -U[2, ..., 3]
    got = _slopes(U, M, W, X, n, h, 6, False, precision)
    _check_fit(f"flags polarized {polarized} precision {precision}", U, M, W, X, n, h, 6, False, precision, got)
    assert np.all(got["used"][[0, 3]] == 1) and not got["used"][[1, 2]].any()
    assert np.all(got["amp"][[1, 2]] == 1.0) and not got["slopes"][[1, 2]].any() and not got["unorm"][1].any() and np.all(got["unorm"][2] > 0)
    assert np.isfinite(got["chi2"]).all() and not got["chi2"][1].any()
    # model = -data on every group of a box so small that Re S stays negative: enough groups, and still not used
    V = _cn(rng, U.shape)
    tiny = _slopes(V, -V, None, np.where(X == 0, 0, 1e-3 * X), (3, 3), [1e-3, 1e-3], 6, True, precision)
    assert not tiny["used"].any() and np.all(tiny["amp"] == 1.0) and not tiny["slopes"].any() and not tiny["power"].any() and np.all(tiny["unorm"] > 0)
    # bad input fails the call with the solve's messages
    for what, (Ub, Mb, Wb) in dict(weight=(U, M, np.where(np.arange(ng) == 30, -1.0, W)), weight_nan=(U, M, np.where(np.arange(ng) == 5, np.nan, W)),
                                   data=(np.where(np.arange(ng) == 30, bad, U), M, W), model=(U, np.where(np.arange(ng) == 30, bad, M), W)).items():
        err = _slopes(Ub, Mb, Wb, X, n, h, 6, False, precision, expect=1)["error"]
        want = {"weight": b"weights are negative or not finite", "weight_nan": b"weights are negative or not finite",
                "data": b"entries of data are not finite where the weight is positive", "model": b"values of the model are not finite"}[what]
        assert want in err, (what, err)


# ---- 5. the solve units -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polarized", [False, True])
@pytest.mark.parametrize("per_time", [False, True])
def test_units(per_time, polarized):
    rng = np.random.default_rng(13)
    ng, n = 70, (15, 9)
    X = _coords(rng, ng, 2)
    extent = np.ptp(X, axis=0)
    h = [2 * np.pi / (4 * extent[0]), 2 * np.pi / (4 * extent[1])]
    U, M, W, phi, eta = _planted_case(rng, X, n, h, 3, polarized, noise=0.05)
    W[1, 1] = 0  # one time of one unit flagged altogether
    got = _slopes(U, M, W, X, n, h, 6, per_time, 2)
    assert got["amp"].shape == (4, 3 if per_time else 1, 2 if polarized else 1)
    _check_fit(f"units per_time {per_time} polarized {polarized}", U, M, W, X, n, h, 6, per_time, 2, got)
    assert np.array_equal(got["used"][1, :, 0] != 0, [True, False, True] if per_time else [True])


# ---- 6. bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
def test_bits_repeat_and_device_blocks_give_the_host_blocks_bits(precision):
    rng = np.random.default_rng(17)
    ng, n = 600, (55, 51)
    X = _coords(rng, ng, 2)
    extent = np.ptp(X, axis=0)
    h = [2 * np.pi / (4 * extent[0]), 2 * np.pi / (4 * extent[1])]
    U, M, W, phi, eta = _planted_case(rng, X, n, h, 2, True, noise=0.1)
    first = _slopes(U, M, W, X, n, h, 6, False, precision)
    for other in (_slopes(U, M, W, X, n, h, 6, False, precision), _slopes(U, M, W, X, n, h, 6, False, precision, on_device=True)):
        for k, v in first.items():
            assert np.array_equal(v, other[k]), k


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def _chain_case(name, seed, polarized, nf=16, nt=2):
    """Every baseline of the array in group order; gains with cable delays (+-150 ns), phases in +-pi and amplitudes in 1 +- 0.1,
    constant in time; random group visibilities (the model) per channel and time; no noise."""
    from tests import firstcal_refs as fr

    rng = np.random.default_rng(seed)
    ants = array(name)
    reds, bls, group = fftvis_amd.redundant_groups(ants)
    a1, a2 = (np.array([bl[i] for bl in bls], dtype=np.int32) for i in (0, 1))
    freqs = 150e6 + 0.5e6 * np.arange(nf)
    nant, nfeed = len(ants), 2 if polarized else 1
    tau = rng.uniform(-150e-9, 150e-9, (nfeed, nant))
    c = rng.uniform(0.9, 1.1, (nfeed, nant)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (nfeed, nant)))
    g = fr.model_gains(c, tau, freqs)
    M = _cn(rng, (nf, nt) + ((2, 2) if polarized else ()) + (len(reds),))
    d = gain_refs.apply_gains(rr.model(M, group), np.broadcast_to(g, (nf, nt) + g.shape[2:]), a1, a2)
    return dict(ants=ants, reds=reds, freqs=freqs, d=d, M=M)


@pytest.mark.parametrize("name,polarized", [("hex19", False), ("hex19", True), ("line6", False)])
def test_chain_firstcal_solve_abscal(name, polarized):
    """firstcal -> redundant solve -> abscal against the planted group visibilities: the averaged data at the returned gains are
    the model.  The solve stops at a relative change of 1e-10; its linear convergence (40-56 iterations from a unit start on
    hex-19, a rate near 0.6) leaves an error of a few times that, and 1e-8 allows a hundred times.  Polarized, the cross-hand
    phase stays free (not covered): the parallel hands are compared."""
    import torch

    case = _chain_case(name, 21, polarized)
    kw = dict(polarized=polarized)
    g1, _, _ = fftvis_amd.redundant_firstcal(case["d"], case["ants"], case["freqs"], max_iter=2000, tol=1e-10, **kw)
    g2, vis, info = fftvis_amd.redundant_gain_solve(case["d"], case["ants"], gains=g1, max_iter=4000, tol=1e-10, **kw)
    assert info["converged"]
    # (on the hexagonal lattice the default box, +-pi / min |b| along the plane's axes, does not hold a whole cell of the
    # reciprocal lattice, whose corners lie at 4 pi / (3 a): the slope the solve left may have no alias inside it)
    kw_fit = dict(kw, max_slope=1.4 * np.pi / 14.6) if name == "hex19" else kw
    g3, fit = fftvis_amd.redundant_abscal(vis, case["M"], case["ants"], g2, **kw_fit)
    avg, _ = fftvis_amd.redundant_average(case["d"], case["ants"], g3, **kw)
    before, _ = fftvis_amd.redundant_average(case["d"], case["ants"], g2, **kw)
    hands = (lambda x: np.stack([x[:, :, 0, 0], x[:, :, 1, 1]])) if polarized else (lambda x: x)
    err, err0 = rel_l2(hands(avg), hands(case["M"])), rel_l2(hands(before), hands(case["M"]))
    print(f"abscal chain {name} polarized {polarized}: solve iterations {info['niter']}, grid {fit['grid']['n']}, averaged data against the "
          f"model: before {err0:.3e}, after {err:.3e}; chi2 / sum |M|^2 {float(fit['chi2'].sum() / (np.abs(hands(case['M'])) ** 2).sum()):.3e}")
    assert g3.shape == g2.shape and g3.dtype == np.complex128 and fit["used"].all() and fit["used"].shape == g2.shape[1:]
    assert fit["slopes"].shape == g2.shape[1:] + (3,) and np.abs(fit["slopes"][..., 2]).max() < 1e-12 and fit["chi2"].shape == (16, 2)
    assert err0 > 1e-3 and err <= 1e-8
    # device tensors in, device tensors out, with the host call's bits
    tg, tfit = fftvis_amd.redundant_abscal(torch.from_numpy(vis).cuda(), torch.from_numpy(case["M"]).cuda(), case["ants"], torch.from_numpy(g2), **kw_fit)
    assert tg.is_cuda and tfit["amp"].is_cuda and tfit["chi2"].is_cuda and np.array_equal(tg.cpu().numpy(), g3)
    for k in ("amp", "slopes", "chi2", "used", "peak", "power", "unorm", "mnorm"):
        assert np.array_equal(tfit[k].cpu().numpy(), fit[k]), k
