"""GPU tests of firstcal (``redundant_firstcal``; ``fv_firstcal_pair_delays`` and ``fv_firstcal_offsets`` alone).

Stage 1 is held to the numpy reference on the same inputs (``firstcal_refs``, whose docstring derives the bounds): the
coarse bin must be one whose reference power is the largest within 2 e, e the bound of one power -- the reference's own
peak, or a bin that ties with it, as two bins next to a delay half-way between them do --; the refined x must agree, within
the reference's ``x_bound``, with the reference's refinement from that bin (the bound is infinite where three points of a
round are equal within the rounding, as at ND = 2 with a delay between the two bins: the rule ``den < 0`` may then go either
way); the power at x within 2 e, e for the rounding on either side, plus the power's largest slope times the bound of x; the
total within (nfreqs + ntimes + 8) eps of itself, a sum of moduli.
Stage 2 is the redundant solve on the derotated block and is held to ``test_gpu_redundant``'s bounds; the derotation adds to
the chi2 bound what it may move a datum by: 8 u |d| in fp64 (sincos and a complex product, on either side), and one unit in
the last place of fp32, 2^-23 |d|, where the derotated datum is rounded to fp32 and the two fp64 values straddle a rounding
boundary; by Cauchy-Schwarz the row's chi2 moves by at most 2 k sqrt(sum w |d|^2 / chi2) relative."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import firstcal_refs as fr
from tests import gain_solve_refs as gsr
from tests import redundant_refs as rr
from tests.helpers import rel_l2
from tests.test_firstcal_host import FREQS, array, fc_case, outside_null_space
from tests.test_gpu_gain_solve import _chi2_bound
from tests.test_gpu_gains import BOUND, CDT, RDT

pytestmark = pytest.mark.gpu

EPS = 2.0**-52


def _rows(x, tpol):
    """A block (nf, nt, [2, 2,] nbls) as the library reads it: (nf, nt, tpol, nbls), pol = 2 q + p for the block's [q, p]."""
    return None if x is None else np.ascontiguousarray(x.reshape(x.shape[:2] + (tpol, x.shape[-1])))


def _device(bufs):
    import torch

    tensors = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
    torch.cuda.synchronize()
    return tensors, [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in tensors]


# ---- 1. the pair delays ----------------------------------------------------------------------------------------------------
def _pd_case(name, nf, nt, pad, polarized, flags, seed=0):
    """Data with a chosen delay for every pair: ``d[f, t, k] = U[f, t, group[k]] A[k] exp(2 pi i f phi[k])`` and along a group's
    members ``phi`` steps down by x / ND, x the pair's target bin.  The first pairs get: a bin exactly (3, or 1 where ND <= 6),
    a point exactly between two bins (-1.5), ND / 2 - 0.7 and -ND / 2 + 0.3 (within one bin of the ends); the others are uniform
    in +-0.45 ND.  With ``flags``: positive random weights, the mid-band channel flagged (nf >= 3) with NaN data, one baseline
    flagged altogether with NaN data, and one baseline turned into an auto-correlation."""
    rng = np.random.default_rng(seed + 7 * nf + pad)
    ants = array(name)
    reds, bls, group = fftvis_amd.redundant_groups(ants)
    a1 = np.array([bl[0] for bl in bls], dtype=np.int32)
    a2 = np.array([bl[1] for bl in bls], dtype=np.int32)
    pair1, pair2 = fr.pairs(group)
    nbls, npairs, nd, nfeed = len(bls), len(pair1), pad * nf, 2 if polarized else 1
    target = rng.uniform(-0.45 * nd, 0.45 * nd, (nfeed, npairs))
    target[:, :4] = [3.0 if nd > 6 else 1.0, -1.5, nd / 2 - 0.7, -nd / 2 + 0.3]
    phi = rng.uniform(-0.5, 0.5, (nfeed, nbls))
    for i in range(npairs):  # (pairs of a group come in the order of its members)
        phi[:, pair2[i]] = phi[:, pair1[i]] - target[:, i] / nd
    f = np.arange(nf)[:, None, None]

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    amp = (1 + 0.2 * c((nfeed, nbls)))
    U = c((nf, nt, nfeed, len(reds)))
    hands = [U[:, :, p][:, :, group] * amp[p] * np.exp(2j * np.pi * f * phi[p]) for p in range(nfeed)]
    if polarized:
        d = c((nf, nt, 2, 2, nbls))
        d[:, :, 0, 0], d[:, :, 1, 1] = hands
    else:
        d = hands[0]
    w, lost = None, np.zeros(npairs, dtype=bool)
    if flags:
        w = rng.uniform(0.5, 2.0, d.shape)
        big = np.flatnonzero(np.bincount(group) >= 4)[0]
        k_flag, k_auto = np.flatnonzero(group == big)[[1, 3]]
        w[..., k_flag] = 0
        d[..., k_flag] = complex(np.nan, np.inf)
        a2[k_auto] = a1[k_auto]
        lost = np.isin(pair1, (k_flag, k_auto)) | np.isin(pair2, (k_flag, k_auto))
        if nf >= 3:
            w[nf // 2] = 0
            d[nf // 2] = np.nan
    return dict(d=d, w=w, a1=a1, a2=a2, group=group, pair1=pair1, pair2=pair2, target=target, lost=lost, nd=nd, tpol=4 if polarized else 1)


def _pair_delays(case, precision, pad, on_device=False):
    d, w = _rows(case["d"].astype(CDT[precision]), case["tpol"]), None if case["w"] is None else _rows(case["w"].astype(RDT[precision]), case["tpol"])
    nf, nt = d.shape[:2]
    nfeed, npairs = (2 if case["tpol"] == 4 else 1), len(case["pair1"])
    outs = [np.full((nfeed, npairs), 7, dtype=np.int32), np.full((nfeed, npairs), 7.0), np.full((nfeed, npairs), 7.0),
            np.full((nfeed, npairs), 7.0), np.full((nfeed, npairs), 7, dtype=np.int32)]
    keep, ptrs = _device([d, w]) if on_device else (None, [_lib.ptr(d), _lib.ptr(w)])
    status = _lib.lib().fv_firstcal_pair_delays(0, precision, nf, nt, d.shape[-1], case["tpol"], npairs, _lib.ptr(case["pair1"]),
                                                _lib.ptr(case["pair2"]), _lib.ptr(case["a1"]), _lib.ptr(case["a2"]), ptrs[0], int(on_device),
                                                ptrs[1], int(on_device), pad, *[_lib.ptr(o) for o in outs])
    assert status == 0, _lib.lib().fv_last_error()
    del keep
    return outs


def _reference_z(case, precision):
    """The products from the inputs as ``precision`` rounds them."""
    d = case["d"].astype(CDT[precision]).astype(np.complex128)
    w = None if case["w"] is None else case["w"].astype(RDT[precision]).astype(np.float64)
    return fr.products(d, w, case["a1"], case["a2"], case["pair1"], case["pair2"])[0]


def _check_pair_delays(label, case, precision, pad, outs):
    peak, x, power, total, used = outs
    z = _reference_z(case, precision)
    ref = fr.pair_delays(z, pad)
    nf, nt, nd = z.shape[-1], case["d"].shape[1], case["nd"]
    assert np.array_equal(used != 0, ref["used"])
    assert np.all(np.abs(total - ref["total"]) <= (nf + nt + 8) * EPS * ref["total"])
    # the coarse bin: a bin of the largest reference power within what the rounding allows
    n = np.where(peak < 0, peak + nd, peak)
    assert np.all((n >= 0) & (n < nd)) and np.all((2 * n >= nd) == (peak < 0))
    y_at = np.take_along_axis(ref["y"], n[..., None], axis=-1)[..., 0]
    ok = ref["used"]
    assert np.all((ref["y"].max(axis=-1) - y_at)[ok] <= 2 * ref["e"][ok])
    moved = ok & (peak != ref["peak_bin"])
    assert np.all(np.abs(((peak - ref["peak_bin"])[moved] + nd // 2) % nd - nd // 2) <= 1)  # (a tie is between neighbours)
    same = fr.pair_delays(z, pad, peak=peak)  # the reference's refinement from the bin the device chose
    worst = float((np.abs(x - same["x"])[ok] / np.maximum(same["x_bound"][ok], 1e-300)).max()) if ok.any() else 0.0
    print(label, "pairs", int(ok.sum()), "of", ok.size, "ties", int(moved.sum()), "worst |dx| / bound", worst, "largest bound",
          float(same["x_bound"][ok].max()) if ok.any() else 0.0)
    assert np.all(np.abs(x - same["x"])[ok] <= same["x_bound"][ok])
    # |dy/dx| <= 2 |P| |dP/dx| <= 4 pi (nfreqs / ND) S^2, S = sum |z|: what the difference in x allows on top of the rounding
    slope = 4 * np.pi / pad * np.abs(z).sum(axis=-1) ** 2
    assert np.all(np.abs(power - same["power"])[ok] <= (2 * ref["e"] + slope * same["x_bound"])[ok])
    assert np.all(peak[~ok] == 0) and np.all(x[~ok] == 0) and np.all(power[~ok] == 0)
    return ref, same


CASES = [("hex7", 2, 1, 1, False), ("hex7", 2, 2, 8, True), ("hex7", 13, 2, 1, True), ("hex7", 16, 1, 8, False),
         ("grid16", 13, 1, 8, True), ("grid16", 16, 2, 1, False), ("hex19", 13, 2, 8, False), ("hex19", 16, 2, 8, True),
         ("hex19", 16, 1, 1, True)]


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("polarized", [False, True])
@pytest.mark.parametrize("name,nf,nt,pad,flags", CASES)
def test_pair_delays(gpu, name, nf, nt, pad, flags, polarized, precision):
    case = _pd_case(name, nf, nt, pad, polarized, flags)
    npairs = len(case["pair1"])
    # (hex-19's 141 rows are more than one block of the delay kernel and no multiple of its four waves; a group of one member)
    assert npairs == {"hex7": 12, "grid16": 96, "hex19": 141}[name] and 1 in np.bincount(case["group"])
    outs = _pair_delays(case, precision, pad)
    ref, same = _check_pair_delays(f"firstcal pair delays {name} {nf} {nt} {pad} {flags} {polarized} {precision}", case, precision, pad, outs)
    used, x = ref["used"], outs[1]
    if flags:
        assert case["lost"].sum() >= 3 and not used[:, case["lost"]].any() and not np.isfinite(case["d"]).all()
    assert used[:, ~case["lost"]].all()
    if nf >= 13 and pad == 8 and precision == 2:  # the case holds what it says: negative delays, and two within a bin of the ends
        keep = ~case["lost"]
        assert np.all(np.abs(same["x"] - case["target"])[:, keep] <= 1e-6) and (x[:, keep] < -1).any()
        assert np.all(np.abs(np.abs(x[:, 2:4]) - nf * pad / 2)[:, keep[2:4]] < 1)
    again = _pair_delays(case, precision, pad)  # the same input gives the same bits
    resident = _pair_delays(case, precision, pad, on_device=True)  # host or device blocks
    for other in (again, resident):
        assert all(np.array_equal(a, b) for a, b in zip(other, outs))


@pytest.mark.parametrize("nf", [512, 513])
def test_pair_delays_beyond_the_lds_budget(gpu, nf):
    """Four rows of 513 complex128 channels are 32 832 bytes: the rows are read from global memory; 512 still fit."""
    assert (4 * 16 * nf > 32768) == (nf == 513)
    case = _pd_case("hex7", nf, 1, 1, False, True)
    outs = _pair_delays(case, 2, 1)
    ref, _ = _check_pair_delays(f"firstcal pair delays beyond LDS {nf}", case, 2, 1, outs)
    assert ref["used"][:, ~case["lost"]].all()


# ---- 2. the offsets --------------------------------------------------------------------------------------------------------
def _offsets(d, w, case, slopes, c0, tpol, precision, max_iter, tol, on_device=False):
    nf, nt = d.shape[:2]
    c = np.ascontiguousarray(c0, dtype=np.complex128).copy()
    niter, change = np.full(1, -1, dtype=np.int32), np.full(1, -1.0)
    chi2, solved = np.full((nf, nt), -1.0), np.full(c.shape, 7, dtype=np.int32)
    U = np.full((nf, nt, tpol, case["ngroups"]), 7.0, dtype=np.complex128)
    vis_solved = np.full(U.shape, 7, dtype=np.int32)
    keep, ptrs = _device([d, w]) if on_device else (None, [_lib.ptr(d), _lib.ptr(w)])
    status = _lib.lib().fv_firstcal_offsets(0, precision, nf, nt, d.shape[-1], tpol, case["nant"], _lib.ptr(case["a1"]), _lib.ptr(case["a2"]),
                                            case["ngroups"], _lib.ptr(case["group"]), _lib.ptr(slopes), ptrs[0], int(on_device), ptrs[1],
                                            int(on_device), _lib.ptr(c), _lib.ptr(U), max_iter, tol, _lib.ptr(niter), _lib.ptr(change),
                                            _lib.ptr(chi2), _lib.ptr(solved), _lib.ptr(vis_solved))
    assert status == 0, _lib.lib().fv_last_error()
    after = None if keep is None else [None if t is None else t.cpu().numpy() for t in keep]
    return (c, U, int(niter[0]), change, chi2, solved != 0, vis_solved != 0), after


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("polarized", [False, True])
def test_offsets_three_iterations(gpu, polarized, precision):
    tpol = 4 if polarized else 1
    case = fc_case("hex19", 4, noise=0.05, nt=3, freqs=FREQS[:5], polarized=polarized)
    rng = np.random.default_rng(9)
    case["w"] = rng.uniform(0.5, 2.0, case["d"].shape)
    case["w"][2, 1, ..., 7] = 0
    case["d"][2, 1, ..., 7] = complex(np.nan, np.inf)
    case["w"][..., case["group"] == 11] = 0  # a group without a used sample
    d32, w32 = case["d"].astype(CDT[precision]), case["w"].astype(RDT[precision])
    d, w = _rows(d32, tpol), _rows(w32, tpol)
    before = d.copy()
    dnu = 0.5e6
    slopes = np.ascontiguousarray(2 * np.pi * dnu * (case["tau"] + rng.uniform(-2e-9, 2e-9, case["tau"].shape)))  # (near the truth)
    c0 = 1 + 0.2 * (rng.normal(size=case["tau"].shape) + 1j * rng.normal(size=case["tau"].shape))
    got, _ = _offsets(d, w, case, slopes, c0, tpol, precision, 3, 0.0)
    c, U, niter, change, chi2, solved, vis_solved = got
    assert np.array_equal(d.view(np.uint8), before.view(np.uint8))  # the caller's data are never written
    db, wb = d32.astype(np.complex128), w32.astype(np.float64)
    c_ref, U_ref, changes, _, solved_ref, vis_solved_ref = fr.offsets(db, wb, case["a1"], case["a2"], case["group"], case["ngroups"], slopes,
                                                                       c0, 3, 0.0, cdt=CDT[precision])
    U = U.reshape(U_ref.shape)
    print("firstcal offsets, three iterations", polarized, precision, rel_l2(c, c_ref), rel_l2(U, U_ref), float(abs(change[0] - changes[-1].max())))
    assert niter == 3 and len(changes) == 3
    assert rel_l2(c, c_ref) <= BOUND[precision] and rel_l2(U, U_ref) <= BOUND[precision]
    assert abs(change[0] - changes[-1][0, 0]) <= BOUND[precision] * max(changes[-1][0, 0], 1.0)
    assert np.array_equal(solved, solved_ref) and solved.all()
    assert np.array_equal(vis_solved.reshape(vis_solved_ref.shape), vis_solved_ref) and not vis_solved_ref[..., 11].any()
    assert vis_solved_ref[..., :11].all() and np.all(U[~vis_solved_ref] == 0)
    # chi2 at the returned offsets and visibilities, on the reference's derotated block
    nf, nt = db.shape[:2]
    rot = fr.derotate(np.where(gsr.used_weights(db, wb, case["a1"], case["a2"]) > 0, db, 0), case["a1"], case["a2"], slopes)
    rot = rot.astype(CDT[precision]).astype(np.complex128)
    g = np.broadcast_to(c[None, None], (nf, nt) + c.shape)
    chi2_ref = rr.chi2_rows(U, rot, wb, g, case["a1"], case["a2"], case["group"])
    wu = gsr.used_weights(rot, wb, case["a1"], case["a2"])
    power = (wu * np.abs(rot) ** 2).reshape(nf, nt, -1).sum(axis=-1)
    moved = 2 * (8 * 2.0**-53 if precision == 2 else 2.0**-23) * np.sqrt(power / chi2_ref)
    bound = _chi2_bound(rr.model(U, case["group"]), wb, g, case["a1"], case["a2"], chi2_ref) + moved
    print("firstcal offsets chi2", float((np.abs(chi2 - chi2_ref) / chi2_ref / bound).max()))
    assert chi2.shape == (nf, nt) and np.all(np.abs(chi2 - chi2_ref) <= bound * chi2_ref)
    again, _ = _offsets(d, w, case, slopes, c0, tpol, precision, 3, 0.0)  # the same input gives the same bits
    resident, after = _offsets(d, w, case, slopes, c0, tpol, precision, 3, 0.0, on_device=True)  # host or device blocks
    for other in (again, resident):
        assert all(np.array_equal(a, b) for a, b in zip(other, got))
    assert np.array_equal(after[0].view(np.uint8), before.view(np.uint8)) and np.array_equal(after[1], w)


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
def test_end_to_end_on_hex19(gpu):
    import torch

    case = fc_case("hex19", 1)
    ants, d = case["ants"], case["d"]
    kw = dict(baselines=case["bls"], tol=1e-10)
    gains, vis, info = fftvis_amd.redundant_firstcal(d, ants, FREQS, **kw)
    ref = fr.firstcal(d, case["w"], case["a1"], case["a2"], case["group"], case["ngroups"], case["nant"], FREQS, tol=1e-10)
    assert gains.shape == (19, 16) and gains.dtype == np.complex128 and vis.shape == (16, 2, 30) and vis.dtype == np.complex128
    assert info["delays"].shape == (19,) and info["offsets"].shape == (19,) and info["chi2"].shape == (16, 2)
    assert len(info["pairs"]) == 141 and info["pair_delays"].shape == (141,) and info["pair_used"].all() and info["solved"].all()
    assert info["pairs"] == [(case["bls"][i], case["bls"][j]) for i, j in zip(ref["pair1"], ref["pair2"])]
    assert info["reds"] == case["reds"] and info["baselines"] == case["bls"] and info["chi2"].sum() <= 1e-16 * (np.abs(d) ** 2).sum()
    assert info["converged"] and abs(info["niter"] - len(ref["changes"])) <= 2 and info["vis_solved"].all()
    # the delays against the truth outside the null space: the reference's bound, once for either implementation
    err, proj = outside_null_space(info["delays"] - case["tau"][0], ants)
    bound = 2 * (ref["tau_bound"] @ proj.T)[0]
    print("firstcal end to end: delay error outside the null space (ns)", float(np.abs(err).max()) * 1e9, "bound", float(bound.max()) * 1e9,
          "stage 2 iterations", info["niter"], len(ref["changes"]))
    assert np.all(np.abs(err) <= bound)
    g, U, solve = fftvis_amd.redundant_gain_solve(d, ants, gains=gains, **kw)
    power = float((np.abs(d) ** 2).sum())
    print("firstcal end to end: redundant solve iterations", solve["niter"], "chi2 / sum |d|^2", float(solve["chi2"].sum()) / power)
    assert solve["converged"] and solve["niter"] <= 4
    assert solve["chi2"].sum() <= 1e-16 * power
    # the gains are the model of the delays and the offsets, and vis the group visibilities at them
    model = info["offsets"][:, None] * np.exp(2j * np.pi * info["delays"][:, None] * (FREQS - FREQS.mean()))
    assert np.abs(gains - model).max() <= 1e-12
    # a device tensor as data: the host call's bits, on the device; and a second call repeats the first
    dev = fftvis_amd.redundant_firstcal(torch.from_numpy(d).cuda(), ants, FREQS, **kw)
    again = fftvis_amd.redundant_firstcal(d, ants, FREQS, **kw)
    for x, y in [(dev[0], gains), (dev[1], vis)] + [(dev[2][k], info[k]) for k in ("delays", "offsets", "pair_delays", "chi2", "solved")]:
        assert isinstance(x, torch.Tensor) and x.device.type == "cuda" and np.array_equal(x.cpu().numpy(), y)
    for x, y in [(again[0], gains), (again[1], vis)] + [(again[2][k], info[k]) for k in ("delays", "offsets", "pair_delays", "chi2")]:
        assert np.array_equal(x, y)
    assert dev[2]["niter"] == again[2]["niter"] == info["niter"]


def test_polarized_flags_and_a_reference_antenna(gpu):
    """Polarized data with the cross-hands flagged, a baseline flagged altogether, weights and ``ref_ant``."""
    case = fc_case("hex7", 2, polarized=True)
    ants, d, w = case["ants"], case["d"], case["w"]
    w[:, :, 0, 1], w[:, :, 1, 0] = 0, 0
    w[..., 4] = 0
    d[..., 4] = np.nan
    gains, vis, info = fftvis_amd.redundant_firstcal(d, ants, FREQS, weights=w, polarized=True, tol=1e-10, ref_ant=3, precision=1)
    assert gains.shape == (7, 2, 16) and info["delays"].shape == (7, 2) and info["pair_used"].shape == (2, 12)
    lost = np.array([4 in (case["bls"].index(a), case["bls"].index(b)) for a, b in info["pairs"]])
    assert lost.any() and not info["pair_used"][:, lost].any() and info["pair_used"][:, ~lost].all()
    assert abs(info["offsets"][3, 0].imag) <= 1e-15 * abs(info["offsets"][3, 0]) and info["offsets"][3, 0].real > 0
    assert info["converged"] and np.isfinite(gains).all() and info["solved"].shape == (7, 2)
    err, proj = outside_null_space(info["delays"].T - case["tau"], ants)
    print("firstcal polarized, fp32, flags: delay error outside the null space (ns)", float(np.abs(err).max()) * 1e9)
    # fp32 inputs: a phase error of 2^-24 rad per datum over 7.5 MHz is 2^-24 / (2 pi 7.5e6) = 1.3e-15 s per pair before any
    # averaging; the pseudo-inverse of hex-7's pairs multiplies a pair's error by less than 10
    assert np.abs(err).max() <= 10 * 1.3e-15


@pytest.mark.parametrize("polarized", [False, True])
def test_a_start_for_the_offsets_is_read_only(gpu, polarized):
    """``offsets=`` through the public function: the caller's array keeps its bits, the result is the reference's from that
    start -- which also holds the (nant, 2) to (nfeed, nant) transposition -- and no output shares memory with the start, so that
    one call's ``info["offsets"]`` can start the next."""
    case = fc_case("hex7", 6, noise=0.05, polarized=polarized)
    ants, d = case["ants"], case["d"]
    rng = np.random.default_rng(12)
    lead = (7, 2) if polarized else (7,)
    start = np.ascontiguousarray(1 + 0.3 * (rng.normal(size=lead) + 1j * rng.normal(size=lead)))
    before = start.copy()
    kw = dict(polarized=polarized, max_iter=3, tol=0.0)
    gains, vis, info = fftvis_amd.redundant_firstcal(d, ants, FREQS, offsets=start, **kw)
    assert np.array_equal(start.view(np.uint8), before.view(np.uint8))
    assert not np.shares_memory(info["offsets"], start) and info["niter"] == 3 and not info["converged"]
    c0 = start.T if polarized else start[None]
    ref = fr.firstcal(d, case["w"], case["a1"], case["a2"], case["group"], case["ngroups"], case["nant"], FREQS, max_iter=3, tol=0.0, c0=c0)
    c_ref = ref["c"].T if polarized else ref["c"][0]
    ones = fftvis_amd.redundant_firstcal(d, ants, FREQS, **kw)[2]["offsets"]
    print("firstcal from a start", polarized, rel_l2(info["offsets"], c_ref), rel_l2(ones, c_ref))
    assert info["offsets"].shape == lead and rel_l2(info["offsets"], c_ref) <= BOUND[2]
    assert rel_l2(ones, c_ref) > 1e-3  # (three iterations from ones end elsewhere: the start was used)
    # one call's result starts the next, and stays what it was
    first = info["offsets"].copy()
    fftvis_amd.redundant_firstcal(d, ants, FREQS, offsets=info["offsets"], **kw)
    assert np.array_equal(info["offsets"].view(np.uint8), first.view(np.uint8))
