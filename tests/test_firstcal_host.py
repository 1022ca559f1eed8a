"""CPU tests of firstcal (``redundant_firstcal``; ``fv_firstcal_pair_delays``, ``fv_firstcal_offsets``): the numpy reference
against its ``longdouble`` variant and against the truth, what it buys the redundant solve, the C surface and the argument
errors raised before any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, redundant
from tests import firstcal_refs as fr
from tests import gain_refs
from tests import redundant_refs as rr
from tests.position_adjoint_refs import hex_positions

FREQS = 150e6 + 0.5e6 * np.arange(16)


def array(name):
    """hex-7, hex-19 or hex-37 at 14.6 m, or a 4 x 4 grid at 14 m."""
    if name == "grid16":
        xy = 14.0 * np.array([(i, j) for j in range(4) for i in range(4)], dtype=float)
    else:
        xy = 14.6 * hex_positions({"hex7": 1, "hex19": 2, "hex37": 3}[name])
    return {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(len(xy))}


def fc_case(name, seed, noise=0.0, nt=2, freqs=FREQS, polarized=False, max_delay=150e-9):
    """Every baseline of the array in group order; gains ``a exp(i phi) exp(2 pi i tau (nu - mean nu))`` with the delays uniform
    in +-``max_delay``, the phases in +-pi and the amplitudes in 1 +- 0.1, constant in time; random group visibilities per
    channel and time, and noise of standard deviation ``noise``.  Returns a dict."""
    rng = np.random.default_rng(seed)
    ants = array(name)
    reds, bls, group = fftvis_amd.redundant_groups(ants)
    a1 = np.array([bl[0] for bl in bls], dtype=np.int32)
    a2 = np.array([bl[1] for bl in bls], dtype=np.int32)
    nf, nant, nfeed = len(freqs), len(ants), 2 if polarized else 1
    pol = (2, 2) if polarized else ()

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    tau = rng.uniform(-max_delay, max_delay, (nfeed, nant))
    c_true = rng.uniform(0.9, 1.1, (nfeed, nant)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (nfeed, nant)))
    g = fr.model_gains(c_true, tau, freqs)
    U = c((nf, nt) + pol + (len(reds),))
    shape = (nf, nt) + pol + (len(bls),)
    d = gain_refs.apply_gains(rr.model(U, group), np.broadcast_to(g, (nf, nt) + g.shape[2:]), a1, a2) + noise * c(shape) / np.sqrt(2)
    return dict(ants=ants, reds=reds, bls=bls, group=group, a1=a1, a2=a2, tau=tau, c=c_true, g=g, U=U, d=d, w=np.ones(shape),
                freqs=np.asarray(freqs), nant=nant, ngroups=len(reds))


def outside_null_space(x, ants):
    """The part of a per-antenna vector (last axis) outside span{1, x, y}, and the modulus of that projector."""
    pos = np.array(list(ants.values()))
    Q, _ = np.linalg.qr(np.column_stack([np.ones(len(pos)), pos[:, 0], pos[:, 1]]))
    proj = np.eye(len(pos)) - Q @ Q.T
    return x @ proj.T, np.abs(proj)


def _reference(case, **kw):
    return fr.firstcal(case["d"], case["w"], case["a1"], case["a2"], case["group"], case["ngroups"], case["nant"], case["freqs"], **kw)


# ---- the reference against its longdouble variant ------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 8])
def test_reference_stays_within_its_bound_of_the_longdouble_variant(pad):
    case = fc_case("hex19", 1)
    pair1, pair2 = fr.pairs(case["group"])
    z, _ = fr.products(case["d"], case["w"], case["a1"], case["a2"], pair1, pair2)
    zl, _ = fr.products(case["d"], case["w"], case["a1"], case["a2"], pair1, pair2, dtype=np.longdouble)
    got, ref = fr.pair_delays(z, pad), fr.pair_delays(zl, pad, dtype=np.longdouble)
    worst = float((np.abs(got["x"] - ref["x"]) / got["x_bound"]).max())
    print("firstcal reference against longdouble: pad, worst |dx| / bound, largest bound (bins)", pad, worst, float(got["x_bound"].max()))
    assert len(pair1) == len(case["bls"]) - case["ngroups"] == 141
    assert got["used"].all() and np.array_equal(got["peak_bin"], ref["peak_bin"])
    assert np.isfinite(got["x_bound"]).all() and got["x_bound"].max() < 1e-6
    assert np.all(np.abs(got["x"] - ref["x"]) <= got["x_bound"])
    assert np.all(np.abs(got["power"] - ref["power"]) <= got["e"]) and np.all(np.abs(got["total"] - ref["total"]) <= got["e"])


@pytest.mark.parametrize("pad,n", [(1, 3), (8, 37), (8, -21)])
def test_a_delay_half_way_between_two_bins(pad, n):
    """|P| is the same at the two bins next to the delay: either may be the peak, and both lead to the same refined x."""
    nf = 16
    nd = pad * nf
    amp = np.random.default_rng(5).uniform(0.5, 1.5, nf)
    z = (amp * np.exp(2j * np.pi * np.arange(nf) * (n + 0.5) / nd) * np.exp(0.7j))[None]
    got, ref = fr.pair_delays(z, pad), fr.pair_delays(z.astype(np.clongdouble), pad, dtype=np.longdouble)
    print("firstcal half-way delay", pad, n, int(got["peak_bin"][0]), int(ref["peak_bin"][0]), float(got["x"][0]), float(ref["x"][0]),
          float(got["x_bound"][0]))
    for r in (got, ref):
        assert r["peak_bin"][0] in (n, n + 1)
        assert abs(float(r["x"][0]) - (n + 0.5)) <= got["x_bound"][0] + ref["x_bound"][0]
    top = np.sort(got["y"][0])[-2:]
    assert top[1] - top[0] <= 2 * got["e"][0]  # the two top bins are equal within what the rounding allows


def test_an_unused_pair_and_a_single_channel():
    z = np.zeros((3, 16), dtype=complex)
    z[1, 5] = 2 - 1j
    z[2, 3], z[2, 9] = 1.0, 1j
    got = fr.pair_delays(z, 8)
    assert got["used"].tolist() == [False, False, True] and got["x"][:2].tolist() == [0, 0] and got["peak_bin"][:2].tolist() == [0, 0]
    assert got["power"][:2].tolist() == [0, 0] and got["total"].tolist() == [0, 5, 2]


# ---- accuracy, and what it buys the redundant solve ----------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", ["hex7", "hex19", "grid16"])
def test_noiseless_delays_and_iteration_counts(name, seed):
    case = fc_case(name, seed)
    got = _reference(case, tol=1e-10)
    err, proj = outside_null_space(got["tau"] - case["tau"], case["ants"])
    bound = got["tau_bound"] @ proj.T
    assert got["pairs"]["used"].all() and got["in_pair"].all() and got["solved"].all()
    # the redundant solve from the firstcal start and from a unit start
    args = (case["a1"], case["a2"], case["group"], case["ngroups"], False, 600, 1e-10)
    start = rr.solve(case["d"], case["w"], got["gains"], *args)
    unit = rr.solve(case["d"], case["w"], np.ones_like(got["gains"]), *args)
    print(f"firstcal {name} seed {seed}: delay error outside the null space {float(np.abs(err).max()) * 1e9:.3e} ns, bound "
          f"{float(bound.max()) * 1e9:.3e} ns; stage 2 iterations {len(got['changes'])}; redundant solve iterations from the "
          f"firstcal start {len(start[2])}, from a unit start {len(unit[2])}; its chi2 / sum |d|^2 "
          f"{float(start[3].sum() / (np.abs(case['d']) ** 2).sum()):.3e}")
    assert np.isfinite(bound).all() and np.all(np.abs(err) <= bound)
    assert len(got["changes"]) < 200 and got["changes"][-1].max() < 1e-10
    assert len(start[2]) <= 4
    assert got["chi2"].sum() <= 1e-16 * (np.abs(case["d"]) ** 2).sum()


@pytest.mark.parametrize("name,seed", [("hex7", 0), ("hex19", 1), ("grid16", 2)])
def test_chi2_under_noise(name, seed):
    case = fc_case(name, seed, noise=0.05)
    got = _reference(case, tol=1e-10)
    solve = rr.solve(case["d"], case["w"], got["gains"], case["a1"], case["a2"], case["group"], case["ngroups"], False, 600, 1e-10)
    ratio = float(got["chi2"].sum() / solve[3].sum())
    print("firstcal under noise 0.05: chi2 / the converged redundant solve's", name, seed, ratio, len(solve[2]))
    assert len(solve[2]) < 600 and 1.0 <= ratio <= 1.25


def test_reference_polarized_and_flags():
    """Feed p reads [p, p]; a baseline flagged altogether leaves its pairs unused and, when it is an antenna's only one, the
    antenna unsolved with delay 0."""
    case = fc_case("hex7", 3, polarized=True)
    got = _reference(case, tol=1e-10)
    err, proj = outside_null_space(got["tau"] - case["tau"], case["ants"])
    assert got["tau"].shape == (2, 7) and np.all(np.abs(err) <= got["tau_bound"] @ proj.T)
    k = 4
    case["w"][..., k] = 0
    case["d"][..., k] = np.nan
    flagged = _reference(case, tol=1e-10)
    touched = (flagged["pair1"] == k) | (flagged["pair2"] == k)
    assert touched.any() and not flagged["pairs"]["used"][:, touched].any() and flagged["pairs"]["used"][:, ~touched].all()
    assert np.all(flagged["pairs"]["x"][:, touched] == 0) and np.isfinite(flagged["gains"]).all() and np.isfinite(flagged["chi2"]).all()


# ---- the C surface ---------------------------------------------------------------------------------------------------------
_NEW = {"fv_firstcal_pair_delays": 21, "fv_firstcal_offsets": 25}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    flat = " ".join(header.split())
    for declared in ("int fv_firstcal_pair_delays(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int npairs, "
                     "const int *pair1, const int *pair2, const int *ant1, const int *ant2, const void *data, int data_on_device, "
                     "const void *weights, int weights_on_device, int pad, int *peak_bin_out, double *delay_bins_out, "
                     "double *power_out, double *total_out, int *used_out);",
                     "int fv_firstcal_offsets(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, "
                     "const int *ant1, const int *ant2, int ngroups, const int *group, const double *slopes, const void *data, "
                     "int data_on_device, const void *weights, int weights_on_device, void *offsets, void *uvis_out, int max_iter, "
                     "double tol, int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, "
                     "int *vis_solved_out);"):
        assert declared in flat, declared
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    flat = flat.replace(" * ", " ")
    for stated in ("z[feed, i, f] = sum_t d[f, t, pol, k] conj(d[f, t, pol, k'])", "P[n] = sum_f z[f] exp(-2 pi i n f / ND)",
                   "n - ND where 2 n >= ND", "h = 1, 1/4, 1/16, 1/64", "den = y- - 2 y0 + y+", "0.5 h (y- - y+) / den clipped to +-h",
                   "at least two channels have a non-zero z", "weights act as flags",
                   "d'[f, t, pol, k] = d exp(-i (f - (nfreqs - 1) / 2) (s[q, ant2] - s[p, ant1]))",
                   "the caller's data are never written", "the whole block as one solve unit"):
        assert stated in flat, stated


def test_public_signature():
    own = inspect.signature(redundant.redundant_firstcal).parameters
    assert list(own) == ["data", "ants", "freqs", "reds", "baselines", "weights", "offsets", "pad", "max_iter", "tol", "ref_ant",
                         "polarized", "precision", "device"]
    defaults = dict(reds=None, baselines=None, weights=None, offsets=None, pad=8, max_iter=200, tol=1e-8, ref_ant=None, polarized=False,
                    precision=2, device=0)
    assert all(own[n].kind.name == "KEYWORD_ONLY" and own[n].default == v for n, v in defaults.items())
    assert fftvis_amd.redundant_firstcal is redundant.redundant_firstcal
    doc = " ".join(redundant.redundant_firstcal.__doc__.split())
    for word in ("fv_firstcal_pair_delays", "fv_firstcal_offsets", "parallel hands", "weights act as flags", "minimum-norm", "alias",
                 "polarity flips", "per-time delays", "non-uniform channels", "Jones matrices", "sharding", "pair_delays", "pair_used"):
        assert word in doc, word
    assert "redundant_firstcal" in redundant.redundant_gain_solve.__doc__ and "redundant_firstcal" in fftvis_amd.__doc__
    # the signature of the solve it starts has not changed
    assert list(inspect.signature(redundant.redundant_gain_solve).parameters)[:5] == ["data", "ants", "reds", "baselines", "gains"]


def test_python_argument_errors_come_before_the_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ants = array("hex19")
    d = np.zeros((4, 2, 171), complex)
    nu = FREQS[:4]
    call = fftvis_amd.redundant_firstcal
    with pytest.raises(ValueError, match=re.escape("data must have shape (nfreqs, ntimes, nbls), got (2, 171)")):
        call(d[0], ants, nu)
    with pytest.raises(ValueError, match=re.escape("data must have shape (nfreqs, ntimes, 2, 2, nbls), got (4, 2, 171)")):
        call(d, ants, nu, polarized=True)
    with pytest.raises(ValueError, match=re.escape("freqs must have shape (4,), got (3,)")):
        call(d, ants, nu[:3])
    with pytest.raises(ValueError, match="at least two channels"):
        call(d[:1], ants, nu[:1])
    bent = nu.copy()
    bent[2] += 2e-6 * 0.5e6
    with pytest.raises(ValueError, match="freqs must be uniformly spaced"):
        call(d, ants, bent)
    with pytest.raises(ValueError, match="freqs must be uniformly spaced"):
        call(d, ants, np.full(4, 150e6))
    for bad in (0, 2.5, -1, (1 << 20) // 4):
        with pytest.raises(ValueError, match="pad must be a positive integer with pad \\* nfreqs < 2\\*\\*20"):
            call(d, ants, nu, pad=bad)
    with pytest.raises(ValueError, match="data holds 170 baselines, baselines lists 171"):
        call(d[..., :170], ants, nu)
    with pytest.raises(ValueError, match=re.escape("weights must have data's shape (4, 2, 171), got (2, 171)")):
        call(d, ants, nu, weights=np.ones((2, 171)))
    with pytest.raises(ValueError, match=re.escape("offsets must be complex of shape (19,), got (19, 2)")):
        call(d, ants, nu, offsets=np.ones((19, 2), complex))
    with pytest.raises(ValueError, match="offsets must be complex"):
        call(d, ants, nu, offsets=np.ones(19))
    with pytest.raises(ValueError, match="ref_ant must be a key of ants, got 1000"):
        call(d, ants, nu, ref_ant=1000)
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match="max_iter must be a positive integer"):
            call(d, ants, nu, max_iter=bad)
    with pytest.raises(ValueError, match="tol must be non-negative"):
        call(d, ants, nu, tol=-1.0)
    with pytest.raises(ValueError, match="precision must be 1 or 2"):
        call(d, ants, nu, precision=3)


def test_pairs_of_the_public_function_are_the_reference():
    for name in ("hex7", "grid16"):
        _, _, group = fftvis_amd.redundant_groups(array(name))
        for grp in (group, group[::-1].copy(), np.random.default_rng(2).permutation(group)):
            got, ref = redundant._firstcal_pairs(grp), fr.pairs(grp)
            assert got[0].dtype == np.int32 and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            assert len(ref[0]) == len(grp) - len(np.unique(grp)) and np.all(ref[0] < ref[1]) and np.all(grp[ref[0]] == grp[ref[1]])


def test_fv_firstcal_pair_delays_argument_checks():
    L = _lib.lib()
    name = b"fv_firstcal_pair_delays"
    buf = (ctypes.c_double * 256)()
    a, b = (ctypes.c_int * 3)(0, 1, 2), (ctypes.c_int * 3)(1, 2, 0)
    p1, p2 = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 2)(1, 2)

    def call(precision=2, nfreqs=4, ntimes=1, nbls=3, tpol=1, npairs=2, p1=p1, p2=p2, a1=a, a2=b, d=buf, flags=(0, 0), pad=2, peak=buf,
             x=buf, power=buf, total=buf, used=buf):
        return L.fv_firstcal_pair_delays(0, precision, nfreqs, ntimes, nbls, tpol, npairs, p1, p2, a1, a2, d, flags[0], None, flags[1], pad,
                                         peak, x, power, total, used)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and name + b": tpol must be 1 or 4" in L.fv_last_error()
    for kw in (dict(nfreqs=-1), dict(ntimes=-1), dict(nbls=-1), dict(npairs=-1)):
        assert call(**kw) == 1 and name + b": negative shape" in L.fv_last_error()
    for kw in (dict(pad=0), dict(pad=-3), dict(pad=1 << 18)):
        assert call(**kw) == 1 and name + b": pad must be positive and pad nfreqs below 2^20" in L.fv_last_error()
    for flags in ((2, 0), (0, -1)):
        assert call(flags=flags) == 1 and name + b": the on_device flags must be 0 or 1" in L.fv_last_error()
    for kw in (dict(peak=None), dict(x=None), dict(power=None), dict(total=None), dict(used=None)):
        assert call(**kw) == 1 and name + b": null peak_bin_out, delay_bins_out, power_out, total_out or used_out" in L.fv_last_error()
    for kw in (dict(p1=None), dict(p2=None), dict(a1=None), dict(a2=None), dict(d=None)):
        assert call(**kw) == 1 and name + b": null pairs or data" in L.fv_last_error()
    low, high = (ctypes.c_int * 2)(0, -1), (ctypes.c_int * 2)(3, 1)
    for kw in (dict(p1=low), dict(p2=low), dict(p1=high), dict(p2=high)):
        assert call(**kw) == 1 and name + b": baseline index outside [0, nbls)" in L.fv_last_error()
    # no pair, and no sample: valid calls that return zeros, without a device
    assert call(npairs=0, p1=None, p2=None, peak=None, x=None, power=None, total=None, used=None) == 0, L.fv_last_error()
    outs = [np.full((2, 2), 7, dtype=np.int32), np.full((2, 2), 7.0), np.full((2, 2), 7.0), np.full((2, 2), 7.0), np.full((2, 2), 7, dtype=np.int32)]
    assert L.fv_firstcal_pair_delays(0, 1, 0, 3, 3, 4, 2, p1, p2, a, b, None, 0, None, 0, 8, *[_lib.ptr(o) for o in outs]) == 0, L.fv_last_error()
    assert not any(o.any() for o in outs)


def test_fv_firstcal_offsets_argument_checks():
    L = _lib.lib()
    fn = L.fv_firstcal_offsets
    name = b"fv_firstcal_offsets"
    buf = (ctypes.c_double * 64)()
    a = (ctypes.c_int * 3)(0, 1, 2)
    niter = (ctypes.c_int * 1)(-1)

    def call(precision=2, nfreqs=1, ntimes=1, nbls=3, tpol=1, nant=3, a1=a, a2=a, ngroups=3, group=a, s=buf, d=buf, flags=(0, 0), c=buf,
             u=buf, max_iter=5, tol=1e-8, n=niter, change=buf, chi2=buf, solved=buf, vis_solved=buf):
        return fn(0, precision, nfreqs, ntimes, nbls, tpol, nant, a1, a2, ngroups, group, s, d, flags[0], None, flags[1], c, u, max_iter,
                  tol, n, change, chi2, solved, vis_solved)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and name + b": tpol must be 1 or 4" in L.fv_last_error()
    for kw in (dict(nfreqs=-1), dict(ntimes=-1), dict(nbls=-1), dict(nfreqs=1 << 16, ntimes=1 << 16)):
        assert call(**kw) == 1 and name + b": negative shape" in L.fv_last_error()
    assert call(nant=0) == 1 and name + b": nant must be positive" in L.fv_last_error()
    assert call(ngroups=0) == 1 and name + b": ngroups must be positive" in L.fv_last_error()
    for bad in (0, -1):
        assert call(max_iter=bad) == 1 and name + b": max_iter must be positive" in L.fv_last_error()
    for bad in (-1e-9, float("nan")):
        assert call(tol=bad) == 1 and name + b": tol must be non-negative" in L.fv_last_error()
    for flags in ((2, 0), (0, -1)):
        assert call(flags=flags) == 1 and name + b": the on_device flags must be 0 or 1" in L.fv_last_error()
    assert call(n=None) == 1 and name + b": null niter_out" in L.fv_last_error()
    for kw in (dict(c=None), dict(u=None), dict(change=None), dict(chi2=None), dict(solved=None), dict(vis_solved=None)):
        assert call(**kw) == 1 and name + b": null offsets, uvis_out, change_out, chi2_ft_out, solved_out or vis_solved_out" in L.fv_last_error()
    for kw in (dict(a1=None), dict(a2=None), dict(group=None), dict(s=None), dict(d=None)):
        assert call(**kw) == 1 and name + b": null pairs, group, slopes or data" in L.fv_last_error()
    low, high = (ctypes.c_int * 3)(0, -1, 2), (ctypes.c_int * 3)(0, 1, 3)
    for a1, a2 in [(low, a), (a, high)]:
        assert call(a1=a1, a2=a2) == 1 and name + b": antenna index outside [0, nant)" in L.fv_last_error()
    for grp in (low, high):
        assert call(group=grp) == 1 and name + b": group index outside [0, ngroups)" in L.fv_last_error()
    assert niter[0] == -1  # (nothing ran)
    # no baseline: the start, U = 0, chi2 0, nothing solved, without a device
    c = np.arange(2 * 3, dtype=complex).reshape(2, 3) + 1j
    start = c.copy()
    change, chi2, solved = np.full(1, 7.0), np.full((2, 3), 7.0), np.full(c.shape, 7, dtype=np.int32)
    u, vis_solved = np.full((2, 3, 4, 5), 7.0, dtype=complex), np.full((2, 3, 4, 5), 7, dtype=np.int32)
    assert fn(0, 1, 2, 3, 0, 4, 3, None, None, 5, None, None, None, 0, None, 0, _lib.ptr(c), _lib.ptr(u), 5, 0.0, niter, _lib.ptr(change),
              _lib.ptr(chi2), _lib.ptr(solved), _lib.ptr(vis_solved)) == 0, L.fv_last_error()
    assert niter[0] == 0 and np.array_equal(c, start) and not change.any() and not chi2.any() and not solved.any()
    assert not u.any() and not vis_solved.any()
