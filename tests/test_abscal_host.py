"""CPU tests of abscal (``redundant_abscal``; ``fv_abscal_slopes``, ``fv_abscal_evaluate``): the numpy reference against its
``longdouble`` variant and against planted degeneracies, how often the search finds the main lobe, the C surface and the
argument errors raised before any device is touched."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, redundant
from tests import abscal_refs as ar
from tests import gain_refs
from tests import redundant_refs as rr
from tests.position_adjoint_refs import hex_positions


def array(name):
    """hex-7/19/37/61 at 14.6 m, a 4 x 4 grid at 14 m rotated by 0.3 rad, a 3 x 5 grid at 14 m or a line of 6 at 14 m."""
    if name.startswith("hex"):
        xy = 14.6 * hex_positions({"hex7": 1, "hex19": 2, "hex37": 3, "hex61": 4}[name])
    elif name == "rot16":
        xy = 14.0 * np.array([(i, j) for j in range(4) for i in range(4)], dtype=float) @ np.array([[np.cos(0.3), np.sin(0.3)],
                                                                                                   [-np.sin(0.3), np.cos(0.3)]])
    elif name == "grid15":
        xy = 14.0 * np.array([(i, j) for j in range(3) for i in range(5)], dtype=float)
    else:
        xy = 14.0 * np.array([(i, 0) for i in range(6)], dtype=float)
    return {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(len(xy))}


def group_baselines(ants):
    reds = fftvis_amd.redundant_groups(ants)[0]
    pos = np.array(list(ants.values()))
    return reds, np.array([pos[r[0][1]] - pos[r[0][0]] for r in reds])


def planted(rng, X, b, noise, frac=0.3):
    """One unit, one time: a random model, ``U = M e^{i Phi . X} / eta`` with ``|Phi| <= frac pi / min |b|`` and eta in 0.5 .. 2,
    random weights, and noise of ``noise`` times the model's scale on U.  Returns ``(U, M, W, eta, Phi)``."""
    ng, ndim = X.shape
    M = rng.normal(size=ng) + 1j * rng.normal(size=ng)
    eta = rng.uniform(0.5, 2.0)
    direction = rng.normal(size=ndim)
    phi = direction / np.linalg.norm(direction) * rng.uniform(0, frac) * np.pi / np.sqrt((b**2).sum(axis=1)).min()
    U = M * np.exp(1j * (X @ phi)) / eta + noise * (rng.normal(size=ng) + 1j * rng.normal(size=ng))
    return U[None, None], M[None, None], rng.uniform(0.5, 1.5, size=(1, 1, ng)), eta, phi


# ---- the reference against its longdouble variant ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hex19", "line6"])
def test_reference_stays_within_its_bounds_of_the_longdouble_variant(name):
    rng = np.random.default_rng(3)
    _, b = group_baselines(array(name))
    _, X = ar.plane(b)
    n, h, _ = ar.grid(X, b, 4)
    ng = len(b)
    shape = (3, 2, 2, 2, ng)
    M = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    phi = 0.3 * np.pi / 14.6 * rng.uniform(-0.7, 0.7, size=X.shape[1])
    U = M * np.exp(1j * (X @ phi)) / 1.3 + 0.05 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    W = rng.uniform(0.5, 1.5, size=shape)
    got = ar.abscal(U, M, W, X, n, h, 6, False)
    ref = ar.abscal(U.astype(np.clongdouble), M.astype(np.clongdouble), W, X, n, h, 6, False, dtype=np.longdouble)
    fast = ar.grid_values(got["prod"]["c"], X, n, h, fast=True)
    print("abscal reference against longdouble:", name, n, "worst |dy| / e", float((np.abs(got["y"] - ref["y"]).max(axis=(-1, -2)) / got["e"]).max()),
          "fast", float((np.abs(fast - ref["y"]).max(axis=(-1, -2)) / got["e"]).max()),
          "worst |dphi| / bound", float((np.abs(got["phi"] - ref["phi"]).max(axis=-1) / got["slope_bound"]).max()),
          "largest bound (rad/m)", float(got["slope_bound"].max()))
    assert got["used"].all() and np.array_equal(got["j"], ref["j"])
    assert np.all(np.abs(got["y"] - ref["y"]) <= got["e"][..., None, None]) and np.all(np.abs(fast - ref["y"]) <= got["e"][..., None, None])
    assert np.isfinite(got["slope_bound"]).all() and got["slope_bound"].max() < 1e-12
    assert np.all(np.abs(got["phi"] - ref["phi"]).max(axis=-1) <= got["slope_bound"])
    s, sb = ar.evaluate(got["prod"]["c"], X, got["phi"], a=got["prod"]["a"], extra=U.shape[1] + 4)
    sl, _ = ar.evaluate(ref["prod"]["c"], X, got["phi"].astype(np.longdouble), dtype=np.longdouble)
    assert np.all(np.abs(s - sl) <= sb)
    assert np.all(np.abs(got["amp"] - ref["amp"]) <= 1e-13 * got["amp"]) and np.all(np.abs(got["amp"] - 1.3) < 0.1)


# ---- how often the search finds the main lobe -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hex7", "hex19", "hex37", "hex61", "rot16", "grid15", "line6"])
def test_recovery_of_planted_degeneracies(name):
    """100 noiseless and 100 noisy (30 %) trials: at pad 4 with 6 rounds every noiseless trial recovers ``e^{i Phi . b}`` to
    rounding (1e-12: 2^-52 times the phases, ~100 rad, the number of groups and the fit's conditioning), and a noisy one
    reaches the maximum of a four times finer search (pad 16) in at least 99 of 100; pad 2 and pad 1 are counted and printed."""
    rng = np.random.default_rng(11)
    _, b = group_baselines(array(name))
    _, X = ar.plane(b)
    grids = {pad: ar.grid(X, b, pad)[:2] for pad in (1, 2, 4, 16)}
    worst, found = 0.0, {1: 0, 2: 0, 4: 0}
    for trial in range(100):
        U, M, W, eta, phi = planted(rng, X, b, 0.0)
        got = ar.abscal(U, M, W, X, *grids[4], 6, True, fast=True)
        worst = max(worst, float(np.abs(np.exp(1j * (X @ got["phi"][0, 0, 0, :X.shape[1]])) - np.exp(1j * (X @ phi))).max()),
                    abs(float(got["amp"][0, 0, 0]) - eta) / eta)
    for trial in range(100):
        U, M, W, eta, phi = planted(rng, X, b, 0.3)
        c = ar.products(U, M, W, X, True)["c"]
        fine = ar.grid_values(c, X, *grids[16], fast=True).max()
        for pad in found:
            _, _, j = ar.search(c, X, *grids[pad], fast=True)
            s = ar.refine(c, X, j, grids[pad][1], 6)[2]
            found[pad] += bool(s[0, 0, 0, 0] >= fine - 1e-9 * np.abs(c).sum())
    print(f"abscal recovery {name}: groups {len(b)}, grid at pad 4 {grids[4][0]}, noiseless worst error {worst:.2e}, "
          f"noisy trials that reach the fine maximum: pad 4 {found[4]}, pad 2 {found[2]}, pad 1 {found[1]} of 100")
    assert worst <= 1e-12
    # The line has 5 groups: at 30 % noise its fine maximum now and then lies on a side lobe next to the box's edge, which a
    # Newton start inside the box does not reach.  With a miss rate of the order of 1 in 100 there, more than 5 misses in
    # 100 trials have a probability below 1e-3; the planar arrays, with 9 groups and more, are held to one miss.
    assert found[4] >= (95 if name == "line6" else 99)


# ---- planted degeneracies on hex-19 -------------------------------------------------------------------------------------------
def _hex19_solution(seed):
    """A noisy hex-19 block, every baseline in group order, and the converged redundant solve of it."""
    rng = np.random.default_rng(seed)
    ants = array("hex19")
    reds, bls, group = fftvis_amd.redundant_groups(ants)
    a1, a2 = (np.array([bl[i] for bl in bls], dtype=np.int32) for i in (0, 1))
    nf, nt, nant, ng = 2, 2, len(ants), len(reds)

    def c(s):
        return rng.normal(size=s) + 1j * rng.normal(size=s)

    g = 1 + 0.1 * c((nf, 1, 1, nant))
    Utrue = c((nf, nt, ng))
    d = gain_refs.apply_gains(rr.model(Utrue, group), np.broadcast_to(g, (nf, nt, 1, nant)), a1, a2) + 0.05 * c((nf, nt, len(bls)))
    w = rng.uniform(0.5, 1.5, size=d.shape)
    got, U, _, chi2, _, _ = rr.solve(d, w, np.ones_like(g), a1, a2, group, ng, False, 60, 0.0)
    return dict(ants=ants, reds=reds, group=group, a1=a1, a2=a2, d=d, w=w, g=got, U=U, chi2=chi2, ng=ng, rng=rng)


@pytest.mark.parametrize("frac", [0.25, 0.6])
def test_planted_degeneracies_are_fixed_and_chi2_stays(frac):
    """The model is the solved U moved by a planted (eta, Phi): abscal finds them, the fixed gains with the U-step at them
    leave the redundant chi2 where it was, and the model chi2 vanishes.  At frac = 0.6 the phase gradient spans more than
    pi across the array, where ``fix_redundant_degeneracies`` -- a plane fit without unwrapping -- fails."""
    s = _hex19_solution(4)
    pos = np.array(list(s["ants"].values()))
    x = pos - pos.mean(axis=0)
    b = np.array([pos[r[0][1]] - pos[r[0][0]] for r in s["reds"]])
    vt, X = ar.plane(b)
    n, h, _ = ar.grid(X, b, 4)
    rng = s["rng"]
    nf = s["U"].shape[0]
    eta = rng.uniform(0.5, 2.0, size=(nf, 1, 1))
    phi = frac * np.pi / 14.6 * np.array([[np.cos(t), np.sin(t)] for t in rng.uniform(0, 2 * np.pi, nf)])[:, None, None, :]
    M = s["U"] * eta * np.exp(-1j * np.einsum("fuqi,gi->fug", phi, X))
    got = ar.abscal(s["U"], M, None, X, n, h, 6, False)
    assert got["used"].all()
    phase = np.exp(1j * np.einsum("fuqi,gi->fuqg", got["phi"], X))
    assert np.abs(phase - np.exp(1j * np.einsum("fuqi,gi->fuqg", phi, X))).max() <= 1e-12
    assert np.abs(got["amp"] - eta).max() <= 1e-12
    total = (np.abs(M) ** 2).sum()
    print("abscal planted", frac, "model chi2 / sum |M|^2", float(got["chi2"].sum() / total), "phase span (rad)",
          float(np.ptp(x @ (phi[0, 0, 0] @ vt))))
    assert got["chi2"].sum() <= 1e-24 * total
    fixed = ar.apply(s["g"], got["amp"], got["phi"] @ vt, pos, got["used"])
    rows = np.broadcast_to(fixed, (nf, s["d"].shape[1]) + fixed.shape[2:])
    U2, _ = rr.vis_step(s["d"], s["w"], rows, s["a1"], s["a2"], s["group"], s["ng"])
    after = rr.chi2_rows(U2, s["d"], s["w"], rows, s["a1"], s["a2"], s["group"])
    assert np.all(np.abs(after - s["chi2"]) <= 1e-12 * s["chi2"])
    # the averaged data at the fixed gains are the model, up to a phase per unit (which cancels in every visibility)
    turn = np.exp(-1j * np.angle((U2 * np.conj(M)).sum(axis=(1, 2), keepdims=True)))
    assert np.abs(U2 * turn - M).max() <= 1e-9 * np.abs(M).max()
    # fix_redundant_degeneracies against the gains the model belongs to
    target = ar.apply(s["g"], eta, phi @ vt, pos, np.ones(eta.shape, dtype=bool))
    public = np.ascontiguousarray(s["g"][:, 0, 0].T)  # (nant, nfreqs)
    plane_fit = fftvis_amd.fix_redundant_degeneracies(public, s["ants"], ref_gains=np.ascontiguousarray(target[:, 0, 0].T))
    off = float(np.abs(plane_fit - target[:, 0, 0].T).max())
    span = float(np.ptp(x @ (phi[0, 0, 0] @ vt)))
    print("fix_redundant_degeneracies on the same case: error", off)
    assert (span > 2 * np.pi and off > 0.1) if frac == 0.6 else (span < 2 * np.pi and off <= 1e-9)


# ---- the C surface ---------------------------------------------------------------------------------------------------------
_NEW = {"fv_abscal_slopes": 28, "fv_abscal_evaluate": 8}


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftvis_hip.h")).read()
    flat = " ".join(header.split())
    for declared in ("int fv_abscal_slopes(int device, int precision, int nfreqs, int ntimes, int tpol, int ngroups, int per_time, "
                     "const void *uvis, int uvis_on_device, const void *model, int model_on_device, const void *gweights, "
                     "int gweights_on_device, const double *coords, int ndim, int n1, int n2, double h1, double h2, int refine, "
                     "int *peak_out, double *slopes_out, double *amp_out, double *power_out, double *unorm_out, double *mnorm_out, "
                     "int *used_out, double *chi2_ft_out);",
                     "int fv_abscal_evaluate(int device, int nrows, int ngroups, const void *c, const double *coords, int ndim, "
                     "const double *slopes, double *out);"):
        assert declared in flat, declared
    for name, n in _NEW.items():
        assert len(_lib.SYMBOLS[name][1]) == n and hasattr(_lib.lib(), name), name
    flat = flat.replace(" * ", " ")
    for stated in ("c_g = sum_t W conj(U) M", "S(Phi) = sum_g c_g exp(i Phi . X_g)", "eta = Re S / N", "lowest flat index i_1 n2 + i_2",
                   "a run of 8 consecutive grid points", "-H^-1 g where H is negative definite", "g / max |eig H|",
                   "clipped to +-h_i per dimension", "at least ndim + 1 groups have a used sample", "a flagged datum is not read",
                   "formed explicitly at the returned parameters", "the same input gives the same bits"):
        assert stated in flat, stated
    source = open(os.path.join(os.path.dirname(__file__), "..", "fftvis_amd", "csrc", "fv_fit.h")).read()
    assert f"constexpr int ABSCAL_RUN = {ar.RUN};" in source  # (the run length the bound e counts on)


def test_public_signature():
    own = inspect.signature(redundant.redundant_abscal).parameters
    assert list(own) == ["vis", "model", "ants", "gains", "reds", "weights", "per_time", "max_slope", "pad", "refine", "polarized",
                         "precision", "device"]
    defaults = dict(reds=None, weights=None, per_time=False, max_slope=None, pad=4, refine=6, polarized=False, precision=2, device=0)
    assert all(own[n].kind.name == "KEYWORD_ONLY" and own[n].default == v for n, v in defaults.items())
    assert all(own[n].kind.name == "POSITIONAL_OR_KEYWORD" for n in ("vis", "model", "ants", "gains"))
    assert fftvis_amd.redundant_abscal is redundant.redundant_abscal
    doc = " ".join(redundant.redundant_abscal.__doc__.split())
    for word in ("fv_abscal_slopes", "parallel hands", "simulate_vis(..., baselines=[red[0] for red in reds])", "redundant_average",
                 "shared by both feeds", "cross-hand phase", "delay slope", "rank-3 arrays", "Jones matrices", "sharding",
                 "Not differentiable", "max_slope", "2**22"):
        assert word in doc, word
    for other in (redundant.redundant_gain_solve, redundant.redundant_firstcal):
        assert "redundant_abscal" in other.__doc__
    assert "redundant_abscal" in fftvis_amd.__doc__ and "redundant_abscal" in redundant.__doc__


def test_python_argument_errors_come_before_the_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ants = array("hex19")
    ng = len(fftvis_amd.redundant_groups(ants)[0])
    v = np.zeros((3, 2, ng), complex)
    g = np.ones((19, 3), complex)
    call = fftvis_amd.redundant_abscal
    with pytest.raises(ValueError, match=re.escape(f"must have shape (nfreqs, ntimes, nbls), got (2, {ng})")):
        call(v[0], v[0], ants, g)
    with pytest.raises(ValueError, match=re.escape(f"must have shape (nfreqs, ntimes, 2, 2, nbls), got (3, 2, {ng})")):
        call(v, v, ants, g, polarized=True)
    with pytest.raises(ValueError, match=f"vis holds {ng - 1} groups, reds lists {ng}"):
        call(v[..., 1:], v[..., 1:], ants, g)
    with pytest.raises(ValueError, match=re.escape(f"model must have simulate_vis's output shape (3, 2, {ng}), got (3, 1, {ng})")):
        call(v, v[:, :1], ants, g)
    with pytest.raises(ValueError, match=re.escape(f"weights must have vis' shape (3, 2, {ng}), got (2, {ng})")):
        call(v, v, ants, g, weights=np.ones((2, ng)))
    with pytest.raises(ValueError, match="weights must be real"):
        call(v, v, ants, g, weights=np.ones(v.shape, complex))
    with pytest.raises(ValueError, match="gains must have shape"):
        call(v, v, ants, g[:, :2])
    with pytest.raises(ValueError, match="per_time=True needs per-time gains"):
        call(v, v, ants, g, per_time=True)
    for bad in (0, 2.5, -1):
        with pytest.raises(ValueError, match="pad must be a positive integer"):
            call(v, v, ants, g, pad=bad)
    for bad in (-1, 1.5, 33):
        with pytest.raises(ValueError, match=re.escape("refine must be an integer in 0 .. 32")):
            call(v, v, ants, g, refine=bad)
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_slope must be positive and finite"):
            call(v, v, ants, g, max_slope=bad)
    with pytest.raises(ValueError, match=re.escape("more than 2**22: pass a smaller max_slope")):
        call(v, v, ants, g, max_slope=40.0)
    with pytest.raises(ValueError, match="precision must be 1 or 2"):
        call(v, v, ants, g, precision=3)
    tower = dict(ants)
    tower[19] = np.array([3.0, 5.0, 40.0])
    nt = len(fftvis_amd.redundant_groups(tower)[0])
    with pytest.raises(ValueError, match="rank-3 arrays are not covered"):
        call(np.zeros((3, 2, nt), complex), np.zeros((3, 2, nt), complex), tower, np.ones((20, 3), complex))


def test_plane_and_grid_of_the_public_function_are_the_reference():
    for name, ndim in (("hex19", 2), ("rot16", 2), ("line6", 1)):
        ants = array(name)
        reds, b = group_baselines(ants)
        got_b, vt, X = redundant._abscal_plane(ants, reds)
        ref_vt, ref_X = ar.plane(b)
        assert X.shape == (len(reds), ndim) and np.array_equal(got_b, b) and np.allclose(vt, ref_vt) and np.allclose(X, ref_X)
        assert np.allclose(X @ vt, b, atol=1e-9)
        for pad, max_slope in ((4, None), (1, None), (3, 0.05)):
            n, h, ms = redundant._abscal_grid(X, b, max_slope, pad)
            rn, rh, rms = ar.grid(ref_X, b, pad, max_slope)
            assert n == rn and np.allclose(h, rh) and ms == rms and n[0] % 2 == 1 and n[1] % 2 == 1 and (ndim == 2 or n[1] == 1)
            assert all((n[i] - 1) // 2 * h[i] >= ms for i in range(ndim))  # (the box reaches max_slope)


def test_fv_abscal_slopes_argument_checks():
    L = _lib.lib()
    name = b"fv_abscal_slopes"
    buf = (ctypes.c_double * 256)()
    xy = (ctypes.c_double * 6)(1, 0, 0, 1, 1, 1)

    def call(precision=2, nfreqs=2, ntimes=1, tpol=1, ngroups=3, per_time=0, u=buf, m=buf, w=None, flags=(0, 0, 0), coords=xy, ndim=2,
             n1=3, n2=3, h1=0.1, h2=0.1, refine=2, peak=buf, slopes=buf, amp=buf, power=buf, unorm=buf, mnorm=buf, used=buf, chi2=buf):
        return L.fv_abscal_slopes(0, precision, nfreqs, ntimes, tpol, ngroups, per_time, u, flags[0], m, flags[1], w, flags[2], coords, ndim,
                                  n1, n2, h1, h2, refine, peak, slopes, amp, power, unorm, mnorm, used, chi2)

    for precision in (0, 3):
        assert call(precision=precision) == 1 and b"precision must be 1 or 2" in L.fv_last_error()
    for tpol in (0, 2, 3, 5):
        assert call(tpol=tpol) == 1 and name + b": tpol must be 1 or 4" in L.fv_last_error()
    for kw in (dict(nfreqs=-1), dict(ntimes=-1), dict(ngroups=-1), dict(nfreqs=1 << 15, ntimes=1 << 15)):
        assert call(**kw) == 1 and name + b": negative shape" in L.fv_last_error()
    for bad in (-1, 2):
        assert call(per_time=bad) == 1 and name + b": per_time must be 0 or 1" in L.fv_last_error()
    for bad in (0, 3):
        assert call(ndim=bad) == 1 and name + b": ndim must be 1 or 2" in L.fv_last_error()
    for kw in (dict(n1=0), dict(n2=-1), dict(n1=4), dict(n2=2)):
        assert call(**kw) == 1 and name + b": n1 and n2 must be positive and odd" in L.fv_last_error()
    assert call(n1=2049, n2=2049) == 1 and name + b": the grid n1 n2 must not exceed 2^22 points" in L.fv_last_error()
    assert call(ndim=1, n2=3) == 1 and name + b": n2 must be 1 for ndim 1" in L.fv_last_error()
    for kw in (dict(h1=0.0), dict(h1=float("nan")), dict(h2=-1.0), dict(h2=float("inf"))):
        assert call(**kw) == 1 and name + b": the grid steps must be positive and finite" in L.fv_last_error()
    for bad in (-1, 33):
        assert call(refine=bad) == 1 and name + b": refine must lie in 0 .. 32" in L.fv_last_error()
    for flags in ((2, 0, 0), (0, -1, 0), (0, 0, 4)):
        assert call(flags=flags) == 1 and name + b": the on_device flags must be 0 or 1" in L.fv_last_error()
    for kw in (dict(peak=None), dict(slopes=None), dict(amp=None), dict(power=None), dict(unorm=None), dict(mnorm=None), dict(used=None),
               dict(chi2=None)):
        assert call(**kw) == 1 and name + b": null peak_out, slopes_out, amp_out" in L.fv_last_error()
    for kw in (dict(u=None), dict(m=None), dict(coords=None)):
        assert call(**kw) == 1 and name + b": null uvis, model or coords" in L.fv_last_error()
    bent = (ctypes.c_double * 6)(1, 0, float("nan"), 1, 1, 1)
    assert call(coords=bent) == 1 and name + b": coords must be finite" in L.fv_last_error()
    # no group, and no sample: the neutral result, without a device
    for kw, units in ((dict(ngroups=0, u=None, m=None, coords=None), 2), (dict(nfreqs=2, ntimes=3, tpol=4, per_time=1, ngroups=0), 12)):
        outs = [np.full((units, 2), 7, dtype=np.int32), np.full((units, 2), 7.0), np.full(units, 7.0), np.full(units, 7.0), np.full(units, 7.0),
                np.full(units, 7.0), np.full(units, 7, dtype=np.int32), np.full(6, 7.0)]
        keys = ("peak", "slopes", "amp", "power", "unorm", "mnorm", "used", "chi2")
        assert call(**kw, **{k: _lib.ptr(o) for k, o in zip(keys, outs)}) == 0, L.fv_last_error()
        nft = 2 * kw.get("ntimes", 1)
        assert np.all(outs[2] == 1.0) and not any(o.any() for i, o in enumerate(outs[:7]) if i != 2) and not outs[7][:nft].any()
    assert call(nfreqs=0, peak=None, slopes=None, amp=None, power=None, unorm=None, mnorm=None, used=None, chi2=None) == 0, L.fv_last_error()


def test_fv_abscal_evaluate_argument_checks():
    L = _lib.lib()
    name = b"fv_abscal_evaluate"
    buf = (ctypes.c_double * 64)()
    xy = (ctypes.c_double * 6)(1, 0, 0, 1, 1, 1)

    def call(nrows=2, ngroups=3, c=buf, coords=xy, ndim=2, slopes=buf, out=buf):
        return L.fv_abscal_evaluate(0, nrows, ngroups, c, coords, ndim, slopes, out)

    for kw in (dict(nrows=-1), dict(ngroups=-1)):
        assert call(**kw) == 1 and name + b": negative shape" in L.fv_last_error()
    for bad in (0, 3):
        assert call(ndim=bad) == 1 and name + b": ndim must be 1 or 2" in L.fv_last_error()
    for kw in (dict(slopes=None), dict(out=None)):
        assert call(**kw) == 1 and name + b": null slopes or out" in L.fv_last_error()
    for kw in (dict(c=None), dict(coords=None)):
        assert call(**kw) == 1 and name + b": null c or coords" in L.fv_last_error()
    bent = (ctypes.c_double * 6)(1, 0, float("inf"), 1, 1, 1)
    assert call(coords=bent) == 1 and name + b": coords must be finite" in L.fv_last_error()
    # no row, and no group: valid calls that need no device
    assert call(nrows=0, c=None, coords=None, slopes=None, out=None) == 0, L.fv_last_error()
    out = np.full((2, 6), 7.0)
    assert call(ngroups=0, c=None, coords=None, out=_lib.ptr(out)) == 0 and not out.any(), L.fv_last_error()
