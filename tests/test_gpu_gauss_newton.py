"""GPU tests of the Gauss-Newton product (``simulate_vis_gauss_newton``, ``fv_sim_weight_block`` and the kernel pair alone
through ``fv_weight_rows``).

The kernel pair is held to its stated arithmetic: U = ((P_0 + P_1) + P_2) + P_3 and G = 2 (w U) in the run's precision T
are reproduced bit for bit by numpy doing the same operations in T (``gauss_newton_refs.weight_rows``); the rows' sums add
non-negative fp64 terms, so by ``test_gpu_objective``'s derivation they stay within ``(row_len + 4) 2^-52`` of ``math.fsum`` of
the terms formed from that U.  Through the engine G and the rows are held to ``test_gpu_objective.BOUND`` against the
composition of the public jvp calls (one per part, summed and weighted in numpy), on directions chosen so that
||U|| >= 0.1 sum ||parts||, and every product to the public pass that owns it, applied to the returned G: bit for bit, the
fluxes under ``test_gpu_sky_adjoint._same_flux``."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from oracle import fftvis_oracle as orc
from tests import basis_source_refs as bsr
from tests import gauss_newton_refs as gnr
from tests.helpers import rel_l2
from tests.objective_refs import row_major_sum, row_sums_exact
from tests.source_adjoint_refs import source_config
from tests.tangent_refs import edge_config, hex19_config
from tests.test_gpu_adjoint import _up
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_lattice_adjoint import _handle
from tests.test_gpu_objective import BASIS_WRT, BOUND, CDT, RDT, ROW_LENS, WRT, _public
from tests.test_gpu_position_adjoint import K32
from tests.test_gpu_sky_adjoint import _same_flux
from tests.test_gpu_source_adjoint import _edge_cfg, _sid

pytestmark = pytest.mark.gpu


# ---- 1. the kernel pair alone --------------------------------------------------------------------------------------------
def _kernel_inputs(nrows, row_len, nparts, precision, weights, seed=0):
    rng = np.random.default_rng(seed + row_len + 7 * nparts)
    shape = (nrows, row_len)
    parts = [(rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(CDT[precision]) for _ in range(nparts)]
    if weights == "none":
        return parts, None
    w = rng.uniform(0.5, 2.0, size=shape).astype(RDT[precision])
    if weights == "flags":
        flagged = rng.random(shape) < 0.3
        flagged[0, 0] = True
        w[flagged] = 0
        for p in parts:
            p[flagged] = np.where(rng.random(int(flagged.sum())) < 0.5, complex(np.nan, 0.0), complex(np.inf, -np.inf))
    return parts, w


def _weight_rows(parts, w, precision):
    own = [p.copy() for p in parts]
    q = np.full(parts[0].shape[0], -1.0)
    ptrs = (ctypes.c_void_p * len(own))(*[p.ctypes.data for p in own])
    status = _lib.lib().fv_weight_rows(0, precision, parts[0].shape[0], parts[0].shape[1], len(own), ptrs, _lib.ptr(w),
                                       _lib.ptr(q))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(own[1:], parts[1:]))  # read only
    return status, own[0], q


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nparts", [1, 2, 4])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_kernel_pair(gpu, row_len, nrows, nparts, precision, weights):
    parts, w = _kernel_inputs(nrows, row_len, nparts, precision, weights)
    status, G, q = _weight_rows(parts, w, precision)
    assert status == 0, _lib.lib().fv_last_error()
    G_ref, U, terms = gnr.weight_rows(parts, w)
    assert G.dtype == G_ref.dtype and np.array_equal(G, G_ref)  # bit for bit (neither side holds a NaN)
    used = np.ones(G.shape, bool) if w is None else w != 0
    assert np.all(G[~used] == 0) and (weights != "flags" or (~used).sum() > 0) and np.isfinite(G).all()
    exact = row_sums_exact(terms)
    print("weight rows q", row_len, nrows, nparts, precision, weights,
          float((np.abs(q - exact) / np.maximum(exact, 1e-300)).max() / 2.0**-52))
    assert np.all(exact > 0) or weights == "flags"
    assert np.all(np.abs(q - exact) <= (row_len + 4) * 2.0**-52 * exact)
    status, G2, q2 = _weight_rows(parts, w, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(G2, G) and np.array_equal(q2, q)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what", ["negative weight", "nan weight"])
def test_bad_weight_fails_the_call_and_the_next_good_call_reproduces_its_bits(gpu, what, precision):
    parts, w = _kernel_inputs(3, 300, 2, precision, "positive")
    good = _weight_rows(parts, w, precision)
    assert good[0] == 0
    bw = w.copy()
    if what == "negative weight":
        bw[1, 257] = -1.0
    else:
        bw[2, 7] = np.nan
    status = _weight_rows(parts, bw, precision)[0]
    assert status == 1 and b"1 weights are negative or not finite" in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    again = _weight_rows(parts, w, precision)
    assert again[0] == 0 and np.array_equal(again[1], good[1]) and np.array_equal(again[2], good[2])


# ---- 2. through the engine -----------------------------------------------------------------------------------------------
def _gn(cfg, **kw):
    return fftvis_amd.simulate_vis_gauss_newton(**cfg, **kw)


def _directions(cfg, seed=11, basis=False):
    """A direction of every parameter block: the fluxes scaled source by source by 0.3 N(0, 1), centimetres of antenna
    motion, milliradians of source motion, and with basis beams 0.1 (N + i N) of coefficient change."""
    rng = np.random.default_rng(seed)
    F = np.asarray(cfg["fluxes"])
    d = dict(d_fluxes=F * 0.3 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1)),
             d_ants=1e-2 * rng.normal(size=(len(cfg["ants"]), 3)), d_radec=1e-3 * rng.normal(size=(F.shape[0], 2)))
    if basis:
        c = np.asarray(cfg["beam_coefs"])
        d["d_beam_coefs"] = 0.1 * (rng.normal(size=c.shape) + 1j * rng.normal(size=c.shape))
    return d


def _weights(cfg, seed=5):
    nbls = len(cfg["baselines"])
    shape = (len(cfg["freqs"]), len(np.atleast_1d(cfg["times"]))) + ((2, 2, nbls) if cfg["polarized"] else (nbls,))
    return np.random.default_rng(seed).uniform(0.5, 2.0, size=shape).astype(RDT[cfg.get("precision", 2)])


def _composition(cfg, dirs, basis=False):
    """The parts of U from the public jvp calls, one per tangent pass of the engine, in fp64."""
    parts = []
    jvp = fftvis_amd.simulate_vis_basis_jvp if basis else fftvis_amd.simulate_vis_jvp
    pos = {k: dirs[k] for k in ("d_ants", "d_baselines") if k in dirs}
    src = {k: dirs[k] for k in ("d_radec", "d_topo") if k in dirs}
    if "d_fluxes" in dirs:
        parts.append(jvp(**cfg, d_fluxes=dirs["d_fluxes"]))
    if "d_beam_coefs" in dirs:
        parts.append(jvp(**cfg, d_beam_coefs=dirs["d_beam_coefs"]))
    if basis:
        if pos:
            parts.append(jvp(**cfg, **pos))
        if src:
            parts.append(fftvis_amd.simulate_vis_basis_source_jvp(**cfg, **src))
    elif pos or src:
        parts.append(jvp(**cfg, **pos, **src))
    return [np.asarray(p).astype(np.complex128) for p in parts]


def _assert_value(label, cfg, dirs, w, quad_ft, G, basis=False):
    p = cfg.get("precision", 2)
    parts = _composition(cfg, dirs, basis)
    U = sum(parts)
    ref_rows, G_ref = gnr.quad_and_gvis(U, w)
    cond = np.linalg.norm(U) / sum(np.linalg.norm(x) for x in parts)
    print("gauss-newton value", label, rel_l2(G, G_ref), float((np.abs(quad_ft - ref_rows) / ref_rows).max()), cond)
    assert cond >= 0.1  # nothing rides on cancellation
    assert G.shape == U.shape and G.dtype == CDT[p]
    assert rel_l2(G, G_ref) <= BOUND[p]
    assert quad_ft.shape == U.shape[:2] and quad_ft.dtype == np.float64
    assert np.all(ref_rows > 0) and np.all(np.abs(quad_ft - ref_rows) <= BOUND[p] * ref_rows)


CELLS = [("unpol", "airy"), ("I", "two"), ("full", "complex")]


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_value(gpu, monkeypatch, precision, sky, beams):
    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w = _directions(cfg), _weights(cfg)
    quad_ft, prods, G = _gn(cfg, **dirs, weights=w, wrt=(), quad_per="freq_time", return_gvis=True)
    assert prods == ()
    _assert_value(f"{precision} {sky} {beams}", cfg, dirs, w, quad_ft, G)
    one = {"d_fluxes": dirs["d_fluxes"]}  # one part, no weights: G = 2 U
    quad_ft, _, G = _gn(cfg, **one, wrt=(), quad_per="freq_time", return_gvis=True)
    _assert_value(f"{precision} {sky} {beams} fluxes", cfg, one, None, quad_ft, G)
    # the total is the rows' sums of the same call, added in row-major order
    rows = []
    real = gs.SimHandle.weight_block
    monkeypatch.setattr(gs.SimHandle, "weight_block", lambda self, *a, **k: rows.append(real(self, *a, **k)) or rows[-1])
    total, prods = _gn(cfg, **dirs, weights=w, wrt=())
    assert isinstance(total, float) and prods == () and len(rows) == 1 and total == row_major_sum(rows[0]) and total > 0


def _assert_products(label, cfg, dirs, w, names, basis=False, **kw):
    quad, prods, G = _gn(cfg, **dirs, weights=w, wrt=names, return_gvis=True, **kw)
    single = isinstance(names, str)
    names = (names,) if single else names
    prods = (prods,) if single else prods
    assert isinstance(prods, tuple) and len(prods) == len(names) and np.isfinite(quad) and quad > 0
    want = _public(cfg, G, names, basis)
    for n, g in zip(names, prods):
        assert g.shape == want[n].shape and g.dtype == want[n].dtype and np.count_nonzero(want[n]) > 0, (label, n)
        print("gauss-newton product", label, names, n, float(np.abs(g - want[n]).max() / np.abs(want[n]).max()))
        if n == "fluxes":
            assert _same_flux(g, want[n]), (label, names)
        else:
            assert np.array_equal(g, want[n]), (label, names, n)
    return G


@pytest.mark.parametrize("beams", ["airy", "two", "complex"])
@pytest.mark.parametrize("sky", ["unpol", "I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_products_are_the_public_passes_on_gvis(gpu, monkeypatch, precision, sky, beams):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w = _directions(cfg), _weights(cfg)
    for names in WRT:
        _assert_products(f"{precision} {sky} {beams}", cfg, dirs, w, names)


@pytest.mark.parametrize("precision", [2, 1])
def test_basis_beams(gpu, monkeypatch, precision):
    """K = 3 complex tables, a full-Stokes sky, the exact form of the (l, k) terms; four parts."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    assert cfg["beam_coefs"].shape[1] == 3
    dirs, w = _directions(cfg, basis=True), _weights(cfg)
    quad_ft, _, G = _gn(cfg, **dirs, weights=w, wrt=(), quad_per="freq_time", return_gvis=True)
    _assert_value(f"basis {precision}", cfg, dirs, w, quad_ft, G, basis=True)
    for names in BASIS_WRT:
        _assert_products(f"basis {precision}", cfg, dirs, w, names, basis=True)


def _quadratic_form(label, cfg, dirs, w, basis=False):
    """sum_names <d_name, prods[name]> against 2 quad, wrt naming exactly the directions given.  Each side is a chain of
    passes held to k base times its cancellation (``test_gpu_tangent.test_dot_identity_with_the_device_adjoints``), so the
    difference is held to k base times the norm products the two sides are rounded in."""
    p = cfg.get("precision", 2)
    quad, prods, G = _gn(cfg, **dirs, weights=w, return_gvis=True)
    order = [k for k in ("d_ants", "d_baselines", "d_radec", "d_topo", "d_fluxes", "d_beam_coefs") if k in dirs]
    assert isinstance(prods, tuple) and len(prods) == len(order) and quad > 0
    lhs = sum(gnr.inner(dirs[k], g) for k, g in zip(order, prods))
    U = G.astype(np.complex128) / (2 * w.astype(np.float64))
    k = 10.0 if p == 2 else K32
    bound = k * _forward_base(cfg) * (np.linalg.norm(G) * np.linalg.norm(U) +
                                      sum(np.linalg.norm(dirs[n]) * np.linalg.norm(g) for n, g in zip(order, prods)))
    print("gauss-newton quadratic form", label, lhs, 2 * quad, abs(lhs - 2 * quad) / bound)
    assert abs(lhs - 2 * quad) <= bound, (lhs, 2 * quad, bound)


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_quadratic_form(gpu, precision, sky, beams):
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    dirs, w = _directions(cfg), _weights(cfg)
    _quadratic_form(f"{precision} {sky} {beams}", cfg, dirs, w)
    _quadratic_form(f"{precision} {sky} {beams} ants", cfg, {"d_ants": dirs["d_ants"]}, w)


@pytest.mark.parametrize("precision", [2, 1])
def test_quadratic_form_basis_beams(gpu, precision):
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    dirs, w = _directions(cfg, basis=True), _weights(cfg)
    _quadratic_form(f"basis {precision}", cfg, dirs, w, basis=True)
    _quadratic_form(f"basis {precision} coefs", cfg, {"d_beam_coefs": dirs["d_beam_coefs"]}, w, basis=True)


def test_small_hessian(gpu):
    """8 sources, 1 channel, 1 time, 6 baselines, Stokes-I fluxes, fp64 at eps 1e-12: H assembled column by column from
    unit ``d_fluxes`` is symmetric and equals 2 Re(J^H W J) with J's columns from ``simulate_vis`` on unit fluxes."""
    cfg = edge_config(nsrc=8, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)],
               coord_method="SiderealRotation")
    cfg["fluxes"] = np.ascontiguousarray(synth.catalog(8, cfg["freqs"], 0, polarized_sky=True)[2][..., 0])
    assert cfg["fluxes"].shape == (8, 1)
    w = _weights(cfg)
    unit = np.eye(8)[:, :, None]
    H = np.stack([_gn(cfg, d_fluxes=unit[j], weights=w, wrt="fluxes")[1][:, 0] for j in range(8)], axis=1)
    J = np.stack([fftvis_amd.simulate_vis(**dict(cfg, fluxes=unit[j])).ravel() for j in range(8)], axis=1)
    H_ref = 2 * (J.conj().T @ (w.ravel()[:, None] * J)).real
    norm = np.linalg.norm(H_ref)
    print("gauss-newton small hessian", np.linalg.norm(H - H.T) / norm, np.linalg.norm(H - H_ref) / norm)
    assert np.linalg.norm(H - H.T) <= 10 * BOUND[2] * norm
    assert np.linalg.norm(H - H_ref) <= 10 * BOUND[2] * norm
    assert np.all(np.diag(H) >= 0) and np.trace(H) > 0


# ---- 3. edge cases -------------------------------------------------------------------------------------------------------
def test_time_blocks_and_a_streamed_coord_mgr(gpu, monkeypatch):
    """A coordinate manager streamed one time step per block against the same manager in one block."""
    from fftvis_amd.gpu import gpu_simulate
    from oracle import astrometry as oa

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg(ntimes=3)
    eq = orc.eq_unit_vectors(cfg["ra"], cfg["dec"])
    ctxs = np.stack([oa.plausible_context(20 + t, synth.HERA_LAT) for t in range(3)])

    class Mgr:  # the slice of matvis' manager the engine consumes
        times = cfg["times"]

        def setup(self):
            pass

        def rotate(self, ti):
            self.all_coords_topo = oa.icrs_to_enu(eq, ctxs[ti])

    kw = dict(cfg, coord_method="CoordinateRotationERFA")
    rng = np.random.default_rng(3)
    d = _directions(cfg)
    dirs = dict(d_fluxes=d["d_fluxes"], d_topo=1e-3 * rng.normal(size=(3, 24, 3)),
                d_baselines=1e-2 * rng.normal(size=(len(cfg["baselines"]), 3)))
    w = _weights(cfg)
    names = ("fluxes", "topo", "baselines")
    one = _gn(kw, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True, coord_mgr=Mgr())
    calls = []
    real = gpu_simulate.SimHandle.weight_block
    monkeypatch.setattr(gpu_simulate.SimHandle, "weight_block",
                        lambda self, *a, **k: calls.append((a[0], a[1], len(a[4]), tuple(a[5].shape))) or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    blk = _gn(kw, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True, coord_mgr=Mgr())
    assert calls == [(0, 1, 2, (3, 1, 2, 2, w.shape[-1]))] * 3, calls
    print("gauss-newton time blocks", float((np.abs(blk[0] - one[0]) / one[0]).max()), rel_l2(blk[2], one[2]),
          [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(blk[1], one[1])])
    assert np.all(one[0] > 0) and np.all(np.abs(blk[0] - one[0]) <= 1e-12 * one[0])
    assert rel_l2(blk[2], one[2]) <= 1e-12
    for a, b in zip(blk[1], one[1]):
        assert np.count_nonzero(b) > 0 and np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    with pytest.raises(ValueError, match="wrt='topo'"):
        _gn(kw, **dirs, weights=w, wrt=("fluxes", "radec"), coord_mgr=Mgr())


def test_time_blocks_are_sized_for_the_parts_and_the_weights(gpu, monkeypatch):
    """``_time_block`` sees one block per part per channel plus half a block of weights; the forward sees what it saw."""
    from fftvis_amd.gpu import gpu_simulate

    cfg = _edge_cfg()
    dirs, w = _directions(cfg), _weights(cfg)
    seen = []
    real = gpu_simulate._time_block
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: seen.append(a[2]) or real(*a, **k))
    _gn(cfg, **dirs, weights=w, wrt=())                  # two parts and weights: 2.5 blocks
    _gn(cfg, d_fluxes=dirs["d_fluxes"], wrt=())          # one part
    fftvis_amd.simulate_vis(**cfg)
    assert seen == [8, 3, 3], seen


def test_source_chunks_a_source_that_never_rises_and_an_empty_time_step(gpu, monkeypatch):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg(nsrc=20)
    t0 = cfg["times"][0]
    lst = orc.gmst_rad(t0) + synth.HERA_LON
    rng = np.random.default_rng(1)
    ra, dec = lst + rng.uniform(-0.3, 0.3, 20), synth.HERA_LAT + rng.uniform(-0.3, 0.3, 20)
    dec[-1] = np.radians(80.0)  # never rises at HERA's latitude
    cfg.update(ra=ra, dec=dec, times=t0 + np.array([0.0, 0.25, 0.5]), min_chunks=3)
    up = _up(cfg)
    assert not np.any(up[:, -1] > 0) and not np.any(up[2] > 0) and np.all(up[0, :-1] > 0)
    dirs, w = _directions(cfg), _weights(cfg)
    names = ("fluxes", "topo", "ants")
    G = _assert_products("chunks, never rises", cfg, dirs, w, names)
    quad_ft, (gf, gt, ga), _ = _gn(cfg, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    # the empty step: U = 0 there, so G = 0 and its rows of quad are 0, exactly
    assert np.all(G[:, 2] == 0) and np.all(quad_ft[:, 2] == 0) and np.all(quad_ft[:, :2] > 0)
    assert np.all(gf[-1] == 0) and np.all(gt[:, -1] == 0) and np.all(gt[2] == 0) and np.all(gt[up <= 0] == 0)
    sub = dict(cfg, times=cfg["times"][:2])
    parts = _composition(sub, dirs)
    ref_rows, G_ref = gnr.quad_and_gvis(sum(parts), w[:, :2])
    assert rel_l2(G[:, :2], G_ref) <= BOUND[2] and np.all(np.abs(quad_ft[:, :2] - ref_rows) <= BOUND[2] * ref_rows)


def test_flagged_samples(gpu, monkeypatch):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg()
    dirs, w = _directions(cfg), _weights(cfg)
    names = ("fluxes", "ants", "radec")
    _, _, G_all = _gn(cfg, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    flagged = np.random.default_rng(2).random(w.shape) < 0.3
    wf = w.copy()
    wf[flagged] = 0
    quad_ft, prods, G = _gn(cfg, **dirs, weights=wf, wrt=names, quad_per="freq_time", return_gvis=True)
    assert np.isfinite(quad_ft).all() and all(np.isfinite(g).all() and np.count_nonzero(g) for g in prods)
    assert np.all(G[flagged] == 0) and np.all(G[~flagged] != 0)
    assert np.array_equal(G[~flagged], G_all[~flagged])  # the unflagged samples: the same bits
    _assert_value("flags", cfg, dirs, wf, quad_ft, G)
    with pytest.raises(_lib.FftvisHipError, match="weights are negative or not finite"):
        _gn(cfg, **dirs, weights=-w, wrt=())
    again = _gn(cfg, **dirs, weights=wf, wrt=(), quad_per="freq_time")[0]  # the handle stays usable
    assert np.all(np.abs(again - quad_ft) <= BOUND[2] * quad_ft)


def test_device_tensors(gpu):
    import torch

    cfg = _edge_cfg()
    d, w = _directions(cfg), _weights(cfg)
    rng = np.random.default_rng(8)
    dirs = dict(d_fluxes=d["d_fluxes"], d_baselines=1e-2 * rng.normal(size=(len(cfg["baselines"]), 3)),
                d_topo=1e-3 * rng.normal(size=(2, 24, 3)))
    names = ("fluxes", "ants", "topo")
    quad_ft, prods, G = _gn(cfg, **dirs, weights=w, wrt=names, quad_per="freq_time", return_gvis=True)
    D = {k: torch.from_numpy(v).cuda() for k, v in dirs.items()}
    W = torch.from_numpy(w).cuda()
    dq, dp, dG = _gn(cfg, **D, weights=W, wrt=names, quad_per="freq_time", return_gvis=True)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dq, dG) + tuple(dp))
    assert np.all(np.abs(dq.cpu().numpy() - quad_ft) <= BOUND[2] * quad_ft) and rel_l2(dG.cpu().numpy(), G) <= BOUND[2]
    for a, b in zip(dp, prods):
        assert a.dtype == torch.float64 and rel_l2(a.cpu().numpy(), b) <= BOUND[2]
    total = _gn(cfg, **D, weights=W, wrt=())[0]  # resident tensors serve the next product; the total is a float
    assert isinstance(total, float) and abs(total - quad_ft.sum()) <= BOUND[2] * total
    mixed = _gn(cfg, **dirs, weights=W, wrt=(), quad_per="freq_time")[0]  # host directions next to device weights
    assert mixed.device.type == "cuda" and np.all(np.abs(mixed.cpu().numpy() - quad_ft) <= BOUND[2] * quad_ft)
    H = {k: torch.from_numpy(v) for k, v in dirs.items()}
    hq, hp, hG = _gn(cfg, **H, weights=torch.from_numpy(w), wrt=names, quad_per="freq_time", return_gvis=True)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cpu" for x in (hq, hG) + tuple(hp))
    assert rel_l2(hG.numpy(), G) <= BOUND[2] and all(rel_l2(a.numpy(), b) <= BOUND[2] for a, b in zip(hp, prods))
    with pytest.raises(ValueError, match="a direction or the weights lives on cuda:0, the run is on cuda:1"):
        _gn(cfg, **dirs, weights=W, device=1)


@pytest.mark.parametrize("path,took", [("type3", 3), ("type2", 2), ("auto", 2)])
def test_lattice_forward_is_type1_for_the_fluxes(gpu, monkeypatch, path, took):
    """An ideal flat hex-19: with ``d_fluxes`` and ``wrt="fluxes"`` alone the handle is a lattice handle -- the forward is
    the type-1 transform, and only such a handle takes the type-2 adjoint."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = hex19_config()
    dirs, w = {"d_fluxes": _directions(cfg)["d_fluxes"]}, _weights(cfg)
    quad_ft, gf, G = _gn(cfg, **dirs, weights=w, wrt="fluxes", quad_per="freq_time", return_gvis=True, adjoint_path=path)
    assert _handle().last_adjoint_path() == took
    _assert_value(f"lattice {path}", cfg, dirs, w, quad_ft, G)
    no_flux = {k: v for k, v in cfg.items() if k != "fluxes"}
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **no_flux, adjoint_path=path))


def test_lattice_with_positions_is_the_type3_composition(gpu, monkeypatch):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = hex19_config()
    t3 = dict(cfg, force_use_type3=True)
    d, w = _directions(cfg), _weights(cfg)
    dirs = dict(d_fluxes=d["d_fluxes"], d_ants=d["d_ants"])
    quad_ft, (gf, ga), G = _gn(cfg, **dirs, weights=w, wrt=("fluxes", "ants"), quad_per="freq_time", return_gvis=True)
    _assert_value("lattice, positions", t3, dirs, w, quad_ft, G)
    assert np.array_equal(ga, fftvis_amd.simulate_vis_position_adjoint(G, **t3, wrt="ants"))
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **{k: v for k, v in t3.items() if k != "fluxes"}))
    with pytest.raises(ValueError, match="adjoint_path='type2' needs the lattice path"):
        _gn(cfg, **dirs, weights=w, adjoint_path="type2")
    with pytest.raises(ValueError, match="adjoint_path='type2' needs the lattice path"):
        _gn(cfg, d_fluxes=d["d_fluxes"], wrt=("fluxes", "ants"), adjoint_path="type2")


def test_staged_weights_are_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the forward."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    dirs, w = _directions(cfg), _weights(cfg)
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _gn(cfg, **dirs, weights=w, wrt=())
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)
    after = held.value
    # the rule covers what the fused objective staged on the same handle: whichever call came last, the same bytes stay
    monkeypatch.delenv("FFTVIS_HIP_ADJ_KEEP_BYTES")
    data = fftvis_amd.simulate_vis(**cfg)
    fftvis_amd.simulate_vis_chi2(data, **cfg, weights=w, wrt=())  # (under the default limit its staged data stay)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - after >= data.nbytes, (after, held.value)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    _gn(cfg, **dirs, weights=w, wrt=())
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - after < data.nbytes // 2, (after, held.value)  # (less than the staged weights alone)


def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu, monkeypatch):
    """The catalog's fluxes are back after the forward part ran on ``d_fluxes``."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _edge_cfg()
    dirs, w = _directions(cfg), _weights(cfg)
    V = fftvis_amd.simulate_vis(**cfg)
    _gn(cfg, **dirs, weights=w)
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), V)


def test_raw_c_abi(gpu):
    """``fv_sim_weight_block`` on the cached handle the last Python call configured: device parts, host and device weights,
    a block of the channels, and the errors a configured handle raises."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    L = _lib.lib()
    fn = L.fv_sim_weight_block
    cfg = _edge_cfg()
    nf, nt, nbls = len(cfg["freqs"]), len(cfg["times"]), len(cfg["baselines"])
    shape = (nf, nt, 2, 2, nbls)
    rng = np.random.default_rng(9)
    parts = [rng.normal(size=shape) + 1j * rng.normal(size=shape) for _ in range(3)]
    w = _weights(cfg)
    w[0, 0, 0, 0, 0] = 0
    G_ref, _, terms = gnr.weight_rows([p.reshape(nf * nt, -1) for p in parts], w.reshape(nf * nt, -1))
    q_ref = row_sums_exact(terms).reshape(nf, nt)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dev = lambda: [torch.from_numpy(p).cuda() for p in parts]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    gs.release_handles()
    fftvis_amd.simulate_vis(**cfg)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        for on_device in (0, 1):
            ts, q = dev(), np.full((nf, nt), -1.0)
            W = torch.from_numpy(w).cuda()
            torch.cuda.synchronize()
            wp = ctypes.c_void_p(W.data_ptr()) if on_device else hp(w)
            assert fn(h._h, 0, nt, 0, nf, 3, ptrs(ts), wp, on_device, hp(q)) == 0, L.fv_last_error()
            assert np.array_equal(ts[0].cpu().numpy().reshape(nf * nt, -1), G_ref) and ts[0][0, 0, 0, 0, 0] == 0
            assert np.all(np.abs(q - q_ref) <= (4 * nbls + 4) * 2.0**-52 * q_ref)
            assert all(np.array_equal(t.cpu().numpy(), p) for t, p in zip(ts[1:], parts[1:]))  # read only
        # one channel, the second time step, one part, no weights: an exact doubling
        blk = torch.from_numpy(np.ascontiguousarray(parts[0][1:2, 1:2])).cuda()
        torch.cuda.synchronize()
        q1 = np.full((1, 1), -1.0)
        assert fn(h._h, 1, 2, 1, 2, 1, ptrs([blk]), None, 0, hp(q1)) == 0, L.fv_last_error()
        assert np.array_equal(blk.cpu().numpy(), 2 * parts[0][1:2, 1:2])
        own = np.sum(np.abs(parts[0][1, 1]) ** 2)
        assert abs(q1[0, 0] - own) <= 1e-13 * own
        ts, q = dev(), np.full((nf, nt), -1.0)
        torch.cuda.synchronize()
        for t0, t1, f0, f1 in [(1, 1, 0, nf), (0, nt, 2, 2)]:
            assert fn(h._h, t0, t1, f0, f1, 3, ptrs(ts), None, 0, hp(q)) == 1
            assert b"empty range" in L.fv_last_error()
        assert fn(h._h, 0, nt + 1, 0, nf, 3, ptrs(ts), None, 0, hp(q)) == 1
        assert b"time range" in L.fv_last_error()
        bad = w.copy()
        bad[1, 0, 0, 0, 0] = -1.0
        assert fn(h._h, 0, nt, 0, nf, 3, ptrs(ts), hp(bad), 0, hp(q)) == 1
        assert b"weights are negative or not finite" in L.fv_last_error()
        ts = dev()
        torch.cuda.synchronize()
        assert fn(h._h, 0, nt, 0, nf, 3, ptrs(ts), hp(w), 0, hp(q)) == 0, L.fv_last_error()
        assert np.array_equal(ts[0].cpu().numpy().reshape(nf * nt, -1), G_ref)
    finally:
        gs._return_handle(key, h)
        gs.release_handles()


def test_hera350_rows_span_many_blocks(gpu):
    """350 antennas, 1 000 sources, two channels, one time, polarized: rows of 244 300 values, 120 blocks each."""
    cfg = synth.make_config("C3", nsrc=1000, nfreq=2, ntimes=1)
    assert 4 * len(cfg["baselines"]) == 244_300
    rng = np.random.default_rng(4)
    F = np.asarray(cfg["fluxes"])
    dirs = {"d_fluxes": F * 0.3 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1))}
    w = _weights(cfg)
    w[rng.random(w.shape) < 0.1] = 0
    quad_ft, gf, G = _gn(cfg, **dirs, weights=w, wrt="fluxes", quad_per="freq_time", return_gvis=True)
    U = fftvis_amd.simulate_vis(**dict(cfg, fluxes=dirs["d_fluxes"]))
    ref_rows, G_ref = gnr.quad_and_gvis(U, w)
    print("gauss-newton hera350", rel_l2(G, G_ref), float((np.abs(quad_ft - ref_rows) / ref_rows).max()))
    assert rel_l2(G, G_ref) <= BOUND[2] and np.all(np.abs(quad_ft - ref_rows) <= BOUND[2] * ref_rows)
    assert np.all(G[w == 0] == 0)
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **{k: v for k, v in cfg.items() if k != "fluxes"}))
