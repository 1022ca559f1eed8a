"""GPU tests of the fused objective (``simulate_vis_chi2``, ``torch_simulate_vis_chi2``, ``fv_sim_run_residual`` and the
kernel pair alone through ``fv_residual_chi2``).

The kernel pair is held to bounds derived from its arithmetic: G = 2 w (V - d) is two roundings and an exact doubling in
the run's precision T, so ``|G - G_ref| <= 2 eps_T |G_ref|`` against the fp64 value of the same T-typed inputs; the rows'
sums add non-negative fp64 terms, so any order stays within ``(row_len - 1) 2^-53`` of the exact sum, and the terms
themselves (three roundings on the device, four in numpy) within ``3.5 * 2^-52``: ``(row_len + 4) 2^-52`` relative to
``math.fsum``.  Through the engine the value is held to ten times the project's bound for two runs of one forward
(``test_gpu_parity``: 1e-12 in fp64, 1e-5 in fp32), the data being chosen so that ||G|| >= 0.1 ||2 w V||, and every gradient
to the public pass that owns it, applied to the returned G: bit for bit, the fluxes under ``test_gpu_sky_adjoint._same_flux``."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from oracle import fftvis_oracle as orc
from tests import basis_source_refs as bsr
from tests.helpers import rel_l2
from tests.objective_refs import chi2_and_gvis, row_major_sum, row_sums_exact
from tests.source_adjoint_refs import gradcheck_config, source_config
from tests.tangent_refs import hex19_config
from tests.test_gpu_adjoint import _up
from tests.test_gpu_lattice_adjoint import _handle
from tests.test_gpu_sky_adjoint import _same_flux
from tests.test_gpu_source_adjoint import _edge_cfg, _sid

pytestmark = pytest.mark.gpu

BOUND = {2: 1e-11, 1: 1e-4}  # ten times test_gpu_parity's bound for two runs of one forward
CDT = {1: np.complex64, 2: np.complex128}
RDT = {1: np.float32, 2: np.float64}


# ---- 1. the kernel pair alone --------------------------------------------------------------------------------------------
ROW_LENS = [1, 63, 64, 65, 255, 256, 257, 1023, 244_300]


def _kernel_inputs(nrows, row_len, precision, weights, seed=0):
    rng = np.random.default_rng(seed + row_len)
    shape = (nrows, row_len)
    V = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(CDT[precision])
    d = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(CDT[precision])
    if weights == "none":
        return V, d, None
    w = rng.uniform(0.5, 2.0, size=shape).astype(RDT[precision])
    if weights == "flags":
        flagged = rng.random(shape) < 0.3
        flagged[0, 0] = True
        w[flagged] = 0
        d[flagged] = np.where(rng.random(int(flagged.sum())) < 0.5, complex(np.nan, 0.0), complex(np.inf, -np.inf))
    return V, d, w


def _residual(V, d, w, precision):
    G, chi2 = V.copy(), np.full(V.shape[0], -1.0)
    status = _lib.lib().fv_residual_chi2(0, precision, V.shape[0], V.shape[1], _lib.ptr(G), _lib.ptr(d), _lib.ptr(w),
                                         _lib.ptr(chi2))
    return status, G, chi2


@pytest.mark.parametrize("weights", ["none", "positive", "flags"])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_kernel_pair(gpu, row_len, nrows, precision, weights):
    V, d, w = _kernel_inputs(nrows, row_len, precision, weights)
    status, G, chi2 = _residual(V, d, w, precision)
    assert status == 0, _lib.lib().fv_last_error()
    used = np.ones(V.shape, bool) if w is None else w != 0
    w64 = np.ones(V.shape) if w is None else w.astype(np.float64)
    dz = d.copy()
    dz[~used] = 0
    G_ref = 2 * w64 * (V.astype(np.complex128) - dz.astype(np.complex128))
    err = np.abs(G.astype(np.complex128) - G_ref)
    eps_t = float(np.finfo(RDT[precision]).eps)
    print("kernel pair G", row_len, nrows, precision, weights, float((err / np.maximum(np.abs(G_ref), 1e-300)).max() / eps_t))
    assert np.all(err <= 2 * eps_t * np.abs(G_ref))
    assert np.all(G[~used] == 0) and (weights != "flags" or (~used).sum() > 0)
    delta = V - dz  # in T, as the kernel forms it
    terms = w64 * (delta.real.astype(np.float64) ** 2 + delta.imag.astype(np.float64) ** 2)
    exact = row_sums_exact(terms)
    print("kernel pair chi2", float((np.abs(chi2 - exact) / np.maximum(exact, 1e-300)).max() / 2.0**-52))
    assert np.all(exact > 0) or weights == "flags"
    assert np.all(np.abs(chi2 - exact) <= (row_len + 4) * 2.0**-52 * exact)
    status, G2, chi2_2 = _residual(V, d, w, precision)  # the same input gives the same bits
    assert status == 0 and np.array_equal(G2, G) and np.array_equal(chi2_2, chi2)


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("what,message", [("negative weight", b"1 weights are negative or not finite"),
                                          ("nan weight", b"1 weights are negative or not finite"),
                                          ("nan datum", b"1 entries of data are not finite where the weight is positive")])
def test_bad_input_fails_the_call_and_the_next_good_call_succeeds(gpu, what, message, precision):
    V, d, w = _kernel_inputs(3, 300, precision, "positive")
    good = _residual(V, d, w, precision)
    assert good[0] == 0
    bw, bd = w.copy(), d.copy()
    if what == "negative weight":
        bw[1, 257] = -1.0
    elif what == "nan weight":
        bw[2, 7] = np.nan
    else:
        bd[0, 299] = complex(1.0, np.nan)
    status = _residual(V, bd, bw, precision)[0]
    assert status == 1 and message in _lib.lib().fv_last_error(), _lib.lib().fv_last_error()
    again = _residual(V, d, w, precision)
    assert again[0] == 0 and np.array_equal(again[1], good[1]) and np.array_equal(again[2], good[2])
    if what == "nan datum":  # under a zero weight the same datum is not an error
        bw[0, 299] = 0
        status, G, chi2 = _residual(V, bd, bw, precision)
        assert status == 0 and G[0, 299] == 0 and np.isfinite(chi2).all()


# ---- 2. through the engine -----------------------------------------------------------------------------------------------
def _chi2(cfg, data, **kw):
    return fftvis_amd.simulate_vis_chi2(data, **cfg, **kw)


def _data(cfg, seed=5):
    """(d, w): the forward of fluxes scaled source by source by 1 + 0.3 N(0, 1), plus noise of half the visibilities' rms;
    weights U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    p = cfg.get("precision", 2)
    F = np.asarray(cfg["fluxes"])
    V0 = fftvis_amd.simulate_vis(**dict(cfg, fluxes=F * (1 + 0.3 * rng.normal(size=(F.shape[0],) + (1,) * (F.ndim - 1)))))
    rms = np.sqrt(np.mean(np.abs(V0) ** 2))
    d = V0 + 0.5 * rms * (rng.normal(size=V0.shape) + 1j * rng.normal(size=V0.shape)) / np.sqrt(2)
    return d.astype(CDT[p]), rng.uniform(0.5, 2.0, size=V0.shape).astype(RDT[p])


def _assert_value(label, cfg, d, w, chi2_ft, G):
    """G and the rows' sums against the composition ``simulate_vis`` then numpy, where G does not ride on cancellation."""
    p = cfg.get("precision", 2)
    V = fftvis_amd.simulate_vis(**cfg)
    ref_rows, G_ref = chi2_and_gvis(V, d, w)
    two_wv = 2 * (1 if w is None else w.astype(np.float64)) * V
    print("objective value", label, rel_l2(G, G_ref), float((np.abs(chi2_ft - ref_rows) / ref_rows).max()),
          np.linalg.norm(G_ref) / np.linalg.norm(two_wv))
    assert np.linalg.norm(G_ref) >= 0.1 * np.linalg.norm(two_wv)
    assert G.shape == V.shape and G.dtype == CDT[p]
    assert rel_l2(G, G_ref) <= BOUND[p]
    assert chi2_ft.shape == V.shape[:2] and chi2_ft.dtype == np.float64
    assert np.all(np.abs(chi2_ft - ref_rows) <= BOUND[p] * ref_rows)
    return V


CELLS = [("unpol", "airy"), ("I", "two"), ("full", "complex")]


@pytest.mark.parametrize("sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_value(gpu, monkeypatch, precision, sky, beams):
    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _sid(source_config("cm", sky, beams, False, precision))
    d, w = _data(cfg)
    chi2_ft, grads, G = _chi2(cfg, np.zeros_like(d), wrt=(), chi2_per="freq_time", return_gvis=True)
    V = fftvis_amd.simulate_vis(**cfg)
    assert grads == () and rel_l2(G / 2, V) <= BOUND[precision]
    norms = (np.abs(V.astype(np.complex128)) ** 2).reshape(V.shape[:2] + (-1,)).sum(axis=-1)
    assert np.all(np.abs(chi2_ft - norms) <= BOUND[precision] * norms)
    chi2_ft, _, G = _chi2(cfg, d, weights=w, wrt=(), chi2_per="freq_time", return_gvis=True)
    _assert_value(f"{precision} {sky} {beams}", cfg, d, w, chi2_ft, G)
    # the total is the rows' sums of the same call, added in row-major order
    rows = []
    real = gs.SimHandle.run_residual
    monkeypatch.setattr(gs.SimHandle, "run_residual", lambda self, *a, **k: rows.append(real(self, *a, **k)) or rows[-1])
    total, grads = _chi2(cfg, d, weights=w, wrt=())
    assert isinstance(total, float) and grads == () and len(rows) == 1 and total == row_major_sum(rows[0])


def _public(cfg, G, names, basis):
    """The gradients ``names`` from the public passes that own them, applied to G."""
    res = {}
    sky = tuple(n for n in names if n in ("fluxes", "topo", "radec"))
    rest = tuple(n for n in names if n not in sky)
    if sky:
        fn = fftvis_amd.simulate_vis_basis_sky_adjoint if basis else fftvis_amd.simulate_vis_sky_adjoint
        res.update(zip(sky, fn(G, **cfg, wrt=sky)))
    if rest:
        fn = fftvis_amd.simulate_vis_basis_adjoint if basis else fftvis_amd.simulate_vis_position_adjoint
        res.update(zip(rest, fn(G, **cfg, wrt=rest)))
    return res


def _assert_gradients(label, cfg, d, w, names, basis=False, **kw):
    chi2, grads, G = _chi2(cfg, d, weights=w, wrt=names, return_gvis=True, **kw)
    single = isinstance(names, str)
    names = (names,) if single else names
    grads = (grads,) if single else grads
    assert isinstance(grads, tuple) and len(grads) == len(names) and np.isfinite(chi2)
    want = _public(cfg, G, names, basis)
    for n, g in zip(names, grads):
        assert g.shape == want[n].shape and g.dtype == want[n].dtype and np.count_nonzero(want[n]) > 0, (label, n)
        print("objective gradient", label, names, n, float(np.abs(g - want[n]).max() / np.abs(want[n]).max()))
        if n == "fluxes":
            assert _same_flux(g, want[n]), (label, names)
        else:
            assert np.array_equal(g, want[n]), (label, names, n)
    return G


WRT = ["fluxes", "topo", ("radec",), "baselines", "ants", ("fluxes", "radec"), ("ants", "fluxes"), ("topo", "baselines"),
       ("fluxes", "ants", "baselines", "topo", "radec")]


@pytest.mark.parametrize("beams", ["airy", "two", "complex"])
@pytest.mark.parametrize("sky", ["unpol", "I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_gradients_are_the_public_passes_on_gvis(gpu, monkeypatch, precision, sky, beams):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(source_config("cm", sky, beams, False, precision))
    d, w = _data(cfg)
    for names in WRT:
        _assert_gradients(f"{precision} {sky} {beams}", cfg, d, w, names)


BASIS_WRT = ["fluxes", "beam_coefs", ("topo",), "ants", ("fluxes", "beam_coefs"), ("radec", "fluxes"),
             ("beam_coefs", "baselines"), ("fluxes", "beam_coefs", "ants", "baselines", "topo", "radec")]


@pytest.mark.parametrize("precision", [2, 1])
def test_basis_beams(gpu, monkeypatch, precision):
    """K = 3 complex tables, a full-Stokes sky, the exact form of the (l, k) terms."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = _sid(bsr.basis_source_config("cm", "complex", "full", False, precision))
    assert cfg["beam_coefs"].shape[1] == 3
    d, w = _data(cfg)
    chi2_ft, _, G = _chi2(cfg, d, weights=w, wrt=(), chi2_per="freq_time", return_gvis=True)
    _assert_value(f"basis {precision}", cfg, d, w, chi2_ft, G)
    for names in BASIS_WRT:
        _assert_gradients(f"basis {precision}", cfg, d, w, names, basis=True)


@pytest.mark.parametrize("path,took", [("type3", 3), ("type2", 2), ("auto", 2)])
def test_lattice_forward_is_type1_for_the_fluxes(gpu, monkeypatch, path, took):
    """An ideal flat hex-19: with ``wrt="fluxes"`` the handle is a lattice handle -- the forward is the type-1 transform, and
    only such a handle takes the type-2 adjoint."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = hex19_config()
    d, w = _data(cfg)
    chi2_ft, gf, G = _chi2(cfg, d, weights=w, wrt="fluxes", chi2_per="freq_time", return_gvis=True, adjoint_path=path)
    assert _handle().last_adjoint_path() == took
    _assert_value(f"lattice {path}", cfg, d, w, chi2_ft, G)
    no_flux = {k: v for k, v in cfg.items() if k != "fluxes"}
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **no_flux, adjoint_path=path))


def test_lattice_with_positions_is_the_type3_composition(gpu, monkeypatch):
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = hex19_config()
    t3 = dict(cfg, force_use_type3=True)
    d, w = _data(cfg)
    chi2_ft, (gf, ga), G = _chi2(cfg, d, weights=w, wrt=("fluxes", "ants"), chi2_per="freq_time", return_gvis=True)
    _assert_value("lattice, positions", t3, d, w, chi2_ft, G)
    assert np.array_equal(ga, fftvis_amd.simulate_vis_position_adjoint(G, **t3, wrt="ants"))
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **{k: v for k, v in t3.items() if k != "fluxes"}))
    with pytest.raises(ValueError, match="adjoint_path='type2' needs the lattice path"):
        _chi2(cfg, d, weights=w, wrt=("fluxes", "ants"), adjoint_path="type2")


def test_flagged_samples(gpu):
    cfg = _edge_cfg()
    d, w = _data(cfg)
    flagged = np.random.default_rng(2).random(d.shape) < 0.3
    w[flagged] = 0
    d[flagged] = np.nan
    names = ("fluxes", "ants", "radec")
    chi2_ft, grads, G = _chi2(cfg, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True)
    assert np.isfinite(chi2_ft).all() and all(np.isfinite(g).all() and np.count_nonzero(g) for g in grads)
    assert np.all(G[flagged] == 0) and np.all(G[~flagged] != 0)
    _assert_value("flags", cfg, d, w, chi2_ft, G)
    with pytest.raises(_lib.FftvisHipError, match="not finite where the weight is positive"):
        _chi2(cfg, d, wrt=())  # the same data without the weights that flag them
    with pytest.raises(_lib.FftvisHipError, match="weights are negative or not finite"):
        _chi2(cfg, d, weights=-w, wrt=())
    again = _chi2(cfg, d, weights=w, wrt=(), chi2_per="freq_time")[0]  # the handle stays usable
    assert np.all(np.abs(again - chi2_ft) <= BOUND[2] * chi2_ft)


def test_device_tensors(gpu):
    import torch

    cfg = _edge_cfg()
    d, w = _data(cfg)
    names = ("fluxes", "ants", "topo")
    chi2_ft, grads, G = _chi2(cfg, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True)
    D, W = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()
    dc, dg, dG = _chi2(cfg, D, weights=W, wrt=names, chi2_per="freq_time", return_gvis=True)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (dc, dG) + tuple(dg))
    assert np.all(np.abs(dc.cpu().numpy() - chi2_ft) <= BOUND[2] * chi2_ft) and rel_l2(dG.cpu().numpy(), G) <= BOUND[2]
    for a, b in zip(dg, grads):
        assert a.dtype == torch.float64 and rel_l2(a.cpu().numpy(), b) <= BOUND[2]
    total = _chi2(cfg, D, weights=W, wrt=())[0]  # resident tensors serve the next iteration; the total is a float
    assert isinstance(total, float) and abs(total - chi2_ft.sum()) <= BOUND[2] * total
    mixed = _chi2(cfg, D, weights=w, wrt=(), chi2_per="freq_time")[0]  # host weights next to device data
    assert mixed.device.type == "cuda" and np.all(np.abs(mixed.cpu().numpy() - chi2_ft) <= BOUND[2] * chi2_ft)
    hc, hg, hG = _chi2(cfg, torch.from_numpy(d), weights=torch.from_numpy(w), wrt=names, chi2_per="freq_time", return_gvis=True)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cpu" for x in (hc, hG) + tuple(hg))
    assert rel_l2(hG.numpy(), G) <= BOUND[2] and all(rel_l2(a.numpy(), b) <= BOUND[2] for a, b in zip(hg, grads))
    with pytest.raises(ValueError, match="data lives on cuda:0, the run is on cuda:1"):
        _chi2(cfg, D, weights=W, device=1)
    with pytest.raises(ValueError, match="weights lives on cuda:0, the run is on cuda:1"):
        _chi2(cfg, d, weights=W, device=1)


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
    shape = (3, 3, 2, 2, len(cfg["baselines"]))
    d = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    w = rng.uniform(0.5, 2.0, size=shape)
    names = ("fluxes", "topo", "baselines")
    one = _chi2(kw, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True, coord_mgr=Mgr())
    calls = []
    real = gpu_simulate.SimHandle.run_residual
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_residual",
                        lambda self, *a, **k: calls.append((a[0], a[1], tuple(a[6].shape))) or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    blk = _chi2(kw, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True, coord_mgr=Mgr())
    assert calls == [(0, 1, (3, 1, 2, 2, shape[-1]))] * 3, calls
    print("objective time blocks", float((np.abs(blk[0] - one[0]) / one[0]).max()), rel_l2(blk[2], one[2]),
          [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(blk[1], one[1])])
    assert np.all(np.abs(blk[0] - one[0]) <= 1e-12 * one[0])
    assert rel_l2(blk[2], one[2]) <= 1e-12
    assert _same_flux(blk[1][0], one[1][0])
    assert np.array_equal(blk[1][1], one[1][1]) and np.count_nonzero(one[1][1]) > 0
    assert np.abs(blk[1][2] - one[1][2]).max() <= 1e-12 * np.abs(one[1][2]).max()
    with pytest.raises(ValueError, match="wrt='topo'"):
        _chi2(kw, d, weights=w, wrt=("fluxes", "radec"), coord_mgr=Mgr())


def test_time_blocks_are_sized_for_gvis_data_and_weights(gpu, monkeypatch):
    """``_time_block`` sees 2.5 blocks per channel with weights and 2 without; the other modes pass what they passed."""
    from fftvis_amd.gpu import gpu_simulate

    cfg = _edge_cfg()
    d, w = _data(cfg)
    seen = []
    real = gpu_simulate._time_block
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: seen.append(a[2]) or real(*a, **k))
    _chi2(cfg, d, weights=w, wrt=())
    _chi2(cfg, d, wrt=())
    fftvis_amd.simulate_vis(**cfg)
    assert seen == [8, 6, 3], seen


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
    d, w = _data(cfg)
    names = ("fluxes", "topo", "ants")
    G = _assert_gradients("chunks, never rises", cfg, d, w, names)
    chi2_ft, (gf, gt, ga), _ = _chi2(cfg, d, weights=w, wrt=names, chi2_per="freq_time", return_gvis=True)
    _assert_value("chunks, never rises", cfg, d, w, chi2_ft, G)
    assert np.all(gf[-1] == 0) and np.all(gt[:, -1] == 0) and np.all(gt[2] == 0) and np.all(gt[up <= 0] == 0)
    # the empty step: V = 0 there, so G = -2 w d and chi2 = sum w |d|^2, exactly
    assert np.array_equal(G[:, 2], (-2 * w[:, 2] * d[:, 2]))
    assert np.all(np.abs(chi2_ft[:, 2] - chi2_and_gvis(0 * d, d, w)[0][:, 2]) <= 1e-13 * chi2_ft[:, 2])


def test_staged_inputs_are_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the forward."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    d, w = _data(cfg)
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _chi2(cfg, d, weights=w, wrt=())
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


def test_raw_c_abi(gpu):
    """``fv_sim_run_residual`` on the cached handle the last Python call configured: host and device buffers, a block of
    the channels, and the errors a configured handle raises."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    L = _lib.lib()
    fn = L.fv_sim_run_residual
    cfg = _edge_cfg()
    d, w = _data(cfg)
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    gs.release_handles()
    V = fftvis_amd.simulate_vis(**cfg)
    chi2_ft, _, G = _chi2(cfg, d, weights=w, wrt=(), chi2_per="freq_time", return_gvis=True)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        hG, hc = np.full(d.shape, 7.0, dtype=np.complex128), np.full((nf, nt), -1.0)
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(w), 0, hp(hG), 0, hp(hc)) == 0, L.fv_last_error()
        assert rel_l2(hG, G) <= BOUND[2] and np.all(np.abs(hc - chi2_ft) <= BOUND[2] * chi2_ft)
        dD, dW = torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()
        dG = torch.full(d.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        dc = np.full((nf, nt), -1.0)
        assert fn(h._h, 0, nt, 0, nf, p(dD), 1, p(dW), 1, p(dG), 1, hp(dc)) == 0, L.fv_last_error()
        assert rel_l2(dG.cpu().numpy(), G) <= BOUND[2] and np.all(np.abs(dc - chi2_ft) <= BOUND[2] * chi2_ft)
        # one channel, the second time step, no weights
        blk = np.ascontiguousarray(d[1:2, 1:2])
        bG, bc = np.zeros_like(blk), np.full((1, 1), -1.0)
        assert fn(h._h, 1, 2, 1, 2, hp(blk), 0, None, 0, hp(bG), 0, hp(bc)) == 0, L.fv_last_error()
        ref_rows, ref_G = chi2_and_gvis(V[1:2, 1:2], blk)
        # (a run of one channel plans its own grid: it agrees with the whole run's slice to the transform's tolerance,
        # test_gpu_sky_adjoint._raw_abi's bound for channel ranges)
        assert rel_l2(bG, ref_G) <= 10 * cfg["eps"] and abs(bc[0, 0] - ref_rows[0, 0]) <= 10 * cfg["eps"] * ref_rows[0, 0]
        own = chi2_and_gvis(bG / 2, 0 * blk)[0][0, 0]  # without weights chi2 = sum |G / 2|^2 of the G it returned
        assert abs(bc[0, 0] - own) <= 1e-13 * own
    finally:
        gs._return_handle(key, h)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)
    try:
        for t0, t1, f0, f1 in [(1, 1, 0, nf), (0, nt, 2, 2)]:
            assert fn(h._h, t0, t1, f0, f1, hp(d), 0, None, 0, hp(hG), 0, hp(hc)) == 1
            assert b"empty range" in L.fv_last_error()
        assert fn(h._h, 0, nt + 1, 0, nf, hp(d), 0, None, 0, hp(hG), 0, hp(hc)) == 1
        assert b"time range" in L.fv_last_error()
        bad = w.copy()
        bad[0, 0, 0, 0, 0] = -1.0
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(bad), 0, hp(hG), 0, hp(hc)) == 1
        assert b"weights are negative or not finite" in L.fv_last_error()
        assert fn(h._h, 0, nt, 0, nf, hp(d), 0, hp(w), 0, hp(hG), 0, hp(hc)) == 0, L.fv_last_error()
        assert rel_l2(hG, G) <= BOUND[2]
    finally:
        gs._return_handle(key, h)
        gs.release_handles()


def test_hera350_rows_span_many_blocks(gpu):
    """350 antennas, 1 000 sources, one channel, one time, polarized: one row of 244 300 values, 120 blocks."""
    cfg = synth.make_config("C3", nsrc=1000, nfreq=1, ntimes=1)
    assert 4 * len(cfg["baselines"]) == 244_300
    V = fftvis_amd.simulate_vis(**cfg)
    rng = np.random.default_rng(4)
    rms = np.sqrt(np.mean(np.abs(V) ** 2))
    d = V + 0.5 * rms * (rng.normal(size=V.shape) + 1j * rng.normal(size=V.shape))
    w = rng.uniform(0.5, 2.0, size=V.shape)
    w[rng.random(V.shape) < 0.1] = 0
    chi2_ft, gf, G = _chi2(cfg, d, weights=w, wrt="fluxes", chi2_per="freq_time", return_gvis=True)
    ref_rows, G_ref = chi2_and_gvis(V, d, w)
    print("objective hera350", rel_l2(G, G_ref), float(abs(chi2_ft[0, 0] - ref_rows[0, 0]) / ref_rows[0, 0]))
    assert np.linalg.norm(G_ref) >= 0.1 * np.linalg.norm(2 * w * V)
    assert rel_l2(G, G_ref) <= BOUND[2] and abs(chi2_ft[0, 0] - ref_rows[0, 0]) <= BOUND[2] * ref_rows[0, 0]
    assert np.all(G[w == 0] == 0)
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **{k: v for k, v in cfg.items() if k != "fluxes"}))


# ---- 3. torch ------------------------------------------------------------------------------------------------------------
def _torch_case(basis):
    """(kw, tensors, data, weights) on the gradcheck cells of the source passes: 8 sources, 1 channel, 1 time, 6 baselines,
    eps 1e-12, the sidereal chain; ``basis``: K = 2."""
    import torch

    cfg = bsr.gradcheck_basis_config() if basis else gradcheck_config()
    cfg["fluxes"] = cfg["fluxes"] + np.array([1.0, 0, 0, 0])
    d, w = _data(cfg)
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec", "beam_coefs", "ants")}
    t = dict(fluxes=torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda"),
             radec=torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda"),
             antpos=torch.tensor(np.array([cfg["ants"][a] for a in cfg["ants"]]), dtype=torch.float64, device="cuda"))
    if basis:
        t["beam_coefs"] = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda")
    kw["antnums"] = list(cfg["ants"])
    return cfg, kw, t, torch.from_numpy(d).cuda(), torch.from_numpy(w).cuda()


def _loss(kw, t, D, W):
    rest = {k: v for k, v in t.items() if k != "fluxes"}
    return fftvis_amd.torch_simulate_vis_chi2(D, t["fluxes"], weights=W, **rest, **kw)


@pytest.mark.parametrize("basis,name", [(False, "fluxes"), (False, "radec"), (False, "antpos"), (True, "fluxes"),
                                        (True, "beam_coefs"), (True, "radec"), (True, "antpos")])
def test_torch_gradcheck(gpu, basis, name):
    """Reverse mode, with the settings of the source passes' gradchecks on these cells (``test_gpu_sky_adjoint``: step 1e-6,
    atol 1e-6, rtol 1e-4, derived in ``test_gpu_source_adjoint``), one input at a time."""
    import torch

    cfg, kw, t, D, W = _torch_case(basis)
    x = t[name].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: _loss(kw, dict(t, **{name: v}), D, W), (x,), eps=1e-6, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize("basis", [False, True])
def test_torch_gradients_are_simulate_vis_chi2s(gpu, monkeypatch, basis):
    import torch

    import fftvis_amd.adjoint as adj

    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg, kw, t, D, W = _torch_case(basis)
    order = ("fluxes", "beam_coefs", "antpos", "radec") if basis else ("fluxes", "antpos", "radec")
    wrt = tuple("ants" if n == "antpos" else n for n in order)
    chi2, want = fftvis_amd.simulate_vis_chi2(D, **cfg, weights=W, wrt=wrt)
    calls = []
    real = adj.simulate_vis_chi2
    monkeypatch.setattr(adj, "simulate_vis_chi2", lambda *a, **k: calls.append(k["wrt"]) or real(*a, **k))
    leaves = {n: t[n].clone().requires_grad_(True) for n in order}
    loss = _loss(kw, leaves, D, W)
    assert loss.shape == () and loss.dtype == torch.float64 and loss.device.type == "cuda" and loss.item() == chi2
    loss.backward()
    assert calls == [wrt], calls  # one call, at the forward, with exactly the inputs that need a gradient
    for n, g in zip(order, want):
        assert torch.equal(leaves[n].grad, g.to(leaves[n].grad.dtype)), n
    scaled = {n: t[n].clone().requires_grad_(True) for n in order}
    (3 * _loss(kw, scaled, D, W)).backward()
    for n in order:
        assert torch.allclose(scaled[n].grad, 3 * leaves[n].grad, rtol=1e-14, atol=0), n
    # inputs that need no gradient get none, and their passes do not run
    del calls[:]
    only = dict(t, radec=t["radec"].clone().requires_grad_(True))
    _loss(kw, only, D, W).backward()
    assert calls == [("radec",)] and all(only[n].grad is None for n in order if n != "radec")
    assert torch.equal(only["radec"].grad, leaves["radec"].grad)
    del calls[:]
    assert not _loss(kw, t, D, W).requires_grad and calls == [()]
