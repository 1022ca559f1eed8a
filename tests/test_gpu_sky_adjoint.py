"""GPU tests of the joint sky adjoint (``simulate_vis_sky_adjoint``, ``simulate_vis_basis_sky_adjoint``,
``fv_sim_run_sky_adjoint``, ``fv_sim_run_basis_sky_adjoint``, and the backward passes of ``torch_simulate_vis_sky`` and
``torch_simulate_vis_basis_sky``): the flux gradient and the sources' direction gradient from one pass.

Each output is held to the bounds of the single-purpose pass it replaces, with that pass's own references, measures and
constants: the flux part element by element against the oracle's exact transpose (``test_gpu_adjoint``'s
``_assert_close_to_oracle``; through basis beams ``basis_adjoint_refs.exact_gflux`` under ``test_gpu_basis_adjoint``'s
``_assert_close``), the direction part against ``exact_gtopo`` (``test_gpu_source_adjoint._assert_close``; through basis
beams ``test_gpu_basis_source._assert_grad``); bases from ``_forward_base``.  Then against the separate calls -- ``gtopo``
bit for bit, the fluxes to 1e-12 of the maximum (the torch tests' bound: the per-lane sums run in the same fixed order) --,
where the joint pass has code of its own (both accumulators in channel blocks, source chunks, empty steps, time blocks),
through the bare C ABI and through torch.  FFTVIS_TEST_METRICS=<file> logs each comparison's ratios."""

import ctypes
import functools
import json
import os

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from fftvis_amd.adjoint import stokes_adjoint
from oracle import fftvis_oracle as orc
from tests import basis_source_refs as bsr
from tests.basis_adjoint_refs import exact_gflux
from tests.helpers import rel_l2
from tests.position_adjoint_refs import hex_positions
from tests.source_adjoint_refs import exact_gtopo, margins, random_complex, source_config, vis_shape
from tests.test_gpu_adjoint import _assert_close_to_oracle, _up
from tests.test_gpu_basis_adjoint import _assert_close as _assert_basis_flux_close
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_basis_source import _assert_grad as _assert_basis_topo_close
from tests.test_gpu_source_adjoint import _assert_close as _assert_topo_close
from tests.test_gpu_source_adjoint import _edge_cfg, _matrix_reference, _normals, _sid

pytestmark = pytest.mark.gpu


def _sky(cfg, G, wrt=("fluxes", "topo"), **kw):
    return fftvis_amd.simulate_vis_sky_adjoint(G, **cfg, wrt=wrt, **kw)


def _basis_sky(cfg, G, wrt=("fluxes", "topo"), **kw):
    return fftvis_amd.simulate_vis_basis_sky_adjoint(G, **cfg, wrt=wrt, **kw)


def _no_flux(cfg):
    return {k: v for k, v in cfg.items() if k != "fluxes"}


def _cdt(cfg):
    return np.complex64 if cfg.get("precision", 2) == 1 else np.complex128


def _assert_flux_close(label, cfg, G, gf, k64=10.0, coord_mgr=None, ref_cfg=None):
    """The flux part against the oracle's exact transpose under ``test_gpu_adjoint``'s measures and constants; fp32 against
    the forward's own error on the same configuration."""
    assert gf.shape == np.shape(cfg["fluxes"]) and gf.dtype == (np.float32 if cfg.get("precision", 2) == 1 else np.float64)
    AF = fftvis_amd.simulate_vis(**cfg) if cfg.get("precision", 2) == 1 else None
    m = _assert_close_to_oracle(ref_cfg or cfg, G, gf, cfg["fluxes"], AF, k64=k64, coord_mgr=coord_mgr)
    rec = {"label": label, "kind": "flux", "precision": cfg.get("precision", 2), **m}
    print("sky-adjoint metrics", json.dumps(rec))
    path = os.environ.get("FFTVIS_TEST_METRICS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _same_flux(got, want):
    """The torch tests' bound: 1e-12 of the maximum."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.count_nonzero(want) > 0
    return np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- 1. against the exact references -------------------------------------------------------------------------------------
CELLS = [("cm", False, sky, beams) for sky in ("unpol", "I", "full") for beams in ("airy", "two", "complex")]
CELLS += [("flat", True, "full", "two"), ("m", False, "full", "two")]


@pytest.mark.parametrize("heights,compat,sky,beams", CELLS)
@pytest.mark.parametrize("precision", [2, 1])
def test_joint_matrix(gpu, precision, heights, compat, sky, beams):
    cfg = _sid(source_config(heights, sky, beams, compat, precision))
    G64, ref = _matrix_reference(heights, sky, beams, compat)
    G = G64.astype(_cdt(cfg))
    gf, gt = _sky(cfg, G)
    label = f"joint matrix {precision} {sky} {beams} {compat} {heights}"
    assert gt.shape == (2, 24, 3) and gt.dtype == np.float64
    n = _normals(cfg)
    assert np.all(gt[n[..., 2] <= 0] == 0)
    _assert_topo_close(label, cfg, gt, ref, _forward_base(cfg))
    _assert_flux_close(label, cfg, G, gf)


# ---- 2. against the separate calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("precision", [2, 1])
def test_joint_equals_the_separate_calls(gpu, monkeypatch, precision, lanes):
    """Four time steps, so that with two lanes each lane sums two steps into its flux accumulator."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    cfg = _sid(source_config("cm", "full", "two", False, precision, nsrc=25, ntimes=4))
    G = random_complex(vis_shape(cfg), 10).astype(_cdt(cfg))
    gf, gt, gr = _sky(cfg, G, wrt=("fluxes", "topo", "radec"))
    st, sr = fftvis_amd.simulate_vis_source_adjoint(G, **cfg, wrt=("topo", "radec"))
    sf = fftvis_amd.simulate_vis_adjoint(G, **_no_flux(cfg), full_stokes=True)
    assert np.array_equal(gt, st) and np.array_equal(gr, sr) and np.count_nonzero(st) > 0
    assert gf.dtype == sf.dtype and _same_flux(gf, sf)
    # the order of wrt is the order of the result; a single name gives a single array
    rf = _sky(cfg, G, wrt=("radec", "fluxes"))
    assert isinstance(rf, tuple) and np.array_equal(rf[0], gr) and np.array_equal(rf[1], gf)


def test_a_wrt_without_both_sides_returns_the_single_purpose_bits(gpu):
    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 8)
    st, sr = fftvis_amd.simulate_vis_source_adjoint(G, **cfg, wrt=("topo", "radec"))
    sf = fftvis_amd.simulate_vis_adjoint(G, **_no_flux(cfg), full_stokes=True)
    assert np.array_equal(_sky(cfg, G, wrt="topo"), st) and np.array_equal(_sky(cfg, G, wrt="radec"), sr)
    both = _sky(cfg, G, wrt=("radec", "topo"))
    assert isinstance(both, tuple) and np.array_equal(both[0], sr) and np.array_equal(both[1], st)
    assert np.array_equal(_sky(cfg, G, wrt="fluxes"), sf)
    one = _sky(cfg, G, wrt=("fluxes",))
    assert isinstance(one, tuple) and len(one) == 1 and np.array_equal(one[0], sf)


def test_a_device_tensor_in_gives_device_tensors_out(gpu):
    import torch

    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 9)
    gf, gt, gr = _sky(cfg, G, wrt=("fluxes", "topo", "radec"))
    df, dt, dr = _sky(cfg, torch.from_numpy(G).cuda(), wrt=("fluxes", "topo", "radec"))
    assert all(x.device.type == "cuda" for x in (df, dt, dr)) and df.dtype == torch.float64 and dt.dtype == torch.float64
    assert np.array_equal(dt.cpu().numpy(), gt) and np.array_equal(df.cpu().numpy(), gf)
    assert rel_l2(dr.cpu().numpy(), gr) <= 1e-14
    hf, ht = _sky(cfg, torch.from_numpy(G))
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cpu" for x in (hf, ht))
    assert np.array_equal(hf.numpy(), gf) and np.array_equal(ht.numpy(), gt)


# ---- 3. where the joint pass can go wrong by itself ----------------------------------------------------------------------
def _check_both(label, cfg, k64=10.0, coord_mgr=None, ref_mgr=None, ref_cfg=None, **kw):
    G = random_complex(vis_shape(cfg), 7)
    extra = {} if coord_mgr is None else {"coord_mgr": coord_mgr}
    gf, gt = _sky(cfg, G, **extra, **kw)
    _assert_topo_close(label, cfg, gt, exact_gtopo(ref_cfg or cfg, G, coord_mgr=ref_mgr), cfg["eps"], k64)
    _assert_flux_close(label, cfg, G, gf, k64, coord_mgr=ref_mgr, ref_cfg=ref_cfg)
    return G, gf, gt


@pytest.mark.parametrize("block_ch,ratio", [(1, 0.99), (2, 0.99), (2, 0.5)])
@pytest.mark.parametrize("sky,comps", [("I", 1), ("full", 8)])
def test_channel_blocks_hold_both_accumulators(gpu, monkeypatch, sky, comps, block_ch, ratio):
    """nf = 5 in channel blocks of block_ch -- FFTVIS_HIP_ADJ_ACC_BYTES at 24 + 8 comps bytes per channel and source, comps 1
    for the Stokes-I sky and 8 for the coherency sky -- with frequency groups cut by FFTVIS_HIP_GROUP_RATIO; the last block
    is short, and every block is reduced into gflux before the next one zeroes the lanes' flux accumulators."""
    cfg = _sid(source_config("cm", sky, "two", False, 2, nsrc=18, nfreq=5))
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * (24 + 8 * comps) * 18))
    monkeypatch.setenv("FFTVIS_HIP_GROUP_RATIO", str(ratio))
    _check_both(f"joint blocks {sky} {block_ch} ratio {ratio}", cfg)


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_source_chunks(gpu, monkeypatch, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    _check_both(f"joint chunks lanes {lanes}", dict(_edge_cfg(nsrc=25, ntimes=4), min_chunks=3))


def test_rows_below_the_horizon_an_empty_time_step_and_a_source_that_never_rises(gpu):
    """``test_gpu_source_adjoint``'s sky around the meridian -- a quarter of a sidereal day later some sources are below
    the horizon, half a day later all are -- with the last source moved to dec = +80 deg, which never rises at HERA's
    latitude: its rows of both outputs are exactly 0."""
    cfg = _edge_cfg(nsrc=20)
    t0 = cfg["times"][0]
    lst = orc.gmst_rad(t0) + synth.HERA_LON
    rng = np.random.default_rng(1)
    ra, dec = lst + rng.uniform(-0.3, 0.3, 20), synth.HERA_LAT + rng.uniform(-0.3, 0.3, 20)
    dec[-1] = np.radians(80.0)
    cfg.update(ra=ra, dec=dec, times=t0 + np.array([0.0, 0.25, 0.5]))
    up = _up(cfg)
    assert np.all(up[0, :-1] > 0) and np.any(up[1] > 0) and np.any(up[1, :-1] <= 0) and not np.any(up[2] > 0)
    assert not np.any(up[:, -1] > 0) and margins(cfg)[0] > 1e-3
    G, gf, gt = _check_both("joint below the horizon, empty time step", cfg)
    assert np.all(gt[up <= 0] == 0) and np.all(gt[2] == 0) and np.all(np.any(gt[up > 0] != 0, axis=-1))
    assert np.all(gf[-1] == 0) and np.all(gt[:, -1] == 0) and np.all(np.any(gf[:-1] != 0, axis=(1, 2)))
    # the empty step alone: both outputs exactly 0
    last = dict(cfg, times=cfg["times"][2:])
    zf, zt = _sky(last, np.ascontiguousarray(G[:, 2:]))
    assert not zf.any() and not zt.any()


def test_upsample_125(gpu):
    _check_both("joint sigma 1.25", dict(_edge_cfg(), upsample_factor=1.25), k64=20.0)


def test_ideal_lattice_goes_through_the_type3_transform(gpu):
    """An exact hex-19, all baselines: the forward takes the lattice path there, the joint pass the type-3 transform."""
    from fftvis_amd.core.antenna_gridding import check_antpos_griddability

    c1 = synth.make_config("C1", nsrc=24, nfreq=3, ntimes=2, seed=2)
    xy = 14.6 * hex_positions(2)
    ants = {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(19)}
    assert check_antpos_griddability(ants)[0]
    bls = [(i, j) for i in range(19) for j in range(i, 19)] + [(7, 3), (18, 0)]
    cfg = _sid(dict(c1, ants=ants, baselines=bls, polarized=True, force_use_type3=False))
    assert margins(cfg)[0] > 1e-3
    _check_both("joint ideal hex-19", cfg, ref_cfg={k: v for k, v in cfg.items() if k != "force_use_type3"})


def test_coord_mgr_in_time_blocks(gpu, monkeypatch):
    """A coordinate manager streamed one time step per block: every block adds to gflux (the first overwrites) and fills its
    own rows of gtopo."""
    from fftvis_amd.gpu import gpu_simulate
    from oracle import astrometry as oa

    cfg = _edge_cfg(ntimes=3)
    eq = orc.eq_unit_vectors(cfg["ra"], cfg["dec"])
    ctxs = np.stack([oa.plausible_context(20 + t, synth.HERA_LAT) for t in range(3)])

    class Mgr:  # the slice of matvis' manager the engine consumes
        times = cfg["times"]

        def setup(self):
            pass

        def rotate(self, ti):
            self.all_coords_topo = oa.icrs_to_enu(eq, ctxs[ti])

    assert margins(cfg, coord_mgr=Mgr())[0] > 1e-3
    kw = dict(cfg, coord_method="CoordinateRotationERFA")
    calls = []
    real = gpu_simulate.SimHandle.run_sky_adjoint
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_sky_adjoint",
                        lambda self, *a, **k: calls.append((a[0], a[1], tuple(a[6].shape), a[7])) or real(self, *a, **k))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    G, gf, gt = _check_both("joint coord_mgr, time blocks", kw, coord_mgr=Mgr(), ref_mgr=Mgr())
    assert calls == [(0, 1, (1, 24, 3), False), (0, 1, (1, 24, 3), True), (0, 1, (1, 24, 3), True)], calls
    monkeypatch.undo()
    assert np.array_equal(gt, fftvis_amd.simulate_vis_source_adjoint(G, **kw, wrt="topo", coord_mgr=Mgr()))
    assert _same_flux(gf, fftvis_amd.simulate_vis_adjoint(G, **_no_flux(kw), full_stokes=True, coord_mgr=Mgr()))
    with pytest.raises(ValueError, match="wrt='topo'"):
        _sky(kw, G, wrt=("fluxes", "radec"), coord_mgr=Mgr())


def test_nan_in_g_fails_and_the_handle_stays_usable(gpu):
    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 7)
    gf, gt = _sky(cfg, G)
    bad = G.copy()
    bad[1, 0, 1, 0, 3] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="NaN"):
        _sky(cfg, bad)
    again = _sky(cfg, G)
    assert np.array_equal(again[0], gf) and np.array_equal(again[1], gt)


def test_bulk_device_memory_is_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the
    forward: neither accumulator, no staged array and no set of strengths stays."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _sky(cfg, random_complex(vis_shape(cfg), 1))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu):
    cfg = _edge_cfg()
    before = fftvis_amd.simulate_vis(**cfg)
    _sky(cfg, random_complex(vis_shape(cfg), 3))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)


def test_reproducible_for_a_lane_count(gpu, monkeypatch):
    cfg = _edge_cfg(nsrc=25, ntimes=4)
    G = random_complex(vis_shape(cfg), 10)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a, b = _sky(cfg, G), _sky(cfg, G)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), lanes
        res[lanes] = a
    assert rel_l2(res["1"][0], res["2"][0]) <= 1e-12 and rel_l2(res["1"][1], res["2"][1]) <= 1e-12


# ---- 4. basis beams ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _basis_flux_reference(tables, sky, compat):
    """The exact flux gradient of a basis cell for ``basis_source_refs.matrix_reference``'s G."""
    cfg = bsr.basis_source_config("cm", tables, sky, compat)
    return exact_gflux(cfg, bsr.matrix_reference("cm", tables, sky, compat)[0])


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("sky", ["I", "full"])
@pytest.mark.parametrize("tables", ["airy", "complex"])
@pytest.mark.parametrize("precision", [2, 1])
def test_basis_joint_matrix(gpu, precision, tables, sky, compat):
    cfg = bsr.basis_source_config("cm", tables, sky, compat, precision)
    G64, gref = bsr.matrix_reference("cm", tables, sky, compat)[:2]
    fref = _basis_flux_reference(tables, sky, compat)
    label = f"joint basis matrix {precision} {sky} {tables} {compat}"
    base = _forward_base(cfg)
    gf, gt = _basis_sky(cfg, G64.astype(_cdt(cfg)))
    assert gf.shape == cfg["fluxes"].shape and gf.dtype == (np.float32 if precision == 1 else np.float64)
    _assert_basis_topo_close(label, cfg, gt, gref, base)
    _assert_basis_flux_close(label, cfg, "flux", gf, fref, base)


def test_one_unit_basis_beam_equals_the_plain_joint_pass(gpu):
    """One Airy basis beam with every coefficient 1 is the same dish without ``beam_coefs``: both at eps 1e-12, agreement
    to the forward bound, 10 eps relative (``test_gpu_basis_source``'s K = 1 comparison, no oracle)."""
    cfg, plain = bsr.k1_configs("cm")
    G = random_complex(vis_shape(cfg), 9)
    bf, bt = _basis_sky(cfg, G)
    pf, pt = _sky(plain, G)
    print("joint basis K = 1", rel_l2(bf, pf) / cfg["eps"], rel_l2(bt, pt) / cfg["eps"])
    assert np.linalg.norm(pf) > 0 and np.linalg.norm(pt) > 0
    assert rel_l2(bf, pf) <= 10 * cfg["eps"] and rel_l2(bt, pt) <= 10 * cfg["eps"]


@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("precision", [2, 1])
def test_basis_joint_equals_the_separate_calls(gpu, monkeypatch, precision, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    cfg = bsr.basis_source_config("cm", "complex", "full", False, precision, nsrc=25, ntimes=4, order=3)
    G = random_complex(vis_shape(cfg), 10).astype(_cdt(cfg))
    gf, gt, gr = _basis_sky(cfg, G, wrt=("fluxes", "topo", "radec"))
    st, sr = fftvis_amd.simulate_vis_basis_source_adjoint(G, **cfg, wrt=("topo", "radec"))
    sf = fftvis_amd.simulate_vis_basis_adjoint(G, **cfg, wrt="fluxes")
    assert np.array_equal(gt, st) and np.array_equal(gr, sr) and np.count_nonzero(st) > 0
    assert gf.dtype == sf.dtype and _same_flux(gf, sf)
    assert np.array_equal(_basis_sky(cfg, G, wrt="topo"), st) and np.array_equal(_basis_sky(cfg, G, wrt="fluxes"), sf)
    one = _basis_sky(cfg, G, wrt=("fluxes",))
    assert isinstance(one, tuple) and len(one) == 1 and np.array_equal(one[0], sf)


# ---- 5. the raw C ABI ----------------------------------------------------------------------------------------------------
def _raw_abi(fn, cfg, G, gf, gt):
    """``fn`` through the cached handle the last Python call configured: device and host outputs, accumulate 0 then 1,
    channel ranges that add up to the whole.  gflux is the coherency gradient: ``stokes_adjoint`` takes it to ``gf``."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    nf, nt, nsrc = len(cfg["freqs"]), len(cfg["times"]), len(cfg["ra"])
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        dG = torch.from_numpy(G).cuda()
        dF = torch.full((nsrc, nf, 2, 2), 7.0, dtype=torch.complex128, device="cuda")
        dT = torch.full((nt, nsrc, 3), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert fn(h._h, 0, nt, 0, nf, p(dG), 1, p(dF), 1, p(dT), 1, 0) == 0, L.fv_last_error()
        assert np.array_equal(dT.cpu().numpy(), gt)  # accumulate = 0 zeroes both first
        assert np.array_equal(stokes_adjoint(dF.cpu().numpy(), True), gf)
        assert fn(h._h, 0, nt, 0, nf, p(dG), 1, p(dF), 1, p(dT), 1, 1) == 0, L.fv_last_error()
        assert rel_l2(dT.cpu().numpy(), 2 * gt) < 1e-14 and rel_l2(stokes_adjoint(dF.cpu().numpy(), True), 2 * gf) < 1e-14
        tot_f, tot_t = np.zeros_like(gf), np.zeros_like(gt)
        for f0, f1 in ((0, 1), (1, nf)):  # channel ranges add up to the whole; gflux only receives its own channels
            blk = dG[f0:f1].contiguous()
            torch.cuda.synchronize()
            assert fn(h._h, 0, nt, f0, f1, p(blk), 1, p(dF), 1, p(dT), 1, 0) == 0, L.fv_last_error()
            part_f = stokes_adjoint(dF.cpu().numpy(), True)
            assert part_f[:, f0:f1].any() and not np.delete(part_f, np.s_[f0:f1], axis=1).any()
            tot_f += part_f
            tot_t += dT.cpu().numpy()
        assert rel_l2(tot_f, gf) <= 10 * cfg["eps"] and rel_l2(tot_t, gt) <= 10 * cfg["eps"]
        hF, hT = np.full((nsrc, nf, 2, 2), 7.0, dtype=np.complex128), np.full((nt, nsrc, 3), 7.0)  # host outputs
        assert fn(h._h, 0, nt, 0, nf, hp(G), 0, hp(hF), 0, hp(hT), 0, 0) == 0, L.fv_last_error()
        assert np.array_equal(hT, gt) and np.array_equal(stokes_adjoint(hF, True), gf)
        assert fn(h._h, 0, nt, 0, nf, p(dG), 1, hp(hF), 0, hp(hT), 0, 1) == 0, L.fv_last_error()
        assert rel_l2(hT, 2 * gt) < 1e-14 and rel_l2(stokes_adjoint(hF, True), 2 * gf) < 1e-14
        dF.fill_(7.0)  # a host gtopo next to a device gflux, one time step of the block
        one = np.zeros((1, nsrc, 3))
        blk = dG[:, 1:2].contiguous()
        torch.cuda.synchronize()
        assert fn(h._h, 1, 2, 0, nf, p(blk), 1, p(dF), 1, hp(one), 0, 0) == 0, L.fv_last_error()
        assert np.array_equal(one[0], gt[1]) and np.isfinite(dF.cpu().numpy()).all()
        bad = G.copy()  # NaN in G fails before anything runs; the next call returns the good result's bits
        bad[1, 0, 1, 0, 3] = np.nan
        assert fn(h._h, 0, nt, 0, nf, hp(bad), 0, hp(hF), 0, hp(hT), 0, 0) == 1
        assert b"NaN" in L.fv_last_error()
        assert fn(h._h, 0, nt, 0, nf, hp(G), 0, hp(hF), 0, hp(hT), 0, 0) == 0, L.fv_last_error()
        assert np.array_equal(hT, gt) and np.array_equal(stokes_adjoint(hF, True), gf)
    finally:
        gs._return_handle(key, h)


def _refused(fn, eps, *words):
    """``fn`` on the cached handle of the last run is an argument error whose message holds ``words``."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    L = _lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    key, h = gs._acquire_handle(0, 2, eps, 2, True)
    try:
        assert fn(h._h, 0, 1, 0, 1, ctypes.c_void_p(buf.data_ptr()), 1, ctypes.c_void_p(buf.data_ptr()), 1,
                  ctypes.c_void_p(buf.data_ptr()), 1, 0) == 1
        assert all(w in L.fv_last_error() for w in words), L.fv_last_error()
    finally:
        gs._return_handle(key, h)


def test_raw_c_abi(gpu):
    from fftvis_amd.gpu import gpu_simulate as gs

    L = _lib.lib()
    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 7)
    gs.release_handles()
    gf, gt = _sky(cfg, G)
    _raw_abi(L.fv_sim_run_sky_adjoint, cfg, G, gf, gt)
    _refused(L.fv_sim_run_basis_sky_adjoint, cfg["eps"], b"fv_sim_set_basis", b"fv_sim_run_sky_adjoint")
    xy = 14.6 * hex_positions(1)
    lat = dict(cfg, ants={i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(7)}, force_use_type3=False)
    gs.release_handles()
    fftvis_amd.simulate_vis(**lat)  # the lattice path
    _refused(L.fv_sim_run_sky_adjoint, cfg["eps"], b"fv_sim_set_array")
    bcfg = bsr.edge_config()
    gs.release_handles()
    bf, bt = _basis_sky(bcfg, G)
    _raw_abi(L.fv_sim_run_basis_sky_adjoint, bcfg, G, bf, bt)
    _refused(L.fv_sim_run_sky_adjoint, bcfg["eps"], b"basis", b"fv_sim_run_basis_sky_adjoint")
    gs.release_handles()


# ---- 6. torch ------------------------------------------------------------------------------------------------------------
def _spy(monkeypatch, adj, calls, names):
    for name in names:
        real = getattr(adj, name)
        monkeypatch.setattr(adj, name, lambda *a, _n=name, _r=real, **k: calls.append((_n, k.get("wrt"))) or _r(*a, **k))


def test_torch_backward_is_one_joint_call(gpu, monkeypatch):
    """With both tensors requiring gradients the backward is exactly one ``simulate_vis_sky_adjoint`` call, and its result;
    the loss Re <W, V> hands G = W over bit for bit."""
    import torch

    import fftvis_amd.adjoint as adj

    cfg = _edge_cfg()
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec")}
    W = random_complex(vis_shape(cfg), 15)
    calls = []
    _spy(monkeypatch, adj, calls, ("simulate_vis_sky_adjoint", "simulate_vis_adjoint", "simulate_vis_source_adjoint"))
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda", requires_grad=True)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True)
    V = fftvis_amd.torch_simulate_vis_sky(F, P, **kw)
    (V * torch.from_numpy(W).cuda().conj()).real.sum().backward()
    assert calls == [("simulate_vis_sky_adjoint", ("fluxes", "radec"))], calls
    monkeypatch.undo()
    gf, gp = _sky(cfg, W, wrt=("fluxes", "radec"))
    assert np.allclose(F.grad.cpu().numpy(), gf, rtol=1e-12, atol=1e-12 * np.abs(gf).max())
    assert np.allclose(P.grad.cpu().numpy(), gp, rtol=1e-12, atol=1e-12 * np.abs(gp).max())


def test_torch_gradcheck_both_inputs_through_the_joint_pass(gpu, monkeypatch):
    """``test_gpu_source_adjoint.test_torch_gradcheck_both_inputs``'s configuration and tolerances (derived in its
    docstring): fp64, 8 sources, 1 channel, 1 time, eps 1e-12, step 1e-6 rad, atol 1e-6, rtol 1e-4.  Every backward of the
    check goes through the joint function."""
    import torch

    import fftvis_amd.adjoint as adj

    cfg = _edge_cfg(nsrc=8, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)])
    _, _, cfg["fluxes"] = synth.catalog(8, cfg["freqs"], 0, polarized_sky=True)
    assert margins(cfg)[0] > 1e-3
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec")}
    calls = []
    _spy(monkeypatch, adj, calls, ("simulate_vis_sky_adjoint", "simulate_vis_adjoint", "simulate_vis_source_adjoint"))
    F = torch.tensor(cfg["fluxes"] + np.array([1.0, 0, 0, 0]), dtype=torch.float64, device="cuda", requires_grad=True)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, p: fftvis_amd.torch_simulate_vis_sky(f, p, **kw), (F, P), eps=1e-6,
                                    atol=1e-6, rtol=1e-4)
    assert calls and {c[0] for c in calls} == {"simulate_vis_sky_adjoint"}, calls


def test_basis_torch_backward_is_one_joint_call_and_the_coefficients(gpu, monkeypatch):
    import torch

    import fftvis_amd.adjoint as adj

    cfg = bsr.edge_config()
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec", "beam_coefs")}
    W = random_complex(vis_shape(cfg), 15)
    calls = []
    _spy(monkeypatch, adj, calls, ("simulate_vis_basis_sky_adjoint", "simulate_vis_basis_adjoint",
                                   "simulate_vis_basis_source_adjoint"))

    def leaves():
        return (torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda", requires_grad=True),
                torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True),
                torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True))

    F, C, P = leaves()
    V = fftvis_amd.torch_simulate_vis_basis_sky(F, C, P, **kw)
    (V * torch.from_numpy(W).cuda().conj()).real.sum().backward()
    assert calls == [("simulate_vis_basis_sky_adjoint", ("fluxes", "radec")), ("simulate_vis_basis_adjoint", ("beam_coefs",))], calls
    del calls[:]
    F2, C2, P2 = leaves()  # the coefficients held fixed: the joint call alone
    fftvis_amd.torch_simulate_vis_basis_sky(F2, C2.detach(), P2, **kw).abs().pow(2).sum().backward()
    assert calls == [("simulate_vis_basis_sky_adjoint", ("fluxes", "radec"))], calls
    monkeypatch.undo()
    gf, gp = _basis_sky(cfg, W, wrt=("fluxes", "radec"))
    gc = fftvis_amd.simulate_vis_basis_adjoint(W, **cfg, wrt="beam_coefs")
    for got, want in ((F.grad, gf), (C.grad, gc), (P.grad, gp)):
        assert np.allclose(got.cpu().numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_basis_torch_gradcheck_all_three_inputs_through_the_joint_pass(gpu, monkeypatch):
    """``test_gpu_basis_source.test_torch_gradcheck_all_three_inputs``'s configuration and tolerances (derived in its
    docstring), reverse mode: the backward of (F, C, P) is the joint call plus the coefficients' pass."""
    import torch

    import fftvis_amd.adjoint as adj

    cfg = bsr.gradcheck_basis_config()
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec", "beam_coefs")}
    calls = []
    _spy(monkeypatch, adj, calls, ("simulate_vis_basis_sky_adjoint", "simulate_vis_basis_source_adjoint"))
    F = torch.tensor(cfg["fluxes"] + np.array([1.0, 0, 0, 0]), dtype=torch.float64, device="cuda", requires_grad=True)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, c, p: fftvis_amd.torch_simulate_vis_basis_sky(f, c, p, **kw), (F, C, P),
                                    eps=1e-6, atol=1e-6, rtol=1e-4)
    assert calls and {c[0] for c in calls} == {"simulate_vis_basis_sky_adjoint"}, calls
