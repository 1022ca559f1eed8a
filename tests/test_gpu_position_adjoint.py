"""GPU tests of the gradient with respect to the antenna positions (``simulate_vis_position_adjoint``,
``torch_simulate_vis_array``, ``fv_sim_run_position_adjoint``).

The baseline gradient ``gbls`` (nbls, 3), ENU per metre, is compared element by element with the exact reference built
from the oracle's forward (``position_adjoint_refs.exact_gbls``, pinned against finite differences of the oracle in
``test_position_adjoint_host``): over a configuration matrix, on an ideal lattice, at HERA-350's size with the packed
transforms and the column plan, at the edges of the device's slicing, through the Python surface and the bare C ABI, and
through torch's gradcheck and backward."""

import ctypes
import functools
import json
import os

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from oracle import fftvis_oracle as orc
from tests.helpers import floored_rel, rel_l2, worst_part
from tests.position_adjoint_refs import exact_gbls, hex_positions, position_config, random_complex, vis_shape
from tests.test_gpu_adjoint import _up
from tests.test_gpu_basis_adjoint import _forward_base

pytestmark = pytest.mark.gpu

# Element-wise tolerances against the exact reference, as multiples of base.  base = eps in fp64; in fp32
# base = max(the forward's own rel l2 error against the oracle on the same configuration, eps) (``_forward_base``).
#   rel l2 of the whole (nbls, 3) result <= 10 base in fp64 (20 at upsample_factor = 1.25): the project's bound for the
#   forward and the adjoints -- the pass is the forward's transform followed by exact fp64 sums;
#   the bounds on a single component (east, north, up; a component below 1e-3 of the whole is measured against that
#   floor), on max |err| / max |exact| and every fp32 factor start at test_gpu_basis_adjoint's constants and are kept
#   where they are at least 2 x the worst ratio measured on an MI355X over this module's comparisons
#   (FFTVIS_TEST_METRICS=<file> logs each comparison's ratios, one JSON line each).  Measured, as ratio / base:
#   fp64 over the 69 comparisons (base 6e-8; 1e-12 at HERA-350's size): whole <= 0.62, a component <= 2.12, max |err| /
#   max |exact| <= 0.95 -- all three at HERA-350's size at eps 1e-12; every comparison at eps 6e-8 is at or below 0.59,
#   1.03, 0.60 (one channel through the C entry point), the matrix at or below 0.11, 0.20, 0.13, upsample_factor = 1.25 at
#   0.17, 0.27, 0.20.
#   fp32 over the 54 matrix cells (base 1e-5: the forward's own error stayed below eps everywhere): whole <= 0.90,
#   a component <= 1.16, max |err| <= 1.08, all on the flat array (height terms and 3-D: 0.35, 0.52, 0.55).
#   Every constant keeps more than twice its measured worst: none moved.
K64_PART = 10.0   # fp64: a component (20 at upsample_factor = 1.25, like the whole)
K32 = 13.0        # fp32: the whole
K32_PART = 40.0   # fp32: a component
C_MAX = 6.0       # fp64: max |err| / (base max |exact|)
C_MAX32 = 12.0    # fp32


def _errors(got, exact):
    got = np.asarray(got).astype(np.float64)
    err = got - exact
    floor = 1e-3 * np.linalg.norm(exact)
    return {"rel_l2": floored_rel(err, exact, floor), "component": worst_part(err, exact, 1, floor),
            "max_abs": float(np.abs(err).max() / max(np.abs(exact).max(), 1e-300))}


def _log(label, cfg, m, base):
    rec = {"label": label, "precision": cfg.get("precision", 2), "base": base, **{k: v / base for k, v in m.items()}}
    print("position-adjoint metrics", json.dumps(rec))
    path = os.environ.get("FFTVIS_TEST_METRICS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _assert_close(label, cfg, got, exact, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert got.shape == exact.shape and np.isfinite(np.asarray(got)).all()
    m = _errors(got, exact)
    _log(label, cfg, m, base)
    fp64 = cfg.get("precision", 2) == 2
    whole, part = (k64, K64_PART * k64 / 10.0) if fp64 else (K32, K32_PART)
    assert m["rel_l2"] <= whole * base, (label, m, base)
    assert m["component"] <= part * base, (label, m, base)
    assert m["max_abs"] <= (C_MAX * k64 / 10.0 if fp64 else C_MAX32) * base, (label, m, base)
    return m


def _gbls(cfg, G, wrt="baselines", **kw):
    return fftvis_amd.simulate_vis_position_adjoint(G, **cfg, wrt=wrt, **kw)


def _handle():
    from fftvis_amd.gpu import gpu_simulate

    (h,) = gpu_simulate._IDLE_HANDLES.values()
    return h


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix_reference(heights, sky, beams, compat):
    """The exact gradient of a matrix cell (it does not depend on the run's precision)."""
    cfg = position_config(heights, sky, beams, compat)
    G = random_complex(vis_shape(cfg), 4)
    return G, exact_gbls(cfg, G)


@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("beams", ["airy", "two", "complex"])
@pytest.mark.parametrize("sky", ["unpol", "I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_position_gradient_matrix(gpu, precision, sky, beams, compat, heights):
    cfg = position_config(heights, sky, beams, compat, precision)
    G64, ref = _matrix_reference(heights, sky, beams, compat)
    got = _gbls(cfg, G64.astype(np.complex64 if precision == 1 else np.complex128))
    assert got.shape == (len(cfg["baselines"]), 3) and got.dtype == np.float64
    assert np.linalg.norm(ref[:, 2]) > 1e-3 * np.linalg.norm(ref)  # the up component is checked on the flat array too
    _assert_close(f"matrix {precision} {sky} {beams} {compat} {heights}", cfg, got, ref, _forward_base(cfg))


@pytest.mark.parametrize("heights,terms", [("flat", False), ("m", False), ("cm", True)])
def test_matrix_arrays_take_the_paths_they_are_named_for(gpu, monkeypatch, heights, terms):
    """The pass is a forward run: on the matrix's three arrays it runs 2-D transforms, the 3-D transform, and 2-D
    transforms with height terms (the gather's WT variants)."""
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    cfg = position_config(heights, "full", "two", False)
    _gbls(cfg, random_complex(vis_shape(cfg), 2))
    st = _handle().stats()
    gpu_simulate.release_handles()
    if terms:
        assert 2 <= st["height_terms"] <= 16 and st["n2_3"] == 1, st
    else:
        assert st["height_terms"] == 0 and (st["n2_3"] > 1) == (heights == "m"), st


# ---- 2. an ideal lattice ---------------------------------------------------------------------------------------------
def test_ideal_lattice_takes_type3_with_redundant_runs(gpu, monkeypatch):
    """An exact hex-19, all baselines in the caller's order: the forward takes the lattice path there, the position pass
    the type-3 transform with the redundant runs; every member's row against the exact reference, and the same result
    without the runs and without the mirror pairs."""
    from fftvis_amd.core.antenna_gridding import check_antpos_griddability
    from fftvis_amd.gpu import gpu_simulate

    c1 = synth.make_config("C1", nsrc=24, nfreq=3, ntimes=2)
    xy = 14.6 * hex_positions(2)
    ants = {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(19)}
    assert check_antpos_griddability(ants)[0]
    bls = [(i, j) for i in range(19) for j in range(i, 19)] + [(7, 3), (18, 0)]
    cfg = dict(c1, ants=ants, baselines=bls, polarized=True, force_use_type3=False)
    G = random_complex(vis_shape(cfg), 5)
    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    got = _gbls(cfg, G)
    st = _handle().stats()
    assert st["lanes"] >= 1 and st["spread_launches"] > 0, st  # the type-3 stages ran (the lattice path sets no lanes)
    items_once = st["interp_items"]
    _assert_close("ideal hex-19", cfg, got, exact_gbls(cfg, G), cfg["eps"])
    for env in ("FFTVIS_HIP_NO_TARGET_DEDUP", "FFTVIS_HIP_NO_TARGET_PAIRS"):
        _handle().reset_stats()
        monkeypatch.setenv(env, "1")
        other = _gbls(cfg, G)
        monkeypatch.delenv(env)
        d = rel_l2(other, got)
        print("position-adjoint lattice", env, d)
        assert d <= 1e-12, (env, d)
        if env.endswith("DEDUP"):
            assert items_once < 0.5 * _handle().stats()["interp_items"]  # most of the 192 vectors repeat
    gpu_simulate.release_handles()


# ---- 3. packings and plans at HERA-350's size ------------------------------------------------------------------------
def _hera350(kind):
    """HERA-350, all 61 075 baselines, 64 sources above the horizon, 2 channels at the top of the band, 1 time: the
    smallest shape whose grid passes the 4e6-cell threshold of the packed transforms and the column plan."""
    c3 = synth.make_config("C3", nsrc=400, nfreq=2, ntimes=1)
    assert len(c3["baselines"]) == 61075
    freqs = np.array([198e6, 200e6])
    up = _up(c3)[0]
    pick = np.flatnonzero(up > 0.05)[:64]
    assert len(pick) == 64
    ra, dec = c3["ra"][pick], c3["dec"][pick]
    _, _, flux = synth.catalog(400, freqs, 0, polarized_sky=kind == "hermitian")
    cfg = dict(c3, freqs=freqs, ra=ra, dec=dec, fluxes=flux[pick], polarized=True, eps=HERA_EPS)
    if kind == "hermitian":  # one beam on both sides, polarized sky: Hermitian strengths
        cfg["beam"] = fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, 14.0, nza=91, naz=180), freqs)
    else:                    # unpolarized sky, two real beams: the cross pairs' strengths are all real
        cfg["beam"] = [fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(12.0)]
        cfg["beam_idx"] = np.arange(350) % 2
    return cfg


# (the packed and the four-transform runs, and the planned and the unplanned ones, are different computations of one sum:
# they agree to the transforms' tolerance, so the comparison at 1e-11 relative needs a tolerance below it)
HERA_EPS = 1e-12


@pytest.mark.parametrize("kind", ["hermitian", "all_real"])
def test_hera350_packings_and_column_plan(gpu, monkeypatch, kind):
    from fftvis_amd.gpu import gpu_simulate

    cfg = _hera350(kind)
    G = random_complex(vis_shape(cfg), 6)
    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    got = _gbls(cfg, G)
    st = _handle().stats()
    sub = list(range(0, 61075, 61075 // 600 + 1))
    assert len(sub) <= 600
    _assert_close(f"hera350 {kind}", cfg, got[sub], exact_gbls(cfg, G, sub=sub), cfg["eps"])
    for env in ("FFTVIS_HIP_NO_HERMITIAN", "FFTVIS_HIP_NO_COLUMN_PLAN"):
        _handle().reset_stats()
        monkeypatch.setenv(env, "1")
        other = _gbls(cfg, G)
        st2 = _handle().stats()
        monkeypatch.delenv(env)
        d = rel_l2(other, got)
        print("position-adjoint hera350", kind, env, d, st["spread_cells"], st2["spread_cells"], st["fft_cells"], st2["fft_cells"])
        assert 0 < d <= 1e-11, (kind, env, d)
        if env.endswith("HERMITIAN"):  # the packed run spreads half the transforms
            assert st["spread_cells"] < 0.8 * st2["spread_cells"], (st, st2)
        else:                          # the planned run moves fewer cells through the FFT passes
            assert st["fft_cells"] < st2["fft_cells"], (st, st2)
    gpu_simulate.release_handles()


# ---- 4. slicing edges ------------------------------------------------------------------------------------------------
def _edge_cfg(**kw):
    """The perturbed hex-7 with centimetre heights (height terms), polarized, full-Stokes sky, two beams, the exact form
    of the flipped baselines, fp64."""
    return position_config("cm", "full", "two", False, 2, **kw)


def _check_edge(label, cfg, k64=10.0, coord_mgr=None, ref_mgr=None, **kw):
    G = random_complex(vis_shape(cfg), 7)
    extra = {} if coord_mgr is None else {"coord_mgr": coord_mgr}
    got = _gbls(cfg, G, **extra, **kw)
    _assert_close(label, cfg, got, exact_gbls(cfg, G, coord_mgr=ref_mgr), cfg["eps"], k64)
    return G, got


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_source_chunks(gpu, monkeypatch, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    _check_edge(f"chunks lanes {lanes}", dict(_edge_cfg(nsrc=25, ntimes=4), min_chunks=3))


def test_free_running_lanes(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    monkeypatch.setenv("FFTVIS_HIP_PIPE", "0")
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = dict(_edge_cfg(nsrc=25, ntimes=5), min_chunks=2)
    G, got = _check_edge("free lanes", cfg)
    assert np.array_equal(got, _gbls(cfg, G))
    st = _handle().stats()
    gpu_simulate.release_handles()
    assert st["lanes"] == 2 and st["lane_mode"] == 0, st


@pytest.mark.parametrize("block_ch,ratio", [(1, 0.99), (2, 0.99), (2, 0.85), (2, 0.5)])
def test_channel_blocks_cut_across_frequency_groups(gpu, monkeypatch, block_ch, ratio):
    """nf = 5 in channel blocks of block_ch (FFTVIS_HIP_ADJ_ACC_BYTES: 48 bytes per channel and baseline) with frequency
    groups cut by FFTVIS_HIP_GROUP_RATIO; the last block is short."""
    cfg = _edge_cfg(nsrc=18, nfreq=5)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * 48 * len(cfg["baselines"])))
    monkeypatch.setenv("FFTVIS_HIP_GROUP_RATIO", str(ratio))
    _check_edge(f"blocks {block_ch} ratio {ratio}", cfg)


def test_upsample_125(gpu):
    _check_edge("sigma 1.25", dict(_edge_cfg(), upsample_factor=1.25), k64=20.0)


def test_empty_time_step(gpu):
    """Sources around the meridian at the first time: half a sidereal day later nothing is above the horizon."""
    cfg = _edge_cfg(nsrc=20)
    t0 = cfg["times"][0]
    lst = orc.gmst_rad(t0) + synth.HERA_LON
    rng = np.random.default_rng(1)
    cfg.update(ra=lst + rng.uniform(-0.3, 0.3, 20), dec=synth.HERA_LAT + rng.uniform(-0.3, 0.3, 20),
               times=t0 + np.array([0.0, 0.25, 0.5]))
    up = _up(cfg)
    assert np.any(up[0] > 0) and not np.any(up[-1] > 0)
    _check_edge("empty time step", cfg)


def test_coord_mgr_in_time_blocks_and_device_astrometry(gpu, monkeypatch):
    """Per-time astrometry contexts: applied on the host and streamed one time step per block (``coord_mgr=``; the blocks
    accumulate), and applied on the device (``astrom=``), both against the reference driven by the same manager."""
    from fftvis_amd.gpu import gpu_simulate
    from oracle import astrometry as oa

    cfg = _edge_cfg(ntimes=3)
    eq = orc.eq_unit_vectors(cfg["ra"], cfg["dec"])
    ctxs = np.stack([oa.plausible_context(20 + t, synth.HERA_LAT) for t in range(3)])

    class Mgr:  # the slice of matvis' manager the engine consumes
        def setup(self):
            pass

        def rotate(self, ti):
            self.all_coords_topo = oa.icrs_to_enu(eq, ctxs[ti])

    kw = dict(cfg, coord_method="CoordinateRotationERFA")
    calls = []
    real = gpu_simulate.SimHandle.run_position_adjoint
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_position_adjoint",
                        lambda self, *a: calls.append((a[0], a[1], a[-1])) or real(self, *a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    G, host = _check_edge("coord_mgr, time blocks", kw, coord_mgr=Mgr(), ref_mgr=Mgr())
    assert calls == [(0, 1, False), (0, 1, True), (0, 1, True)], calls
    monkeypatch.undo()
    dev = _gbls(kw, G, astrom=ctxs, device_astrometry=True)
    _assert_close("device astrometry", cfg, dev, exact_gbls(cfg, G, coord_mgr=Mgr()), cfg["eps"])
    assert rel_l2(host, _gbls(cfg, G)) > 1e-3  # and it is not the sidereal answer


# ---- 5. the surface --------------------------------------------------------------------------------------------------
def test_wrt_and_the_scatter_helper(gpu):
    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 8)
    gb = _gbls(cfg, G)
    ga = _gbls(cfg, G, wrt="ants")
    both = _gbls(cfg, G, wrt=("ants", "baselines"))
    one = _gbls(cfg, G, wrt=("baselines",))
    assert isinstance(both, tuple) and isinstance(one, tuple) and len(one) == 1
    assert ga.shape == (7, 3) and ga.dtype == np.float64
    assert np.array_equal(ga, fftvis_amd.baseline_to_antenna_gradient(gb, cfg["ants"], cfg["baselines"]))
    assert np.array_equal(both[0], ga) and np.array_equal(both[1], gb) and np.array_equal(one[0], gb)
    assert np.abs(ga.sum(axis=0)).max() <= 1e-12 * np.abs(gb).sum()
    autos = [k for k, (i, j) in enumerate(cfg["baselines"]) if i == j]
    assert len(autos) == 7 and np.any(gb[autos] != 0)  # an auto's own row is a derivative like any other; the scatter cancels it
    with pytest.raises(ValueError, match="force_use_type3"):  # the engine's own entry refuses the lattice path
        from fftvis_amd.wrapper import create_simulation_engine

        xy = 14.6 * hex_positions(1)
        lat = {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(7)}
        kw = {k: v for k, v in cfg.items() if k not in ("beam", "coord_method", "ants", "force_use_type3", "eps")}
        create_simulation_engine(backend="gpu").simulate(
            ants=lat, beam_list=cfg["beam"], coord_method="SiderealRotation", eps=cfg["eps"], force_use_type3=False,
            adjoint_of=(G, np.zeros((len(cfg["baselines"]), 3))), adjoint_wrt="positions", **kw)


def test_reproducible_for_a_lane_count(gpu, monkeypatch):
    cfg = _edge_cfg(nsrc=40, ntimes=4)
    G = random_complex(vis_shape(cfg), 10)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a, b = _gbls(cfg, G), _gbls(cfg, G)
        assert np.array_equal(a, b), lanes
        res[lanes] = a
    assert rel_l2(res["1"], res["2"]) <= 1e-12


def test_raw_c_abi_with_device_pointers(gpu):
    """fv_sim_run_position_adjoint through a bare ctypes handle configured by the engine's own setters, with device
    pointers for G and gbls: accumulate = 1 doubles the result, a sub-block of channels gives that block's share, and a
    lattice handle and a basis handle are refused."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs
    from tests.basis_adjoint_refs import basis_config

    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 7)
    gb = _gbls(cfg, G)
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        dG = torch.from_numpy(G).cuda()
        dB = torch.full((len(cfg["baselines"]), 3), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert L.fv_sim_run_position_adjoint(h._h, 0, nt, 0, nf, p(dG), 1, p(dB), 1, 0) == 0, L.fv_last_error()
        assert np.array_equal(dB.cpu().numpy(), gb)  # accumulate = 0 zeroes first
        assert L.fv_sim_run_position_adjoint(h._h, 0, nt, 0, nf, p(dG), 1, p(dB), 1, 1) == 0, L.fv_last_error()
        assert rel_l2(dB.cpu().numpy(), 2 * gb) < 1e-14
        # channel blocks add up to the whole
        parts = []
        for f0, f1 in ((0, 1), (1, nf)):
            blk = dG[f0:f1].contiguous()
            torch.cuda.synchronize()
            assert L.fv_sim_run_position_adjoint(h._h, 0, nt, f0, f1, p(blk), 1, p(dB), 1, 0) == 0, L.fv_last_error()
            parts.append(dB.cpu().numpy())
        assert np.linalg.norm(parts[0]) > 0 and rel_l2(parts[0] + parts[1], gb) <= 10 * cfg["eps"]
        sub = dict(cfg, freqs=cfg["freqs"][:1], fluxes=cfg["fluxes"][:, :1])
        _assert_close("c abi, one channel", sub, parts[0], exact_gbls(sub, G[:1]), cfg["eps"])
        # a host gbls with accumulate = 1
        hB = np.ascontiguousarray(gb.copy())
        assert L.fv_sim_run_position_adjoint(h._h, 0, nt, 0, nf, p(dG), 1, hB.ctypes.data_as(ctypes.c_void_p), 0, 1) == 0
        assert rel_l2(hB, 2 * gb) < 1e-14
    finally:
        gs._return_handle(key, h)
    buf = torch.zeros(1 << 16, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    xy = 14.6 * hex_positions(1)
    lat = dict(cfg, ants={i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(7)}, force_use_type3=False)
    fftvis_amd.simulate_vis(**lat)  # the lattice path
    bcfg = basis_config()
    for run_cfg, eps, word in ((None, cfg["eps"], b"fv_sim_set_array"), (bcfg, bcfg["eps"], b"basis")):
        if run_cfg is not None:
            fftvis_amd.simulate_vis(**run_cfg)
        key, h = gs._acquire_handle(0, 2, eps, 2, True)
        try:
            assert L.fv_sim_run_position_adjoint(h._h, 0, 1, 0, 1, p(buf), 1, p(buf), 1, 0) == 1
            assert word in L.fv_last_error(), L.fv_last_error()
        finally:
            gs._return_handle(key, h)


def test_nan_in_g_fails_and_the_handle_stays_usable(gpu):
    cfg = _edge_cfg()
    G = random_complex(vis_shape(cfg), 7)
    good = _gbls(cfg, G)
    bad = G.copy()
    bad[1, 0, 1, 0, 3] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="NaN"):
        _gbls(cfg, bad)
    assert np.array_equal(_gbls(cfg, G), good)


def test_bulk_device_memory_is_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the
    forward: no S buffer, staged array or tripled strength buffer stays."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _gbls(cfg, random_complex(vis_shape(cfg), 1))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


@pytest.mark.parametrize("heights", ["flat", "cm"])
def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu, heights):
    cfg = position_config(heights, "full", "two", False)
    before = fftvis_amd.simulate_vis(**cfg)
    _gbls(cfg, random_complex(vis_shape(cfg), 3))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)


# ---- 6. torch --------------------------------------------------------------------------------------------------------
def _torch_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k not in ("fluxes", "ants")}


def test_torch_gradcheck_both_inputs(gpu):
    """fp64, 8 sources, 1 channel, 1 time, eps 1e-12, position step 1e-3 m: the central difference's truncation is
    (k h)^2 / 6 with k = 2 pi nu / c = 3.1 / m, about 2e-6 relative, against rtol 1e-4."""
    import torch

    cfg = position_config("cm", "full", "two", False, nsrc=8, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)])
    _, _, cfg["fluxes"] = synth.catalog(8, cfg["freqs"], 0, polarized_sky=True)
    kw = _torch_kwargs(cfg)
    F = torch.tensor(cfg["fluxes"] + np.array([1.0, 0, 0, 0]), dtype=torch.float64, device="cuda", requires_grad=True)
    P = torch.tensor(np.array(list(cfg["ants"].values())), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, p: fftvis_amd.torch_simulate_vis_array(f, p, **kw), (F, P), eps=1e-3,
                                    atol=1e-7, rtol=1e-4)
    out = fftvis_amd.torch_simulate_vis_array(F, P, **kw)
    assert out.device == F.device and out.is_complex() and tuple(out.shape) == vis_shape(cfg)


def test_torch_backward_equals_the_direct_calls(gpu, monkeypatch):
    """d/d(F, P) sum |V - Dat|^2 through torch equals the direct calls on G = 2 (V - Dat); a tensor that does not require a
    gradient gets none, and its pass does not run; ``antnums`` names the rows."""
    import torch

    import fftvis_amd.adjoint as adj

    cfg = _edge_cfg()
    keys = [10 * (i + 1) for i in range(7)]
    ants = {k: v for k, v in zip(keys, cfg["ants"].values())}
    bls = [(keys[i], keys[j]) for i, j in cfg["baselines"]]
    kw = dict(_torch_kwargs(cfg), baselines=bls)
    Dat = random_complex(vis_shape(cfg), 15)
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda", requires_grad=True)
    P = torch.tensor(np.array(list(ants.values())), dtype=torch.float64, device="cuda", requires_grad=True)
    V = fftvis_amd.torch_simulate_vis_array(F, P, antnums=keys, **kw)
    (V - torch.from_numpy(Dat).cuda()).abs().pow(2).sum().backward()
    G = 2 * (V.detach().cpu().numpy() - Dat)
    direct = dict(cfg, ants=ants, baselines=bls)
    gp = _gbls(direct, G, wrt="ants")
    gf = fftvis_amd.simulate_vis_adjoint(G, **{k: v for k, v in direct.items() if k != "fluxes"}, full_stokes=True)
    assert np.allclose(P.grad.cpu().numpy(), gp, rtol=1e-12, atol=1e-12 * np.abs(gp).max())
    assert np.allclose(F.grad.cpu().numpy(), gf, rtol=1e-12, atol=1e-12 * np.abs(gf).max())
    ran = []
    real_p, real_f = adj.simulate_vis_position_adjoint, adj.simulate_vis_adjoint
    monkeypatch.setattr(adj, "simulate_vis_position_adjoint", lambda *a, **k: ran.append("positions") or real_p(*a, **k))
    monkeypatch.setattr(adj, "simulate_vis_adjoint", lambda *a, **k: ran.append("fluxes") or real_f(*a, **k))
    F2 = F.detach().clone().requires_grad_(True)
    fftvis_amd.torch_simulate_vis_array(F2, P.detach(), antnums=keys, **kw).abs().pow(2).sum().backward()
    assert ran == ["fluxes"] and F2.grad is not None
    P3 = P.detach().clone().requires_grad_(True)
    fftvis_amd.torch_simulate_vis_array(F.detach(), P3, antnums=keys, **kw).abs().pow(2).sum().backward()
    assert ran == ["fluxes", "positions"] and P3.grad is not None
    with pytest.raises(TypeError, match="antpos"):
        fftvis_amd.torch_simulate_vis_array(F, P, ants=ants, **kw)
