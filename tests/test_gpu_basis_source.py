"""GPU tests of the source-position derivatives through basis beams: ``simulate_vis_basis_source_adjoint``,
``simulate_vis_basis_source_jvp``, ``torch_simulate_vis_basis_sky`` and the C entry points
``fv_sim_run_basis_source_adjoint`` / ``fv_sim_run_basis_source_tangent``.

Both passes are compared element by element with the exact references built from the oracle's basis forward
(``basis_source_refs``; pinned on the CPU in ``test_basis_source_host``): over a configuration matrix, through the
transpose identity -- between the two passes, and over all four unknowns with the existing basis passes --, against the
passes without basis beams at K = 1, in the exact form of the (l, k) terms, at spline order 0, at the edges of the device's
slicing, on an ideal lattice, at HERA-350's size, through the bare C ABI and through torch.

Element-wise tolerances against the exact reference, as multiples of base.  base = eps in fp64; in fp32
base = max(the forward's own rel l2 error against the oracle on the same configuration, eps) (``_forward_base``).
  The gradient: rel l2 of the whole (ntimes, nsrc, 3) result, of an ENU component (below 1e-3 of the whole: against that
  floor) and max |err| / max |exact|, ``test_gpu_source_adjoint``'s measure.  The tangent: rel l2 of the whole, of a part
  (a channel, a time, a feed index) and max |err| / max |exact|, times the reference's cancellation factor kappa (asserted
  <= 4), ``test_gpu_basis_position``'s measure.  The constants are ``test_gpu_position_adjoint``'s, unchanged: whole 10 base
  in fp64 (20 at upsample_factor = 1.25), K64_PART 10, C_MAX 6, K32 13, K32_PART 40, C_MAX32 12.
  FFTVIS_TEST_METRICS=<file> logs each comparison's ratios, one JSON line each; the measured table is in
  profiles/MEASUREMENTS.md, "Basis source passes".
  Measured on an MI355X, as ratio / base (whole, part, max |err|):
  fp64 (base 6e-8), the 36 matrix cells: gradient 0.49, 0.63, 0.45; tangent 0.16, 0.39, 0.32.  The edges (chunks x lanes,
  free lanes, channel blocks, empty step, the two forms, hex-19, the C ABI's blocks): gradient 0.22, 0.23, 0.21; tangent
  0.34, 0.44, 0.67.  Order 0 (closed forms, sources on a jump whole and row by row, the Airy mix): gradient 0.08, 0.47, 0.09;
  tangent 0.18, 0.56, 0.30.  upsample_factor = 1.25 (bounds doubled): gradient 0.15, 0.21, 0.36; tangent 0.82, 1.74, 1.60.
  HERA-350's size (base 1e-12, phase-split references): gradient 2.81, 2.91, 2.21; tangent 4.78, 4.84, 3.10.
  fp32 (base 1e-5: the forward's own error stayed below eps in every cell), the 36 matrix cells: gradient 2.42, 3.02,
  2.31; tangent 0.79, 1.68, 1.36.  kappa of the tangent references <= 1.78.
  No constant moved.  Every one keeps at least twice its measured worst but C_MAX = 6 at HERA-350's size, which keeps
  1.94 x the tangent's 3.10 (the results are bitwise reproducible, and the sibling's reason for its 10 -- K^2 weighted terms
  adding at rounding level at eps 1e-12 -- is the same here).
"""

import ctypes
import json
import os

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from oracle import fftvis_oracle as orc
from tests.basis_position_refs import DB_SEED, hera_subset, random_dbls
from tests.basis_source_refs import (DT_SEED, G_SEED, basis_source_config, edge_config, empty_step_basis_config,
                                     exact_dv_topo, exact_gtopo, frozen_beam_dv_topo, frozen_beam_gtopo,
                                     gradcheck_basis_config, hera350_basis_source_config, hex19_basis_config,
                                     jump_basis_config, k1_configs, kappa, matrix_reference, mixed_order0_config,
                                     order0_reference, random_complex, random_dtopo, sidereal_jacobian, slicing_configs,
                                     split_dv_topo, split_gtopo, vis_shape)
from tests.helpers import rel_l2
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_basis_position import _tan_errors
from tests.test_gpu_position_adjoint import C_MAX, C_MAX32, K32, K32_PART, K64_PART
from tests.test_gpu_source_adjoint import _errors as _grad_errors

pytestmark = pytest.mark.gpu


def _check(kind, label, cfg, m, base, k64, kap=1.0):
    rec = {"pass": kind, "label": label, "precision": cfg.get("precision", 2), "base": base, "kappa": kap,
           **{k: v / (base * kap) for k, v in m.items()}}
    print("basis-source metrics", json.dumps(rec))
    path = os.environ.get("FFTVIS_TEST_METRICS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    fp64 = cfg.get("precision", 2) == 2
    whole, part = (k64, K64_PART * k64 / 10.0) if fp64 else (K32, K32_PART)
    part_key = "component" if kind == "adjoint" else "part"
    assert m["rel_l2"] <= whole * base * kap, (kind, label, m, base, kap)
    assert m[part_key] <= part * base * kap, (kind, label, m, base, kap)
    assert m["max_abs"] <= (C_MAX * k64 / 10.0 if fp64 else C_MAX32) * base * kap, (kind, label, m, base, kap)


def _assert_grad(label, cfg, got, exact, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert tuple(got.shape) == exact.shape and got.dtype == np.float64 and np.isfinite(got).all()
    _check("adjoint", label, cfg, _grad_errors(got, exact), base, k64)


def _assert_tan(label, cfg, got, exact, terms, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert got.shape == exact.shape and np.isfinite(np.asarray(got)).all()
    kap = kappa(exact, terms)
    assert kap <= 4.0, (label, kap)
    _check("tangent", label, cfg, _tan_errors(got, exact), base, k64, kap)


def _gtopo(cfg, G, wrt="topo", **kw):
    return fftvis_amd.simulate_vis_basis_source_adjoint(G, **cfg, wrt=wrt, **kw)


def _jvp(cfg, **kw):
    return fftvis_amd.simulate_vis_basis_source_jvp(**cfg, **kw)


def _cdt(cfg):
    return np.complex64 if cfg.get("precision", 2) == 1 else np.complex128


def _handle():
    from fftvis_amd.gpu import gpu_simulate

    (h,) = gpu_simulate._IDLE_HANDLES.values()
    return h


def _normals(cfg, coord_mgr=None):
    m = coord_mgr or orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    m.setup()
    return np.stack([orc._topo_of(m, ti).T for ti in range(len(cfg["times"]))])


def _assert_tangential_and_cut(cfg, got, coord_mgr=None):
    """n . g = 0 to rounding, and exact zeros below the horizon."""
    n = _normals(cfg, coord_mgr)
    tol = 1e-12 if cfg.get("precision", 2) == 2 else 1e-6
    assert np.abs(np.einsum("tjd,tjd->tj", n, got)).max() <= tol * np.abs(got).max()
    assert np.all(got[n[..., 2] <= 0] == 0)


def _both_against_references(label, cfg, k64=10.0, **kw):
    """Both passes of ``cfg`` against the references; returns (G, gtopo, dtopo, dV)."""
    G = random_complex(vis_shape(cfg), 7)
    dtopo = random_dtopo(cfg, DT_SEED)
    gt = _gtopo(cfg, G.astype(_cdt(cfg)), **kw)
    dv = _jvp(cfg, d_topo=dtopo, **kw)
    ref = {k: v for k, v in cfg.items() if k not in ("min_chunks", "upsample_factor")}
    _assert_grad(label, cfg, gt, exact_gtopo(ref, G), cfg["eps"], k64)
    dref, _, terms = exact_dv_topo(ref, dtopo)
    _assert_tan(label, cfg, dv, dref, terms, cfg["eps"], k64)
    _assert_tangential_and_cut(cfg, gt)
    return G, gt, dtopo, dv


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("tables", ["airy", "real", "complex"])
@pytest.mark.parametrize("sky", ["I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_basis_source_matrix(gpu, monkeypatch, precision, sky, tables, compat, heights):
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    cfg = basis_source_config(heights, tables, sky, compat, precision)
    G64, gref, dtopo, dref, terms = matrix_reference(heights, tables, sky, compat)
    label = f"matrix {precision} {sky} {tables} {compat} {heights}"
    base = _forward_base(cfg)
    gpu_simulate.release_handles()
    got = _gtopo(cfg, G64.astype(_cdt(cfg)))
    assert got.shape == (2, 24, 3)
    # (the adjoint has one path per array -- the transposed type-3 transform on the lanes' own plans, 2-D on the flat array
    # and 3-D otherwise, no height terms -- and those plans do not report to the handle's statistics, which describe the
    # forward's stages: the path assertion below is the tangent's, whose run is the forward's)
    _assert_tangential_and_cut(cfg, got)
    _assert_grad(label, cfg, got, gref, base)
    gpu_simulate.release_handles()
    dv = _jvp(cfg, d_topo=dtopo)
    st = _handle().stats()
    assert dv.shape == vis_shape(cfg) and dv.dtype == _cdt(cfg)
    _assert_tan(label, cfg, dv, dref, terms, base)
    # the run took the path the cell is named for: 2-D transforms, 2-D with height terms, the 3-D transform
    if heights == "cm":
        assert 2 <= st["height_terms"] <= 16 and st["n2_3"] == 1, st
    else:
        assert st["height_terms"] == 0 and (st["n2_3"] > 1) == (heights == "m"), st
    gpu_simulate.release_handles()


# ---- 2. the transpose identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("precision", [2, 1])
def test_dot_identity_between_the_two_passes_and_over_all_four_unknowns(gpu, precision, compat):
    """Re <dV, G> = sum d_topo . gtopo between the two new passes, then
    Re <dV, G> = d_topo . gtopo + d_baselines . gbls + Re <D, gcoefs> + <d_fluxes, gflux> with the existing basis passes, each
    to 10 eps |dV| |G| (the basis modules' bound).  d_topo keeps its radial part: the tangent removes it."""
    cfg = basis_source_config("cm", "complex", "full", compat, precision)
    G = random_complex(vis_shape(cfg), 4).astype(_cdt(cfg))
    dtopo = random_dtopo(cfg, DT_SEED)
    ds = _jvp(cfg, d_topo=dtopo).astype(np.complex128)
    gt = _gtopo(cfg, G)
    G128 = G.astype(np.complex128)
    lhs, rhs = np.vdot(G128, ds).real, float(np.sum(dtopo * gt))
    bound = 10 * cfg["eps"] * np.linalg.norm(ds) * np.linalg.norm(G)
    print("basis-source dot", precision, compat, abs(lhs - rhs) / bound)
    assert abs(lhs) > 1e-3 * np.linalg.norm(ds) * np.linalg.norm(G) and abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    D = random_complex(np.shape(cfg["beam_coefs"]), 5)
    dF = np.random.default_rng(3).normal(size=cfg["fluxes"].shape)
    dbls = random_dbls(cfg, DB_SEED)
    dv = ds + fftvis_amd.simulate_vis_basis_jvp(**cfg, d_baselines=dbls, d_beam_coefs=D, d_fluxes=dF).astype(np.complex128)
    gf, gc, gb = fftvis_amd.simulate_vis_basis_adjoint(G, **cfg, wrt=("fluxes", "beam_coefs", "baselines"))
    lhs = np.vdot(G128, dv).real
    parts = (rhs, float(np.sum(dbls * gb)), np.vdot(gc.astype(np.complex128), D).real, float(np.sum(dF * gf.astype(np.float64))))
    bound = 10 * cfg["eps"] * np.linalg.norm(dv) * np.linalg.norm(G)
    print("basis-source dot, four unknowns", precision, compat, abs(lhs - sum(parts)) / bound, parts)
    assert all(abs(x) > 1e-3 * abs(lhs) for x in parts)  # every part is a share of the sum
    assert abs(lhs - sum(parts)) <= bound, (lhs, parts, bound)


# ---- 3. K = 1 equals the passes without basis beams ---------------------------------------------------------------------
@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
def test_one_unit_basis_beam_equals_the_plain_passes(gpu, heights):
    """One Airy basis beam with every coefficient 1 is the same dish without ``beam_coefs``: both at eps 1e-12, agreement
    to the forward bound, 10 eps relative (no oracle)."""
    cfg, plain = k1_configs(heights)
    G = random_complex(vis_shape(cfg), 9)
    dtopo = random_dtopo(cfg, DT_SEED)
    gt, dv = _gtopo(cfg, G), _jvp(cfg, d_topo=dtopo)
    pg = fftvis_amd.simulate_vis_source_adjoint(G, **plain, wrt="topo")
    pv = fftvis_amd.simulate_vis_jvp(**plain, d_topo=dtopo)
    print("basis-source K = 1", heights, rel_l2(gt, pg) / cfg["eps"], rel_l2(dv, pv) / cfg["eps"])
    assert np.linalg.norm(pg) > 0 and np.linalg.norm(pv) > 0
    assert rel_l2(gt, pg) <= 10 * cfg["eps"] and rel_l2(dv, pv) <= 10 * cfg["eps"]


# ---- 4. the exact form with complex tables --------------------------------------------------------------------------------
def test_exact_form_takes_the_mirrored_half(gpu):
    """With complex tables the two forms of the (l, k) terms are different maps: the gradients and the tangents differ by
    far more than the tolerance, and each matches its own reference (the matrix compares them again, cell by cell)."""
    res = {}
    for compat in (True, False):
        cfg = basis_source_config("cm", "complex", "full", compat)
        G, gref, dtopo, dref, terms = matrix_reference("cm", "complex", "full", compat)
        gt, dv = _gtopo(cfg, G), _jvp(cfg, d_topo=dtopo)
        _assert_grad(f"forms, compat {compat}", cfg, gt, gref, cfg["eps"])
        _assert_tan(f"forms, compat {compat}", cfg, dv, dref, terms, cfg["eps"])
        res[compat] = gt, dv
    dg, dd = rel_l2(res[False][0], res[True][0]), rel_l2(res[False][1], res[True][1])
    print("basis-source forms differ by", dg, dd)
    assert dg > 0.1 and dd > 0.1  # (the references': 0.15 and 0.28; the tolerance is 6e-7)


# ---- 5. order 0 tables -----------------------------------------------------------------------------------------------------
def test_order_0_tables_against_the_frozen_beam_closed_forms(gpu):
    cfg, G, gref, dtopo, dref, terms = order0_reference()
    _assert_grad("order 0", cfg, _gtopo(cfg, G), gref, cfg["eps"])
    _assert_tan("order 0", cfg, _jvp(cfg, d_topo=dtopo), dref, terms, cfg["eps"])


def test_order_0_with_sources_on_a_jump(gpu):
    """Two sources inside the device's 1e-6 rad stencil of a jump of the order-0 tables: the beam term is 0 by definition
    for every term, so both passes equal the closed forms that hold the beams fixed, whole and row by row.  (A difference
    across the jump would put (jump) / 2e-6 into those rows.)"""
    cfg, mgr, rows = jump_basis_config()
    G = random_complex(vis_shape(cfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    gt = _gtopo(cfg, G, coord_mgr=mgr)
    gref = frozen_beam_gtopo(cfg, G, coord_mgr=mgr)
    assert np.all(np.any(gref[0, rows] != 0, axis=-1))
    _assert_grad("order 0 on a jump", cfg, gt, gref, cfg["eps"])
    for j in rows:
        _assert_grad(f"order 0 on a jump, row {j}", cfg, gt[:1, j:j + 1], gref[:1, j:j + 1], cfg["eps"])
    _assert_tangential_and_cut(cfg, gt, mgr)
    dref, terms = frozen_beam_dv_topo(cfg, dtopo, coord_mgr=mgr)
    _assert_tan("order 0 on a jump", cfg, _jvp(cfg, d_topo=dtopo, coord_mgr=mgr), dref, terms, cfg["eps"])
    only = np.zeros_like(dtopo)  # the two sources alone
    only[0, rows] = dtopo[0, rows]
    dref, terms = frozen_beam_dv_topo(cfg, only, coord_mgr=mgr)
    _assert_tan("order 0 on a jump, the two sources", cfg, _jvp(cfg, d_topo=only, coord_mgr=mgr), dref, terms, cfg["eps"])


def test_an_airy_and_order_0_table_mix_keeps_its_differences(gpu):
    """K = 3 with an Airy dish and two order-0 tables: the (Airy, table) terms vary smoothly through the dish and keep the
    beam term, so the results match the references by differences and are NOT the frozen-beam closed forms."""
    cfg = mixed_order0_config()
    G = random_complex(vis_shape(cfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    gt, dv = _gtopo(cfg, G), _jvp(cfg, d_topo=dtopo)
    _assert_grad("order 0 mix", cfg, gt, exact_gtopo(cfg, G), cfg["eps"])
    dref, _, terms = exact_dv_topo(cfg, dtopo)
    _assert_tan("order 0 mix", cfg, dv, dref, terms, cfg["eps"])
    assert rel_l2(gt, frozen_beam_gtopo(cfg, G)) > 1e-3 and rel_l2(dv, frozen_beam_dv_topo(cfg, dtopo)[0]) > 1e-3


# ---- 6. slicing edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_source_chunks(gpu, monkeypatch, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    _both_against_references(f"chunks lanes {lanes}", slicing_configs()["chunks"])


def test_free_running_lanes(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    monkeypatch.setenv("FFTVIS_HIP_PIPE", "0")
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = slicing_configs()["free lanes"]
    G, gt, dtopo, dv = _both_against_references("free lanes", cfg)
    assert np.array_equal(gt, _gtopo(cfg, G)) and np.array_equal(dv, _jvp(cfg, d_topo=dtopo))
    st = _handle().stats()
    gpu_simulate.release_handles()
    assert st["lanes"] == 2 and st["lane_mode"] == 0, st


@pytest.mark.parametrize("block_ch,ratio", [(1, 0.99), (2, 0.99), (2, 0.85)])
def test_channel_blocks_cut_across_frequency_groups(gpu, monkeypatch, block_ch, ratio):
    """nf = 5 in channel blocks of block_ch with frequency groups cut by FFTVIS_HIP_GROUP_RATIO; the last block is short.
    FFTVIS_HIP_ADJ_ACC_BYTES: the adjoint's accumulator takes 24 bytes per channel and source (18 sources), so it runs
    block_ch channels per block; the tangent cuts at 48 bytes per channel and baseline and then runs one channel per block."""
    cfg = slicing_configs()["blocks"]
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * 24 * 18))
    monkeypatch.setenv("FFTVIS_HIP_GROUP_RATIO", str(ratio))
    _both_against_references(f"blocks {block_ch} ratio {ratio}", cfg)


def test_upsample_125(gpu):
    _both_against_references("sigma 1.25", dict(edge_config(), upsample_factor=1.25), k64=20.0)


def test_empty_time_step(gpu):
    """Nothing above the horizon at the last time: its gradient rows and its tangent are exactly zero, some sources are
    below the horizon at the middle time and get exact zeros there, and the rest matches the references."""
    cfg = empty_step_basis_config()
    n = _normals(cfg)
    assert np.any(n[1, :, 2] <= 0) and np.any(n[1, :, 2] > 0) and not np.any(n[2, :, 2] > 0)
    G, gt, _, dv = _both_against_references("empty time step", cfg)
    assert not gt[2].any() and gt[0].any() and not dv[:, -1].any() and dv[:, 0].any()
    short = dict(cfg, times=cfg["times"][:-1])
    assert np.array_equal(gt[:-1], _gtopo(short, np.ascontiguousarray(G[:, :-1])))


def test_raw_c_abi(gpu):
    """Both entry points through a bare ctypes handle configured by the engine's own setters: device and host
    destinations, accumulate 0 and 1, the t0 / f0 offsets -- channel and time sub-blocks that add up to the whole --,
    values that are not finite refused with the handle left usable, and a handle without basis beams refused."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 7)
    dtopo = random_dtopo(cfg, 3)
    gt, dv = _gtopo(cfg, G), _jvp(cfg, d_topo=dtopo)
    nf, nt, nsrc = len(cfg["freqs"]), len(cfg["times"]), len(cfg["ra"])
    L = _lib.lib()
    adj, tan = L.fv_sim_run_basis_source_adjoint, L.fv_sim_run_basis_source_tangent
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        dG = torch.from_numpy(G).cuda()
        dT = torch.full((nt, nsrc, 3), 7.0, dtype=torch.float64, device="cuda")
        dD = torch.from_numpy(dtopo).cuda()
        dV = torch.full(dv.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        assert adj(h._h, 0, nt, 0, nf, p(dG), 1, p(dT), 1, 0) == 0, L.fv_last_error()
        assert np.array_equal(dT.cpu().numpy(), gt)  # accumulate = 0 zeroes first
        assert adj(h._h, 0, nt, 0, nf, p(dG), 1, p(dT), 1, 1) == 0, L.fv_last_error()
        assert rel_l2(dT.cpu().numpy(), 2 * gt) < 1e-14
        hT = np.ascontiguousarray(gt.copy())  # a host gtopo with accumulate = 1
        assert adj(h._h, 0, nt, 0, nf, hp(G), 0, hp(hT), 0, 1) == 0, L.fv_last_error()
        assert rel_l2(hT, 2 * gt) < 1e-14
        assert tan(h._h, 0, nt, 0, nf, p(dD), 1, p(dV), 1) == 0, L.fv_last_error()
        assert np.array_equal(dV.cpu().numpy(), dv)  # always overwritten
        hV = np.full(dv.shape, 7.0, dtype=np.complex128)
        assert tan(h._h, 0, nt, 0, nf, hp(dtopo), 0, hp(hV), 0) == 0, L.fv_last_error()
        assert np.array_equal(hV, dv)
        # channel blocks add up to the whole; a time block fills its own rows and slots
        total = np.zeros_like(gt)
        for f0, f1 in ((0, 1), (1, nf)):
            blk = dG[f0:f1].contiguous()
            out = torch.full((f1 - f0,) + dv.shape[1:], 7.0, dtype=torch.complex128, device="cuda")
            torch.cuda.synchronize()
            assert adj(h._h, 0, nt, f0, f1, p(blk), 1, p(dT), 1, 0) == 0, L.fv_last_error()
            part = dT.cpu().numpy()
            assert np.linalg.norm(part) > 0
            total += part
            assert tan(h._h, 0, nt, f0, f1, p(dD), 1, p(out), 1) == 0, L.fv_last_error()
            assert rel_l2(out.cpu().numpy(), dv[f0:f1]) <= 10 * cfg["eps"]
        assert rel_l2(total, gt) <= 10 * cfg["eps"]
        blk = dG[:, 1:2].contiguous()
        one = np.zeros((1, nsrc, 3))
        out = torch.full((nf, 1) + dv.shape[2:], 7.0, dtype=torch.complex128, device="cuda")
        row = dD[1:2].contiguous()
        torch.cuda.synchronize()
        assert adj(h._h, 1, 2, 0, nf, p(blk), 1, hp(one), 0, 0) == 0, L.fv_last_error()
        assert np.array_equal(one[0], gt[1])
        assert tan(h._h, 1, 2, 0, nf, p(row), 1, p(out), 1) == 0, L.fv_last_error()
        assert rel_l2(out.cpu().numpy(), dv[:, 1:2]) <= 10 * cfg["eps"]
        # NaN in G and a dtopo that is not finite fail before anything runs; the next call returns the good result's bits
        bad = G.copy()
        bad[1, 0, 1, 0, 3] = np.nan
        assert adj(h._h, 0, nt, 0, nf, hp(bad), 0, hp(hT), 0, 0) == 1
        assert b"NaN" in L.fv_last_error()
        assert adj(h._h, 0, nt, 0, nf, hp(G), 0, hp(hT), 0, 0) == 0, L.fv_last_error()
        assert np.array_equal(hT, gt)
        for device in (0, 1):
            B = dtopo.copy()
            B[1, 4, 1] = np.inf
            dBad = torch.from_numpy(B).cuda()
            torch.cuda.synchronize()
            assert (tan(h._h, 0, nt, 0, nf, p(dBad), 1, hp(hV), 0) if device else
                    tan(h._h, 0, nt, 0, nf, hp(B), 0, hp(hV), 0)) == 1
            assert b"not finite" in L.fv_last_error()
            hV[...] = 7.0
            assert tan(h._h, 0, nt, 0, nf, hp(dtopo), 0, hp(hV), 0) == 0, L.fv_last_error()
            assert np.array_equal(hV, dv)
        # the entry points of the handle without basis beams keep refusing this one, with their present messages
        assert L.fv_sim_run_source_adjoint(h._h, 0, nt, 0, nf, p(dG), 1, p(dT), 1, 0) == 1
        assert b"does not cover basis beams" in L.fv_last_error()
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, nf, None, 0, p(dD), 1, p(dV), 1) == 1
        assert b"does not cover basis beams" in L.fv_last_error()
    finally:
        gs._return_handle(key, h)
    buf = torch.zeros(1 << 16, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    plain = dict(synth.make_config("C1", nsrc=20, nfreq=3, ntimes=2), polarized=True)
    gs.release_handles()
    fftvis_amd.simulate_vis(**plain)
    key, h = gs._acquire_handle(0, 2, plain["eps"], 2, True)
    try:
        assert adj(h._h, 0, 1, 0, 1, p(buf), 1, p(buf), 1, 0) == 1
        assert b"fv_sim_set_basis" in L.fv_last_error() and b"fv_sim_run_source_adjoint" in L.fv_last_error()
        assert tan(h._h, 0, 1, 0, 1, p(buf), 1, p(buf), 1) == 1
        assert b"fv_sim_set_basis" in L.fv_last_error() and b"fv_sim_run_tangent" in L.fv_last_error()
    finally:
        gs._return_handle(key, h)


# ---- 7. an ideal lattice -----------------------------------------------------------------------------------------------
def test_ideal_hex19_with_redundant_runs_and_mirror_pairs(gpu, monkeypatch):
    """Redundant runs and mirror pairs on, against the references; then each against the run with the pruning switched off.
    In the tangent the switches only change which lane group writes a slot: 1e-12, ``test_gpu_basis_position``'s bound.  In
    the adjoint the runs are the transform's SOURCES -- without them every baseline is a source of its own --, so the two
    are different computations of one sum and agree to the transforms' tolerance, 10 eps."""
    cfg = hex19_basis_config()
    G, gt, dtopo, dv = _both_against_references("ideal hex-19", cfg)
    for env in ("FFTVIS_HIP_NO_TARGET_DEDUP", "FFTVIS_HIP_NO_TARGET_PAIRS"):
        monkeypatch.setenv(env, "1")
        d = rel_l2(_gtopo(cfg, G), gt), rel_l2(_jvp(cfg, d_topo=dtopo), dv)
        monkeypatch.delenv(env)
        print("basis-source lattice", env, d)
        assert d[0] <= 10 * cfg["eps"] and d[1] <= 1e-12, (env, d)


# ---- 8. HERA-350's size ------------------------------------------------------------------------------------------------
def test_hera350_packed_transforms_and_column_plan(gpu, monkeypatch):
    """61 075 baselines, 64 sources, 2 channels, 1 time, eps 1e-12.  G is supported on a seeded subset of 600 baselines, so
    the gradient's reference needs the oracle on those alone, and the tangent is compared on them: the device runs all
    baselines either way.  The references are the phase-split ones (``split_gtopo`` / ``split_dv_topo``): differences
    through the phase of an 876 m baseline carry a remainder of 4e-9, four hundred times this test's bound."""
    from fftvis_amd.gpu import gpu_simulate

    cfg = hera350_basis_source_config()
    sub = hera_subset(cfg)
    scfg = dict(cfg, baselines=[cfg["baselines"][i] for i in sub])
    G = np.zeros(vis_shape(cfg), dtype=np.complex128)
    G[..., sub] = random_complex(vis_shape(scfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    gpu_simulate.release_handles()
    gt = _gtopo(cfg, G)
    dv = _jvp(cfg, d_topo=dtopo)
    _assert_grad("hera350", cfg, gt, split_gtopo(scfg, G[..., sub]), cfg["eps"])
    dref, terms = split_dv_topo(scfg, dtopo)
    _assert_tan("hera350", cfg, dv[..., sub], dref, terms, cfg["eps"])
    for env in ("FFTVIS_HIP_NO_HERMITIAN", "FFTVIS_HIP_NO_COLUMN_PLAN"):
        monkeypatch.setenv(env, "1")
        d = rel_l2(_gtopo(cfg, G), gt), rel_l2(_jvp(cfg, d_topo=dtopo), dv)
        monkeypatch.delenv(env)
        print("basis-source hera350", env, d)
        # the adjoint's transforms have the baselines as sources: neither switch reaches them, only the tangent's gathers
        assert 0 < d[1] and max(d) <= 1e-11, (env, d)
    gpu_simulate.release_handles()


# ---- 9. failure and clean-up behaviour -----------------------------------------------------------------------------------
def test_values_that_are_not_finite_fail_through_python(gpu):
    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 7)
    dtopo = random_dtopo(cfg, 3)
    gt, dv = _gtopo(cfg, G), _jvp(cfg, d_topo=dtopo)
    bad = G.copy()
    bad[1, 0, 1, 0, 3] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="NaN"):
        _gtopo(cfg, bad)
    B = dtopo.copy()
    B[0, 2, 0] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="finite"):
        _jvp(cfg, d_topo=B)
    assert np.array_equal(_gtopo(cfg, G), gt) and np.array_equal(_jvp(cfg, d_topo=dtopo), dv)


def test_reproducible_for_a_lane_count(gpu, monkeypatch):
    cfg = slicing_configs()["lanes"]
    G = random_complex(vis_shape(cfg), 10)
    dtopo = random_dtopo(cfg, 4)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a, b = _gtopo(cfg, G), _gtopo(cfg, G)
        c, d = _jvp(cfg, d_topo=dtopo), _jvp(cfg, d_topo=dtopo)
        assert np.array_equal(a, b) and np.array_equal(c, d), lanes
        res[lanes] = (a, c)
    assert rel_l2(res["1"][0], res["2"][0]) <= 1e-12 and rel_l2(res["1"][1], res["2"][1]) <= 1e-12


def test_the_flux_pass_and_this_pass_alternate_on_one_handle(gpu):
    """``adjoint_flux`` and the source pass share a term's source coordinates on the handle (with the mirrored set in the
    exact form): alternating them returns each one's own bits."""
    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 7)
    flux = lambda: fftvis_amd.simulate_vis_basis_adjoint(G, **cfg, wrt="fluxes")
    f0, g0 = flux(), _gtopo(cfg, G)
    assert np.array_equal(flux(), f0) and np.array_equal(_gtopo(cfg, G), g0) and np.array_equal(flux(), f0)


@pytest.mark.parametrize("heights", ["flat", "cm"])
def test_a_forward_call_after_each_pass_returns_the_same_bits(gpu, heights):
    cfg = basis_source_config(heights, "complex", "full", False)
    before = fftvis_amd.simulate_vis(**cfg)
    _gtopo(cfg, random_complex(vis_shape(cfg), 3))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)
    _jvp(cfg, d_topo=random_dtopo(cfg, 3))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)


def test_bulk_device_memory_is_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after either pass no more than it held after the
    forward: no accumulator, staged array or multiplied strength buffer stays."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = edge_config()
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _gtopo(cfg, random_complex(vis_shape(cfg), 1))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)
    _jvp(cfg, d_topo=random_dtopo(cfg, 1))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


# ---- 10. the surface and torch --------------------------------------------------------------------------------------------
def test_wrt_radec_and_d_radec_are_the_chained_topo_results(gpu):
    import torch

    cfg = edge_config()
    G, gref, _, _, _ = matrix_reference("cm", "complex", "full", False)
    gt = _gtopo(cfg, G)
    gr = _gtopo(cfg, G, wrt="radec")
    both = _gtopo(cfg, G, wrt=("radec", "topo"))
    assert isinstance(both, tuple) and gr.shape == (24, 2) and gr.dtype == np.float64
    J = fftvis_amd.radec_jacobian(cfg["ra"], cfg["dec"], cfg["times"], cfg["telescope_loc"])
    assert np.array_equal(gr, fftvis_amd.topo_to_radec_gradient(gt, J))
    assert np.array_equal(both[0], gr) and np.array_equal(both[1], gt)
    assert rel_l2(gr, np.einsum("tjd,tjdc->jc", gref, sidereal_jacobian(cfg))) <= 10 * cfg["eps"]
    dr = np.random.default_rng(5).normal(size=(24, 2))
    dv = _jvp(cfg, d_radec=dr)
    assert np.array_equal(dv, _jvp(cfg, d_topo=np.einsum("tjdc,jc->tjd", J, dr)))
    assert abs(np.vdot(G, dv).real - float(np.sum(dr * gr))) <= 10 * cfg["eps"] * np.linalg.norm(G) * np.linalg.norm(dv)
    # tensors on the device in, tensors on the device out; host tensors in, host tensors out
    tt, tr_ = _gtopo(cfg, torch.from_numpy(G).cuda(), wrt=("topo", "radec"))
    assert tt.device.type == "cuda" and tt.dtype == torch.float64 and np.array_equal(tt.cpu().numpy(), gt)
    assert tr_.device.type == "cuda" and rel_l2(tr_.cpu().numpy(), gr) <= 1e-14
    tdv = _jvp(cfg, d_radec=torch.from_numpy(dr).cuda())
    assert tdv.device.type == "cuda" and tdv.dtype == torch.complex128 and np.array_equal(tdv.cpu().numpy(), dv)
    host = _jvp(cfg, d_radec=torch.from_numpy(dr))
    assert isinstance(host, torch.Tensor) and host.device.type == "cpu" and np.array_equal(host.numpy(), dv)


def _torch_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec", "beam_coefs")}


def test_torch_gradcheck_all_three_inputs(gpu):
    """fp64: 8 sources, 1 channel (150 MHz), 1 time, 6 baselines, K = 2 bilinear tables, eps 1e-12; reverse and forward
    mode over fluxes, coefficients and (ra, dec).  Angular step 1e-6 rad -- the nearest node of a table is 4.5e-4 rad away
    (``test_basis_source_host``), so torch's differences stay inside one bilinear patch --: the central difference's
    truncation is (k h)^2 / 6 with k = 2 pi nu |b| / c <= 92 / rad, 1.4e-9 relative, against rtol 1e-4; atol 1e-6 is 1e-8 of
    the entries' scale (``test_gpu_source_adjoint``'s figures for this shape)."""
    import torch

    cfg = gradcheck_basis_config()
    kw = _torch_kwargs(cfg)
    F = torch.tensor(cfg["fluxes"] + np.array([1.0, 0, 0, 0]), dtype=torch.float64, device="cuda", requires_grad=True)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, c, p: fftvis_amd.torch_simulate_vis_basis_sky(f, c, p, **kw), (F, C, P),
                                    eps=1e-6, atol=1e-6, rtol=1e-4, check_forward_ad=True)
    out = fftvis_amd.torch_simulate_vis_basis_sky(F, C, P, **kw)
    assert out.device == F.device and out.is_complex() and tuple(out.shape) == vis_shape(cfg)


def test_torch_backward_equals_the_direct_calls_and_runs_only_what_is_needed(gpu, monkeypatch):
    """d/d(F, C, radec) Re <W, V> through torch equals the direct calls on G = W -- a loss whose gradient torch hands over
    bit for bit: the beam term is a central difference at 1e-6 rad of sums that are linear in G, so a G that differs in
    its last bit (as 2 |x| x / |x| does from 2 x) moves it by 1e-10 of those sums, which an equality to 1e-12 would meet.
    With only ``radec`` requiring a gradient the backward is one ``simulate_vis_basis_source_adjoint`` call and no
    ``simulate_vis_basis_adjoint`` call, and the other way round."""
    import torch

    import fftvis_amd.adjoint as adj

    cfg = edge_config()
    kw = _torch_kwargs(cfg)
    G = random_complex(vis_shape(cfg), 15)
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda", requires_grad=True)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True)
    V = fftvis_amd.torch_simulate_vis_basis_sky(F, C, P, **kw)
    (V * torch.from_numpy(G).cuda().conj()).real.sum().backward()
    gf, gc = fftvis_amd.simulate_vis_basis_adjoint(G, **cfg, wrt=("fluxes", "beam_coefs"))
    gp = _gtopo(cfg, G, wrt="radec")
    for got, want in ((F.grad, gf), (C.grad, gc), (P.grad, gp)):
        assert np.allclose(got.cpu().numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    calls = []
    real_b, real_s = adj.simulate_vis_basis_adjoint, adj.simulate_vis_basis_source_adjoint
    monkeypatch.setattr(adj, "simulate_vis_basis_adjoint", lambda *a, **k: calls.append(tuple(k["wrt"])) or real_b(*a, **k))
    monkeypatch.setattr(adj, "simulate_vis_basis_source_adjoint", lambda *a, **k: calls.append(k["wrt"]) or real_s(*a, **k))
    P2 = P.detach().clone().requires_grad_(True)
    fftvis_amd.torch_simulate_vis_basis_sky(F.detach(), C.detach(), P2, **kw).abs().pow(2).sum().backward()
    assert calls == ["radec"] and P2.grad is not None
    F3, C3 = F.detach().clone().requires_grad_(True), C.detach().clone().requires_grad_(True)
    fftvis_amd.torch_simulate_vis_basis_sky(F3, C3, P.detach(), **kw).abs().pow(2).sum().backward()
    assert calls == ["radec", ("fluxes", "beam_coefs")] and F3.grad is not None and C3.grad is not None
    C4 = C.detach().clone().requires_grad_(True)
    fftvis_amd.torch_simulate_vis_basis_sky(F.detach(), C4, P.detach(), **kw).abs().pow(2).sum().backward()
    assert calls[2:] == [("beam_coefs",)] and C4.grad is not None


def test_forward_ad_equals_the_direct_jvp_calls(gpu):
    import torch
    import torch.autograd.forward_ad as fwAD

    cfg = edge_config()
    kw = _torch_kwargs(cfg)
    dr = np.random.default_rng(6).normal(size=(24, 2))
    D = random_complex(np.shape(cfg["beam_coefs"]), 5)
    dF = np.random.default_rng(3).normal(size=cfg["fluxes"].shape)
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda")
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda")
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda")
    tF = torch.tensor(dF, dtype=torch.float64, device="cuda")
    tC = torch.tensor(D, dtype=torch.complex128, device="cuda")
    tP = torch.tensor(dr, dtype=torch.float64, device="cuda")
    src = _jvp(cfg, d_radec=dr)
    rest = fftvis_amd.simulate_vis_basis_jvp(**cfg, d_beam_coefs=D, d_fluxes=dF)
    with fwAD.dual_level():
        for f, c, pp, want in ((F, C, fwAD.make_dual(P, tP), src),
                               (fwAD.make_dual(F, tF), fwAD.make_dual(C, tC), fwAD.make_dual(P, tP), src + rest)):
            tangent = fwAD.unpack_dual(fftvis_amd.torch_simulate_vis_basis_sky(f, c, pp, **kw)).tangent
            assert tangent is not None and tangent.device == F.device
            assert rel_l2(tangent.cpu().numpy(), want) <= 1e-12
