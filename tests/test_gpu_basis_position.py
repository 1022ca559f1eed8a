"""GPU tests of the position derivatives through basis beams: ``simulate_vis_basis_adjoint`` with ``wrt="ants"`` /
``"baselines"``, ``simulate_vis_basis_jvp`` with ``d_ants`` / ``d_baselines``, ``torch_simulate_vis_basis_array`` and the C
entry points ``fv_sim_run_basis_position_adjoint`` / ``fv_sim_run_basis_position_tangent``.

Both passes are compared element by element with the exact references built from the oracle's basis forward
(``position_adjoint_refs.exact_gbls``, ``tangent_refs.exact_dv_baselines`` on a configuration with ``beam_coefs``; pinned
against finite differences of the oracle in ``test_basis_position_host``): over a configuration matrix, through the
transpose identity with the flux and coefficient passes, against the passes without basis beams at K = 1, at the edges of
the device's slicing, on an ideal lattice, at HERA-350's size, through the bare C ABI and through torch.

Element-wise tolerances against the exact reference, as multiples of base.  base = eps in fp64; in fp32
base = max(the forward's own rel l2 error against the oracle on the same configuration, eps) (``_forward_base``).
  The gradient: rel l2 of the whole (nbls, 3) result, of a component (east, north, up; below 1e-3 of the whole: against
  that floor) and max |err| / max |exact|, with ``test_gpu_position_adjoint``'s constants.  The tangent: rel l2 of the
  whole, of a part (a channel, a time, a feed index) and max |err| / max |exact|, times the reference's cancellation
  factor kappa (asserted <= 4), with the same constants, as ``test_gpu_tangent`` uses them.  The whole-result bound of 10
  base in fp64 (20 at upsample_factor = 1.25) is the project's forward bound.  FFTVIS_TEST_METRICS=<file> logs each
  comparison's ratios, one JSON line each; the measured table is in profiles/MEASUREMENTS.md, "Basis position passes".
  Measured on an MI355X, as ratio / base (whole, part, max |err|):
  fp64 (base 6e-8), the 36 matrix cells: gradient 0.12, 0.14, 0.15; tangent 0.11, 0.21, 0.11.  The edges: gradient 0.28,
  0.38, 0.29; tangent 0.19, 0.23, 0.21; at upsample_factor = 1.25 gradient 0.30, 0.94, 0.37; tangent 0.10, 1.14, 0.07.
  HERA-350's size (base 1e-12): gradient 1.20, 1.90, 4.16; tangent 0.67, 0.81, 1.20.
  fp32 (base 1e-5: the forward's own error stayed below eps in every cell), the 36 matrix cells: gradient 0.75, 0.89,
  0.68; tangent 0.51, 0.93, 0.49.  kappa of the tangent references <= 1.15 (edges <= 1.52).
"""

import ctypes
import json
import os

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from tests.basis_position_refs import (DB_SEED, G_SEED, basis_position_config, edge_config, empty_step_basis_config,
                                       exact_dv_baselines, exact_gbls, hera350_basis_config, hera_subset,
                                       hex19_basis_config, k1_configs, kappa, matrix_reference, random_complex, random_dbls,
                                       vis_shape)
from tests.helpers import floored_rel, rel_l2, worst_part
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_position_adjoint import C_MAX32, K32, K32_PART, K64_PART

pytestmark = pytest.mark.gpu

# fp64: max |err| / (base max |exact|).  The sibling modules' 6 is 1.4 x this module's worst (4.16, the gradient at
# HERA-350's size at eps 1e-12, where the K^2 weighted terms of a baseline add at the level of fp64 rounding of the
# transforms); 10 is 2.4 x.  Every other constant is the siblings' and keeps more than twice its measured worst.
C_MAX = 10.0


def _grad_errors(got, exact):
    err = np.asarray(got).astype(np.float64) - exact
    floor = 1e-3 * np.linalg.norm(exact)
    return {"rel_l2": floored_rel(err, exact, floor), "part": worst_part(err, exact, 1, floor),
            "max_abs": float(np.abs(err).max() / max(np.abs(exact).max(), 1e-300))}


def _tan_errors(got, exact):
    err = np.asarray(got).astype(np.complex128) - exact
    floor = 1e-3 * np.linalg.norm(exact)
    return {"rel_l2": floored_rel(err, exact, floor), "part": max(worst_part(err, exact, ax, floor) for ax in (0, 1, 2, 3)),
            "max_abs": float(np.abs(err).max() / max(np.abs(exact).max(), 1e-300))}


def _check(kind, label, cfg, m, base, k64, kap=1.0):
    rec = {"pass": kind, "label": label, "precision": cfg.get("precision", 2), "base": base, "kappa": kap,
           **{k: v / (base * kap) for k, v in m.items()}}
    print("basis-position metrics", json.dumps(rec))
    path = os.environ.get("FFTVIS_TEST_METRICS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    fp64 = cfg.get("precision", 2) == 2
    whole, part = (k64, K64_PART * k64 / 10.0) if fp64 else (K32, K32_PART)
    assert m["rel_l2"] <= whole * base * kap, (kind, label, m, base, kap)
    assert m["part"] <= part * base * kap, (kind, label, m, base, kap)
    assert m["max_abs"] <= (C_MAX * k64 / 10.0 if fp64 else C_MAX32) * base * kap, (kind, label, m, base, kap)


def _assert_grad(label, cfg, got, exact, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert got.shape == exact.shape and got.dtype == np.float64 and np.isfinite(got).all()
    _check("adjoint", label, cfg, _grad_errors(got, exact), base, k64)


def _assert_tan(label, cfg, got, exact, terms, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert got.shape == exact.shape and np.isfinite(np.asarray(got)).all()
    kap = kappa(exact, terms)
    assert kap <= 4.0, (label, kap)
    _check("tangent", label, cfg, _tan_errors(got, exact), base, k64, kap)


def _gbls(cfg, G, wrt="baselines", **kw):
    return fftvis_amd.simulate_vis_basis_adjoint(G, **cfg, wrt=wrt, **kw)


def _jvp(cfg, **kw):
    return fftvis_amd.simulate_vis_basis_jvp(**cfg, **kw)


def _cdt(cfg):
    return np.complex64 if cfg.get("precision", 2) == 1 else np.complex128


def _handle():
    from fftvis_amd.gpu import gpu_simulate

    (h,) = gpu_simulate._IDLE_HANDLES.values()
    return h


def _both_against_references(label, cfg, k64=10.0, **kw):
    """Both passes of ``cfg`` against the references; returns (G, gbls, dbls, dV)."""
    G = random_complex(vis_shape(cfg), 7)
    dbls = random_dbls(cfg, DB_SEED)
    gb = _gbls(cfg, G.astype(_cdt(cfg)), **kw)
    dv = _jvp(cfg, d_baselines=dbls, **kw)
    ref = dict(cfg)
    _assert_grad(label, cfg, gb, exact_gbls(ref, G), cfg["eps"], k64)
    _assert_tan(label, cfg, dv, *exact_dv_baselines(ref, dbls), cfg["eps"], k64)
    return G, gb, dbls, dv


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("tables", ["airy", "real", "complex"])
@pytest.mark.parametrize("sky", ["I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_basis_position_matrix(gpu, monkeypatch, precision, sky, tables, compat, heights):
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    cfg = basis_position_config(heights, tables, sky, compat, precision)
    G64, gref, dbls, dref, terms = matrix_reference(heights, tables, sky, compat)
    label = f"matrix {precision} {sky} {tables} {compat} {heights}"
    base = _forward_base(cfg)
    gpu_simulate.release_handles()
    got = _gbls(cfg, G64.astype(_cdt(cfg)))
    st = _handle().stats()
    assert got.shape == (len(cfg["baselines"]), 3)
    assert np.linalg.norm(gref[:, 2]) > 1e-3 * np.linalg.norm(gref)  # the up component is checked on the flat array too
    _assert_grad(label, cfg, got, gref, base)
    dv = _jvp(cfg, d_baselines=dbls)
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
def test_dot_identity_over_all_three_unknowns(gpu, precision, compat):
    """Re <dV, G> = d_baselines . gbls + Re <D, gcoefs> + <d_fluxes, gflux>: one jvp call with the three tangents, one joint
    adjoint call, to 10 eps |dV| |G| (the basis-tangent module's bound)."""
    cfg = basis_position_config("cm", "complex", "full", compat, precision)
    G = random_complex(vis_shape(cfg), 4).astype(_cdt(cfg))
    D = random_complex(np.shape(cfg["beam_coefs"]), 5)
    dF = np.random.default_rng(3).normal(size=cfg["fluxes"].shape)
    dbls = random_dbls(cfg, DB_SEED)
    dv = _jvp(cfg, d_baselines=dbls, d_beam_coefs=D, d_fluxes=dF).astype(np.complex128)
    gf, gc, gb = _gbls(cfg, G, wrt=("fluxes", "beam_coefs", "baselines"))
    lhs = np.vdot(G.astype(np.complex128), dv).real
    parts = (float(np.sum(dbls * gb)), np.vdot(gc.astype(np.complex128), D).real, float(np.sum(dF * gf.astype(np.float64))))
    bound = 10 * cfg["eps"] * np.linalg.norm(dv) * np.linalg.norm(G)
    print("basis-position dot", precision, compat, abs(lhs - sum(parts)) / bound, parts)
    assert all(abs(x) > 1e-3 * abs(lhs) for x in parts)  # every part is a share of the sum
    assert abs(lhs - sum(parts)) <= bound, (lhs, parts, bound)


# ---- 3. a joint call is the sum of its parts ---------------------------------------------------------------------------
def test_joint_calls_are_the_sums_of_their_parts(gpu):
    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 8)
    D = random_complex(np.shape(cfg["beam_coefs"]), 5)
    dF = np.random.default_rng(3).normal(size=cfg["fluxes"].shape)
    da = np.random.default_rng(6).normal(size=(7, 3))
    joint = _jvp(cfg, d_ants=da, d_beam_coefs=D, d_fluxes=dF)
    single = [_jvp(cfg, d_ants=da), _jvp(cfg, d_beam_coefs=D), _jvp(cfg, d_fluxes=dF)]
    assert all(np.linalg.norm(x) > 0 for x in single)
    assert rel_l2(joint, single[0] + single[1] + single[2]) <= 1e-14
    db = fftvis_amd.antenna_to_baseline_tangent(da, cfg["ants"], cfg["baselines"])
    assert np.array_equal(single[0], _jvp(cfg, d_baselines=db))
    gb = _gbls(cfg, G)
    gf, gb2, gc, ga = _gbls(cfg, G, wrt=("fluxes", "baselines", "beam_coefs", "ants"))
    assert np.array_equal(gb2, gb) and gb.dtype == np.float64 and gb.shape == (len(cfg["baselines"]), 3)
    assert ga.shape == (7, 3) and np.array_equal(ga, fftvis_amd.baseline_to_antenna_gradient(gb, cfg["ants"], cfg["baselines"]))
    assert np.array_equal(_gbls(cfg, G, wrt="ants"), ga)
    f1, c1 = fftvis_amd.simulate_vis_basis_adjoint(G, **cfg)  # the passes that existed return the bits they returned alone
    assert np.array_equal(f1, gf) and np.array_equal(c1, gc)
    (one,) = _gbls(cfg, G, wrt=("baselines",))
    assert np.array_equal(one, gb)


def test_tensors_in_give_tensors_out(gpu):
    import torch

    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 8)
    dbls = random_dbls(cfg, 2)
    gb, dv = _gbls(cfg, G), _jvp(cfg, d_baselines=dbls)
    tgb, tga = _gbls(cfg, torch.from_numpy(G).cuda(), wrt=("baselines", "ants"))
    assert tgb.device.type == "cuda" and tgb.dtype == torch.float64 and np.array_equal(tgb.cpu().numpy(), gb)
    assert tga.device.type == "cuda" and tuple(tga.shape) == (7, 3)
    tdv = _jvp(cfg, d_baselines=torch.from_numpy(dbls).cuda())
    assert tdv.device.type == "cuda" and tdv.dtype == torch.complex128 and np.array_equal(tdv.cpu().numpy(), dv)
    host = _jvp(cfg, d_baselines=torch.from_numpy(dbls))
    assert isinstance(host, torch.Tensor) and host.device.type == "cpu" and np.array_equal(host.numpy(), dv)


# ---- 4. K = 1 equals the passes without basis beams ---------------------------------------------------------------------
@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
def test_one_unit_basis_beam_equals_the_plain_passes(gpu, heights):
    """One Airy basis beam with every coefficient 1 is the same dish without ``beam_coefs``: both at eps 1e-12, agreement
    to 1e-11 relative (the transforms' tolerance, as at HERA-350's size)."""
    cfg, plain = k1_configs(heights)
    G = random_complex(vis_shape(cfg), 9)
    dbls = random_dbls(cfg, DB_SEED)
    gb = _gbls(cfg, G)
    dv = _jvp(cfg, d_baselines=dbls)
    pg = fftvis_amd.simulate_vis_position_adjoint(G, **plain, wrt="baselines")
    pv = fftvis_amd.simulate_vis_jvp(**plain, d_baselines=dbls)
    print("basis-position K = 1", heights, rel_l2(gb, pg), rel_l2(dv, pv))
    assert np.linalg.norm(pg) > 0 and np.linalg.norm(pv) > 0
    assert rel_l2(gb, pg) <= 1e-11 and rel_l2(dv, pv) <= 1e-11


# ---- 5. slicing edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_source_chunks(gpu, monkeypatch, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    _both_against_references(f"chunks lanes {lanes}", dict(edge_config(nsrc=25, ntimes=4), min_chunks=2))


def test_free_running_lanes(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    monkeypatch.setenv("FFTVIS_HIP_PIPE", "0")
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = dict(edge_config(nsrc=25, ntimes=5), min_chunks=2)
    G, gb, dbls, dv = _both_against_references("free lanes", cfg)
    assert np.array_equal(gb, _gbls(cfg, G)) and np.array_equal(dv, _jvp(cfg, d_baselines=dbls))
    st = _handle().stats()
    gpu_simulate.release_handles()
    assert st["lanes"] == 2 and st["lane_mode"] == 0, st


@pytest.mark.parametrize("block_ch,ratio", [(1, 0.99), (2, 0.99), (2, 0.85)])
def test_channel_blocks_cut_across_frequency_groups(gpu, monkeypatch, block_ch, ratio):
    """nf = 5 in channel blocks of block_ch (FFTVIS_HIP_ADJ_ACC_BYTES: 48 bytes per channel and baseline, whatever K) with
    frequency groups cut by FFTVIS_HIP_GROUP_RATIO; the last block is short."""
    cfg = edge_config(nsrc=18, nfreq=5)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * 48 * len(cfg["baselines"])))
    monkeypatch.setenv("FFTVIS_HIP_GROUP_RATIO", str(ratio))
    _both_against_references(f"blocks {block_ch} ratio {ratio}", cfg)


def test_upsample_125(gpu):
    _both_against_references("sigma 1.25", dict(edge_config(), upsample_factor=1.25), k64=20.0)


def test_empty_time_step(gpu):
    """Nothing above the horizon at the last time: its tangent rows are exactly zero, and the gradient is that of the run
    without that step."""
    cfg = empty_step_basis_config()
    G, gb, _, dv = _both_against_references("empty time step", cfg)
    assert not dv[:, -1].any() and dv[:, 0].any()
    short = dict(cfg, times=cfg["times"][:-1])
    assert np.array_equal(gb, _gbls(short, np.ascontiguousarray(G[:, :-1])))


# ---- 6. an ideal lattice -----------------------------------------------------------------------------------------------
def test_ideal_hex19_with_redundant_runs_and_mirror_pairs(gpu, monkeypatch):
    cfg = hex19_basis_config()
    G, gb, dbls, dv = _both_against_references("ideal hex-19", cfg)
    for env in ("FFTVIS_HIP_NO_TARGET_DEDUP", "FFTVIS_HIP_NO_TARGET_PAIRS"):
        monkeypatch.setenv(env, "1")
        d = rel_l2(_gbls(cfg, G), gb), rel_l2(_jvp(cfg, d_baselines=dbls), dv)
        monkeypatch.delenv(env)
        print("basis-position lattice", env, d)
        assert max(d) <= 1e-12, (env, d)


# ---- 7. HERA-350's size ------------------------------------------------------------------------------------------------
def test_hera350_packed_transforms_and_column_plan(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    cfg = hera350_basis_config()
    sub = hera_subset(cfg)
    G = random_complex(vis_shape(cfg), G_SEED)
    dbls = random_dbls(cfg, DB_SEED)
    gpu_simulate.release_handles()
    gb = _gbls(cfg, G)
    dv = _jvp(cfg, d_baselines=dbls)
    _assert_grad("hera350", cfg, gb[sub], exact_gbls(cfg, G, sub=sub), cfg["eps"])
    _assert_tan("hera350", cfg, dv[..., sub], *exact_dv_baselines(cfg, dbls[sub], sub=sub), cfg["eps"])
    for env in ("FFTVIS_HIP_NO_HERMITIAN", "FFTVIS_HIP_NO_COLUMN_PLAN"):
        monkeypatch.setenv(env, "1")
        d = rel_l2(_gbls(cfg, G), gb), rel_l2(_jvp(cfg, d_baselines=dbls), dv)
        monkeypatch.delenv(env)
        print("basis-position hera350", env, d)
        assert 0 < min(d) and max(d) <= 1e-11, (env, d)
    gpu_simulate.release_handles()


# ---- 8. the raw C ABI --------------------------------------------------------------------------------------------------
def test_raw_c_abi(gpu):
    """Both entry points through a bare ctypes handle configured by the engine's own setters: device and host pointers,
    accumulate 0 and 1, channel and time sub-blocks that add up to the whole, values that are not finite refused with the
    handle left usable, and a handle without basis beams and a lattice handle refused."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs
    from tests.position_adjoint_refs import hex_positions

    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 7)
    dbls = random_dbls(cfg, 3)
    gb, dv = _gbls(cfg, G), _jvp(cfg, d_baselines=dbls)
    nf, nt, nbls = len(cfg["freqs"]), len(cfg["times"]), len(cfg["baselines"])
    L = _lib.lib()
    adj, tan = L.fv_sim_run_basis_position_adjoint, L.fv_sim_run_basis_position_tangent
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        dG = torch.from_numpy(G).cuda()
        dB = torch.full((nbls, 3), 7.0, dtype=torch.float64, device="cuda")
        dD = torch.from_numpy(dbls).cuda()
        dV = torch.full(dv.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        assert adj(h._h, 0, nt, 0, nf, p(dG), 1, p(dB), 1, 0) == 0, L.fv_last_error()
        assert np.array_equal(dB.cpu().numpy(), gb)  # accumulate = 0 zeroes first
        assert adj(h._h, 0, nt, 0, nf, p(dG), 1, p(dB), 1, 1) == 0, L.fv_last_error()
        assert rel_l2(dB.cpu().numpy(), 2 * gb) < 1e-14
        hB = np.ascontiguousarray(gb.copy())  # a host gbls with accumulate = 1
        assert adj(h._h, 0, nt, 0, nf, hp(G), 0, hp(hB), 0, 1) == 0, L.fv_last_error()
        assert rel_l2(hB, 2 * gb) < 1e-14
        assert tan(h._h, 0, nt, 0, nf, p(dD), 1, p(dV), 1) == 0, L.fv_last_error()
        assert np.array_equal(dV.cpu().numpy(), dv)  # always overwritten
        hV = np.full(dv.shape, 7.0, dtype=np.complex128)
        assert tan(h._h, 0, nt, 0, nf, hp(dbls), 0, hp(hV), 0) == 0, L.fv_last_error()
        assert np.array_equal(hV, dv)
        # channel blocks and time blocks add up to the whole
        for blocks in ([(0, nt, 0, 1), (0, nt, 1, nf)], [(0, 1, 0, nf), (1, nt, 0, nf)]):
            total = np.zeros((nbls, 3))
            for t0, t1, f0, f1 in blocks:
                blk = dG[f0:f1, t0:t1].contiguous()
                out = torch.full((f1 - f0, t1 - t0) + dv.shape[2:], 7.0, dtype=torch.complex128, device="cuda")
                torch.cuda.synchronize()
                assert adj(h._h, t0, t1, f0, f1, p(blk), 1, p(dB), 1, 0) == 0, L.fv_last_error()
                part = dB.cpu().numpy()
                assert np.linalg.norm(part) > 0
                total += part
                assert tan(h._h, t0, t1, f0, f1, p(dD), 1, p(out), 1) == 0, L.fv_last_error()
                assert rel_l2(out.cpu().numpy(), dv[f0:f1, t0:t1]) <= 10 * cfg["eps"]
            assert rel_l2(total, gb) <= 10 * cfg["eps"]
        # NaN in G and inf in dbls fail before anything runs; the next call returns the good result's bits
        bad = G.copy()
        bad[1, 0, 1, 0, 3] = np.nan
        assert adj(h._h, 0, nt, 0, nf, hp(bad), 0, hp(hB), 0, 0) == 1
        assert b"NaN" in L.fv_last_error()
        assert adj(h._h, 0, nt, 0, nf, hp(G), 0, hp(hB), 0, 0) == 0, L.fv_last_error()
        assert np.array_equal(hB, gb)
        for device in (0, 1):
            B = dbls.copy()
            B[4, 1] = np.inf
            dBad = torch.from_numpy(B).cuda()
            torch.cuda.synchronize()
            assert (tan(h._h, 0, nt, 0, nf, p(dBad), 1, hp(hV), 0) if device else
                    tan(h._h, 0, nt, 0, nf, hp(B), 0, hp(hV), 0)) == 1
            assert b"not finite" in L.fv_last_error()
            hV[...] = 7.0
            assert tan(h._h, 0, nt, 0, nf, hp(dbls), 0, hp(hV), 0) == 0, L.fv_last_error()
            assert np.array_equal(hV, dv)
    finally:
        gs._return_handle(key, h)
    buf = torch.zeros(1 << 16, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    plain = dict(synth.make_config("C1", nsrc=20, nfreq=3, ntimes=2), polarized=True)
    xy = 14.6 * hex_positions(1)
    lat = dict(plain, ants={i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(7)}, force_use_type3=False)
    for run_cfg, words in ((plain, (b"fv_sim_set_basis", b"fv_sim_run_position_adjoint", b"fv_sim_run_tangent")),
                           (lat, (b"lattice", b"lattice", b"lattice"))):
        gs.release_handles()
        fftvis_amd.simulate_vis(**run_cfg)
        key, h = gs._acquire_handle(0, 2, run_cfg["eps"], 2, True)
        try:
            assert adj(h._h, 0, 1, 0, 1, p(buf), 1, p(buf), 1, 0) == 1
            assert words[0] in L.fv_last_error() and words[1] in L.fv_last_error(), L.fv_last_error()
            assert tan(h._h, 0, 1, 0, 1, p(buf), 1, p(buf), 1) == 1
            assert words[0] in L.fv_last_error() and words[2] in L.fv_last_error(), L.fv_last_error()
        finally:
            gs._return_handle(key, h)


def test_values_that_are_not_finite_fail_through_python(gpu):
    cfg = edge_config()
    G = random_complex(vis_shape(cfg), 7)
    dbls = random_dbls(cfg, 3)
    gb, dv = _gbls(cfg, G), _jvp(cfg, d_baselines=dbls)
    bad = G.copy()
    bad[1, 0, 1, 0, 3] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="NaN"):
        _gbls(cfg, bad)
    B = dbls.copy()
    B[2, 0] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="finite"):
        _jvp(cfg, d_baselines=B)
    assert np.array_equal(_gbls(cfg, G), gb) and np.array_equal(_jvp(cfg, d_baselines=dbls), dv)


# ---- 9. reproducibility and hygiene ------------------------------------------------------------------------------------
def test_reproducible_for_a_lane_count(gpu, monkeypatch):
    cfg = edge_config(nsrc=40, ntimes=4)
    G = random_complex(vis_shape(cfg), 10)
    dbls = random_dbls(cfg, 4)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a, b = _gbls(cfg, G), _gbls(cfg, G)
        c, d = _jvp(cfg, d_baselines=dbls), _jvp(cfg, d_baselines=dbls)
        assert np.array_equal(a, b) and np.array_equal(c, d), lanes
        res[lanes] = (a, c)
    assert rel_l2(res["1"][0], res["2"][0]) <= 1e-12 and rel_l2(res["1"][1], res["2"][1]) <= 1e-12


@pytest.mark.parametrize("heights", ["flat", "cm"])
def test_a_forward_call_after_each_pass_returns_the_same_bits(gpu, heights):
    cfg = basis_position_config(heights, "complex", "full", False)
    before = fftvis_amd.simulate_vis(**cfg)
    _gbls(cfg, random_complex(vis_shape(cfg), 3))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)
    _jvp(cfg, d_baselines=random_dbls(cfg, 3))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)


def test_bulk_device_memory_is_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after either pass no more than it held after the
    forward: no S buffer, staged array or tripled strength buffer stays."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = edge_config()
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _gbls(cfg, random_complex(vis_shape(cfg), 1))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)
    _jvp(cfg, d_baselines=random_dbls(cfg, 1))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


# ---- 10. torch ---------------------------------------------------------------------------------------------------------
def _torch_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k not in ("fluxes", "ants", "beam_coefs")}


def test_torch_gradcheck_all_three_inputs(gpu):
    """fp64, tiny: 4 antennas, 3 sources, 2 channels, 1 time, K = 2, eps 1e-12, step 1e-3 (metres for the positions): the
    central difference's truncation in the positions is (k h)^2 / 6 with k = 2 pi nu / c <= 3.6 / m, about 2e-6 relative,
    against rtol 1e-4; reverse and forward mode."""
    import torch

    cfg = basis_position_config("cm", "complex", "full", False, nsrc=3, nfreq=2, ntimes=1)
    cfg.update(eps=1e-12, beam=cfg["beam"][:2], beam_coefs=cfg["beam_coefs"][:4, :2],
               ants={k: cfg["ants"][k] for k in range(4)}, baselines=[(0, 1), (2, 3), (3, 0), (1, 1)])
    kw = _torch_kwargs(cfg)
    rng = np.random.default_rng(8)
    F = torch.tensor(rng.uniform(0.5, 1.5, (3, 2, 4)), dtype=torch.float64, device="cuda", requires_grad=True)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True)
    P = torch.tensor(np.array(list(cfg["ants"].values())), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, c, p: fftvis_amd.torch_simulate_vis_basis_array(f, c, p, **kw), (F, C, P),
                                    eps=1e-3, atol=1e-7, rtol=1e-4, check_forward_ad=True)
    out = fftvis_amd.torch_simulate_vis_basis_array(F, C, P, **kw)
    assert out.device == F.device and out.is_complex() and tuple(out.shape) == vis_shape(cfg)


def test_torch_backward_equals_the_direct_calls_and_runs_only_what_is_needed(gpu, monkeypatch):
    """d/d(F, C, P) sum |V - Dat|^2 through torch equals the direct calls on G = 2 (V - Dat); with only ``antpos`` requiring
    a gradient the backward is one ``simulate_vis_basis_adjoint`` call with wrt = ("ants",), and the handle's statistics
    show the position pass's launches and no others; ``antnums`` names the rows."""
    import torch

    import fftvis_amd.adjoint as adj
    from fftvis_amd.gpu import gpu_simulate

    cfg = edge_config()
    keys = [10 * (i + 1) for i in range(7)]
    ants = {k: v for k, v in zip(keys, cfg["ants"].values())}
    bls = [(keys[i], keys[j]) for i, j in cfg["baselines"]]
    kw = dict(_torch_kwargs(cfg), baselines=bls)
    Dat = random_complex(vis_shape(cfg), 15)
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda", requires_grad=True)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True)
    P = torch.tensor(np.array(list(ants.values())), dtype=torch.float64, device="cuda", requires_grad=True)
    V = fftvis_amd.torch_simulate_vis_basis_array(F, C, P, antnums=keys, **kw)
    (V - torch.from_numpy(Dat).cuda()).abs().pow(2).sum().backward()
    G = 2 * (V.detach().cpu().numpy() - Dat)
    direct = dict(cfg, ants=ants, baselines=bls)
    gf, gc, gp = _gbls(direct, G, wrt=("fluxes", "beam_coefs", "ants"))
    for got, want in ((F.grad, gf), (C.grad, gc), (P.grad, gp)):
        assert np.allclose(got.cpu().numpy(), want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    calls = []
    real = adj.simulate_vis_basis_adjoint
    monkeypatch.setattr(adj, "simulate_vis_basis_adjoint", lambda *a, **k: calls.append(tuple(k["wrt"])) or real(*a, **k))
    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    P2 = P.detach().clone().requires_grad_(True)
    V2 = fftvis_amd.torch_simulate_vis_basis_array(F.detach(), C.detach(), P2, antnums=keys, **kw)
    forward = _handle().stats()["spread_launches"]
    _handle().reset_stats()
    V2.abs().pow(2).sum().backward()
    st = _handle().stats()
    _handle().reset_stats()
    real(G, **direct, wrt=("beam_coefs", "ants"))
    joint = _handle().stats()["spread_launches"]
    gpu_simulate.release_handles()
    assert calls == [("ants",)] and P2.grad is not None
    # the position pass alone: three rounds per launch of the forward; the coefficient pass would add the forward's own
    assert forward > 0 and st["spread_launches"] == 3 * forward and joint == 4 * forward, (forward, st, joint)
    F3 = F.detach().clone().requires_grad_(True)
    C3 = C.detach().clone().requires_grad_(True)
    fftvis_amd.torch_simulate_vis_basis_array(F3, C3, P.detach(), antnums=keys, **kw).abs().pow(2).sum().backward()
    assert calls == [("ants",), ("fluxes", "beam_coefs")] and F3.grad is not None and C3.grad is not None
    with pytest.raises(TypeError, match="antpos"):
        fftvis_amd.torch_simulate_vis_basis_array(F, C, P, ants=ants, **kw)


def test_forward_ad_equals_the_direct_calls(gpu):
    import torch
    import torch.autograd.forward_ad as fwAD

    cfg = edge_config()
    kw = _torch_kwargs(cfg)
    da = np.random.default_rng(6).normal(size=(7, 3))
    D = random_complex(np.shape(cfg["beam_coefs"]), 5)
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda")
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda")
    P = torch.tensor(np.array(list(cfg["ants"].values())), dtype=torch.float64, device="cuda")
    tC = torch.tensor(D, dtype=torch.complex128, device="cuda")
    tP = torch.tensor(da, dtype=torch.float64, device="cuda")
    with fwAD.dual_level():
        for c, pp, want in ((C, fwAD.make_dual(P, tP), _jvp(cfg, d_ants=da)),
                            (fwAD.make_dual(C, tC), fwAD.make_dual(P, tP), _jvp(cfg, d_ants=da, d_beam_coefs=D))):
            tangent = fwAD.unpack_dual(fftvis_amd.torch_simulate_vis_basis_array(F, c, pp, **kw)).tangent
            assert tangent is not None and tangent.device == F.device
            assert rel_l2(tangent.cpu().numpy(), want) <= 1e-12
