"""GPU tests of the forward-mode tangent (``simulate_vis_jvp``, ``fv_sim_run_tangent``, the ``jvp`` of the torch
operations).

The tangent dV, an array of ``simulate_vis``'s shape, is compared element by element with the exact references built from
the oracle's forward (``tangent_refs.exact_dv_baselines``, closed form; ``tangent_refs.exact_dv_topo``, Richardson
differences with all sources moved at once; both pinned in ``test_tangent_host``): over a configuration matrix, on an
ideal lattice with redundant runs, at HERA-350's size with the packed transforms and the column plan, at the edges of the
device's slicing, through the Python surface and the bare C ABI, against the two position adjoints through
Re <J v, G> = <v, J^T G>, and through torch's forward-mode AD.  The direction tangent through a table beam is compared
at every spline order, 0 .. 5, on configurations that keep every source away from the table's knot lines
(``source_adjoint_refs.knot_margin``, asserted in ``test_tangent_host``), at the table's edges one source at a time, and
at order 0 -- where the beam term is 0 by definition -- with sources within the device's stencil of a jump against the
closed form that holds the beam fixed (``frozen_beam_dv_topo``).

Tolerances, as multiples of base: base = eps in fp64; in fp32 base = max(the forward's own rel l2 error against the oracle
on the same configuration, eps) (``_forward_base``).  Every term of dV is one forward transform, which the project holds
to 10 base in rel l2 (20 at upsample_factor = 1.25), so the whole is held to 10 base kappa, kappa = sum ||term|| / ||dV||
taken from the REFERENCE's terms (three for the baselines; three phase terms and the beam part for the directions;
``test_tangent_host`` asserts kappa <= 4 for every configuration here: measured 1.06 .. 1.68).  The bounds on the worst
channel, time step and product slot (a part below 1e-3 of the whole is measured against that floor), on max |err| / max
|exact| and every fp32 factor are ``test_gpu_position_adjoint``'s constants, scaled by kappa, and are kept where they hold at least twice the worst ratio
measured on an MI355X over this module's comparisons (FFTVIS_TEST_METRICS=<file> logs each comparison's ratios, one JSON
line each).  Measured over the 243 comparisons, as ratio / (base kappa):
  fp64 (base 6e-8; 1e-12 at HERA-350's size): whole <= 0.57, a part <= 0.60, max |err| / max |exact| <= 1.81 -- all three
  at HERA-350's size, all-real packing, at eps 1e-12; every comparison at eps 6e-8 is at or below 0.37, 0.46, 0.51 (channel
  blocks of one, the directions), the matrix at or below 0.10, 0.20, 0.13 (baselines) and 0.15, 0.45, 0.27 (directions), the
  ideal hex-19 at 0.06, 0.23, 0.06, upsample_factor = 1.25 at 0.15, 2.35, 0.26 (bounds 20, 20, 12 there).
  fp32 over the 108 matrix comparisons (base 1e-5: the forward's own error stayed below eps everywhere): whole <= 0.63,
  a part <= 1.64, max |err| <= 1.06, all on the flat array with the complex table, the directions.
  Table beams beyond order 3's matrix, the directions, 38 comparisons: the cell at orders 0, 1, 2, 4, 5 and unpolarized at
  order 1, fp64 whole <= 0.25, a part <= 0.43, max |err| <= 0.44, fp32 0.26, 0.35, 0.23 (order 0); the table edges, all
  sources and one at a time, 0.34, 0.53, 0.69 (the sources either side of az = 0 on the full-sky table); order 0 on a
  jump 0.25, 0.55, 0.43 -- on the parent commit 5.3e9 (rel l2 453): the difference across the jump, gone since the beam
  term of order-0 tables is 0.
  Every constant keeps more than twice its measured worst (the closest: fp64 max |err|, 6 against 1.81): none moved.
The dot identity between the tangent and the two adjoint passes came out at or below 1e-3 of its bound (the order-1 and
order-0 tables: 3e-4).
"""

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
from tests.tangent_refs import (DB_SEED, DT_SEED, ORDERS, edge_config, edge_table_config, empty_step_config,
                                exact_dv_baselines, exact_dv_topo, frozen_beam_dv_topo, hera_subset, hex19_config,
                                jump_config, kappa, knot_margin, margins, order_config, random_complex, random_dbls,
                                random_dtopo, source_config, vis_shape)
from tests.test_gpu_basis_adjoint import _forward_base
from tests.test_gpu_position_adjoint import C_MAX, C_MAX32, HERA_EPS, K32, K32_PART, K64_PART, _hera350

pytestmark = pytest.mark.gpu


def _errors(got, exact):
    got = np.asarray(got).astype(np.complex128)
    err = got - exact
    floor = 1e-3 * np.linalg.norm(exact)
    parts = {"channel": 0, "time": 1}
    if exact.ndim == 5:
        parts.update(feed1=2, feed2=3)
    m = {"rel_l2": floored_rel(err, exact, floor),
         "max_abs": float(np.abs(err).max() / max(np.abs(exact).max(), 1e-300))}
    m["part"] = max(worst_part(err, exact, ax, floor) for ax in parts.values())
    return m


def _log(label, cfg, m, base, kap):
    rec = {"label": label, "precision": cfg.get("precision", 2), "base": base, "kappa": kap,
           **{k: v / (base * kap) for k, v in m.items()}}
    print("tangent metrics", json.dumps(rec))
    path = os.environ.get("FFTVIS_TEST_METRICS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _assert_close(label, cfg, got, exact, terms, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert got.shape == exact.shape and np.isfinite(np.asarray(got)).all()
    kap = kappa(exact, terms)
    assert kap <= 4.0, (label, kap)
    m = _errors(got, exact)
    _log(label, cfg, m, base, kap)
    fp64 = cfg.get("precision", 2) == 2
    whole, part = (k64, K64_PART * k64 / 10.0) if fp64 else (K32, K32_PART)
    assert m["rel_l2"] <= whole * base * kap, (label, m, base, kap)
    assert m["part"] <= part * base * kap, (label, m, base, kap)
    assert m["max_abs"] <= (C_MAX * k64 / 10.0 if fp64 else C_MAX32) * base * kap, (label, m, base, kap)
    return m


def _jvp(cfg, **kw):
    return fftvis_amd.simulate_vis_jvp(**cfg, **kw)


def _handle():
    from fftvis_amd.gpu import gpu_simulate

    (h,) = gpu_simulate._IDLE_HANDLES.values()
    return h


def _unit_vectors(cfg):
    m = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    return np.stack([orc._topo_of(m, ti).T for ti in range(len(cfg["times"]))])


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix_reference(heights, sky, beams, compat):
    """The exact tangents of a matrix cell (they do not depend on the run's precision)."""
    cfg = source_config(heights, sky, beams, compat)
    db, dt = random_dbls(cfg, DB_SEED), random_dtopo(cfg, DT_SEED)
    return db, dt, exact_dv_baselines(cfg, db), exact_dv_topo(cfg, dt)


@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("beams", ["airy", "two", "complex"])
@pytest.mark.parametrize("sky", ["unpol", "I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_tangent_matrix(gpu, precision, sky, beams, compat, heights):
    cfg = source_config(heights, sky, beams, compat, precision)
    db, dt, (eb, tb), (et, phase, tt) = _matrix_reference(heights, sky, beams, compat)
    base = _forward_base(cfg)
    label = f"{precision} {sky} {beams} {compat} {heights}"
    gb = _jvp(cfg, d_baselines=db)
    assert gb.shape == vis_shape(cfg) and gb.dtype == (np.complex64 if precision == 1 else np.complex128)
    _assert_close("matrix baselines " + label, cfg, gb, eb, tb, base)
    gt = _jvp(cfg, d_topo=dt)
    _assert_close("matrix directions " + label, cfg, gt, et, tt, base)
    if beams != "airy" or heights == "flat":  # (beam-sensitive cells: the beam part is a visible share of the whole)
        assert np.linalg.norm(et - phase) > 1e-3 * np.linalg.norm(et)
    if heights == "flat":  # the up component of dbls changes dV although the forward drops the heights
        assert np.linalg.norm(tb[2]) > 1e-3 * np.linalg.norm(eb)
        flat = db.copy()
        flat[:, 2] = 0.0
        assert rel_l2(_jvp(cfg, d_baselines=flat), gb) > 1e-3


# ---- 1b. table beams at every spline order, the table's edges, order 0 on a jump -------------------------------------
@functools.lru_cache(maxsize=None)
def _order_reference(order, sky):
    """The exact direction tangent of ``order_config(order, sky)`` (it does not depend on the run's precision)."""
    cfg = order_config(order, sky)
    dt = random_dtopo(cfg, DT_SEED)
    return dt, exact_dv_topo(cfg, dt)


@pytest.mark.parametrize("order,sky", [(o, "full") for o in ORDERS] + [(1, "unpol")])
@pytest.mark.parametrize("precision", [2, 1])
def test_direction_tangent_table_orders(gpu, precision, order, sky):
    """The cell "cm heights, full Stokes, exact flips, complex table" at the orders the matrix does not run: 1 (bilinear,
    the default, unrolled) and 0, 2, 4, 5 (the run-time path); unpolarized at order 1, the power table's bilinear branch."""
    cfg = order_config(order, sky, precision)
    dt, (et, phase, tt) = _order_reference(order, sky)
    gt = _jvp(cfg, d_topo=dt)
    assert gt.shape == vis_shape(cfg) and gt.dtype == (np.complex64 if precision == 1 else np.complex128)
    _assert_close(f"table order {order} {sky} {precision}", cfg, gt, et, tt, _forward_base(cfg))
    if order > 0:  # the beam part is a visible share of the whole
        assert np.linalg.norm(et - phase) > 1e-3 * np.linalg.norm(et)


def _one_row(dt, t, j):
    out = np.zeros_like(dt)
    out[t, j] = dt[t, j]
    return out


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("kind", ["fullsky", "horizon"])
def test_table_edges_source_by_source(gpu, kind, order):
    """Sources placed by hand at the edges of a table (``edge_table_config``: the azimuth wrap from both sides and, at
    order 3, across it, the first za cell at za = 1e-2 and 3e-3, the last cell above the horizon; a table that ends at
    the horizon), one time step, their vectors through a coordinate manager: all moved at once, and -- each source is one
    edge -- one at a time (kappa 1.2 .. 1.7 for each)."""
    cfg, mgr = edge_table_config(kind, order)
    assert margins(cfg, coord_mgr=mgr)[0] > 1e-3 and (order == 3 or knot_margin(cfg, order, coord_mgr=mgr) > 1e-4)
    dt = random_dtopo(cfg, DT_SEED)
    for label, d in [("all", dt)] + [(f"source {j}", _one_row(dt, 0, j)) for j in range(dt.shape[1])]:
        et, _, tt = exact_dv_topo(cfg, d, coord_mgr=mgr)
        _assert_close(f"table edges {kind} order {order}, {label}", cfg, _jvp(cfg, d_topo=d, coord_mgr=mgr), et, tt, cfg["eps"])


def test_order_0_with_sources_on_a_jump(gpu):
    """Order 0 is piecewise constant: the beam term is 0 by definition, also for a source whose difference stencil
    (1e-6 rad) straddles a jump of the table -- one 3e-7 rad from a za half-node line, one 3e-7 rad from an az half-node
    line, the others of ``order_config(0)`` where they were.  Reference: the closed form with the beam held fixed; all
    sources moved at once, and the two on a jump one at a time."""
    cfg, mgr, rows = jump_config()
    assert knot_margin(cfg, 0, coord_mgr=mgr) < 1e-6 and margins(cfg, coord_mgr=mgr)[0] > 1e-3
    dt = random_dtopo(cfg, DT_SEED)
    for label, d in [("all", dt)] + [(f"source {j}", _one_row(dt, 0, j)) for j in rows]:
        et, tt = frozen_beam_dv_topo(cfg, d, coord_mgr=mgr)
        _assert_close(f"order 0 on a jump, {label}", cfg, _jvp(cfg, d_topo=d, coord_mgr=mgr), et, tt, cfg["eps"])


@pytest.mark.parametrize("heights,terms", [("flat", False), ("m", False), ("cm", True)])
def test_matrix_arrays_take_the_paths_they_are_named_for(gpu, monkeypatch, heights, terms):
    """The pass is a forward run: on the matrix's three arrays it runs 2-D transforms, the 3-D transform, and 2-D
    transforms with height terms (the gather's WT variants)."""
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    cfg = source_config(heights, "full", "two", False)
    _jvp(cfg, d_baselines=random_dbls(cfg, 1), d_topo=random_dtopo(cfg, 2))
    st = _handle().stats()
    gpu_simulate.release_handles()
    if terms:
        assert 2 <= st["height_terms"] <= 16 and st["n2_3"] == 1, st
    else:
        assert st["height_terms"] == 0 and (st["n2_3"] > 1) == (heights == "m"), st


def test_a_joint_call_is_the_sum_of_the_separate_calls(gpu):
    cfg = dict(edge_config(), coord_method="SiderealRotation")
    rng = np.random.default_rng(3)
    da, dr = rng.normal(size=(7, 3)), 1e-3 * rng.normal(size=(24, 2))
    df = rng.normal(size=np.shape(cfg["fluxes"]))
    parts = _jvp(cfg, d_ants=da).astype(complex) + _jvp(cfg, d_radec=dr) + _jvp(cfg, d_fluxes=df)
    joint = _jvp(cfg, d_ants=da, d_radec=dr, d_fluxes=df)
    assert rel_l2(joint, parts) <= 1e-12
    assert np.array_equal(_jvp(cfg, d_fluxes=df), fftvis_amd.simulate_vis(**dict(cfg, fluxes=df)))
    db = fftvis_amd.antenna_to_baseline_tangent(da, cfg["ants"], cfg["baselines"])
    assert np.array_equal(_jvp(cfg, d_ants=da), _jvp(cfg, d_baselines=db))
    J = fftvis_amd.radec_jacobian(cfg["ra"], cfg["dec"], cfg["times"], cfg["telescope_loc"])
    assert np.array_equal(_jvp(cfg, d_radec=dr), _jvp(cfg, d_topo=np.einsum("tjdc,jc->tjd", J, dr)))
    z = _jvp(cfg)
    assert z.shape == vis_shape(cfg) and not z.any()


# ---- 2. an ideal lattice ---------------------------------------------------------------------------------------------
def test_ideal_lattice_takes_type3_with_redundant_runs(gpu, monkeypatch):
    """An exact hex-19, all baselines in the caller's order: the pass takes the type-3 transform with the redundant runs;
    dbls is random per baseline, so the members of one run carry different weights and mirrored runs both gather."""
    from fftvis_amd.core.antenna_gridding import check_antpos_griddability
    from fftvis_amd.gpu import gpu_simulate

    cfg = hex19_config()
    assert check_antpos_griddability(cfg["ants"])[0] and margins(cfg)[0] > 1e-3
    db, dt = random_dbls(cfg, DB_SEED), random_dtopo(cfg, DT_SEED)
    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    gb = _jvp(cfg, d_baselines=db)
    st = _handle().stats()
    assert st["lanes"] >= 1 and st["spread_launches"] > 0, st  # the type-3 stages ran (the lattice path sets no lanes)
    items_once = st["interp_items"]
    gt = _jvp(cfg, d_topo=dt)
    eb, tb = exact_dv_baselines(cfg, db)
    et, _, tt = exact_dv_topo(cfg, dt)
    _assert_close("ideal hex-19 baselines", cfg, gb, eb, tb, cfg["eps"])
    _assert_close("ideal hex-19 directions", cfg, gt, et, tt, cfg["eps"])
    for env in ("FFTVIS_HIP_NO_TARGET_DEDUP", "FFTVIS_HIP_NO_TARGET_PAIRS"):
        _handle().reset_stats()
        monkeypatch.setenv(env, "1")
        ob = _jvp(cfg, d_baselines=db)
        items = _handle().stats()["interp_items"]
        ot = _jvp(cfg, d_topo=dt)
        monkeypatch.delenv(env)
        d = max(rel_l2(ob, gb), rel_l2(ot, gt))
        print("tangent lattice", env, d)
        assert d <= 1e-12, (env, d)
        if env.endswith("DEDUP"):
            assert items_once < 0.5 * items  # most of the 192 vectors repeat
    gpu_simulate.release_handles()


# ---- 3. packings and plans at HERA-350's size ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hermitian", "all_real"])
def test_hera350_packings_and_column_plan(gpu, monkeypatch, kind):
    from fftvis_amd.gpu import gpu_simulate

    cfg = _hera350(kind)
    db = random_dbls(cfg, DB_SEED)
    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    got = _jvp(cfg, d_baselines=db)
    st = _handle().stats()
    sub = hera_subset(cfg)
    eb, tb = exact_dv_baselines(cfg, db[sub], sub=sub)
    _assert_close(f"hera350 {kind}", cfg, got[..., sub], eb, tb, HERA_EPS)
    for env in ("FFTVIS_HIP_NO_HERMITIAN", "FFTVIS_HIP_NO_COLUMN_PLAN"):
        _handle().reset_stats()
        monkeypatch.setenv(env, "1")
        other = _jvp(cfg, d_baselines=db)
        st2 = _handle().stats()
        monkeypatch.delenv(env)
        d = rel_l2(other, got)
        print("tangent hera350", kind, env, d)
        assert 0 < d <= 1e-11, (kind, env, d)
        if env.endswith("HERMITIAN"):  # the packed run spreads half the transforms
            assert st["spread_cells"] < 0.8 * st2["spread_cells"], (st, st2)
        else:                          # the planned run moves fewer cells through the FFT passes
            assert st["fft_cells"] < st2["fft_cells"], (st, st2)
    gpu_simulate.release_handles()


# ---- 4. slicing edges ------------------------------------------------------------------------------------------------
def _check_edge(label, cfg, k64=10.0, coord_mgr=None, ref_mgr=None, **kw):
    db, dt = random_dbls(cfg, DB_SEED), random_dtopo(cfg, DT_SEED)
    extra = {} if coord_mgr is None else {"coord_mgr": coord_mgr}
    gb = _jvp(cfg, d_baselines=db, **extra, **kw)
    gt = _jvp(cfg, d_topo=dt, **extra, **kw)
    eb, tb = exact_dv_baselines(cfg, db, coord_mgr=ref_mgr)
    et, _, tt = exact_dv_topo(cfg, dt, coord_mgr=ref_mgr)
    _assert_close(label + ", baselines", cfg, gb, eb, tb, cfg["eps"], k64)
    _assert_close(label + ", directions", cfg, gt, et, tt, cfg["eps"], k64)
    both = _jvp(cfg, d_baselines=db, d_topo=dt, **extra, **kw)
    assert rel_l2(both, gb + gt) <= 1e-12
    return db, dt, gb, gt


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_source_chunks_add(gpu, monkeypatch, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    _check_edge(f"chunks lanes {lanes}", dict(edge_config(nsrc=25, ntimes=4), min_chunks=2))


def test_free_running_lanes(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    monkeypatch.setenv("FFTVIS_HIP_PIPE", "0")
    monkeypatch.setenv("FFTVIS_HIP_LANES", "2")
    cfg = dict(edge_config(nsrc=25, ntimes=5), min_chunks=2)
    db, dt, gb, gt = _check_edge("free lanes", cfg)
    assert np.array_equal(gb, _jvp(cfg, d_baselines=db)) and np.array_equal(gt, _jvp(cfg, d_topo=dt))
    st = _handle().stats()
    gpu_simulate.release_handles()
    assert st["lanes"] == 2 and st["lane_mode"] == 0, st


@pytest.mark.parametrize("block_ch,ratio", [(1, 0.99), (2, 0.99), (2, 0.85), (2, 0.5)])
def test_channel_blocks_cut_across_frequency_groups(gpu, monkeypatch, block_ch, ratio):
    """nf = 5 in channel blocks of block_ch (FFTVIS_HIP_ADJ_ACC_BYTES: 48 bytes per channel and baseline) with frequency
    groups cut by FFTVIS_HIP_GROUP_RATIO; the last block is short."""
    cfg = edge_config(nsrc=18, nfreq=5)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * 48 * len(cfg["baselines"])))
    monkeypatch.setenv("FFTVIS_HIP_GROUP_RATIO", str(ratio))
    _check_edge(f"blocks {block_ch} ratio {ratio}", cfg)


def test_upsample_125(gpu):
    _check_edge("sigma 1.25", dict(edge_config(), upsample_factor=1.25), k64=20.0)


def test_empty_time_step_is_exactly_zero(gpu):
    from tests.test_gpu_adjoint import _up

    cfg = empty_step_config()
    up = _up(cfg)
    assert np.any(up[0] > 0) and not np.any(up[-1] > 0)
    _, _, gb, gt = _check_edge("empty time step", cfg)
    assert not gb[:, -1].any() and not gt[:, -1].any() and gb[:, 0].any() and gt[:, 0].any()


def test_rows_below_the_horizon_change_no_bit(gpu):
    cfg = edge_config()
    below = _unit_vectors(cfg)[..., 2] <= 0
    assert below.any() and not below.all()
    dt = random_dtopo(cfg, DT_SEED)
    other = dt.copy()
    other[below] = 1e6 * np.random.default_rng(4).normal(size=(int(below.sum()), 3))
    assert np.array_equal(_jvp(cfg, d_topo=dt), _jvp(cfg, d_topo=other))
    radial = dt + 2.5 * _unit_vectors(cfg)  # and the radial part is projected away
    assert rel_l2(_jvp(cfg, d_topo=radial), _jvp(cfg, d_topo=dt)) <= 1e-12


def test_coord_mgr_in_time_blocks_and_device_astrometry(gpu, monkeypatch):
    """Per-time astrometry contexts: applied on the host and streamed one time step per block (``coord_mgr=``; every
    block takes its row of d_topo), and applied on the device (``astrom=``), d_topo and d_radec."""
    from fftvis_amd.gpu import gpu_simulate
    from oracle import astrometry as oa

    cfg = edge_config(ntimes=3)
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
    real = gpu_simulate.SimHandle.run_tangent
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_tangent",
                        lambda self, *a: calls.append((a[0], a[1], None if a[5] is None else tuple(a[5].shape))) or real(self, *a))
    monkeypatch.setattr(gpu_simulate, "_time_block", lambda *a, **k: 1)
    db, dt, gb, gt = _check_edge("coord_mgr, time blocks", kw, coord_mgr=Mgr(), ref_mgr=Mgr())
    assert calls[:3] == [(0, 1, None)] * 3 and calls[3:6] == [(0, 1, (1, 24, 3))] * 3, calls
    monkeypatch.undo()
    with pytest.raises(ValueError, match="d_topo"):
        _jvp(kw, d_radec=np.zeros((24, 2)), coord_mgr=Mgr())
    et, _, tt = exact_dv_topo(cfg, dt, coord_mgr=Mgr())
    dev = _jvp(kw, d_topo=dt, astrom=ctxs, device_astrometry=True)
    _assert_close("device astrometry, d_topo", cfg, dev, et, tt, cfg["eps"])
    assert rel_l2(gt, _jvp(cfg, d_topo=dt)) > 1e-3  # and it is not the sidereal answer
    h = 1e-5  # central differences of the oracle's chain: h^2 / 6 = 2e-11, rounding 1e-16 / h = 1e-11
    J = np.empty((3, 24, 3, 2))
    for t in range(3):
        for c, (da, dd) in enumerate(((h, 0.0), (0.0, h))):
            p = oa.icrs_to_enu(orc.eq_unit_vectors(cfg["ra"] + da, cfg["dec"] + dd), ctxs[t])
            m = oa.icrs_to_enu(orc.eq_unit_vectors(cfg["ra"] - da, cfg["dec"] - dd), ctxs[t])
            J[t, :, :, c] = ((p - m) / (2 * h)).T
    dr = np.random.default_rng(5).normal(size=(24, 2))
    er, _, tr_ = exact_dv_topo(cfg, np.einsum("tjdc,jc->tjd", J, dr), coord_mgr=Mgr())
    _assert_close("device astrometry, d_radec", cfg, _jvp(kw, d_radec=dr, astrom=ctxs, device_astrometry=True), er, tr_, cfg["eps"])


# ---- 5. bits, memory, the C ABI --------------------------------------------------------------------------------------
def test_reproducible_for_a_lane_count(gpu, monkeypatch):
    cfg = edge_config(nsrc=40, ntimes=4, seed=3)
    db, dt = random_dbls(cfg, 1), random_dtopo(cfg, 2)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a, b = _jvp(cfg, d_baselines=db, d_topo=dt), _jvp(cfg, d_baselines=db, d_topo=dt)
        assert np.array_equal(a, b), lanes
        res[lanes] = a
    assert rel_l2(res["1"], res["2"]) <= 1e-12


@pytest.mark.parametrize("heights", ["flat", "cm"])
def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu, heights):
    cfg = source_config(heights, "full", "two", False)
    before = fftvis_amd.simulate_vis(**cfg)
    _jvp(cfg, d_baselines=random_dbls(cfg, 1), d_topo=random_dtopo(cfg, 2))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)


def test_bulk_device_memory_is_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the
    forward: no staged input and no multiplied strength buffer stays."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = edge_config()
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _jvp(cfg, d_baselines=random_dbls(cfg, 1), d_topo=random_dtopo(cfg, 2))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


def test_a_value_that_is_not_finite_fails_and_the_handle_stays_usable(gpu):
    cfg = edge_config()
    db, dt = random_dbls(cfg, 1), random_dtopo(cfg, 2)
    good = _jvp(cfg, d_baselines=db, d_topo=dt)
    for bad_b, bad_t in ((np.nan, None), (None, np.inf), (None, np.nan)):
        b, t = db.copy(), dt.copy()
        if bad_b is not None:
            b[3, 1] = bad_b
        if bad_t is not None:
            t[1, 5, 2] = bad_t
        with pytest.raises(_lib.FftvisHipError, match="finite"):
            _jvp(cfg, d_baselines=b, d_topo=t)
        assert np.array_equal(_jvp(cfg, d_baselines=db, d_topo=dt), good)


def test_raw_c_abi(gpu):
    """fv_sim_run_tangent through a bare ctypes handle configured by the engine's own setters: device and host pointers,
    either input NULL, sub-blocks in time and frequency, and a lattice handle and a basis handle refused."""
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs
    from tests.basis_adjoint_refs import basis_config
    from tests.position_adjoint_refs import hex_positions

    cfg = edge_config()
    db, dt = random_dbls(cfg, 1), random_dtopo(cfg, 2)
    gb, gt, both = _jvp(cfg, d_baselines=db), _jvp(cfg, d_topo=dt), _jvp(cfg, d_baselines=db, d_topo=dt)
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        dB, dT = torch.from_numpy(db).cuda(), torch.from_numpy(dt).cuda()
        dV = torch.full(vis_shape(cfg), 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, nf, p(dB), 1, p(dT), 1, p(dV), 1) == 0, L.fv_last_error()
        assert np.array_equal(dV.cpu().numpy(), both)  # always overwritten
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, nf, p(dB), 1, None, 0, p(dV), 1) == 0, L.fv_last_error()
        assert np.array_equal(dV.cpu().numpy(), gb)
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, nf, None, 0, p(dT), 1, p(dV), 1) == 0, L.fv_last_error()
        assert np.array_equal(dV.cpu().numpy(), gt)
        hV = np.full(vis_shape(cfg), 7.0, dtype=np.complex128)  # host pointers
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, nf, hp(db), 0, hp(dt), 0, hp(hV), 0) == 0, L.fv_last_error()
        assert np.array_equal(hV, both)
        blk = np.zeros((nf - 1, 1) + vis_shape(cfg)[2:], dtype=np.complex128)  # one time step, the upper channels
        row = np.ascontiguousarray(dt[1:2])
        assert L.fv_sim_run_tangent(h._h, 1, 2, 1, nf, hp(db), 0, hp(row), 0, hp(blk), 0) == 0, L.fv_last_error()
        assert rel_l2(blk, both[1:, 1:2]) <= 10 * cfg["eps"] and blk.any()
        sub = dict(cfg, freqs=cfg["freqs"][:1], fluxes=cfg["fluxes"][:, :1])  # one channel against the reference
        one = np.zeros((1,) + vis_shape(cfg)[1:], dtype=np.complex128)
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, 1, hp(db), 0, None, 0, hp(one), 0) == 0, L.fv_last_error()
        eb, tb = exact_dv_baselines(sub, db)
        _assert_close("c abi, one channel", sub, one, eb, tb, cfg["eps"])
        assert L.fv_sim_run_tangent(h._h, 0, nt, 0, nf, None, 0, None, 0, hp(hV), 0) == 1
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
            assert L.fv_sim_run_tangent(h._h, 0, 1, 0, 1, p(buf), 1, None, 0, p(buf), 1) == 1
            assert word in L.fv_last_error(), L.fv_last_error()
        finally:
            gs._return_handle(key, h)


def test_device_tensors_in_give_a_device_tensor_out(gpu):
    import torch

    cfg = edge_config()
    db, dt = random_dbls(cfg, 1), random_dtopo(cfg, 2)
    want = _jvp(cfg, d_baselines=db, d_topo=dt)
    got = _jvp(cfg, d_baselines=torch.from_numpy(db).cuda(), d_topo=torch.from_numpy(dt).cuda())
    assert got.device.type == "cuda" and got.dtype == torch.complex128 and np.array_equal(got.cpu().numpy(), want)
    host = _jvp(cfg, d_baselines=torch.from_numpy(db))
    assert isinstance(host, torch.Tensor) and host.device.type == "cpu"


# ---- 6. against the adjoints -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("cell", [("cm", "full", "complex", False), ("flat", "unpol", "two", True), ("m", "I", "airy", True),
                                  ("order", 1), ("order", 0)])
def test_dot_identity_with_the_device_adjoints(gpu, cell, precision):
    """Re <dV, G> = sum dbls . gbls + sum dtopo . gtopo between independently written passes.  Secondary: each side is one
    pass held to 10 base (fp32: K32 base) times its cancellation, so the difference is held to the sum of the two bounds,
    relative to sum |conj(G) dV| and sum |v . g|, the sums the two sides are rounded in.  ("order", n): the complex table at
    spline order n, ``order_config``."""
    cfg = order_config(cell[1], precision=precision) if cell[0] == "order" else source_config(*cell, precision)
    cdt = np.complex64 if precision == 1 else np.complex128
    G = random_complex(vis_shape(cfg), 4).astype(cdt)
    db, dt = random_dbls(cfg, DB_SEED), random_dtopo(cfg, DT_SEED)
    dv = _jvp(cfg, d_baselines=db, d_topo=dt).astype(np.complex128)
    gb = fftvis_amd.simulate_vis_position_adjoint(G, **cfg, wrt="baselines")
    gt = fftvis_amd.simulate_vis_source_adjoint(G, **cfg, wrt="topo")
    lhs = float(np.sum((np.conj(G.astype(np.complex128)) * dv).real))
    rhs = float(np.sum(db * gb) + np.sum(dt * gt))
    k = 10.0 if precision == 2 else K32
    base = _forward_base(cfg)
    bound = k * base * (np.linalg.norm(G) * np.linalg.norm(dv) +
                        np.linalg.norm(db) * np.linalg.norm(gb) + np.linalg.norm(dt) * np.linalg.norm(gt))
    print("tangent dot identity", cell, precision, lhs, rhs, abs(lhs - rhs) / bound)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ---- 7. torch --------------------------------------------------------------------------------------------------------
def _small_cfg():
    cfg = edge_config(nsrc=8, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)],
               coord_method="SiderealRotation")
    _, _, cfg["fluxes"] = synth.catalog(8, cfg["freqs"], 0, polarized_sky=True)
    assert margins(cfg)[0] > 1e-3
    return cfg


def test_forward_ad_through_the_three_operations_equals_the_direct_calls(gpu):
    import torch
    import torch.autograd.forward_ad as fwAD

    cfg = dict(edge_config(), coord_method="SiderealRotation")
    rng = np.random.default_rng(6)
    df, da, dr = rng.normal(size=cfg["fluxes"].shape), rng.normal(size=(7, 3)), 1e-3 * rng.normal(size=(24, 2))
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda")
    P = torch.tensor(np.array(list(cfg["ants"].values())), dtype=torch.float64, device="cuda")
    R = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda")
    tF, tP, tR = (torch.tensor(x, dtype=torch.float64, device="cuda") for x in (df, da, dr))
    V = fftvis_amd.simulate_vis(**cfg)

    def check(out, want):
        primal, tangent = fwAD.unpack_dual(out)
        assert tangent is not None and tangent.device == F.device and tangent.dtype == torch.complex128
        assert rel_l2(primal.cpu().numpy(), V) <= 1e-12
        assert rel_l2(tangent.cpu().numpy(), want) <= 1e-12

    with fwAD.dual_level():
        kw = {k: v for k, v in cfg.items() if k != "fluxes"}
        check(fftvis_amd.torch_simulate_vis(fwAD.make_dual(F, tF), **kw), _jvp(cfg, d_fluxes=df))
        kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ants")}
        check(fftvis_amd.torch_simulate_vis_array(fwAD.make_dual(F, tF), fwAD.make_dual(P, tP), **kw),
              _jvp(cfg, d_fluxes=df, d_ants=da))
        check(fftvis_amd.torch_simulate_vis_array(F, fwAD.make_dual(P, tP), **kw), _jvp(cfg, d_ants=da))  # a missing tangent
        kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec")}
        check(fftvis_amd.torch_simulate_vis_sky(fwAD.make_dual(F, tF), fwAD.make_dual(R, tR), **kw),
              _jvp(cfg, d_fluxes=df, d_radec=dr))
        check(fftvis_amd.torch_simulate_vis_sky(F, fwAD.make_dual(R, tR), **kw), _jvp(cfg, d_radec=dr))


def test_torch_gradcheck_forward_ad_array(gpu):
    """The existing gradcheck's sizes and steps (fp64, 8 sources, 1 channel, 1 time, eps 1e-12, position step 1e-3 m), with
    forward-mode AD checked as well."""
    import torch

    cfg = _small_cfg()
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ants")}
    F = torch.tensor(cfg["fluxes"] + np.array([1.0, 0, 0, 0]), dtype=torch.float64, device="cuda", requires_grad=True)
    P = torch.tensor(np.array(list(cfg["ants"].values())), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, p: fftvis_amd.torch_simulate_vis_array(f, p, **kw), (F, P), eps=1e-3,
                                    atol=1e-7, rtol=1e-4, check_forward_ad=True)


def test_torch_gradcheck_forward_ad_sky(gpu):
    """The existing gradcheck's sizes and steps (angular step 1e-6 rad, atol 1e-6, rtol 1e-4), with forward-mode AD."""
    import torch

    cfg = _small_cfg()
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec")}
    F = torch.tensor(cfg["fluxes"] + np.array([1.0, 0, 0, 0]), dtype=torch.float64, device="cuda", requires_grad=True)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, p: fftvis_amd.torch_simulate_vis_sky(f, p, **kw), (F, P), eps=1e-6,
                                    atol=1e-6, rtol=1e-4, check_forward_ad=True)
