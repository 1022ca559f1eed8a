"""CPU tests of the forward-mode tangent's host side (``simulate_vis_jvp``, ``fv_sim_run_tangent``): the exports, the C
entry point's argument checking, the Python argument errors that are raised before a device is needed, the map from the
antennas' tangent to the baselines', and the exact references the GPU tests compare with (``tangent_refs``), pinned here on
the CPU -- against finite differences of the oracle, against each other at two step sizes, and through the identity
Re <J v, G> = <v, J^T G> against the adjoints' references (``position_adjoint_refs.exact_gbls``,
``source_adjoint_refs.exact_gtopo``), which were written independently.

Bounds: 1e-9 for the closed form against Richardson differences of the oracle in the positions (2 mm and 1 mm: the
position host test's figure), for the two extrapolations of the direction reference, (h, h / 2) against (h / 2, h / 4)
-- a decade under the 1e-8 the source tests keep --, and for both dot identities.  Measured over the three cells below:
the closed form against the differences 3.4e-12; the two extrapolations 8.1e-11 rel l2 of the whole and 9.4e-11 of the
largest entry; the dot identities 5e-16 (baselines) and 5.9e-11 (directions) relative.  The beam part is 24 - 52 % of the
direction tangent in these cells, and kappa is 1.06 - 1.68 over every configuration of the GPU module.

A table beam has a direction reference at every spline order wherever no source sits within the stencil of a knot line
(``source_adjoint_refs.knot_margin``, asserted here for every configuration of the GPU module); at order 0 the closed form
with the beam frozen (``tangent_refs.frozen_beam_dv_topo``) is the whole tangent and is pinned against the differences.
Measured: the two extrapolations 1.7e-10 / 1.4e-10 at worst over the orders 0, 1, 2, 4 and 5, 1.5e-9 / 1.2e-9 on the
full-sky table's edge sources at order 1 (1.7e-10 at order 3), 6e-12 on the table that ends at the horizon; what the
differences leave beside the closed form at order 0 is 5.6e-11 of the tangent; kappa 1.42 - 1.70 on the new configurations.
"""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.helpers import oracle_simulate
from tests.position_adjoint_refs import exact_gbls
from tests.source_adjoint_refs import exact_gtopo, frozen_beam_gtopo
from tests.tangent_refs import (DT_SEED, H_REF, ORDERS, all_configs, edge_table_config, exact_dv_baselines, exact_dv_topo,
                                frozen_beam_dv_topo, jump_config, kappa, knot_margin, margins, order_config,
                                random_complex, random_dbls, random_dtopo, source_config, vis_shape)

REF_BOUND = 1e-9
KAPPA_MAX = 4.0


def test_tangent_is_exported():
    for name in ("simulate_vis_jvp", "antenna_to_baseline_tangent"):
        assert callable(getattr(fftvis_amd, name)), name
    assert "fv_sim_run_tangent" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "fv_sim_run_tangent")
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_tangent)


def test_run_tangent_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    fake = ctypes.c_void_p(1)
    assert L.fv_sim_run_tangent(None, 0, 1, 0, 1, buf, 0, buf, 0, buf, 0) == 1
    assert b"handle" in L.fv_last_error()
    assert L.fv_sim_run_tangent(fake, 0, 1, 0, 1, buf, 0, buf, 0, None, 0) == 1
    assert b"null output" in L.fv_last_error()
    assert L.fv_sim_run_tangent(fake, 0, 1, 0, 1, None, 0, None, 0, buf, 0) == 1
    assert b"both null" in L.fv_last_error()
    for flags in [(2, 0, 0), (0, -1, 0), (0, 0, 3)]:
        assert L.fv_sim_run_tangent(fake, 0, 1, 0, 1, buf, flags[0], buf, flags[1], buf, flags[2]) == 1
        assert b"on_device" in L.fv_last_error()
    for dbls, dtopo in [(None, buf), (buf, None)]:  # either input alone passes the pointer checks: the handle is looked at next
        assert L.fv_sim_run_tangent(None, 0, 1, 0, 1, dbls, 0, dtopo, 0, buf, 0) == 1
        assert b"handle" in L.fv_last_error()


def test_argument_errors_come_before_device_work():
    cfg = dict(source_config(sky="I"), coord_method="SiderealRotation")
    nbls = len(cfg["baselines"])
    call = fftvis_amd.simulate_vis_jvp
    da, db = np.zeros((7, 3)), np.zeros((nbls, 3))
    dr, dt = np.zeros((24, 2)), np.zeros((2, 24, 3))
    with pytest.raises(ValueError, match="d_ants or as d_baselines"):
        call(**cfg, d_ants=da, d_baselines=db)
    with pytest.raises(ValueError, match="d_radec or as d_topo"):
        call(**cfg, d_radec=dr, d_topo=dt)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        call(**cfg, d_ants=da, beam_coefs=np.ones((7, 1, 3), complex))
    with pytest.raises(ValueError, match="backend"):
        call(**cfg, d_ants=da, backend="cpu")

    class Mgr:
        pass

    with pytest.raises(ValueError, match="d_topo"):  # the manager's chain is the caller's
        call(**cfg, d_radec=dr, coord_mgr=Mgr())
    with pytest.raises(ValueError, match="d_topo"):  # ... and so is a matvis manager the engine would build
        call(**dict(cfg, coord_method="CoordinateRotationERFA"), d_radec=dr)
    for kw in (dict(d_ants=np.zeros((6, 3))), dict(d_baselines=np.zeros((nbls, 2))), dict(d_radec=np.zeros((24, 3))),
               dict(d_topo=np.zeros((2, 23, 3))), dict(d_fluxes=np.zeros((24, 2)))):
        with pytest.raises(ValueError, match="must have"):
            call(**cfg, **kw)
    with pytest.raises(ValueError, match="fluxes must have shape"):
        call(**dict(cfg, fluxes=np.ones((5, 3))), d_ants=da)
    # no input at all: zeros of simulate_vis's shape and dtype, and no device work
    z = call(**cfg)
    assert z.shape == vis_shape(cfg) and z.dtype == np.complex128 and not z.any()
    z32 = call(**dict(cfg, precision=1))
    assert z32.dtype == np.complex64


def test_antenna_tangent_is_the_transpose_of_the_gradient_scatter():
    import torch

    cfg = source_config()
    rng = np.random.default_rng(5)
    da, gb = rng.normal(size=(7, 3)), rng.normal(size=(len(cfg["baselines"]), 3))
    db = fftvis_amd.antenna_to_baseline_tangent(da, cfg["ants"], cfg["baselines"])
    assert db.shape == gb.shape and db.dtype == np.float64
    for k, (i, j) in enumerate(cfg["baselines"]):
        assert np.array_equal(db[k], da[j] - da[i])
    ga = fftvis_amd.baseline_to_antenna_gradient(gb, cfg["ants"], cfg["baselines"])
    assert abs(np.sum(db * gb) - np.sum(da * ga)) <= 1e-13 * np.abs(db * gb).sum()
    tb = fftvis_amd.antenna_to_baseline_tangent(torch.from_numpy(da), cfg["ants"], cfg["baselines"])
    assert isinstance(tb, torch.Tensor) and np.array_equal(tb.numpy(), db)
    keys = {10 * (i + 1): v for i, v in cfg["ants"].items()}  # rows follow the dictionary's order, whatever the keys
    bls = [(10 * (i + 1), 10 * (j + 1)) for i, j in cfg["baselines"]]
    assert np.array_equal(fftvis_amd.antenna_to_baseline_tangent(da, keys, bls), db)
    with pytest.raises(ValueError, match="d_ants must have shape"):
        fftvis_amd.antenna_to_baseline_tangent(da[:6], cfg["ants"], cfg["baselines"])


CELLS = [("cm", "full", "complex", False), ("flat", "unpol", "two", True), ("m", "I", "airy", True)]


@pytest.mark.parametrize("cell", CELLS)
def test_baseline_reference_against_differences_of_the_oracle(cell):
    """The closed form along d_ants against (4 D(1 mm) - D(2 mm)) / 3 of the oracle in the antenna positions."""
    cfg = source_config(*cell)
    da = np.random.default_rng(6).normal(size=(7, 3))
    da /= np.linalg.norm(da, axis=1).max()
    dv, terms = exact_dv_baselines(cfg, fftvis_amd.antenna_to_baseline_tangent(da, cfg["ants"], cfg["baselines"]))
    assert np.linalg.norm(terms[2]) > 1e-3 * np.linalg.norm(dv)  # the up component takes part, on the flat array too

    def D(h):
        p = {k: v + h * da[i] for i, (k, v) in enumerate(cfg["ants"].items())}
        m = {k: v - h * da[i] for i, (k, v) in enumerate(cfg["ants"].items())}
        return (oracle_simulate(dict(cfg, ants=p)) - oracle_simulate(dict(cfg, ants=m))) / (2.0 * h)

    fd = (4.0 * D(1e-3) - D(2e-3)) / 3.0
    d = np.linalg.norm(dv - fd) / np.linalg.norm(fd)
    print("tangent reference, baselines against differences", cell, d)
    assert d <= REF_BOUND, d


TABLE_CELLS = [("order", o) for o in ORDERS] + [("fullsky", 1), ("fullsky", 3), ("horizon", 1), ("horizon", 3)]


def _cell_config(cell):
    if cell[0] == "order":
        return order_config(cell[1]), None
    if cell[0] in ("fullsky", "horizon"):
        return edge_table_config(*cell)
    return source_config(*cell), None


@pytest.mark.parametrize("cell", CELLS + TABLE_CELLS)
def test_direction_reference_extrapolations_agree(cell):
    """(h, h / 2) against (h / 2, h / 4), rel l2 of the whole; the beam part is not negligible in these cells -- except at
    spline order 0, where it is none of the tangent.  The table-edge configurations are held to the source host test's
    5e-9 instead of 1e-9: a source at za = 3e-3 turns in az by h / za = 3e-3 rad over the stencil, so the remainder
    carries (h / za)^4 next to (k h)^4 (measured 1.5e-9 on the full-sky table at order 1, 1.7e-10 at order 3)."""
    cfg, mgr = _cell_config(cell)
    dt = random_dtopo(cfg, 7)
    d1, phase, terms = exact_dv_topo(cfg, dt, coord_mgr=mgr)
    d2, _, _ = exact_dv_topo(cfg, dt, coord_mgr=mgr, h=H_REF / 2)
    whole = np.linalg.norm(d1 - d2) / np.linalg.norm(d1)
    worst = np.abs(d1 - d2).max() / np.abs(d1).max()
    share = np.linalg.norm(d1 - phase) / np.linalg.norm(d1)
    print("tangent reference, extrapolations", cell, whole, worst, "beam share", share)
    bound = 5e-9 if mgr is not None else REF_BOUND
    assert whole <= bound and worst <= bound, (whole, worst)
    if cell == ("order", 0):
        assert share <= REF_BOUND, share  # the closed form with the beam frozen is the whole tangent
        return
    assert share > 1e-3, share
    if mgr is None:  # the radial part of dtopo changes nothing
        n = _unit_vectors(cfg)
        d3, _, _ = exact_dv_topo(cfg, dt + 3.0 * n)
        assert np.linalg.norm(d3 - d1) <= 1e-12 * np.linalg.norm(d1)


def test_frozen_beam_tangent_on_a_jump_is_dual_to_the_frozen_beam_gradient():
    """With a source on a jump of an order-0 table both closed forms stay what they are, and they are each other's
    transpose: Re <dV, G> = sum dtopo . gtopo to rounding, no differences on either side."""
    cfg, mgr, rows = jump_config()
    G = random_complex(vis_shape(cfg), 4)
    dt = random_dtopo(cfg, DT_SEED)
    dv, terms = frozen_beam_dv_topo(cfg, dt, coord_mgr=mgr)
    assert np.isfinite(dv).all() and dv.any() and np.allclose(dv, terms[0] + terms[1] + terms[2], rtol=0, atol=0)
    lhs = float(np.sum((np.conj(G) * dv).real))
    rhs = float(np.sum(dt * frozen_beam_gtopo(cfg, G, coord_mgr=mgr)))
    print("tangent reference, frozen beam, dot identity", lhs, rhs)
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(np.conj(G) * dv))


def _unit_vectors(cfg):
    from oracle import fftvis_oracle as orc

    m = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    return np.stack([orc._topo_of(m, ti).T for ti in range(len(cfg["times"]))])


@pytest.mark.parametrize("cell", CELLS)
def test_dot_identities_with_the_adjoint_references(cell):
    """Re <dV, G> = sum dbls . gbls and = sum dtopo . gtopo (gtopo is tangential: the radial part of dtopo drops out)."""
    cfg = source_config(*cell)
    G = random_complex(vis_shape(cfg), 4)
    db, dt = random_dbls(cfg, 8), random_dtopo(cfg, 9)
    lhs = float(np.sum((np.conj(G) * exact_dv_baselines(cfg, db)[0]).real))
    rhs = float(np.sum(db * exact_gbls(cfg, G)))
    print("tangent reference, dot identity, baselines", cell, lhs, rhs)
    assert abs(lhs - rhs) <= REF_BOUND * abs(rhs)
    lhs = float(np.sum((np.conj(G) * exact_dv_topo(cfg, dt)[0]).real))
    rhs = float(np.sum(dt * exact_gtopo(cfg, G)))
    print("tangent reference, dot identity, directions", cell, lhs, rhs)
    assert abs(lhs - rhs) <= REF_BOUND * abs(rhs)


def test_every_gpu_configuration_is_well_conditioned():
    """Every configuration the GPU module compares with a reference: nothing within 1e-3 rad of the horizon or (unpolarized
    runs with two dishes) of a beam null, and the reference's terms do not cancel beyond a factor KAPPA_MAX -- for the
    tangents the GPU module uses, which are seeded here and there alike."""
    for label, cfg, db, dt, mgr, order, bound in all_configs():
        hor, null = margins(cfg, coord_mgr=mgr)
        assert hor > 1e-3 and null > 1e-3, (label, hor, null)
        if bound is not None:
            knot = knot_margin(cfg, order, coord_mgr=mgr)
            assert knot > bound, (label, knot, bound)
        if db is not None:
            dv, terms = exact_dv_baselines(cfg, db)
            k = kappa(dv, terms)
            print("tangent kappa, baselines", label, k)
            assert k <= KAPPA_MAX, (label, k)
        if dt is not None:
            dv, _, terms = exact_dv_topo(cfg, dt, coord_mgr=mgr)
            k = kappa(dv, terms)
            print("tangent kappa, directions", label, k)
            assert k <= KAPPA_MAX, (label, k)
