"""CPU tests of the source-position gradient's host side: the exports, the C entry point's argument checking, the Python
argument errors that are raised before a device is needed, the chain from the topocentric gradient to (ra, dec), and the
exact reference the GPU tests compare with (``source_adjoint_refs.exact_gtopo``), pinned here on the CPU.

The reference is a Richardson-extrapolated central difference of the oracle's forward at h = 1e-5 rad and h / 2; its
remainder is about (k h)^4 with k = 2 pi nu |b| / c <~ 500 on these arrays (a few 1e-10 with the constants).  Measured
here, the extrapolations from (h, h / 2) and from (h / 2, h / 4) agree to 5.8e-11 rel l2 of the whole (ntimes, nsrc, 3)
result and 4.5e-11 of its largest entry at worst over the three cells below, and the reference taken in (ra, dec) agrees
with the chained one to 5.1e-11: more than twice better than 1e-8, which is therefore the bound kept.

A table beam has a reference at every spline order wherever no source sits within the stencil of a knot line
(``knot_margin``; the condition is asserted here for every configuration the GPU modules use).  Measured here on the
cell "cm, full Stokes, exact flips, complex table" at catalog seed 3, the two extrapolations agree to 7.4e-11 of the whole
and 9.3e-11 at worst over the orders 0, 1, 2, 4 and 5 (G of seed 4); on the table-edge configurations every single row
agrees to 1.5e-9 (full-sky table, order 1; 2.3e-10 at order 3) and 2.5e-10 (the table that ends at the horizon).  At
order 0 the closed form with the beam frozen equals the differences to 2.7e-11 of the whole, 2.9e-11 of the largest entry.
"""

import ctypes
import functools

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.source_adjoint_refs import (H_REF, JUMP_OFFSET, ORDERS, GivenTopo, edge_table_config, exact_gradec, exact_gtopo,
                                       frozen_beam_gtopo, gradcheck_config, jump_config, knot_margin, margins,
                                       order_config, random_complex, sidereal_jacobian, source_config, table_config,
                                       table_configs, vis_shape)

REF_BOUND = 1e-8


def test_source_adjoint_is_exported():
    for name in ("simulate_vis_source_adjoint", "torch_simulate_vis_sky", "topo_to_radec_gradient", "radec_jacobian"):
        assert callable(getattr(fftvis_amd, name)), name
    assert "fv_sim_run_source_adjoint" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "fv_sim_run_source_adjoint")
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_source_adjoint)


def test_run_source_adjoint_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    assert L.fv_sim_run_source_adjoint(None, 0, 1, 0, 1, buf, 0, buf, 0, 0) == 1
    assert b"handle" in L.fv_last_error()
    for g, out in [(None, buf), (buf, None)]:
        assert L.fv_sim_run_source_adjoint(None, 0, 1, 0, 1, g, 0, out, 0, 0) == 1
        assert b"null adjoint" in L.fv_last_error()
    for flags in [(2, 0), (0, -1), (3, 3)]:
        assert L.fv_sim_run_source_adjoint(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], 0) == 1
        assert b"on_device" in L.fv_last_error()
    for acc in (2, -1):
        assert L.fv_sim_run_source_adjoint(None, 0, 1, 0, 1, buf, 0, buf, 0, acc) == 1
        assert b"accumulate" in L.fv_last_error()


def test_argument_errors_come_before_device_work():
    cfg = dict(source_config(sky="I"), coord_method="SiderealRotation")
    good = np.zeros(vis_shape(cfg), complex)
    nbls = len(cfg["baselines"])
    call = fftvis_amd.simulate_vis_source_adjoint
    for wrt in ("sources", (), ("topo", "topo"), ("radec", "fluxes")):
        with pytest.raises(ValueError, match="wrt"):
            call(good, **cfg, wrt=wrt)
    for shape in [(3, 2, nbls), (3, 2, 2, 2, nbls - 1), (2, 3, 2, 2, nbls)]:
        with pytest.raises(ValueError, match="output shape"):
            call(np.zeros(shape, complex), **cfg)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        call(good, **cfg, beam_coefs=np.ones((7, 1, 3), complex))
    with pytest.raises(ValueError, match="backend"):
        call(good, **cfg, backend="cpu")
    with pytest.raises(ValueError, match="fluxes must have shape"):
        call(good, **dict(cfg, fluxes=np.ones((5, 3))))
    with pytest.raises(TypeError, match="adjoint_path"):
        call(good, **cfg, adjoint_path="type3")

    class Mgr:
        pass

    for wrt in ("radec", ("topo", "radec")):  # the manager's chain is the caller's
        with pytest.raises(ValueError, match="wrt='topo'"):
            call(good, **cfg, wrt=wrt, coord_mgr=Mgr())
    with pytest.raises(ValueError, match="wrt='topo'"):  # ... and so is a matvis manager the engine would build
        call(good, **dict(cfg, coord_method="CoordinateRotationERFA"), wrt="radec")
    import torch

    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec")}
    F, P = torch.ones(24, 3), torch.zeros(24, 2)
    for bad in ({"ra": cfg["ra"]}, {"dec": cfg["dec"]}):
        with pytest.raises(TypeError, match="radec"):
            fftvis_amd.torch_simulate_vis_sky(F, P, **kw, **bad)
    with pytest.raises(ValueError, match="radec must be"):
        fftvis_amd.torch_simulate_vis_sky(F, torch.zeros(24, 3), **kw)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.torch_simulate_vis_sky(F, P, **kw, beam_coefs=np.ones((7, 1, 3), complex))


def test_chain_helper_against_its_closed_form():
    """J from ``radec_jacobian`` equals the oracle-side closed form and, independently, central differences of the unit
    vectors; the helper is sum_t J_t^T gtopo[t], in numpy and in torch; d n / d(ra, dec) is perpendicular to n."""
    import torch

    from oracle import fftvis_oracle as orc

    cfg = source_config()
    J = fftvis_amd.radec_jacobian(cfg["ra"], cfg["dec"], cfg["times"], cfg["telescope_loc"])
    assert J.shape == (2, 24, 3, 2) and J.dtype == np.float64
    assert np.abs(J - sidereal_jacobian(cfg)).max() <= 1e-14

    def topo(ra, dec):
        m = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], ra, dec)
        return np.stack([orc._topo_of(m, ti).T for ti in range(2)])  # (nt, nsrc, 3)

    h = 1e-6
    fd = np.stack([(topo(cfg["ra"] + h, cfg["dec"]) - topo(cfg["ra"] - h, cfg["dec"])) / (2 * h),
                   (topo(cfg["ra"], cfg["dec"] + h) - topo(cfg["ra"], cfg["dec"] - h)) / (2 * h)], axis=-1)
    assert np.abs(J - fd).max() <= 1e-9  # h^2 / 6 and 1e-16 / h
    n = topo(cfg["ra"], cfg["dec"])
    assert np.abs(np.einsum("tjd,tjdc->tjc", n, J)).max() <= 1e-14
    g = np.random.default_rng(3).normal(size=(2, 24, 3))
    want = np.zeros((24, 2))
    for t in range(2):
        for j in range(24):
            want[j] += J[t, j].T @ g[t, j]
    got = fftvis_amd.topo_to_radec_gradient(g, J)
    assert got.shape == (24, 2) and got.dtype == np.float64 and np.abs(got - want).max() <= 1e-13
    tg = fftvis_amd.topo_to_radec_gradient(torch.from_numpy(g), J)
    assert isinstance(tg, torch.Tensor) and np.abs(tg.numpy() - want).max() <= 1e-13
    with pytest.raises(ValueError, match="gtopo must be"):
        fftvis_amd.topo_to_radec_gradient(g[0], J)
    with pytest.raises(ValueError, match="gtopo must be"):
        fftvis_amd.topo_to_radec_gradient(g, J[..., :1])


def _all_configs():
    """(cfg, manager or None, spline order, knot bound) of every configuration the GPU tests compare with the reference
    (``test_gpu_source_adjoint`` builds them the same way).  knot bound: what ``knot_margin`` has to exceed, None where no
    table is differenced below order 3."""
    out = []
    for heights in ("flat", "cm", "m"):
        for sky in ("unpol", "I", "full"):
            for beams in ("airy", "two", "complex"):
                out.append((source_config(heights, sky, beams), None, 3, None))
    out.append((source_config("cm", "full", "two", False, nsrc=25, ntimes=4), None, 3, None))
    out.append((source_config("cm", "full", "two", False, nsrc=18, nfreq=5), None, 3, None))
    out.append((source_config("cm", "full", "two", False, ntimes=3), None, 3, None))
    out.append((source_config("cm", "full", "two", False, nsrc=8, nfreq=1, ntimes=1), None, 3, None))
    # (the lane-agreement runs: the device against itself, only the horizon's condition)
    out.append((table_config(0, nsrc=40, ntimes=4, seed=3), None, 0, None))
    out += [(cfg, mgr, order, bound) for _, cfg, order, mgr, bound in table_configs()]
    out.append((gradcheck_config(), None, 1, 1e-4))  # a hundred times its perturbation step of 1e-6 rad
    return out


def test_no_source_of_a_test_configuration_is_near_the_horizon_or_a_null():
    """... nor, where a table below order 3 is differenced, near one of its knot lines."""
    for cfg, mgr, order, bound in _all_configs():
        hor, null = margins(cfg, coord_mgr=mgr)
        assert hor > 1e-3 and null > 1e-3, (hor, null)
        if bound is not None:
            knot = knot_margin(cfg, order, coord_mgr=mgr)
            assert knot > bound, (order, knot, bound)


def test_knot_margin_against_hand_placed_sources():
    """The margin finds what was placed: the figures of the seeded cell, odd and even orders half a node apart, the
    az distance scaled by sin(za), the grid taken from the beam; and the two sources of the order-0 jump configuration
    are the only ones near a line."""
    assert abs(knot_margin(order_config(0), 0) - 1.30e-3) < 1e-5 and abs(knot_margin(order_config(1), 1) - 2.29e-3) < 1e-5
    assert knot_margin(order_config(2), 2) == knot_margin(order_config(0), 0)
    assert knot_margin(table_config(1), 1) < 1e-3  # the catalog seed of the other configurations does not satisfy it
    assert knot_margin(source_config(), 1) == np.inf  # no table
    cfg, mgr = edge_table_config("fullsky", 3)
    assert abs(knot_margin(cfg, 3, mgr) - 1e-7 * np.sin(12.6 * np.pi / 45)) < 1e-12  # the source at az = 1e-7
    assert knot_margin(cfg, 2, mgr) < 1e-12  # the near-zenith sources' mid-cell az is ON an even order's line
    cfg, mgr = edge_table_config("horizon", 1)
    want = 0.45 * (2 * np.pi / 90) * np.sin(0.6 * np.pi / 46)  # az 80.45 nodes at za 0.6 nodes of pi / 46
    assert abs(knot_margin(cfg, 1, mgr) - want) < 1e-9
    cfg, mgr, rows = jump_config()
    assert abs(knot_margin(cfg, 0, mgr) - JUMP_OFFSET) < 1e-9 and margins(cfg, mgr)[0] > 1e-3
    topos = mgr.topos.copy()
    topos[0, :, rows] = [0.0, 0.0, -1.0]
    assert knot_margin(cfg, 0, GivenTopo(cfg["times"], topos)) > 1e-3


CELLS = [("cm", "full", "complex", False), ("flat", "unpol", "two", True), ("m", "I", "airy", True)]
ORDER_CELLS = [("order", o) for o in ORDERS]
EDGE_CELLS = [("fullsky", 1), ("fullsky", 3), ("horizon", 1), ("horizon", 3)]


@functools.lru_cache(maxsize=None)
def _cell(*cell):
    """(cfg, manager or None, G, exact gtopo) of a matrix cell, of ("order", n) or of a table-edge configuration."""
    mgr = None
    if cell[0] == "order":
        cfg = order_config(cell[1])
    elif cell[0] in ("fullsky", "horizon"):
        cfg, mgr = edge_table_config(*cell)
    else:
        cfg = source_config(*cell)
    G = random_complex(vis_shape(cfg), 4)
    return cfg, mgr, G, exact_gtopo(cfg, G, coord_mgr=mgr)


@pytest.mark.parametrize("cell", CELLS + ORDER_CELLS + EDGE_CELLS)
def test_reference_extrapolations_agree(cell):
    """(h, h / 2) against (h / 2, h / 4): rel l2 of the whole and max |difference| / max |value| within REF_BOUND / 2; on
    the table-edge configurations, whose sources are placed by hand one per edge, every row's rel l2 as well."""
    cfg, mgr, G, g1 = _cell(*cell)
    g2 = exact_gtopo(cfg, G, coord_mgr=mgr, h=H_REF / 2)
    assert np.count_nonzero(g1) > 0 and np.isfinite(g1).all()
    whole = np.linalg.norm(g1 - g2) / np.linalg.norm(g1)
    worst = np.abs(g1 - g2).max() / np.abs(g1).max()
    print("source reference, extrapolations", cell, whole, worst)
    assert whole <= 0.5 * REF_BOUND and worst <= 0.5 * REF_BOUND, (whole, worst)
    if cell in EDGE_CELLS:
        rows = np.linalg.norm(g1 - g2, axis=-1) / np.linalg.norm(g1, axis=-1)
        print("source reference, extrapolations, rows", cell, rows.max())
        assert rows.max() <= 0.5 * REF_BOUND, rows


def test_frozen_beam_closed_form_is_the_whole_gradient_at_order_0():
    """Away from the jumps a piecewise-constant beam has no beam term: the closed form equals the differences.  At order 1
    it does not (the beam term is a visible share of the gradient), and on a jump it stays finite and tangential."""
    cfg, mgr, G, g1 = _cell("order", 0)
    fz = frozen_beam_gtopo(cfg, G)
    whole = np.linalg.norm(fz - g1) / np.linalg.norm(g1)
    worst = np.abs(fz - g1).max() / np.abs(g1).max()
    print("source reference, frozen beam at order 0", whole, worst)
    assert whole <= REF_BOUND and worst <= REF_BOUND, (whole, worst)
    assert np.array_equal(fz == 0, g1 == 0)
    cfg1, _, G1, g11 = _cell("order", 1)
    assert np.linalg.norm(frozen_beam_gtopo(cfg1, G1) - g11) > 1e-3 * np.linalg.norm(g11)
    jcfg, jmgr, rows = jump_config()
    fj = frozen_beam_gtopo(jcfg, G, coord_mgr=jmgr)
    n = jmgr.topos[0].T
    assert np.isfinite(fj).all() and np.all(np.any(fj[0, rows] != 0, axis=-1))
    assert np.abs(np.einsum("jd,jd->j", n, fj[0])).max() <= 1e-12 * np.abs(fj).max()
    keep = np.ones(24, bool)
    keep[rows] = False
    assert np.array_equal(fj[0, keep], fz[0, keep]) and np.array_equal(fj[1], fz[1])  # the others did not move


@pytest.mark.parametrize("cell", CELLS)
def test_reference_in_radec_is_the_chained_reference(cell):
    cfg, _, G, g1 = _cell(*cell)
    direct = exact_gradec(cfg, G)
    chained = np.einsum("tjd,tjdc->jc", g1, sidereal_jacobian(cfg))
    d = np.linalg.norm(direct - chained) / np.linalg.norm(direct)
    print("source reference, radec", cell, d)
    assert d <= REF_BOUND, d


@pytest.mark.parametrize("cell", CELLS)
def test_reference_is_tangential_and_zero_below_the_horizon(cell):
    from oracle import fftvis_oracle as orc

    cfg, _, G, g1 = _cell(*cell)
    m = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    n = np.stack([orc._topo_of(m, ti).T for ti in range(len(cfg["times"]))])
    assert np.abs(np.einsum("tjd,tjd->tj", n, g1)).max() <= 1e-12 * np.abs(g1).max()
    below = n[..., 2] <= 0
    assert below.any() and np.all(g1[below] == 0) and np.all(np.any(g1[~below] != 0, axis=-1))
