"""CPU tests of the source-position derivatives through basis beams: the exports and signatures, the Python argument errors
that are raised before a device is needed, the C entry points' argument checking, and the exact references the GPU tests
compare with (``basis_source_refs``), pinned here on the oracle's basis forward to 1e-8:

* the Richardson extrapolations from (h, h/2) against those from (h/2, h/4), for the gradient and for the tangent;
* Re <dV, G> against sum dtopo . gtopo between the two references, which are built independently (one source at a time
  against all sources at once);
* at spline order 0 the closed forms that hold the beams fixed against the differences;
* at K = 1 with unit coefficients the basis references against ``source_adjoint_refs`` / ``tangent_refs`` on the plain dish.

Measured (rel l2): the extrapolations 4e-11 ... 7e-11 (gradient) and 8e-11 ... 1.4e-10 (tangent); the identity 2e-13 ...
2e-12 of |G| |dV|; order 0 3e-11 and 7e-11; K = 1 exactly 0 (the same arithmetic); (ra, dec) 2e-11.  The margins of the table cells: horizon 1.2e-2 rad, knot lines
2.3e-3 rad at order 1, 1.3e-3 rad at orders 0 and 2; kappa of the tangent references 1.40 ... 1.78.
"""

import ctypes
import inspect

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests import source_adjoint_refs as sar
from tests import tangent_refs as tr
from tests.basis_position_refs import hera_subset
from tests.basis_source_refs import (DT_SEED, G_SEED, H_BEAM, basis_source_config, empty_step_basis_config, exact_dv_topo,
                                     exact_gradec, hera350_basis_config, hera350_basis_source_config, hex19_basis_config,
                                     slicing_configs,
                                     exact_gtopo, frozen_beam_dv_topo, frozen_beam_gtopo, gradcheck_basis_config,
                                     jump_basis_config, k1_configs, kappa, knot_margin, margins, matrix_cells,
                                     matrix_reference, mixed_order0_config, order0_reference, random_complex, random_dtopo,
                                     sidereal_jacobian, split_dv_topo, split_gtopo, vis_shape)
from tests.helpers import rel_l2

PIN = 1e-8
KAPPA_MAX = 4.0
HOST_CELLS = [("flat", "airy", "I", True), ("cm", "complex", "full", False), ("m", "real", "I", True),
              ("cm", "complex", "full", True)]
ROWS = [0, 5, 11, 17, 23]  # the catalogue rows the gradient's extrapolations are compared on


def test_basis_source_passes_are_exported():
    from fftvis_amd.gpu import gpu_simulate

    for name in ("simulate_vis_basis_source_adjoint", "simulate_vis_basis_source_jvp", "torch_simulate_vis_basis_sky"):
        assert callable(getattr(fftvis_amd, name))
    for sym, method in (("fv_sim_run_basis_source_adjoint", "run_basis_source_adjoint"),
                        ("fv_sim_run_basis_source_tangent", "run_basis_source_tangent")):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)
        assert callable(getattr(gpu_simulate.SimHandle, method))
    assert "basis_source_of" in inspect.signature(gpu_simulate.GPUSimulationEngine.simulate).parameters


def test_signatures():
    """Positional arguments as the siblings', then the pass's own keywords, then ``simulate_vis_basis_adjoint``'s trailing
    keywords with their defaults."""
    def params(f):
        return [(p.name, p.kind.name, p.default) for p in inspect.signature(f).parameters.values()]

    basis = params(fftvis_amd.simulate_vis_basis_adjoint)
    trailing = basis[[p[0] for p in basis].index("beam_idx"):]
    assert ("polarized", "KEYWORD_ONLY", True) in trailing and ("reference_compat", "KEYWORD_ONLY", True) in trailing
    pos = ["ants", "fluxes", "ra", "dec", "freqs", "times", "beam", "beam_coefs", "telescope_loc"]
    adj = params(fftvis_amd.simulate_vis_basis_source_adjoint)
    assert [p[0] for p in adj[:10]] == ["vis"] + pos and all(p[1] == "POSITIONAL_OR_KEYWORD" for p in adj[:10])
    assert adj[10] == ("wrt", "KEYWORD_ONLY", "radec") and adj[11:] == trailing
    jvp = params(fftvis_amd.simulate_vis_basis_source_jvp)
    assert [p[0] for p in jvp[:9]] == pos and all(p[1] == "POSITIONAL_OR_KEYWORD" for p in jvp[:9])
    assert jvp[9:11] == [("d_radec", "KEYWORD_ONLY", None), ("d_topo", "KEYWORD_ONLY", None)] and jvp[11:] == trailing
    sky = params(fftvis_amd.torch_simulate_vis_basis_sky)
    assert [(p[0], p[1]) for p in sky] == [("fluxes", "POSITIONAL_OR_KEYWORD"), ("beam_coefs", "POSITIONAL_OR_KEYWORD"),
                                           ("radec", "POSITIONAL_OR_KEYWORD"), ("kwargs", "VAR_KEYWORD")]


def test_c_entry_points_check_their_arguments():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    fake = ctypes.c_void_p(1)
    adj, tan = L.fv_sim_run_basis_source_adjoint, L.fv_sim_run_basis_source_tangent
    assert adj(None, 0, 1, 0, 1, buf, 0, buf, 0, 0) == 1
    assert b"null handle" in L.fv_last_error()
    assert tan(None, 0, 1, 0, 1, buf, 0, buf, 0) == 1
    assert b"null handle" in L.fv_last_error()
    for h in (None, fake):  # the buffers and the flags are checked before the handle is looked at
        for g, b in [(None, buf), (buf, None)]:
            assert adj(h, 0, 1, 0, 1, g, 0, b, 0, 0) == 1
            assert b"null adjoint input or output" in L.fv_last_error()
        for flags in [(2, 0), (0, -1)]:
            assert adj(h, 0, 1, 0, 1, buf, flags[0], buf, flags[1], 0) == 1
            assert b"on_device" in L.fv_last_error()
        for acc in (2, -1):
            assert adj(h, 0, 1, 0, 1, buf, 0, buf, 0, acc) == 1
            assert b"accumulate" in L.fv_last_error()
        assert tan(h, 0, 1, 0, 1, buf, 0, None, 0) == 1
        assert b"null output" in L.fv_last_error()
        assert tan(h, 0, 1, 0, 1, None, 0, buf, 0) == 1
        assert b"dtopo" in L.fv_last_error()
        for flags in [(2, 0), (-1, 0), (0, 3), (0, -1)]:
            assert tan(h, 0, 1, 0, 1, buf, flags[0], buf, flags[1]) == 1
            assert b"on_device" in L.fv_last_error()


def test_argument_errors_come_before_device_work():
    import torch

    cfg = basis_source_config()
    nsrc, nt = len(cfg["ra"]), len(cfg["times"])
    G = np.zeros(vis_shape(cfg), complex)
    adj, jvp = fftvis_amd.simulate_vis_basis_source_adjoint, fftvis_amd.simulate_vis_basis_source_jvp
    for wrt in (("topo", "ants"), (), ("topo", "topo"), "sources"):
        with pytest.raises(ValueError, match="wrt"):
            adj(G, **cfg, wrt=wrt)
    with pytest.raises(ValueError, match="vis must have"):
        adj(G[:1], **cfg, wrt="topo")
    with pytest.raises(ValueError, match="fluxes must have shape"):
        adj(G, **dict(cfg, fluxes=cfg["fluxes"][:-1]), wrt="topo")
    dr, dt = np.zeros((nsrc, 2)), np.zeros((nt, nsrc, 3))
    with pytest.raises(ValueError, match="d_radec or as d_topo"):
        jvp(**cfg, d_radec=dr, d_topo=dt)
    for kw in (dict(d_radec=np.zeros((nsrc, 3))), dict(d_radec=np.zeros((nsrc + 1, 2))), dict(d_topo=np.zeros((nt, nsrc, 2))),
               dict(d_topo=np.zeros((nt + 1, nsrc, 3)))):
        with pytest.raises(ValueError, match="must have shape"):
            jvp(**cfg, **kw)
    # the chain from (ra, dec) must be this package's own
    mgr = sar.GivenTopo(cfg["times"], np.zeros((nt, 3, nsrc)))
    with pytest.raises(ValueError, match="coord_mgr"):
        adj(G, **cfg, wrt="radec", coord_mgr=mgr)
    with pytest.raises(ValueError, match="coord_mgr"):
        jvp(**cfg, d_radec=dr, coord_mgr=mgr)
    erfa = dict(cfg, coord_method="CoordinateRotationERFA")
    with pytest.raises(ValueError, match="SiderealRotation"):
        adj(G, **erfa, wrt=("topo", "radec"))
    with pytest.raises(ValueError, match="SiderealRotation"):
        jvp(**erfa, d_radec=dr)
    # basis beams, polarized, the gpu backend
    for call in (lambda **k: adj(G, **k, wrt="topo"), lambda **k: jvp(**k, d_topo=dt)):
        with pytest.raises(ValueError, match="needs beam_coefs"):
            call(**dict(cfg, beam_coefs=None))
        with pytest.raises(ValueError, match="not compatible with unpolarized"):
            call(**dict(cfg, polarized=False))
        with pytest.raises(ValueError, match="backend"):
            call(**dict(cfg, backend="cpu"))
        with pytest.raises(ValueError, match="beam_coefs must have shape"):
            call(**dict(cfg, beam_coefs=cfg["beam_coefs"][:, :2]))
    # neither input: zeros of simulate_vis's shape and dtype, and no device work
    z = jvp(**cfg)
    assert z.shape == vis_shape(cfg) and z.dtype == np.complex128 and not z.any()
    z = jvp(**dict(cfg, precision=1))
    assert z.dtype == np.complex64 and not z.any()
    # the entry points without basis beams keep refusing beam_coefs
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.simulate_vis_source_adjoint(G, **cfg)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.simulate_vis_jvp(**cfg, d_topo=dt)
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "ra", "dec", "beam_coefs")}
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128)
    P = torch.tensor(np.stack([cfg["ra"], cfg["dec"]], axis=1), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.torch_simulate_vis_sky(F, P, beam_coefs=cfg["beam_coefs"], **kw)
    with pytest.raises(TypeError, match="radec"):
        fftvis_amd.torch_simulate_vis_basis_sky(F, C, P, ra=cfg["ra"], **kw)
    with pytest.raises(ValueError, match="radec must be"):
        fftvis_amd.torch_simulate_vis_basis_sky(F, C, P[:, :1], **kw)


def test_engine_route_checks_its_mode():
    from fftvis_amd.gpu.gpu_simulate import GPUSimulationEngine

    cfg = basis_source_config()
    kw = {k: v for k, v in cfg.items() if k != "beam"}
    eng = GPUSimulationEngine()
    for bad, match, extra in ((("gradient", None, None), "basis_source_of", {}),
                              (("adjoint", None, None), "needs basis beams", {"beam_coefs": None}),
                              (("adjoint", None, None), "pass one of", {"tangent_of": (None, None, None)})):
        with pytest.raises(ValueError, match=match):
            eng.simulate(beam_list=cfg["beam"], **dict(kw, **extra), basis_source_of=bad)


# ---- the references ----------------------------------------------------------------------------------------------------
def test_every_table_cell_keeps_its_sources_off_the_horizon_and_the_knot_lines():
    """The condition the differences rely on, for every configuration with a table that a test of either module uses:
    both margins above 1e-3 rad at the order the cell interpolates at.  Nothing is excluded from a comparison."""
    seen = 0
    for heights, tables, sky, compat in matrix_cells():
        cfg = basis_source_config(heights, tables, sky, compat)
        assert margins(cfg)[0] > 1e-3, (heights, tables)
        if tables != "airy":
            assert knot_margin(cfg, 1) > 1e-3, (heights, tables, knot_margin(cfg, 1))
            seen += 1
    assert seen == 24
    for cfg in (order0_reference()[0], mixed_order0_config()):
        assert margins(cfg)[0] > 1e-3 and knot_margin(cfg, 0) > 1e-3, (margins(cfg), knot_margin(cfg, 0))
    # torch's gradcheck compares the device with its own forward at a step of 1e-6 rad, no reference: its 8 sources stay
    # 100 steps (and 100 of the device's stencils) from a node, ``test_gpu_source_adjoint``'s condition for that shape
    cfg = gradcheck_basis_config()
    assert margins(cfg)[0] > 1e-3 and knot_margin(cfg, 1) > 1e-4, (margins(cfg), knot_margin(cfg, 1))
    for label, cfg in slicing_configs().items():  # order 3: C^2, no condition on the nodes
        assert cfg["beam_spline_opts"] == {"order": 3} and margins(cfg)[0] > 1e-3, label
    for cfg in (hex19_basis_config(), empty_step_basis_config()):  # Airy basis beams
        assert margins(cfg)[0] > 1e-3 and knot_margin(cfg, 1) == np.inf
    cfg = hera350_basis_source_config()
    assert margins(cfg)[0] > 1e-3 and knot_margin(cfg, 1) > 1e-3 and knot_margin(hera350_basis_config(), 1) < 1e-3
    # ... and the default catalogue seed would not do
    assert knot_margin(basis_source_config("cm", "complex", seed=0), 1) < 1e-3
    # the jump configuration is the exception by construction: two sources inside the device's stencil of a jump, and no
    # differences in its reference
    cfg, mgr, rows = jump_basis_config()
    assert knot_margin(cfg, 0, coord_mgr=mgr) < 1e-6 and margins(cfg, coord_mgr=mgr)[0] > 1e-3 and len(rows) == 2


@pytest.mark.parametrize("cell", HOST_CELLS)
def test_extrapolations_from_two_step_pairs_agree(cell):
    cfg = basis_source_config(*cell)
    G, gref, dtopo, dref, _ = matrix_reference(*cell)
    h = sar.H_REF
    fine = exact_gtopo(cfg, G, sources=ROWS, h=0.5 * h)
    rows = gref[:, ROWS]
    assert np.count_nonzero(rows) > 0
    dg = rel_l2(fine[:, ROWS], rows)
    dv = rel_l2(exact_dv_topo(cfg, dtopo, h=0.5 * tr.H_REF)[0], dref)
    print("basis source references, (h, h/2) against (h/2, h/4)", cell, dg, dv)
    assert dg <= PIN and dv <= PIN


@pytest.mark.parametrize("cell", HOST_CELLS)
def test_the_two_references_are_transposes(cell):
    G, gtopo, dtopo, dv, _ = matrix_reference(*cell)
    lhs, rhs = np.vdot(G, dv).real, float(np.sum(dtopo * gtopo))
    scale = np.linalg.norm(G) * np.linalg.norm(dv)
    print("basis source references, dot identity", cell, abs(lhs - rhs) / scale)
    assert abs(lhs) > 1e-3 * scale and abs(lhs - rhs) <= PIN * scale


def test_order_0_closed_forms_equal_the_differences():
    cfg, G, gfrozen, dtopo, dfrozen, _ = order0_reference()
    dg = rel_l2(exact_gtopo(cfg, G), gfrozen)
    dv = rel_l2(exact_dv_topo(cfg, dtopo)[0], dfrozen)
    print("basis source references, order 0: frozen beams against differences", dg, dv)
    assert dg <= PIN and dv <= PIN
    # ... which is not so at order 1: the beam term is a share of the result
    cfg1 = basis_source_config("cm", "complex", "full", False)
    G1, g1, dt1, dv1, _ = matrix_reference("cm", "complex", "full", False)
    assert rel_l2(frozen_beam_gtopo(cfg1, G1), g1) > 1e-3 and rel_l2(frozen_beam_dv_topo(cfg1, dt1)[0], dv1) > 1e-3


@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
def test_one_unit_basis_beam_equals_the_plain_references(heights):
    cfg, plain = k1_configs(heights)
    G = random_complex(vis_shape(cfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    dg = rel_l2(exact_gtopo(cfg, G, sources=ROWS), sar.exact_gtopo(plain, G, sources=ROWS))
    dv = rel_l2(exact_dv_topo(cfg, dtopo)[0], tr.exact_dv_topo(plain, dtopo)[0])
    print("basis source references, K = 1 against the plain dish", heights, dg, dv)
    assert dg <= PIN and dv <= PIN


def test_radec_reference_is_the_chained_topo_reference():
    cfg = basis_source_config("cm", "complex", "full", False)
    G, gtopo = matrix_reference("cm", "complex", "full", False)[:2]
    chained = fftvis_amd.topo_to_radec_gradient(gtopo, sidereal_jacobian(cfg))
    d = rel_l2(chained[ROWS], exact_gradec(cfg, G, sources=ROWS)[ROWS])
    print("basis source references, (ra, dec) differences against the chained gradient", d)
    assert d <= PIN


def test_every_gpu_matrix_cell_is_well_conditioned():
    """What the GPU module's bounds rely on, on the references alone: the tangent's terms do not cancel (kappa <= 4 for the
    seed used) and no time step's gradient is negligible."""
    assert set(HOST_CELLS) <= set(matrix_cells())
    for cell in matrix_cells():
        _, gtopo, _, dv, terms = matrix_reference(*cell)
        assert kappa(dv, terms) <= KAPPA_MAX, (cell, kappa(dv, terms))
        assert all(np.linalg.norm(gtopo[t]) > 1e-2 * np.linalg.norm(gtopo) for t in range(gtopo.shape[0])), cell
    assert kappa(*order0_reference()[4:]) <= KAPPA_MAX


def test_phase_split_references_for_long_baselines():
    """``split_gtopo`` / ``split_dv_topo`` -- closed-form phase part plus differenced beam part -- equal the plain
    references on the hex-7 (to 1e-8, where both hold), and at HERA-350's size, where the plain ones carry (k h)^4 / 480 =
    4e-9, their own two step pairs agree to 2e-12: a fifth of the GPU test's bound of 10 eps = 1e-11 (measured 8e-13 and
    4e-13), and they are each other's transposes."""
    cell = ("cm", "complex", "full", False)
    cfg = basis_source_config(*cell)
    G, gref, dtopo, dref, _ = matrix_reference(*cell)
    dg, dv = rel_l2(split_gtopo(cfg, G), gref), rel_l2(split_dv_topo(cfg, dtopo)[0], dref)
    print("basis source references, phase-split against plain", dg, dv)
    assert dg <= PIN and dv <= PIN
    cfg = hera350_basis_source_config()
    sub = hera_subset(cfg)
    scfg = dict(cfg, baselines=[cfg["baselines"][i] for i in sub])
    G = random_complex(vis_shape(scfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    g, (dv, terms) = split_gtopo(scfg, G), split_dv_topo(scfg, dtopo)
    dg, dd = rel_l2(split_gtopo(scfg, G, h=0.5 * H_BEAM), g), rel_l2(split_dv_topo(scfg, dtopo, h=0.5 * H_BEAM)[0], dv)
    plain = rel_l2(exact_gtopo(scfg, G), g)
    dot = abs(np.vdot(G, dv).real - float(np.sum(dtopo * g))) / (np.linalg.norm(G) * np.linalg.norm(dv))
    print("basis source references at HERA-350's size: step pairs", dg, dd, "plain", plain, "dot", dot, "kappa", kappa(dv, terms))
    assert dg <= 2e-12 and dd <= 2e-12 and dot <= 2e-12 and kappa(dv, terms) <= KAPPA_MAX
    assert plain > 1e-10  # the plain reference would not do here
