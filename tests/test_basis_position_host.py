"""CPU tests of the position derivatives through basis beams: the exports, the C entry points' argument checking, the Python
argument errors that are raised before a device is needed, and the exact references the GPU tests compare with
(``position_adjoint_refs.exact_gbls`` and ``tangent_refs.exact_dv_baselines`` on a configuration with ``beam_coefs``),
pinned here on the oracle's basis forward.

Measured: ``exact_gbls`` scattered to the antennas against Richardson-extrapolated central differences (h = 1e-3 m) of
the oracle, relative to max |g|, 2e-12 ... 8e-12 over the twelve cells (bound 1e-9, ``test_position_adjoint_host``'s);
|Re <dV, G> - sum dbls . gbls| 2e-16 of the product (bound 1e-12); kappa of the tangent reference 1.13 ... 1.14; the up
component 97 - 98 % of |gbls|.
"""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.basis_position_refs import (DB_SEED, G_SEED, basis_position_config, exact_dv_baselines, exact_gbls,
                                       hera350_basis_config, hera_subset, kappa, matrix_cells, matrix_reference,
                                       random_complex, random_dbls, vis_shape)
from tests.helpers import oracle_simulate

FD_BOUND = 1e-9
KAPPA_MAX = 4.0
# (antenna, component) entries differenced per cell: the up component on two antennas, east and north on others
FD_ENTRIES = [(0, 2), (3, 2), (1, 0), (4, 1)]
FD_CELLS = [(h, t, "full" if t == "complex" else "I", c) for h in ("flat", "cm", "m") for t in ("airy", "complex")
            for c in (True, False)]


def test_basis_position_passes_are_exported():
    assert callable(fftvis_amd.torch_simulate_vis_basis_array)
    from fftvis_amd.gpu import gpu_simulate

    for sym, method in (("fv_sim_run_basis_position_adjoint", "run_basis_position_adjoint"),
                        ("fv_sim_run_basis_position_tangent", "run_basis_position_tangent")):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)
        assert callable(getattr(gpu_simulate.SimHandle, method))


def test_c_entry_points_check_their_arguments():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    fake = ctypes.c_void_p(1)
    adj, tan = L.fv_sim_run_basis_position_adjoint, L.fv_sim_run_basis_position_tangent
    assert adj(None, 0, 1, 0, 1, buf, 0, buf, 0, 0) == 1
    assert b"null handle" in L.fv_last_error()
    assert tan(None, 0, 1, 0, 1, buf, 0, buf, 0) == 1
    assert b"null handle" in L.fv_last_error()
    for h in (None, fake):  # the buffers and the flags are checked before the handle is looked at
        for g, b in [(None, buf), (buf, None)]:
            assert adj(h, 0, 1, 0, 1, g, 0, b, 0, 0) == 1
            assert b"null adjoint input or output" in L.fv_last_error()
        for flags in [(2, 0, 0), (0, -1, 0)]:
            assert adj(h, 0, 1, 0, 1, buf, flags[0], buf, flags[1], 0) == 1
            assert b"on_device" in L.fv_last_error()
        for acc in (2, -1):
            assert adj(h, 0, 1, 0, 1, buf, 0, buf, 0, acc) == 1
            assert b"accumulate" in L.fv_last_error()
        assert tan(h, 0, 1, 0, 1, buf, 0, None, 0) == 1
        assert b"null output" in L.fv_last_error()
        assert tan(h, 0, 1, 0, 1, None, 0, buf, 0) == 1
        assert b"dbls" in L.fv_last_error()
        for flags in [(2, 0), (-1, 0), (0, 3), (0, -1)]:
            assert tan(h, 0, 1, 0, 1, buf, flags[0], buf, flags[1]) == 1
            assert b"on_device" in L.fv_last_error()


def test_argument_errors_come_before_device_work():
    import torch

    cfg = basis_position_config()
    nbls = len(cfg["baselines"])
    G = np.zeros(vis_shape(cfg), complex)
    adj, jvp = fftvis_amd.simulate_vis_basis_adjoint, fftvis_amd.simulate_vis_basis_jvp
    for wrt in (("fluxes", "positions"), (), ("ants", "ants"), "antennas"):
        with pytest.raises(ValueError, match="wrt"):
            adj(G, **cfg, wrt=wrt)
    with pytest.raises(ValueError, match="vis must have"):
        adj(G[:1], **cfg, wrt="ants")
    da, db = np.zeros((7, 3)), np.zeros((nbls, 3))
    with pytest.raises(ValueError, match="d_ants or as d_baselines"):
        jvp(**cfg, d_ants=da, d_baselines=db)
    for kw in (dict(d_ants=np.zeros((6, 3))), dict(d_ants=np.zeros((7, 2))), dict(d_baselines=np.zeros((nbls, 2))),
               dict(d_baselines=np.zeros((nbls + 1, 3)))):
        with pytest.raises(ValueError, match="must have shape"):
            jvp(**cfg, **kw)
    stack = np.zeros((2, 7, 3, 3), complex)
    for kw in (dict(d_ants=da), dict(d_baselines=db)):
        with pytest.raises(ValueError, match="stack"):
            jvp(**cfg, d_beam_coefs=stack, **kw)
    with pytest.raises(ValueError, match="backend"):
        jvp(**cfg, d_ants=da, backend="cpu")
    # no input at all: zeros of simulate_vis's shape and dtype, and no device work
    z = jvp(**cfg)
    assert z.shape == vis_shape(cfg) and z.dtype == np.complex128 and not z.any()
    # the non-basis entry points keep refusing beam_coefs
    plain = {k: v for k, v in cfg.items() if k != "beam_coefs"}
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.simulate_vis_position_adjoint(G, **cfg)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.simulate_vis_jvp(**cfg, d_ants=da)
    kw = {k: v for k, v in plain.items() if k not in ("fluxes", "ants")}
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128)
    P = torch.tensor(np.array(list(cfg["ants"].values())), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.torch_simulate_vis_array(F, P, beam_coefs=cfg["beam_coefs"], **kw)
    with pytest.raises(TypeError, match="antpos"):
        fftvis_amd.torch_simulate_vis_basis_array(F, C, P, ants=cfg["ants"], **kw)
    with pytest.raises(ValueError, match="antpos must be"):
        fftvis_amd.torch_simulate_vis_basis_array(F, C, P[:, :2], **kw)
    with pytest.raises(ValueError, match="antnums"):
        fftvis_amd.torch_simulate_vis_basis_array(F, C, P, antnums=[0, 1, 2], **kw)


def _fd_entry(cfg, G, a, d, h=1e-3):
    """dL/d ants[a][d], L = Re <G, V(ants)>, by Richardson-extrapolated central differences of the oracle's basis forward."""

    def loss(step):
        ants = {k: np.array(v, dtype=float) for k, v in cfg["ants"].items()}
        ants[a][d] += step
        return np.vdot(G, oracle_simulate(dict(cfg, ants=ants))).real

    def central(step):
        return (loss(step) - loss(-step)) / (2 * step)

    return (4 * central(0.5 * h) - central(h)) / 3


@pytest.mark.parametrize("heights,tables,sky,compat", FD_CELLS)
def test_gradient_reference_equals_finite_differences_of_the_oracle(heights, tables, sky, compat):
    """``exact_gbls`` on a basis configuration, scattered to the antennas, against differences of the oracle's basis forward
    on four (antenna, component) entries, two of them the up component; full-Stokes sky on the complex tables."""
    cfg = basis_position_config(heights, tables, sky, compat)
    G, gbls = matrix_reference(heights, tables, sky, compat)[:2]
    gants = fftvis_amd.baseline_to_antenna_gradient(gbls, cfg["ants"], cfg["baselines"])
    scale = np.abs(gants).max()
    worst = 0.0
    for a, d in FD_ENTRIES:
        fd = _fd_entry(cfg, G, a, d)
        assert fd != 0.0
        worst = max(worst, abs(gants[a, d] - fd) / scale)
    print("basis position reference vs finite differences", heights, tables, compat, worst)
    assert worst <= FD_BOUND, worst


HOST_CELLS = [("flat", "airy", "I", True), ("cm", "complex", "full", False), ("m", "real", "I", True),
              ("cm", "complex", "full", True)]


@pytest.mark.parametrize("cell", HOST_CELLS)
def test_the_two_references_are_transposes(cell):
    G, gbls, dbls, dv, _ = matrix_reference(*cell)
    lhs, rhs = np.vdot(G, dv).real, float(np.sum(dbls * gbls))
    scale = np.linalg.norm(G) * np.linalg.norm(dv)
    print("basis position references, dot identity", cell, abs(lhs - rhs) / scale)
    assert abs(lhs - rhs) <= 1e-12 * scale


def test_every_gpu_matrix_cell_is_well_conditioned():
    """What the GPU module's bounds rely on, on the references alone: the tangent's three terms do not cancel
    (kappa <= 4 for the seed used) and the up component of the gradient is not negligible."""
    assert set(FD_CELLS + HOST_CELLS) <= set(matrix_cells())
    for cell in matrix_cells():
        _, gbls, _, dv, terms = matrix_reference(*cell)
        assert kappa(dv, terms) <= KAPPA_MAX, (cell, kappa(dv, terms))
        assert np.linalg.norm(gbls[:, 2]) > 1e-3 * np.linalg.norm(gbls), cell


def test_hera350_subset_is_well_conditioned():
    cfg = hera350_basis_config()
    sub = hera_subset(cfg)
    G = random_complex(vis_shape(cfg), G_SEED)
    gb = exact_gbls(cfg, G, sub=sub)
    dv, terms = exact_dv_baselines(cfg, random_dbls(cfg, DB_SEED)[sub], sub=sub)
    assert kappa(dv, terms) <= KAPPA_MAX
    assert np.linalg.norm(gb[:, 2]) > 1e-3 * np.linalg.norm(gb)
