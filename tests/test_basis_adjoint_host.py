"""CPU tests of the basis-beam gradients' host side: the exports, argument checks that come before any device work,
the C entry point's argument checking, and the exact references the GPU tests compare with (``basis_adjoint_refs``),
pinned here against the oracle where there is no GPU."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.basis_adjoint_refs import (basis_config, basis_visibilities, closed_form_gcoefs, exact_dv, exact_gcoefs,
                                      exact_gflux, random_complex)
from tests.helpers import oracle_simulate, rel_l2


def test_basis_adjoint_is_exported():
    assert callable(fftvis_amd.simulate_vis_basis_adjoint) and callable(fftvis_amd.torch_simulate_vis_basis)
    assert "fv_sim_run_basis_adjoint" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "fv_sim_run_basis_adjoint")


def test_argument_errors_come_before_device_work():
    cfg = basis_config()
    nbls = len(cfg["baselines"])
    good = np.zeros((3, 2, 2, 2, nbls), complex)
    for shape in [(3, 2, nbls), (3, 2, 2, 2, nbls - 1), (2, 3, 2, 2, nbls)]:
        with pytest.raises(ValueError, match="output shape"):
            fftvis_amd.simulate_vis_basis_adjoint(np.zeros(shape, complex), **cfg)
    with pytest.raises(ValueError, match=r"beam_coefs must have shape \(nant, nbasis, nfreqs\)"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **dict(cfg, beam_coefs=np.ones((7, 2, 3), complex)))
    with pytest.raises(ValueError, match="not compatible with unpolarized"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **dict(cfg, polarized=False))
    with pytest.raises(ValueError, match="beam_idx should not be provided"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **dict(cfg, beam_idx=np.zeros(7, int)))
    with pytest.raises(ValueError, match="needs beam_coefs"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **dict(cfg, beam_coefs=None))
    with pytest.raises(ValueError, match="wrt"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **cfg, wrt=("fluxes", "positions"))
    with pytest.raises(ValueError, match="wrt"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **cfg, wrt=())
    with pytest.raises(ValueError, match="fluxes must have shape"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **dict(cfg, fluxes=np.ones((5, 3))))
    with pytest.raises(ValueError, match="full_stokes"):
        fftvis_amd.simulate_vis_basis_adjoint(good, **cfg, full_stokes=True)


def test_run_basis_adjoint_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()
    assert L.fv_sim_run_basis_adjoint(None, 0, 1, 0, 1, buf, 0, buf, 0, buf, 0, 0) == 1
    assert b"handle" in L.fv_last_error()
    assert L.fv_sim_run_basis_adjoint(None, 0, 1, 0, 1, None, 0, buf, 0, buf, 0, 0) == 1
    assert b"null adjoint" in L.fv_last_error()
    assert L.fv_sim_run_basis_adjoint(None, 0, 1, 0, 1, buf, 0, None, 0, None, 0, 0) == 1
    assert b"neither gradient" in L.fv_last_error()
    for flags in [(3, 0, 0), (0, 2, 0), (0, 0, -1)]:
        assert L.fv_sim_run_basis_adjoint(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], buf, flags[2], 0) == 1
        assert b"on_device" in L.fv_last_error()
    # one output alone is a valid request: the call gets as far as the handle
    assert L.fv_sim_run_basis_adjoint(None, 0, 1, 0, 1, buf, 0, None, 0, buf, 0, 0) == 1
    assert b"handle" in L.fv_last_error()


@pytest.mark.parametrize("compat", [True, False])
def test_references_satisfy_the_identities_on_the_oracle(compat):
    """The yardstick of the GPU tests: on the oracle, with complex tables (the two forms of the forward differ), a
    full-Stokes sky, a flipped pair and an auto -- V is an exact quadratic form in C; Re <G, dV[C; D]> = Re <gcoefs, D>
    for a random D with gcoefs built element by element; the closed form the device evaluates, from oracle-made M_kl,
    agrees with it; and <F, A^T G> = Re <A F, G> with A^T G built column by column.  All to 1e-12."""
    cfg = basis_config(tables="complex", sky="full", compat=compat, nsrc=6)
    C = cfg["beam_coefs"]
    V = oracle_simulate(cfg)
    G = random_complex(V.shape, 21)
    D = random_complex(C.shape, 22)
    quad = (oracle_simulate(dict(cfg, beam_coefs=C + D)) + oracle_simulate(dict(cfg, beam_coefs=C - D)) - 2 * V
            - 2 * oracle_simulate(dict(cfg, beam_coefs=D)))
    assert np.linalg.norm(quad) <= 1e-12 * np.linalg.norm(V)
    gc = exact_gcoefs(cfg, G)
    assert np.isfinite(gc).all() and np.count_nonzero(gc) == gc.size
    lhs = np.vdot(G, exact_dv(cfg, D)).real
    rhs = np.vdot(gc, D).real
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(G) * np.linalg.norm(exact_dv(cfg, D)), (lhs, rhs)
    M = basis_visibilities(cfg)
    a1 = [list(cfg["ants"]).index(p) for p, _ in cfg["baselines"]]
    a2 = [list(cfg["ants"]).index(q) for _, q in cfg["baselines"]]
    Vm = np.einsum("bkf,blf,klftpqb->ftpqb", np.conj(C[a1]), C[a2], M)
    assert rel_l2(Vm, V) <= 1e-12
    if compat:  # the reference's form: M_lk = M_kl^T (feed axes swapped)
        assert rel_l2(M[1, 0], np.swapaxes(M[0, 1], 2, 3)) <= 1e-12
    assert rel_l2(closed_form_gcoefs(cfg, G, M), gc) <= 1e-12
    F = np.random.default_rng(23).normal(size=cfg["fluxes"].shape)
    gf = exact_gflux(cfg, G)
    assert np.count_nonzero(gf) > 0
    lhs = np.vdot(G, oracle_simulate(dict(cfg, fluxes=F))).real
    assert abs(lhs - np.sum(F * gf)) <= 1e-12 * np.linalg.norm(G) * np.linalg.norm(V)


def test_the_two_forms_differ_for_complex_tables_only():
    """What makes ``reference_compat=False`` testable: with complex tables the two forms of the forward differ by tens
    of per cent, with real ones they are the same map."""
    for tables, differ in (("complex", True), ("real", False)):
        cfg = basis_config(tables=tables, nsrc=6)
        a, b = oracle_simulate(cfg), oracle_simulate(dict(cfg, reference_compat=False))
        assert (rel_l2(a, b) > 0.05) == differ, (tables, rel_l2(a, b))
