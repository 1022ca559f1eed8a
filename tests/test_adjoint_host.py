"""CPU tests of the adjoint's host logic: argument checks that come before any device work, the transpose of the
Stokes -> coherency conversion, and the C entry point's argument checking."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from fftvis_amd.adjoint import stokes_adjoint
from fftvis_amd.core import utils


def _cfg():
    c = synth.make_config("C1", nsrc=20, nfreq=3, ntimes=2)
    return {k: v for k, v in c.items() if k != "fluxes"}


def test_adjoint_is_exported():
    assert callable(fftvis_amd.simulate_vis_adjoint) and callable(fftvis_amd.torch_simulate_vis)
    assert "fv_sim_run_adjoint" in _lib.SYMBOLS


@pytest.mark.parametrize("shape", [(3, 2, 20), (3, 2, 2, 2, 21), (2, 3, 21), (3, 2, 22)])
def test_wrongly_shaped_vis_raises_before_device_work(shape):
    cfg = _cfg()
    assert len(cfg["baselines"]) == 21
    with pytest.raises(ValueError, match="output shape"):
        fftvis_amd.simulate_vis_adjoint(np.zeros(shape, complex), **cfg)
    with pytest.raises(ValueError, match="output shape"):
        fftvis_amd.simulate_vis_adjoint(np.zeros((3, 2, 21), complex), **dict(cfg, polarized=True))


def test_basis_beams_and_full_stokes_without_polarization_are_refused():
    cfg = _cfg()
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.simulate_vis_adjoint(np.zeros((3, 2, 2, 2, 21), complex), **dict(cfg, polarized=True),
                                        beam_coefs=np.ones((7, 1, 3)))
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.torch_simulate_vis(None, **dict(cfg, beam_coefs=np.ones((7, 1, 3))))
    with pytest.raises(ValueError, match="polarized"):
        fftvis_amd.simulate_vis_adjoint(np.zeros((3, 2, 21), complex), **cfg, full_stokes=True)


@pytest.mark.parametrize("full", [False, True])
def test_stokes_adjoint_is_the_transpose_of_prepare_source_catalog(full):
    """Re sum conj(Gc) C(S) = <S, stokes_adjoint(Gc)> for real S (C = the coherency the engine is given)."""
    rng = np.random.default_rng(1)
    S = rng.normal(size=(6, 3, 4) if full else (6, 3))
    C, pol_sky = utils.prepare_source_catalog(S, polarized_beam=True)
    assert pol_sky == full
    Gc = rng.normal(size=C.shape) + (1j * rng.normal(size=C.shape) if full else 0)
    lhs = np.sum(np.conj(Gc) * C).real
    rhs = np.sum(S * stokes_adjoint(Gc, full))
    assert np.isclose(lhs, rhs, rtol=1e-13, atol=0)
    assert stokes_adjoint(Gc, full).shape == S.shape


def test_run_adjoint_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()
    assert L.fv_sim_run_adjoint(None, 0, 1, 0, 1, buf, 0, buf, 0, 0) == 1
    assert b"handle" in L.fv_last_error()
    assert L.fv_sim_run_adjoint(None, 0, 1, 0, 1, None, 0, buf, 0, 0) == 1
    assert b"null adjoint" in L.fv_last_error()
    assert L.fv_sim_run_adjoint(None, 0, 1, 0, 1, buf, 3, buf, 0, 0) == 1
    assert b"on_device" in L.fv_last_error()
