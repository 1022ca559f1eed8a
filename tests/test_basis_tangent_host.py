"""CPU tests of the basis-beam tangent's host side (``simulate_vis_basis_jvp``, ``fv_sim_run_basis_tangent``): the exports,
the C entry point's argument checking, the Python argument errors that are raised before a device is needed, and the exact
reference the GPU tests compare with (``basis_adjoint_refs.exact_dv``), pinned here on the oracle.

The map is sesquilinear in the coefficients, V_b = sum_kl conj(C[a1,k]) C[a2,l] M_kl(b), so the derivative along D,
dV[C; D] = (V(C + D) - V(C - D)) / 2, is exact, equals the closed form sum_kl (conj(D1k) C2l + conj(C1k) D2l) M_kl with M
from ``basis_visibilities`` (whose M_lk is what each ``reference_compat`` form makes it), and satisfies dV[C; C] = 2 V,
dV[C; i C] = 0 and V(C + D) + V(C - D) - 2 V(C) - 2 V(D) = 0.  All four are held to 1e-9 relative on three cells of the GPU
matrix; measured: closed form 4e-16, dV[C; C] - 2 V exactly 0, dV[C; i C] 1e-16 |V|, second-order residual 6e-16 |V|.
"""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.basis_adjoint_refs import basis_config, basis_visibilities, exact_dv, random_complex
from tests.helpers import oracle_simulate

REF_BOUND = 1e-9
CELLS = [("airy", True, "coplanar"), ("complex", False, "height_terms"), ("complex", True, "non_coplanar")]


def test_basis_tangent_is_exported():
    assert callable(fftvis_amd.simulate_vis_basis_jvp)
    assert "fv_sim_run_basis_tangent" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "fv_sim_run_basis_tangent")
    from fftvis_amd.gpu import gpu_simulate

    assert callable(gpu_simulate.SimHandle.run_basis_tangent)


def test_run_basis_tangent_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    fake = ctypes.c_void_p(1)
    call = L.fv_sim_run_basis_tangent
    assert call(None, 0, 1, 0, 1, buf, 0, 1, buf, 0) == 1
    assert b"null handle" in L.fv_last_error()
    for h in (None, fake):  # the buffers, the count and the flags are checked before the handle is looked at
        assert call(h, 0, 1, 0, 1, buf, 0, 1, None, 0) == 1
        assert b"null output" in L.fv_last_error()
        assert call(h, 0, 1, 0, 1, None, 0, 1, buf, 0) == 1
        assert b"dcoefs" in L.fv_last_error()
        for ndir in (0, -3):
            assert call(h, 0, 1, 0, 1, buf, 0, ndir, buf, 0) == 1
            assert b"ndir" in L.fv_last_error()
        for flags in [(2, 0), (-1, 0), (0, 3), (0, -1)]:
            assert call(h, 0, 1, 0, 1, buf, flags[0], 1, buf, flags[1]) == 1
            assert b"on_device" in L.fv_last_error()


def test_argument_errors_come_before_device_work():
    cfg = basis_config()
    call = fftvis_amd.simulate_vis_basis_jvp
    D = np.zeros((7, 3, 3), complex)
    for shape in [(7, 3, 2), (7, 2, 3), (6, 3, 3), (2, 7, 3, 2), (0, 7, 3, 3), (1, 2, 7, 3, 3)]:
        with pytest.raises(ValueError, match="d_beam_coefs must have"):
            call(**cfg, d_beam_coefs=np.zeros(shape, complex))
    with pytest.raises(ValueError, match="d_beam_coefs must be complex"):
        call(**cfg, d_beam_coefs=np.zeros((7, 3, 3)))
    for shape in [(24, 2), (23, 3), (24, 3, 4)]:
        with pytest.raises(ValueError, match="d_fluxes must have"):
            call(**cfg, d_fluxes=np.zeros(shape))
    with pytest.raises(ValueError, match="needs beam_coefs"):
        call(**dict(cfg, beam_coefs=None), d_beam_coefs=D)
    with pytest.raises(ValueError, match=r"beam_coefs must have shape \(nant, nbasis, nfreqs\)"):
        call(**dict(cfg, beam_coefs=np.ones((7, 2, 3), complex)), d_beam_coefs=D)
    with pytest.raises(ValueError, match="not compatible with unpolarized"):
        call(**dict(cfg, polarized=False), d_beam_coefs=D)
    with pytest.raises(ValueError, match="beam_idx should not be provided"):
        call(**dict(cfg, beam_idx=np.zeros(7, int)), d_beam_coefs=D)
    with pytest.raises(ValueError, match="not with a stack"):
        call(**cfg, d_beam_coefs=np.zeros((2, 7, 3, 3), complex), d_fluxes=np.zeros((24, 3)))
    with pytest.raises(ValueError, match="backend"):
        call(**cfg, d_beam_coefs=D, backend="cpu")
    with pytest.raises(ValueError, match="fluxes must have shape"):
        call(**dict(cfg, fluxes=np.ones((5, 3))), d_beam_coefs=D)
    # no input at all: zeros of simulate_vis's shape and dtype, and no device work
    z = call(**cfg)
    assert z.shape == (3, 2, 2, 2, len(cfg["baselines"])) and z.dtype == np.complex128 and not z.any()
    assert call(**dict(cfg, precision=1)).dtype == np.complex64


def test_torch_operation_documents_its_jvp():
    doc = fftvis_amd.torch_simulate_vis_basis.__doc__
    assert "simulate_vis_basis_jvp" in doc and "defines no" not in doc


@pytest.mark.parametrize("tables,compat,array", CELLS)
def test_reference_pins_on_the_oracle(tables, compat, array):
    cfg = basis_config(tables, "full", compat, array, nsrc=8)
    C = cfg["beam_coefs"]
    V = oracle_simulate(cfg)
    nV = np.linalg.norm(V)
    D = random_complex(C.shape, 31)
    dv = exact_dv(cfg, D)
    assert np.linalg.norm(dv) > 0.1 * nV
    # the closed form, M_lk as this form of the forward defines it
    M = basis_visibilities(cfg)
    a1 = [list(cfg["ants"]).index(p) for p, _ in cfg["baselines"]]
    a2 = [list(cfg["ants"]).index(q) for _, q in cfg["baselines"]]
    closed = (np.einsum("bkf,blf,klftpqb->ftpqb", np.conj(D[a1]), C[a2], M)
              + np.einsum("bkf,blf,klftpqb->ftpqb", np.conj(C[a1]), D[a2], M))
    d = np.linalg.norm(closed - dv) / np.linalg.norm(dv)
    same = np.linalg.norm(exact_dv(cfg, C) - 2 * V) / nV
    quarter = np.linalg.norm(exact_dv(cfg, 1j * C)) / nV
    second = np.linalg.norm(oracle_simulate(dict(cfg, beam_coefs=C + D)) + oracle_simulate(dict(cfg, beam_coefs=C - D))
                            - 2 * V - 2 * oracle_simulate(dict(cfg, beam_coefs=D))) / nV
    print("basis tangent reference", (tables, compat, array), "closed form", d, "dV[C;C]-2V", same, "dV[C;iC]", quarter,
          "second order", second)
    assert d <= REF_BOUND and same <= REF_BOUND and quarter <= REF_BOUND and second <= REF_BOUND
