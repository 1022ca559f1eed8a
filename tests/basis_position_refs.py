"""Configurations and exact references for the position derivatives through basis beams (``simulate_vis_basis_adjoint`` with
``wrt="ants" / "baselines"``, ``simulate_vis_basis_jvp`` with ``d_ants`` / ``d_baselines``,
``fv_sim_run_basis_position_adjoint`` / ``_tangent``).

With V_b = sum_kl conj(C[a1,k]) C[a2,l] M_kl(b) every M_kl is a sum over sources of strengths that do not depend on the
positions times exp(2 pi i nu s_b b . topo_j / c), so dV_b / db_d = i (2 pi nu / c) D_d with D_d the BASIS forward of the
fluxes times topo_d: the formulas of ``position_adjoint_refs.exact_gbls`` and ``tangent_refs.exact_dv_baselines``, which
forward ``beam_coefs`` to the oracle with the rest of the configuration.  ``test_basis_position_host`` pins them against
Richardson-extrapolated central differences of the oracle's basis forward.
"""

import functools

import numpy as np

import fftvis_amd
from fftvis_amd import synth
from tests.basis_adjoint_refs import basis_config, random_complex  # noqa: F401
from tests.position_adjoint_refs import exact_gbls, hex_positions, perturbed_hex7, vis_shape  # noqa: F401
from tests.tangent_refs import (DB_SEED, empty_step_config, exact_dv_baselines, hera_subset, hex19_config, kappa,  # noqa: F401
                                random_dbls)

G_SEED = 4
HEIGHTS = ("flat", "cm", "m")
TABLES = ("airy", "real", "complex")


def position_baselines():
    """The position matrix's list: every pair with the autos, plus the flipped (3, 1) and (6, 0)."""
    return [(i, j) for i in range(7) for j in range(i, 7)] + [(3, 1), (6, 0)]


def basis_position_config(heights="flat", tables="airy", sky="I", compat=True, precision=2, **kw):
    """``basis_config(tables, sky, compat)`` (24 sources, 3 channels, 2 times, K = 3) on the perturbed hex-7 of the
    position tests with their baseline list."""
    cfg = basis_config(tables, sky, compat, precision=precision, **kw)
    cfg["ants"] = perturbed_hex7(heights)
    cfg["baselines"] = position_baselines()
    return cfg


def edge_config(**kw):
    """Centimetre heights (height terms), complex tables, full-Stokes sky, the exact form of the (l, k) terms, fp64."""
    return basis_position_config("cm", "complex", "full", False, 2, **kw)


def matrix_cells():
    return [(h, t, s, c) for h in HEIGHTS for t in TABLES for s in ("I", "full") for c in (True, False)]


@functools.lru_cache(maxsize=None)
def matrix_reference(heights, tables, sky, compat):
    """(G, gbls, dbls, dV, terms) of a matrix cell; the references do not depend on the run's precision."""
    cfg = basis_position_config(heights, tables, sky, compat)
    G = random_complex(vis_shape(cfg), G_SEED)
    dbls = random_dbls(cfg, DB_SEED)
    dv, terms = exact_dv_baselines(cfg, dbls)
    return G, exact_gbls(cfg, G), dbls, dv, terms


def hex19_basis_config():
    """The exact hex-19 of the tangent tests with K = 2 Airy basis beams and random coefficients."""
    cfg = hex19_config()
    nf = len(cfg["freqs"])
    rng = np.random.default_rng(9)
    cfg.update(beam=[fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(10.0)],
               beam_coefs=rng.normal(size=(19, 2, nf)) + 1j * rng.normal(size=(19, 2, nf)))
    cfg.pop("force_use_type3", None)
    return cfg


def empty_step_basis_config():
    """``tangent_refs.empty_step_config``'s sky and times (nothing above the horizon at the last time) on the edge cell."""
    src = empty_step_config()
    cfg = edge_config(nsrc=20, ntimes=3)
    cfg.update(ra=src["ra"], dec=src["dec"], times=src["times"])
    return cfg


def hera350_basis_config():
    """``test_gpu_position_adjoint._hera350("hermitian")``'s shape (61 075 baselines, 64 sources, 2 channels, 1 time, eps
    1e-12) with K = 2 real-valued tables and random coefficients."""
    from tests.test_gpu_position_adjoint import _hera350

    cfg = _hera350("hermitian")
    freqs = cfg["freqs"]
    tabs = [synth.synthetic_efield_table(freqs, d, nza=91, naz=180).real.astype(complex) for d in (14.0, 11.0)]
    rng = np.random.default_rng(13)
    cfg.update(beam=[fftvis_amd.TabulatedBeam(t, freqs) for t in tabs],
               beam_coefs=rng.normal(size=(350, 2, len(freqs))) + 1j * rng.normal(size=(350, 2, len(freqs))))
    cfg.pop("beam_idx", None)
    return cfg


def k1_configs(heights="cm"):
    """(basis, plain): one Airy basis beam with every coefficient 1, and the same dish without ``beam_coefs``."""
    cfg = basis_position_config(heights, "airy", "full", True)
    cfg.update(beam=[fftvis_amd.AiryBeam(14.0)], beam_coefs=np.ones((7, 1, len(cfg["freqs"])), dtype=complex), eps=1e-12)
    plain = {k: v for k, v in cfg.items() if k != "beam_coefs"}
    plain["beam"] = fftvis_amd.AiryBeam(14.0)
    return cfg, plain
