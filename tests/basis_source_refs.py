"""Configurations and exact references for the source-position derivatives through basis beams
(``simulate_vis_basis_source_adjoint``, ``simulate_vis_basis_source_jvp``, ``torch_simulate_vis_basis_sky``,
``fv_sim_run_basis_source_adjoint`` / ``_tangent``), built from the oracle's basis FORWARD alone.

The gradient: ``source_adjoint_refs.exact_gtopo`` / ``frozen_beam_gtopo`` / ``exact_gradec`` -- Richardson-extrapolated
central differences of L_tj(n) = Re <G[:, t], V_j(n)>, V_j the oracle's run of source j alone at one time with its vector
given, and the closed form with the strengths held fixed -- with a one-source runner that hands ``beam_coefs`` to the
oracle (``_OneSourceBasis``; that module's own runner does not).  The tangent: ``tangent_refs.exact_dv_topo`` /
``frozen_beam_dv_topo``, which go through ``helpers.oracle_simulate`` and so forward ``beam_coefs`` as they are.  The two
are built independently -- one source at a time against all sources at once -- and ``test_basis_source_host`` pins each
and their transpose identity.

The tables of ``basis_config`` are bilinear (no ``beam_spline_opts``: order 1), so the differences need every
above-horizon source away from the nodes of the tables: the catalogue seed is ``SEED`` = 3, for which the horizon margin
is 1.2e-2 rad and the knot margin 2.3e-3 rad at order 1 and 1.3e-3 rad at orders 0 and 2 (``basis_config``'s default seed
0 leaves 1.9e-4 rad at order 1).  The host test asserts both margins above 1e-3 rad for every table cell used: nothing is
excluded from a comparison.
"""

import functools

import numpy as np

import fftvis_amd
from fftvis_amd import synth
from oracle import fftvis_oracle as orc
from tests import source_adjoint_refs as sar
from tests.basis_position_refs import (HEIGHTS, TABLES, basis_position_config, hera350_basis_config,  # noqa: F401
                                       hex19_basis_config, matrix_cells)
from tests.position_adjoint_refs import _TopoAt, random_complex, vis_shape  # noqa: F401
from tests.source_adjoint_refs import GivenTopo, knot_margin, margins, sidereal_jacobian  # noqa: F401
from tests.tangent_refs import (DT_SEED, empty_step_config, exact_dv_topo, frozen_beam_dv_topo, kappa,  # noqa: F401
                                random_dtopo)

SEED = 3   # catalogue seed: nothing within 1e-3 rad of the horizon or of a knot line of the tables at orders 0, 1, 2
G_SEED = 4


class _OneSourceBasis(sar._OneSource):
    """``source_adjoint_refs._OneSource`` on a configuration with basis beams: the same one-source run of the oracle
    with ``beam_coefs`` handed over."""

    def vis(self, t, j, n):
        cfg = self.cfg
        flux = self.fluxes[j:j + 1]
        coh = orc.prepare_source_catalog(flux, cfg["polarized"])[0]
        mgr = _TopoAt(coh, t, cfg["telescope_loc"], self.ra[j:j + 1], self.dec[j:j + 1], np.asarray(n, float).reshape(3, 1))
        V = orc.simulate(cfg["ants"], cfg["freqs"], flux, self.ob, self.ra[j:j + 1], self.dec[j:j + 1], np.array([t]),
                         cfg["telescope_loc"], baselines=cfg.get("baselines"), polarized=cfg["polarized"],
                         beam_coefs=cfg["beam_coefs"], force_use_type3=True,
                         reference_compat=cfg.get("reference_compat", True), coord_mgr=mgr)
        return V[:, 0]


def _with_basis_runner(fn):
    """``fn`` of ``source_adjoint_refs`` with ``_OneSourceBasis`` in the place of its one-source runner.  Those functions
    construct their runner by the module-level name ``_OneSource`` and take no runner argument (and that module stays as
    it is), so the name is rebound for the duration of the call and restored in ``finally``: not re-entrant, which the
    single-threaded tests do not need.  A swap that silently did not take place would hand ``beam_idx=None`` runs of the K
    beams to the oracle; ``test_basis_source_host`` would fail its K = 1, order-0 and transpose pins."""

    @functools.wraps(fn)
    def run(cfg, *args, **kw):
        assert cfg.get("beam_coefs") is not None
        plain = sar._OneSource
        sar._OneSource = _OneSourceBasis
        try:
            return fn(cfg, *args, **kw)
        finally:
            sar._OneSource = plain

    return run


exact_gtopo = _with_basis_runner(sar.exact_gtopo)
frozen_beam_gtopo = _with_basis_runner(sar.frozen_beam_gtopo)
exact_gradec = _with_basis_runner(sar.exact_gradec)


def basis_source_config(heights="flat", tables="airy", sky="I", compat=True, precision=2, order=None, **kw):
    """``basis_position_config`` -- the perturbed hex-7, 24 sources, 3 channels, 2 times, K = 3, every pair with the autos
    and two flipped baselines -- at catalogue seed ``SEED``.  ``order``: the tables' spline order (default: bilinear)."""
    kw.setdefault("seed", SEED)
    cfg = basis_position_config(heights, tables, sky, compat, precision, **kw)
    if order is not None:
        cfg["beam_spline_opts"] = {"order": order}
    return cfg


def edge_config(**kw):
    """Centimetre heights (height terms), complex tables, full-Stokes sky, the exact form of the (l, k) terms, fp64."""
    return basis_source_config("cm", "complex", "full", False, 2, **kw)


@functools.lru_cache(maxsize=None)
def matrix_reference(heights, tables, sky, compat):
    """(G, gtopo, dtopo, dV, terms) of a matrix cell; the references do not depend on the run's precision."""
    cfg = basis_source_config(heights, tables, sky, compat)
    G = random_complex(vis_shape(cfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    dv, _, terms = exact_dv_topo(cfg, dtopo)
    return G, exact_gtopo(cfg, G), dtopo, dv, terms


@functools.lru_cache(maxsize=None)
def order0_reference(tables="complex"):
    """(cfg, G, gtopo, dtopo, dV, terms) at spline order 0 from the closed forms that hold the beams fixed: between two
    order-0 tables they are the whole derivative."""
    cfg = basis_source_config("cm", tables, "full", False, order=0)
    G = random_complex(vis_shape(cfg), G_SEED)
    dtopo = random_dtopo(cfg, DT_SEED)
    dv, terms = frozen_beam_dv_topo(cfg, dtopo)
    return cfg, G, frozen_beam_gtopo(cfg, G), dtopo, dv, terms


def jump_basis_config():
    """(cfg, manager, rows): ``source_adjoint_refs.jump_config``'s vectors -- at the first time one source 3e-7 rad from a za
    half-node line and one 3e-7 rad from an az half-node line, inside the device's 1e-6 rad stencil -- under the order-0
    edge cell.  The basis tables share ``order_config``'s grid (46 x 90 nodes to za = pi) and the catalogue its seed."""
    _, mgr, rows = sar.jump_config()
    cfg = basis_source_config("cm", "complex", "full", False, order=0)
    assert np.array_equal(cfg["ra"], sar.order_config(0)["ra"]) and np.array_equal(cfg["times"], mgr.times)
    return cfg, mgr, rows


def mixed_order0_config():
    """An Airy dish next to two order-0 tables: the (Airy, table) terms keep their differences (the dish's factor varies
    smoothly), the (table, table) terms have none."""
    cfg = basis_source_config("cm", "complex", "full", False, order=0)
    cfg["beam"] = [fftvis_amd.AiryBeam(14.0)] + cfg["beam"][1:]
    return cfg


def empty_step_basis_config():
    """``tangent_refs.empty_step_config``'s sky and times (nothing above the horizon at the last time) on the edge cell
    with Airy basis beams (the hand-placed catalogue is not held away from the tables' nodes)."""
    src = empty_step_config()
    cfg = basis_source_config("cm", "airy", "full", False, nsrc=20, ntimes=3)
    cfg.update(ra=src["ra"], dec=src["dec"], times=src["times"])
    return cfg


def k1_configs(heights="cm"):
    """(basis, plain): one Airy basis beam with every coefficient 1, and the same dish without ``beam_coefs``."""
    cfg = basis_source_config(heights, "airy", "full", True)
    cfg.update(beam=[fftvis_amd.AiryBeam(14.0)], beam_coefs=np.ones((7, 1, len(cfg["freqs"])), dtype=complex), eps=1e-12)
    plain = {k: v for k, v in cfg.items() if k != "beam_coefs"}
    plain["beam"] = fftvis_amd.AiryBeam(14.0)
    return cfg, plain


def gradcheck_basis_config():
    """``source_adjoint_refs.gradcheck_config``'s shape -- 8 sources, 1 channel (150 MHz), 1 time, 6 baselines, eps 1e-12,
    a bilinear table, the sidereal chain -- with K = 2: that table and an 11 m one, and random coefficients."""
    cfg = sar.gradcheck_config()
    freqs = cfg["freqs"]
    rng = np.random.default_rng(8)
    cfg.update(beam=[cfg["beam"], fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, 11.0, nza=46, naz=90), freqs)],
               beam_coefs=rng.normal(size=(7, 2, 1)) + 1j * rng.normal(size=(7, 2, 1)))
    return cfg


def hera350_basis_source_config():
    """``basis_position_refs.hera350_basis_config`` -- 61 075 baselines, 2 channels, 1 time, eps 1e-12, K = 2 real-valued
    bilinear tables on a 91 x 180 grid -- with its 64 sources chosen by condition: the first 64 of the 400-source catalogue
    that are more than 0.05 above the horizon (that configuration's rule) and more than 1e-3 rad from every node line of
    the tables (this module's: 64 rows picked by the first rule alone leave 2e-5 rad)."""
    cfg = hera350_basis_config()
    freqs = cfg["freqs"]
    c3 = synth.make_config("C3", nsrc=400, nfreq=2, ntimes=1)
    mgr = orc.SimpleCoordinateRotation(None, np.atleast_1d(cfg["times"]), cfg["telescope_loc"], c3["ra"], c3["dec"])
    mgr.setup()
    n = orc._topo_of(mgr, 0)
    n = n / np.linalg.norm(n, axis=0)
    az, za = orc.enu_to_az_za(n[0], n[1])
    nza, naz = cfg["beam"][0].data.shape[-2:]
    dz, da = cfg["beam"][0].za_max / (nza - 1), 2 * np.pi / naz
    dist = np.minimum(np.abs(za / dz - np.rint(za / dz)) * dz, np.abs(az / da - np.rint(az / da)) * da * np.sin(za))
    pick = np.flatnonzero((n[2] > 0.05) & (dist > 1e-3))[:64]
    assert len(pick) == 64
    _, _, flux = synth.catalog(400, freqs, 0, polarized_sky=True)
    cfg.update(ra=c3["ra"][pick], dec=c3["dec"][pick], fluxes=flux[pick])
    return cfg


def slicing_configs():
    """label -> configuration of the GPU module's slicing edges: the edge cell at other catalogue sizes.  Those catalogues
    are not held away from the tables' nodes, so the tables are interpolated at spline order 3 (C^2: the differences need
    no margin there); the horizon margin is asserted in ``test_basis_source_host``."""
    return {"chunks": dict(edge_config(nsrc=25, ntimes=4, order=3), min_chunks=2),
            "free lanes": dict(edge_config(nsrc=25, ntimes=5, order=3), min_chunks=2),
            "blocks": edge_config(nsrc=18, nfreq=5, order=3),
            "lanes": edge_config(nsrc=40, ntimes=4, order=3)}


# ---- references for long baselines ---------------------------------------------------------------------------------------
# The differences above run through the phase exp(2 pi i nu b . n / c): their Richardson remainder is (k h)^4 / 480,
# k = 2 pi nu |b| / c -- 1e-11 on the hex-7 (k <~ 300, h = 1e-5) but 4e-9 at HERA-350's 876 m (k = 3700), far above that
# test's eps of 1e-12, and a smaller step only trades it for rounding, 1e-16 / h.  One source's visibility is
# V_j[f, r, k](n) = A[f, r, k](n) exp(i kappa_f b_k . n), kappa_f = 2 pi nu_f / c and b_k the listed baseline's own vector
# (both forms of the (l, k) terms, whose mirrored half is conj(c) exp(+i kappa b . n)), with A moving through the beams
# alone, on the scale of a table cell, not of 1 / k.  So the derivative is the closed form with the beams held fixed
# (``frozen_beam_gtopo`` / ``frozen_beam_dv_topo``: exact) plus the derivative of A, taken by the same extrapolated
# differences on V_j(n') exp(-i kappa_f b_k . (n' - n)) at H_BEAM = 4e-4 rad (inside the 1e-3 rad margin to the nodes):
# the remainder, (h / cell)^4 / 480 = 4e-11 of the beam part on a 2 degree cell, and the rounding, which goes as 1 / h,
# both stay below 1e-12 of the whole, of which the beam part is 0.9 % at these baselines (``test_basis_source_host``:
# the results from (h, h/2) and (h/2, h/4) differ by 8e-13 at HERA-350's size; at h = 1e-4 by 3e-12, at 2.5e-5 by 6e-12).
H_BEAM = 4e-4


def _beam_part_runner(cfg, coord_mgr=None):
    times, mgr = sar._manager(cfg, coord_mgr)
    L = _OneSourceBasis(cfg, np.zeros(vis_shape(cfg)))
    b = sar.baseline_vectors(cfg)
    kf = 2 * np.pi * np.asarray(cfg["freqs"], dtype=float) / orc.speed_of_light

    def amplitude(t, j, n, at):
        """V_j(at) with the phase it has beyond the one at n taken out: (nf, 2, 2, nbls)."""
        ph = np.exp(-1j * kf[:, None] * (b @ (at - n))[None, :])
        return L.vis(t, j, at) * ph[:, None, None, :]

    def d_amplitude(t, j, n, e, h):
        def D(s):
            p, m = n + s * e, n - s * e
            return (amplitude(t, j, n, p / np.linalg.norm(p)) - amplitude(t, j, n, m / np.linalg.norm(m))) / (2.0 * s)

        return (4.0 * D(0.5 * h) - D(h)) / 3.0

    return times, mgr, d_amplitude


def split_gtopo(cfg, G, coord_mgr=None, h=H_BEAM):
    """``exact_gtopo``'s quantity as closed-form phase part plus differenced beam part (above)."""
    times, mgr, dA = _beam_part_runner(cfg, coord_mgr)
    G = np.asarray(G).astype(np.complex128)
    out = frozen_beam_gtopo(cfg, G, coord_mgr=coord_mgr)
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        for j in range(topo.shape[1]):
            n = topo[:, j] / np.linalg.norm(topo[:, j])
            if not n[2] > 0:
                continue
            for e in sar.tangent_pair(n):
                out[ti, j] += float(np.sum((np.conj(G[:, ti]) * dA(t, j, n, e, h)).real)) * e
    return out


def split_dv_topo(cfg, dtopo, coord_mgr=None, h=H_BEAM):
    """(dV, terms): ``exact_dv_topo``'s quantity as closed-form phase part plus differenced beam part, source by source;
    terms: the three phase terms and the beam part."""
    from tests.tangent_refs import project

    times, mgr, dA = _beam_part_runner(cfg, coord_mgr)
    phase, terms = frozen_beam_dv_topo(cfg, dtopo, coord_mgr=coord_mgr)
    beam = np.zeros_like(phase)
    for ti, t in enumerate(times):
        n, delta = project(orc._topo_of(mgr, ti), np.asarray(dtopo, dtype=float)[ti])
        for j in range(n.shape[0]):
            mag = float(np.linalg.norm(delta[j]))
            if mag > 0.0:
                beam[:, ti] += mag * dA(t, j, n[j], delta[j] / mag, h)
    return phase + beam, terms + [beam]
