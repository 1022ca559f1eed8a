"""Exact reference for the gradient with respect to the source directions, built from the oracle's FORWARD alone.

Every forward path approximates out[f, t, r, k] = cj_k(sum_j c_jr(f, t; n_j(t)) exp(2 pi i nu_f s_k b_k . n_j(t) / c)), n_j(t)
the source's topocentric unit vector (ENU).  V is linear in the sources, so with G = dL/dV, dL = Re sum conj(G) dV,
    L = sum_t sum_j L_tj(n_j(t)),    L_tj(n) = Re sum conj(G[:, t]) V_j(n),
V_j(n) the oracle's run of source j alone at the one time t with its vector GIVEN as n (``_TopoAt``).  The tangential
gradient is
    gtopo[t, j] = sum_i e_i d/dh L_tj(normalize(n + h e_i)) |_{h = 0},    (e_1, e_2) an orthonormal tangent pair at n,
each derivative a Richardson-extrapolated central difference, (4 D(h / 2) - D(h)) / 3 with
D(h) = (L(+h) - L(-h)) / (2 h): the h^2 term cancels, the remainder is about (k h)^4 with k = 2 pi nu |b| / c <~ 500 on
these arrays, 6e-10 at h = 1e-5 rad (``test_source_adjoint_host`` pins the figure by comparing the extrapolations from
(h, h/2) and (h/2, h/4)).  A source below the horizon at time t gets exactly 0: the cut is not differentiated.

Differences need a smooth interpolant: the table beam of these configurations is interpolated at spline order 3 (a C^2
cubic B-spline).  Orders 0 and 1 (nearest node, bilinear) have no reference here; the GPU tests check them only through
the agreement of the device with itself (lane counts, repeats).

Exclusions are a condition on the configurations, not a measurement: ``margins`` returns the smallest angular distance of
any (t, j) from the horizon and, for an unpolarized run with two dishes -- where the strength is sqrt(B_i B_j) = |e_i e_j|,
which has a kink at a null of either dish -- from a beam null; the host test asserts both stay above 1e-3 rad, so that
nothing is excluded from any comparison.
"""

import numpy as np

import fftvis_amd
from fftvis_amd import synth
from oracle import fftvis_oracle as orc
from tests.helpers import oracle_beam, spline_order
from tests.position_adjoint_refs import _TopoAt, position_config, random_complex, vis_shape  # noqa: F401

H_REF = 1e-5  # rad


SEED = 2  # catalog seed of every configuration here: nothing within 1e-3 rad of the horizon or of a null (``margins``)


def source_config(heights="flat", sky="I", beams="airy", compat=True, precision=2, **kw):
    """``position_config`` (perturbed hex-7, 24 sources, 3 channels, 2 times) at catalog seed ``SEED``, with the table beam
    interpolated at spline order 3: ``beams`` "airy", "two" or "complex" (the complex-valued E-field table)."""
    kw.setdefault("seed", SEED)
    cfg = position_config(heights, sky, beams, compat, precision, **kw)
    if beams == "complex":
        cfg["beam_spline_opts"] = {"order": 3}
    return cfg


def table_config(order, **kw):
    """A table-beam configuration at spline order 0 or 1 (no reference: device against itself)."""
    kw.setdefault("seed", SEED)
    cfg = position_config("cm", "full", "complex", False, 2, **kw)
    cfg["beam_spline_opts"] = {"order": order}
    return cfg


def tangent_pair(n):
    """An orthonormal pair (e1, e2) perpendicular to the unit vector n."""
    n = np.asarray(n, dtype=float)
    ax = np.zeros(3)
    ax[np.argmin(np.abs(n))] = 1.0
    e1 = np.cross(n, ax)
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(n, e1)


def _manager(cfg, coord_mgr):
    times = np.atleast_1d(np.asarray(cfg["times"], dtype=float))
    mgr = coord_mgr
    if mgr is None:
        mgr = orc.SimpleCoordinateRotation(None, times, cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    mgr.setup()
    return times, mgr


class _OneSource:
    """L_tj(n): the oracle's forward of one source at one time with a given vector, contracted with G[:, t]."""

    def __init__(self, cfg, G):
        self.cfg = cfg
        self.G = np.asarray(G).astype(np.complex128)
        beams = cfg["beam"] if isinstance(cfg["beam"], list) else [cfg["beam"]]
        order = spline_order(cfg.get("beam_spline_opts"))
        self.ob = [oracle_beam(b, cfg["polarized"], cfg["freqs"], order, cfg.get("use_feed", "x")) for b in beams]
        self.fluxes = np.asarray(cfg["fluxes"], dtype=float)
        self.ra, self.dec = np.asarray(cfg["ra"], dtype=float), np.asarray(cfg["dec"], dtype=float)

    def __call__(self, ti, t, j, n):
        cfg = self.cfg
        flux = self.fluxes[j:j + 1]
        coh = orc.prepare_source_catalog(flux, cfg["polarized"])[0]
        mgr = _TopoAt(coh, t, cfg["telescope_loc"], self.ra[j:j + 1], self.dec[j:j + 1], np.asarray(n, float).reshape(3, 1))
        V = orc.simulate(cfg["ants"], cfg["freqs"], flux, self.ob, self.ra[j:j + 1], self.dec[j:j + 1], np.array([t]),
                         cfg["telescope_loc"], baselines=cfg.get("baselines"), beam_idx=cfg.get("beam_idx"),
                         polarized=cfg["polarized"], force_use_type3=True,
                         reference_compat=cfg.get("reference_compat", True), coord_mgr=mgr)
        return float(np.sum((np.conj(self.G[:, ti]) * V[:, 0]).real))


def _directional(L, ti, t, j, n, e, h):
    """Richardson-extrapolated central difference of L_tj along normalize(n + s e) at s = 0, from the steps h and h / 2."""
    def D(s):
        p, m = n + s * e, n - s * e
        return (L(ti, t, j, p / np.linalg.norm(p)) - L(ti, t, j, m / np.linalg.norm(m))) / (2.0 * s)

    return (4.0 * D(0.5 * h) - D(h)) / 3.0


def exact_gtopo(cfg, G, coord_mgr=None, sources=None, h=H_REF):
    """``gtopo`` (ntimes, nsrc, 3) float64, ENU, tangential.  ``coord_mgr``: the test's manager (its vectors through
    ``orc._topo_of``); the oracle's ``SimpleCoordinateRotation`` by default.  ``sources``: catalog indices -- only those
    rows are computed, the others stay 0."""
    times, mgr = _manager(cfg, coord_mgr)
    L = _OneSource(cfg, G)
    nsrc = L.ra.size
    out = np.zeros((len(times), nsrc, 3))
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        for j in (range(nsrc) if sources is None else sources):
            n = topo[:, j] / np.linalg.norm(topo[:, j])
            if not n[2] > 0:
                continue
            for e in tangent_pair(n):
                out[ti, j] += _directional(L, ti, t, j, n, e, h) * e
    return out


def sidereal_jacobian(cfg):
    """J[t, j] = d n_j(t) / d(ra, dec) (ntimes, nsrc, 3, 2) under the oracle's sidereal rotation, in closed form."""
    times = np.atleast_1d(np.asarray(cfg["times"], dtype=float))
    ra, dec = np.asarray(cfg["ra"], float), np.asarray(cfg["dec"], float)
    mgr = orc.SimpleCoordinateRotation(None, times, cfg["telescope_loc"], ra, dec)
    d_ra = np.stack([-np.cos(dec) * np.sin(ra), np.cos(dec) * np.cos(ra), np.zeros_like(ra)])
    d_dec = np.stack([-np.sin(dec) * np.cos(ra), -np.sin(dec) * np.sin(ra), np.cos(dec)])
    J = np.empty((len(times), ra.size, 3, 2))
    for ti in range(len(times)):
        R = mgr.rotation_matrix(ti)
        J[ti, :, :, 0] = (R @ d_ra).T
        J[ti, :, :, 1] = (R @ d_dec).T
    return J


def exact_gradec(cfg, G, sources=None, h=H_REF):
    """``gradec`` (nsrc, 2) float64, columns (ra, dec): the same differences taken in the angles themselves, the vectors
    from ``SimpleCoordinateRotation`` at (ra, dec) displaced by +-h and +-h / 2.  The cut is decided at the undisplaced
    position."""
    times, _ = _manager(cfg, None)
    L = _OneSource(cfg, G)
    nsrc = L.ra.size
    out = np.zeros((nsrc, 2))

    def vec(ti, ra, dec):
        one = orc.SimpleCoordinateRotation(None, times, cfg["telescope_loc"], np.array([ra]), np.array([dec]))
        return orc._topo_of(one, ti)[:, 0]

    for ti, t in enumerate(times):
        for j in (range(nsrc) if sources is None else sources):
            if not vec(ti, L.ra[j], L.dec[j])[2] > 0:
                continue
            for c, (da, dd) in enumerate(((1.0, 0.0), (0.0, 1.0))):
                def D(s):
                    return (L(ti, t, j, vec(ti, L.ra[j] + s * da, L.dec[j] + s * dd)) -
                            L(ti, t, j, vec(ti, L.ra[j] - s * da, L.dec[j] - s * dd))) / (2.0 * s)

                out[j, c] += (4.0 * D(0.5 * h) - D(h)) / 3.0
    return out


_J1_ZEROS = np.array([3.8317059702075125, 7.015586669815619, 10.173468135062722, 13.323691936314223, 16.470630050877634,
                      19.615858510468243, 22.760084380592772, 25.903672087618382, 29.046828534916855, 32.189679910974405])


def margins(cfg, coord_mgr=None):
    """(horizon, null): the smallest angular distance [rad] of any (t, j) of the configuration from the horizon, and -- an
    unpolarized run with more than one Airy dish -- from a null of a dish at a channel of the run (inf otherwise, and
    for sources below the horizon, which take no part)."""
    times, mgr = _manager(cfg, coord_mgr)
    beams = cfg["beam"] if isinstance(cfg["beam"], list) else [cfg["beam"]]
    kink = not cfg["polarized"] and len(beams) > 1
    hor, null = np.inf, np.inf
    for ti in range(len(times)):
        topo = orc._topo_of(mgr, ti)
        el = np.arcsin(np.clip(topo[2] / np.linalg.norm(topo, axis=0), -1, 1))
        hor = min(hor, float(np.abs(el).min()))
        if kink:
            za = 0.5 * np.pi - el[el > 0]
            for b in beams:
                assert isinstance(b, fftvis_amd.AiryBeam)
                for f in np.asarray(cfg["freqs"], float):
                    s = _J1_ZEROS * orc.speed_of_light / (np.pi * b.diameter * f)
                    zn = np.arcsin(s[s < 1.0])
                    if zn.size and za.size:
                        null = min(null, float(np.abs(za[:, None] - zn[None, :]).min()))
    return hor, null


__all__ = ["H_REF", "SEED", "exact_gtopo", "exact_gradec", "margins", "position_config", "random_complex", "sidereal_jacobian",
           "source_config", "synth", "table_config", "tangent_pair", "vis_shape"]
