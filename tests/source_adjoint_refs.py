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

Differences need an interpolant that is smooth over the stencil n +- h.  A table beam is a polynomial patch between two
knot lines at EVERY spline order, composed with the smooth map n -> (az, za), so the condition is one on the
configuration: no source within a margin of a knot line of its table (``knot_margin``: the nodes at odd orders, half a
node off at even orders and for order 0's jumps).  ``source_config`` interpolates its table at order 3 (a C^2 cubic
B-spline, whose third derivative's jump costs the difference about h^2 times that jump: orders 3 .. 5 need no margin);
``order_config`` is the same cell at any order, at a catalog seed for which the margin holds at orders 0, 1 and 2.  At
order 0 the beam is piecewise constant, so the gradient with the strengths held fixed is the whole gradient:
``frozen_beam_gtopo`` gives it in closed form, with no differences, and stays valid with a source ON a jump.

Exclusions are a condition on the configurations, not a measurement: ``margins`` returns the smallest angular distance of
any (t, j) from the horizon and, for an unpolarized run with two dishes -- where the strength is sqrt(B_i B_j) = |e_i e_j|,
which has a kink at a null of either dish -- from a beam null, ``knot_margin`` the one from a knot line; the host test
asserts that all stay above 1e-3 rad (the knot margin at orders 0, 1 and 2; 1e-4 rad = 10 H_REF for the sources the
table-edge configurations place by hand), so that nothing is excluded from any comparison.
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
    """A table-beam configuration at spline order 0 or 1 for the runs that compare the device with itself (its sources are
    not held away from the knot lines: ``order_config`` is the one with a reference)."""
    kw.setdefault("seed", SEED)
    cfg = position_config("cm", "full", "complex", False, 2, **kw)
    cfg["beam_spline_opts"] = {"order": order}
    return cfg


KNOT_SEED = 3  # catalog seed of ``order_config``: at the matrix shape nothing within 1e-3 rad of a knot line at any order


def order_config(order, sky="full", precision=2, **kw):
    """The matrix cell "cm heights, exact flips, complex table" at spline order ``order`` and catalog seed ``KNOT_SEED``
    (24 sources, 3 channels, 2 times): every above-horizon (t, j) is more than 1e-3 rad from the horizon and from a knot
    line of the table at orders 0, 1 and 2 (``test_source_adjoint_host`` asserts it)."""
    kw.setdefault("seed", KNOT_SEED)
    cfg = position_config("cm", sky, "complex", False, precision, **kw)
    cfg["beam_spline_opts"] = {"order": order}
    return cfg


class GivenTopo:
    """The slice of matvis' coordinate manager the engine and the oracle consume, with the ENU unit vectors given:
    ``topos`` (ntimes, 3, nsrc)."""

    def __init__(self, times, topos):
        self.times = np.atleast_1d(np.asarray(times, dtype=float))
        self.topos = np.asarray(topos, dtype=float)

    def setup(self):
        pass

    def rotate(self, ti):
        self.all_coords_topo = self.topos[ti]


def enu_of(az, za):
    """(3, n) ENU unit vectors at beam coordinates (az from east through north, as ``orc.enu_to_az_za`` returns it)."""
    az, za = np.asarray(az, dtype=float), np.asarray(za, dtype=float)
    return np.stack([np.sin(za) * np.cos(az), np.sin(za) * np.sin(az), np.cos(za)])


# Table-edge sources as (az, za) in nodes of the table.  Full sky: synth's 46 x 90 table, za_max = pi, both node
# spacings pi / 45.  Horizon: 24 x 90 nodes, za_max = pi / 2, za nodes at pi / 46.
_NODE = np.pi / 45
_FULLSKY = [(0.3, 8.4), (89.7, 17.6), (20.5, 1e-2 / _NODE), (55.5, 3e-3 / _NODE), (33.4, (0.5 * np.pi - 5e-3) / _NODE)]
_FULLSKY_WRAP = (1e-7 / _NODE, 12.6)  # order 3 only: both stencils straddle az = 0
_HORIZON = [(17.3, 5.4), (61.6, 14.7), (80.45, 0.6), (40.5, (0.5 * np.pi - 5e-3) / (np.pi / 46))]


def edge_table_config(kind, order):
    """(cfg, manager): one time step with the sources placed by hand at the edges of a table, their ENU vectors handed
    in through the manager, on the matrix cell's array, full Stokes, exact flips, fp64.
    "fullsky": the 46 x 90 table to za = pi; az 0.3 of a cell above 0 and 0.3 below 2 pi (the wrap-around node), za = 1e-2
    and 3e-3 inside the first za cell (mirror extension, az ill-conditioned; az in mid-cell), za = pi / 2 - 5e-3, and at
    order 3 az = 1e-7.  "horizon": a table that ends at za_max = pi / 2, nodes at pi / 46; one source at za = pi / 2 - 5e-3
    in its last za cell (the cell index at its upper clamp, the mirror at the far end)."""
    pts = {"fullsky": _FULLSKY + ([_FULLSKY_WRAP] if order == 3 else []), "horizon": _HORIZON}[kind]
    cfg = order_config(order, nsrc=len(pts), ntimes=1)
    freqs = cfg["freqs"]
    if kind == "horizon":
        tab = synth.synthetic_efield_table(freqs, 14.0, nza=47, naz=90)[..., :24, :]
        cfg["beam"] = fftvis_amd.TabulatedBeam(tab, freqs, za_max=np.pi / 2)
    da, dz = 2 * np.pi / cfg["beam"].data.shape[-1], cfg["beam"].za_max / (cfg["beam"].data.shape[-2] - 1)
    topo = enu_of([p[0] * da for p in pts], [p[1] * dz for p in pts])
    return cfg, GivenTopo(cfg["times"], topo[None])


JUMP_OFFSET = 3e-7  # rad: inside the device's 1e-6 rad stencil


def jump_config():
    """(cfg, manager, rows): ``order_config(0)`` with, at the first time, one above-horizon source moved to JUMP_OFFSET from
    a za half-node line and one to JUMP_OFFSET (as an angle on the sky) from an az half-node line -- order 0's jumps --;
    every other (t, j) keeps its sidereal vector.  rows: the two catalog indices."""
    cfg = order_config(0)
    times, mgr = _manager(cfg, None)
    topos = np.stack([orc._topo_of(mgr, ti) for ti in range(len(times))])
    b = cfg["beam"]
    da, dz = 2 * np.pi / b.data.shape[-1], b.za_max / (b.data.shape[-2] - 1)
    rows = [int(j) for j in np.flatnonzero(topos[0, 2] > 0.3)[:2]]
    za = 9.5 * dz + JUMP_OFFSET  # the line between nodes 9 and 10; az well inside a cell
    topos[0, :, rows[0]] = enu_of(31.1 * da, za)
    za = 6.2 * dz  # za well inside a cell; the line between az nodes 70 and 71
    topos[0, :, rows[1]] = enu_of(70.5 * da - JUMP_OFFSET / np.sin(za), za)
    return cfg, GivenTopo(times, topos), rows


ORDERS = (0, 1, 2, 4, 5)  # with ``source_config``'s 3: every order the device interpolates


def table_configs():
    """(label, cfg, order, manager or None, knot bound) of every comparison of the two GPU modules on a table beam beyond
    order 3's matrix: the orders, the unpolarized order-1 cell and the table edges.  knot bound [rad]: what
    ``knot_margin`` has to exceed -- 1e-3 at orders 0, 1 and 2, 1e-4 (10 H_REF) for the hand-placed edge sources at order 1,
    None at orders 3 .. 5 (C^2: no condition)."""
    out = [(f"order {o}", order_config(o), o, None, 1e-3 if o < 3 else None) for o in ORDERS]
    out.append(("order 1 unpolarized", order_config(1, sky="unpol"), 1, None, 1e-3))
    for kind in ("fullsky", "horizon"):
        for o in (1, 3):
            cfg, mgr = edge_table_config(kind, o)
            out.append((f"{kind} order {o}", cfg, o, mgr, 1e-4 if o < 3 else None))
    return out


def gradcheck_config():
    """torch's gradcheck on a table beam at the DEFAULT order (no ``beam_spline_opts``: bilinear): ``order_config``'s cell
    at 8 sources, 1 channel (150 MHz), 1 time, 6 baselines, eps 1e-12 -- the sizes of the dish gradcheck."""
    cfg = order_config(1, nsrc=8, nfreq=1, ntimes=1)
    del cfg["beam_spline_opts"]
    cfg.update(eps=1e-12, freqs=np.array([150e6]), baselines=[(0, 1), (2, 5), (3, 6), (1, 4), (6, 0), (2, 2)],
               coord_method="SiderealRotation")
    _, _, cfg["fluxes"] = synth.catalog(8, cfg["freqs"], KNOT_SEED, polarized_sky=True)
    cfg["beam"] = fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(cfg["freqs"], 14.0, nza=46, naz=90), cfg["freqs"])
    return cfg


def baseline_vectors(cfg):
    """(nbls, 3): every listed baseline's own vector ants[j] - ants[i], ENU metres."""
    a = cfg["ants"]
    return np.array([np.asarray(a[j], float) - np.asarray(a[i], float) for i, j in cfg["baselines"]])


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

    def vis(self, t, j, n):
        """V_j(n) at the one time t: (nf, [2, 2,] nbls)."""
        cfg = self.cfg
        flux = self.fluxes[j:j + 1]
        coh = orc.prepare_source_catalog(flux, cfg["polarized"])[0]
        mgr = _TopoAt(coh, t, cfg["telescope_loc"], self.ra[j:j + 1], self.dec[j:j + 1], np.asarray(n, float).reshape(3, 1))
        V = orc.simulate(cfg["ants"], cfg["freqs"], flux, self.ob, self.ra[j:j + 1], self.dec[j:j + 1], np.array([t]),
                         cfg["telescope_loc"], baselines=cfg.get("baselines"), beam_idx=cfg.get("beam_idx"),
                         polarized=cfg["polarized"], force_use_type3=True,
                         reference_compat=cfg.get("reference_compat", True), coord_mgr=mgr)
        return V[:, 0]

    def __call__(self, ti, t, j, n):
        return float(np.sum((np.conj(self.G[:, ti]) * self.vis(t, j, n)).real))


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


def frozen_beam_gtopo(cfg, G, coord_mgr=None):
    """The gradient with the strengths c held fixed, in closed form: V_j[f, r, k] = cj_k(c exp(2 pi i nu_f s_k b_k . n / c))
    moves with n through its phase alone, d V_j / d n = i (2 pi nu_f / c) b_k V_j (b_k the listed baseline's own vector;
    a flipped baseline conjugates -i nu X to +i nu conj(X): no sign case, as in ``position_adjoint_refs``), so
        gtopo[t, j] = -P_n sum_{f, r, k} (2 pi nu_f / c) b_k Im(conj(G[f, t, r, k]) V_j[f, r, k]),
    one oracle run per (t, j) and no differences.  At spline order 0, where the beam is piecewise constant, this is the
    whole gradient; it stays valid with a source on a jump of the table."""
    times, mgr = _manager(cfg, coord_mgr)
    L = _OneSource(cfg, G)
    b = baseline_vectors(cfg)
    kf = 2 * np.pi * np.asarray(cfg["freqs"], dtype=float) / orc.speed_of_light
    out = np.zeros((len(times), L.ra.size, 3))
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        for j in range(L.ra.size):
            n = topo[:, j] / np.linalg.norm(topo[:, j])
            if not n[2] > 0:
                continue
            x = (np.conj(L.G[:, ti]) * L.vis(t, j, n)).imag  # (nf, [2, 2,] nbls)
            x = x.reshape(len(kf), -1, x.shape[-1]).sum(axis=1)
            g = -(kf @ x) @ b
            out[ti, j] = g - n * (n @ g)
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


def knot_margin(cfg, order, coord_mgr=None):
    """The smallest angular distance [rad] of any above-horizon (t, j) from a knot line of the configuration's table
    beams at spline order ``order``: the nodes at odd orders, half a node off at even orders (the centred B-spline's
    knots, and order 0's jumps: the device's ``spline_setup``).  The distance to an az line is |az - line| sin(za).  The
    grid comes from the beam objects; inf without a table."""
    times, mgr = _manager(cfg, coord_mgr)
    beams = cfg["beam"] if isinstance(cfg["beam"], list) else [cfg["beam"]]
    half = 0.0 if order & 1 else 0.5
    out = np.inf
    for ti in range(len(times)):
        topo = orc._topo_of(mgr, ti)
        n = topo / np.linalg.norm(topo, axis=0)
        up = n[2] > 0
        if not up.any():
            continue
        az, za = orc.enu_to_az_za(n[0, up], n[1, up])
        for b in beams:
            if not isinstance(b, fftvis_amd.TabulatedBeam):
                continue
            nza, naz = b.data.shape[-2:]
            dz, da = b.za_max / (nza - 1), 2 * np.pi / naz
            xz, xa = za / dz - half, az / da - half
            out = min(out, float((np.abs(xz - np.rint(xz)) * dz).min()),
                      float((np.abs(xa - np.rint(xa)) * da * np.sin(za)).min()))
    return out


__all__ = ["H_REF", "JUMP_OFFSET", "KNOT_SEED", "SEED", "GivenTopo", "baseline_vectors", "edge_table_config", "enu_of",
           "exact_gtopo", "exact_gradec", "frozen_beam_gtopo", "gradcheck_config", "jump_config", "knot_margin", "margins", "order_config",
           "position_config", "random_complex", "sidereal_jacobian", "source_config", "synth", "table_config",
           "table_configs", "tangent_pair", "vis_shape", "ORDERS"]
