"""Exact references for the forward-mode tangent (``simulate_vis_jvp``, ``fv_sim_run_tangent``), built from the oracle's
FORWARD alone.

Every forward path approximates out[f, t, r, k] = cj_k(sum_j c_jr(f, t; n_j(t)) exp(2 pi i nu_f s_k b_k . n_j(t) / c)),
b_k = ants[j] - ants[i] in ENU metres, n_j(t) the source's topocentric unit vector.

Baselines (closed form).  The strengths do not depend on the positions and topo_d is real, so along a change dbls
    dV[f, t, ..., k] = sum_d i (2 pi nu_f / c) dbls[k, d] D_d[f, t, ..., k],
D_d what the forward writes when every source's fluxes are multiplied by topo_j,d(t) (a flipped baseline conjugates
-i nu X to +i nu conj(X): no sign case).

Directions.  V is linear in the sources, so ALL sources move at once: per time step the oracle runs at one time with
the vectors given (``_TopoAt``) at normalize(n +- h delta) and at h / 2, delta = P_n dtopo scaled so that max |delta_j| = 1
and rescaled afterwards, and the tangent is the Richardson-extrapolated central difference (4 D(h / 2) - D(h)) / 3,
D(h) = (V(+h) - V(-h)) / 2h, h = 1e-5: the remainder is about (k h)^4, k = 2 pi nu |b| / c <~ 500 on these arrays
(``test_tangent_host`` pins the figure by comparing the extrapolations from (h, h/2) and (h/2, h/4)).  Rows of sources
below the horizon are set to 0: the cut is not differentiated.  The phase part has a closed form as well,
    sum_d i (2 pi nu_f / c) b_k,d . oracle(fluxes x (P_n delta)_d),
so the beam part is what remains.

The differences need a beam that is smooth over n +- h delta.  A table beam is a polynomial patch between two knot lines
at every spline order, so the condition is ``source_adjoint_refs.knot_margin``'s: the configurations with a table at
orders 0, 1 and 2 (``order_config``) keep every source more than 1e-3 rad from a knot line, the hand-placed table-edge
sources (``edge_table_config``) more than 1e-4 rad = 10 h (``test_tangent_host`` asserts both); orders 3 .. 5 are C^2 and
need none.  At order 0 the beam is piecewise constant and the phase part is the whole tangent: ``frozen_beam_dv_topo``,
closed form, valid with a source on a jump of the table.
"""

import numpy as np

from oracle import fftvis_oracle as orc
from tests.helpers import oracle_simulate
from tests.position_adjoint_refs import _TopoAt, position_config, random_complex, vis_shape  # noqa: F401
from tests.source_adjoint_refs import (ORDERS, baseline_vectors, edge_table_config, jump_config, knot_margin,  # noqa: F401
                                       margins, order_config, source_config, table_configs, tangent_pair)

H_REF = 1e-5  # rad


def _setup(cfg, coord_mgr):
    freqs = np.asarray(cfg["freqs"], dtype=float)
    times = np.atleast_1d(np.asarray(cfg["times"], dtype=float))
    fluxes = np.asarray(cfg["fluxes"], dtype=float)
    mgr = coord_mgr
    if mgr is None:
        mgr = orc.SimpleCoordinateRotation(None, times, cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    mgr.setup()
    return freqs, times, fluxes, mgr


def _forward_at(cfg, t, fluxes, topo):
    """The oracle's forward at the one time t with the fluxes and the (3, nsrc) topocentric vectors given: (nf, ..., nbls)."""
    one = dict(cfg, times=np.array([t]), fluxes=fluxes)
    coh = orc.prepare_source_catalog(fluxes, cfg["polarized"])[0]
    return oracle_simulate(one, coord_mgr=_TopoAt(coh, t, cfg["telescope_loc"], cfg["ra"], cfg["dec"], topo))[:, 0]


def _kf(freqs, ndim):
    return (2 * np.pi * freqs / orc.speed_of_light).reshape((-1,) + (1,) * (ndim - 2))  # per channel, over (r..., k)


def exact_dv_baselines(cfg, dbls, coord_mgr=None, sub=None):
    """(dV, terms): the tangent along ``dbls`` (nbls, 3) in simulate_vis's shape, complex128, and its three terms (one per
    component d, same shape).  ``sub``: indices into cfg's baselines -- only those are computed (``dbls`` then has their
    rows), in that order."""
    if sub is not None:
        cfg = dict(cfg, baselines=[cfg["baselines"][i] for i in sub])
    dbls = np.asarray(dbls, dtype=float)
    assert dbls.shape == (len(cfg["baselines"]), 3)
    freqs, times, fluxes, mgr = _setup(cfg, coord_mgr)
    shape = vis_shape(cfg)
    terms = [np.zeros(shape, dtype=np.complex128) for _ in range(3)]
    kf = _kf(freqs, len(shape))
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        for d in range(3):
            w = topo[d].reshape((-1,) + (1,) * (fluxes.ndim - 1))
            D = _forward_at(cfg, t, fluxes * w, topo)
            terms[d][:, ti] = 1j * kf * dbls[:, d] * D
    return terms[0] + terms[1] + terms[2], terms


def project(topo, dtopo_t):
    """delta = P_n dtopo for one time step: topo (3, nsrc), dtopo_t (nsrc, 3) -> (nsrc, 3); rows below the horizon 0."""
    n = (topo / np.linalg.norm(topo, axis=0)).T
    d = dtopo_t - n * np.sum(n * dtopo_t, axis=1, keepdims=True)
    d[~(n[:, 2] > 0)] = 0.0
    return n, d


def exact_dv_topo(cfg, dtopo, coord_mgr=None, h=H_REF):
    """(dV, phase, terms): the tangent along ``dtopo`` (ntimes, nsrc, 3) in simulate_vis's shape, its phase part in
    closed form, and the terms that sum to dV: the three phase terms and the beam part dV - phase."""
    dtopo = np.asarray(dtopo, dtype=float)
    freqs, times, fluxes, mgr = _setup(cfg, coord_mgr)
    shape = vis_shape(cfg)
    dV = np.zeros(shape, dtype=np.complex128)
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        n, delta = project(topo, dtopo[ti])
        s = float(np.linalg.norm(delta, axis=1).max())
        if s == 0.0:
            continue
        dh = delta / s

        def D(step):
            p, m = n + step * dh, n - step * dh
            p /= np.linalg.norm(p, axis=1, keepdims=True)
            m /= np.linalg.norm(m, axis=1, keepdims=True)
            return (_forward_at(cfg, t, fluxes, p.T) - _forward_at(cfg, t, fluxes, m.T)) / (2.0 * step)

        dV[:, ti] = s * (4.0 * D(0.5 * h) - D(h)) / 3.0
    phase, pterms = frozen_beam_dv_topo(cfg, dtopo, coord_mgr)
    return dV, phase, pterms + [dV - phase]


def frozen_beam_dv_topo(cfg, dtopo, coord_mgr=None):
    """(dV, terms): the tangent along ``dtopo`` with the strengths held fixed -- the phase part, in closed form, and its
    three terms (one per ENU component of delta = P_n dtopo).  At spline order 0, where the beam is piecewise constant,
    this is the whole tangent; it stays valid with a source on a jump of the table."""
    dtopo = np.asarray(dtopo, dtype=float)
    freqs, times, fluxes, mgr = _setup(cfg, coord_mgr)
    shape = vis_shape(cfg)
    terms = [np.zeros(shape, dtype=np.complex128) for _ in range(3)]
    kf = _kf(freqs, len(shape))
    b = baseline_vectors(cfg)
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        _, delta = project(topo, dtopo[ti])
        if not delta.any():
            continue
        for d in range(3):
            w = delta[:, d].reshape((-1,) + (1,) * (fluxes.ndim - 1))
            terms[d][:, ti] = 1j * kf * b[:, d] * _forward_at(cfg, t, fluxes * w, topo)
    return terms[0] + terms[1] + terms[2], terms


def kappa(dV, terms):
    """Cancellation factor of a sum of terms: sum ||term|| / ||sum||."""
    return float(sum(np.linalg.norm(x) for x in terms) / np.linalg.norm(dV))


def random_dbls(cfg, seed):
    return np.random.default_rng(seed).normal(size=(len(cfg["baselines"]), 3))


def random_dtopo(cfg, seed):
    """Random rows with a radial part (the projection is part of what is tested)."""
    nt = len(np.atleast_1d(cfg["times"]))
    return np.random.default_rng(seed).normal(size=(nt, int(np.size(cfg["ra"])), 3))


# ---- the configurations of the GPU module (``test_gpu_tangent``), shared with the host test's conditions ----------------
DB_SEED, DT_SEED = 1, 2  # seeds of the tangents: the reference alone satisfies kappa <= 4 for them (test_tangent_host)
HERA_SUB = 600


def matrix_cells():
    return [(h, s, b, c) for h in ("flat", "cm", "m") for s in ("unpol", "I", "full") for b in ("airy", "two", "complex")
            for c in (True, False)]


def edge_config(**kw):
    """The perturbed hex-7 with centimetre heights (height terms), polarized, full-Stokes sky, two beams, the exact form
    of the flipped baselines, fp64 (the position and source tests' edge configuration)."""
    return source_config("cm", "full", "two", False, 2, **kw)


def hex19_config():
    """An exact hex-19, all baselines in the caller's order plus two flipped ones: redundant runs and mirror pairs."""
    from fftvis_amd import synth
    from tests.position_adjoint_refs import hex_positions

    c1 = synth.make_config("C1", nsrc=24, nfreq=3, ntimes=2, seed=2)
    xy = 14.6 * hex_positions(2)
    ants = {i: np.array([xy[i, 0], xy[i, 1], 0.0]) for i in range(19)}
    bls = [(i, j) for i in range(19) for j in range(i, 19)] + [(7, 3), (18, 0)]
    return dict(c1, ants=ants, baselines=bls, polarized=True, force_use_type3=False)


def hera_subset(cfg):
    """A seeded subset of HERA-350's baselines."""
    n = len(cfg["baselines"])
    return sorted(np.random.default_rng(3).choice(n, size=HERA_SUB, replace=False).tolist())


def empty_step_config():
    """Sources around the meridian at the first time: half a sidereal day later nothing is above the horizon."""
    from fftvis_amd import synth

    cfg = edge_config(nsrc=20)
    t0 = cfg["times"][0]
    lst = orc.gmst_rad(t0) + synth.HERA_LON
    rng = np.random.default_rng(1)
    cfg.update(ra=lst + rng.uniform(-0.3, 0.3, 20), dec=synth.HERA_LAT + rng.uniform(-0.3, 0.3, 20),
               times=t0 + np.array([0.0, 0.25, 0.5]))
    return cfg


def all_configs():
    """(label, cfg, dbls, dtopo, manager, order, knot bound) of every comparison of the GPU module with a reference (fp64
    inputs; the references do not depend on the run's precision).  HERA-350: the baselines tangent on the seeded subset.
    The table configurations beyond order 3's matrix (``table_configs``: the direction tangent alone) carry their manager,
    spline order and the bound ``knot_margin`` has to exceed; the others None."""
    out = []
    for cell in matrix_cells():
        cfg = source_config(*cell)
        out.append(("matrix " + " ".join(map(str, cell)), cfg, random_dbls(cfg, DB_SEED), random_dtopo(cfg, DT_SEED)))
    for label, cfg in (("chunks", dict(edge_config(nsrc=25, ntimes=4), min_chunks=2)),
                       ("free lanes", dict(edge_config(nsrc=25, ntimes=5), min_chunks=2)),
                       ("blocks", edge_config(nsrc=18, nfreq=5)),
                       ("edge", edge_config()),
                       ("three times", edge_config(ntimes=3)),
                       ("empty step", empty_step_config()),
                       ("hex-19", hex19_config())):
        out.append((label, cfg, random_dbls(cfg, DB_SEED), random_dtopo(cfg, DT_SEED)))
    from tests.test_gpu_position_adjoint import _hera350

    for kind in ("hermitian", "all_real"):
        cfg = _hera350(kind)
        sub = hera_subset(cfg)
        out.append((f"hera350 {kind}", dict(cfg, baselines=[cfg["baselines"][i] for i in sub]),
                    random_dbls(cfg, DB_SEED)[sub], None))
    out = [c + (None, None, None) for c in out]
    for label, cfg, order, mgr, bound in table_configs():
        out.append((label, cfg, None, random_dtopo(cfg, DT_SEED), mgr, order, bound))
    return out
