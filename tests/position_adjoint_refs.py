"""Exact reference for the gradient with respect to the antenna positions, built from the oracle's FORWARD alone.

Every forward path approximates out[f, t, r, k] = cj_k(sum_j c_jr(f, t) exp(2 pi i nu_f s_k b_k . topo_j(t) / c)),
b_k = ants[j] - ants[i] in ENU metres; the strengths c do not depend on the positions and topo_d is real, so
    d out[f, t, r, k] / d b_k,d = i (2 pi nu_f / c) D_d[f, t, r, k],
D_d what the forward writes when every source's fluxes are multiplied by topo_j,d(t) (a flipped baseline conjugates
-i nu X to +i nu conj(X): no sign case), and with G = dL/dV, dL = Re sum conj(G) dV
    gbls[k, d] = -sum_{f, t, r} (2 pi nu_f / c) Im(conj(G[f, t, r, k]) D_d[f, t, r, k]),
    gants[a]   = sum_{k: a = j_k} gbls[k] - sum_{k: a = i_k} gbls[k].
``test_position_adjoint_host`` pins this against Richardson-extrapolated central differences of the oracle.
"""

import numpy as np

import fftvis_amd
from fftvis_amd import synth
from oracle import fftvis_oracle as orc
from tests.helpers import oracle_simulate


def random_complex(shape, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)


class _TopoAt(orc.SimpleCoordinateRotation):
    """One time step whose topocentric vectors are given (a caller's manager evaluated at that time)."""

    def __init__(self, flux, t, telescope_loc, ra, dec, topo):
        super().__init__(flux, [t], telescope_loc, ra, dec)
        self._fixed = np.array(topo, dtype=float)

    def rotate(self, ti):
        self._topo = self._fixed


def vis_shape(cfg):
    nf, nt, nb = len(cfg["freqs"]), len(np.atleast_1d(cfg["times"])), len(cfg["baselines"])
    return (nf, nt, 2, 2, nb) if cfg["polarized"] else (nf, nt, nb)


def exact_gbls(cfg, G, coord_mgr=None, sub=None):
    """``gbls`` (nbls, 3) float64 from the oracle's forward: per time step t and component d one run with ``times=[t]`` and
    the fluxes times topo_d(t), contracted with G as in the formula above.  ``coord_mgr``: the test's manager (its vectors
    through ``orc._topo_of``); the oracle's ``SimpleCoordinateRotation`` by default.  ``sub``: indices into cfg's
    baselines -- only those rows are computed, and returned in that order."""
    G = np.asarray(G).astype(np.complex128)
    bls = cfg["baselines"]
    if sub is not None:
        cfg = dict(cfg, baselines=[bls[i] for i in sub])
        G = G[..., np.asarray(sub)]
    freqs = np.asarray(cfg["freqs"], dtype=float)
    times = np.atleast_1d(np.asarray(cfg["times"], dtype=float))
    fluxes = np.asarray(cfg["fluxes"], dtype=float)
    mgr = coord_mgr
    if mgr is None:
        mgr = orc.SimpleCoordinateRotation(None, times, cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    mgr.setup()
    out = np.zeros((len(cfg["baselines"]), 3))
    kf = (2 * np.pi * freqs / orc.speed_of_light).reshape((-1,) + (1,) * (G.ndim - 2))  # per channel, over (r..., k)
    for ti, t in enumerate(times):
        topo = orc._topo_of(mgr, ti)
        for d in range(3):
            w = topo[d].reshape((-1,) + (1,) * (fluxes.ndim - 1))
            one = dict(cfg, times=np.array([t]), fluxes=fluxes * w)
            if coord_mgr is None:
                D = oracle_simulate(one)
            else:
                coh = orc.prepare_source_catalog(one["fluxes"], cfg["polarized"])[0]
                D = oracle_simulate(one, coord_mgr=_TopoAt(coh, t, cfg["telescope_loc"], cfg["ra"], cfg["dec"], topo))
            x = kf * (np.conj(G[:, ti]) * D[:, 0]).imag  # (nf, [2, 2,] nbls)
            out[:, d] -= x.reshape(-1, x.shape[-1]).sum(axis=0)
    return out


def exact_gants(cfg, G, **kw):
    return fftvis_amd.baseline_to_antenna_gradient(exact_gbls(cfg, G, **kw), cfg["ants"], cfg["baselines"])


def hex_positions(rings):
    """Unit hexagonal lattice: 3 rings (rings + 1) + 1 points, rows ordered by (y, x)."""
    pts = []
    for q in range(-rings, rings + 1):
        for r in range(max(-rings, -q - rings), min(rings, -q + rings) + 1):
            pts.append((q + 0.5 * r, np.sqrt(3.0) / 2.0 * r))
    return np.array(sorted(pts, key=lambda p: (round(p[1], 9), p[0])))


def perturbed_hex7(heights, seed=11, spacing=14.6):
    """A hex-7 with seeded N(0, 2 cm) errors in x and y, so that no two baselines repeat.  ``heights``: "flat" (exactly
    0: the transforms are 2-D), "cm" (N(0, 3 cm): 2-D transforms with height terms) or "m" (+-3 m: the 3-D transform)."""
    rng = np.random.default_rng(seed)
    xy = spacing * hex_positions(1) + 0.02 * rng.normal(size=(7, 2))
    z = {"flat": np.zeros(7), "cm": 0.03 * rng.normal(size=7), "m": 3.0 * np.where(np.arange(7) % 2, 1.0, -1.0)}[heights]
    z = z - (z.mean() if heights == "cm" else 0.0)
    return {i: np.array([xy[i, 0], xy[i, 1], z[i]]) for i in range(7)}


def position_config(heights="flat", sky="I", beams="airy", compat=True, precision=2, nsrc=24, nfreq=3, ntimes=2, seed=0):
    """The perturbed hex-7 with C1's catalog, band and times (``basis_config``'s shapes), every pair with the autos plus
    two flipped baselines.  ``sky``: "unpol" (an unpolarized run), "I" (polarized, Stokes I) or "full" (polarized, full
    Stokes).  ``beams``: "airy" (one dish), "two" (two dishes through ``beam_idx``, both orders of a mixed pair listed) or
    "complex" (one complex-valued E-field table)."""
    c1 = synth.make_config("C1", seed=seed, nsrc=nsrc, nfreq=nfreq, ntimes=ntimes)
    freqs = c1["freqs"]
    ants = perturbed_hex7(heights)
    cfg = dict(c1, ants=ants, polarized=sky != "unpol", precision=precision, reference_compat=compat,
               eps=6e-8 if precision == 2 else 1e-5)
    if sky == "full":
        _, _, cfg["fluxes"] = synth.catalog(nsrc, freqs, seed, polarized_sky=True)
    cfg["baselines"] = [(i, j) for i in range(7) for j in range(i, 7)] + [(3, 1), (6, 0)]
    if beams == "airy":
        cfg["beam"] = fftvis_amd.AiryBeam(14.0)
    elif beams == "two":
        cfg["beam"] = [fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(9.0)]
        cfg["beam_idx"] = np.array([0, 1, 0, 1, 1, 0, 1])  # (1, 3) and (3, 1): same pair of beams; (0, 6) and (6, 0): mixed
    else:
        cfg["beam"] = fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, 14.0, nza=46, naz=90), freqs)
    return cfg
