"""Shared helpers for the parity tests: oracle twins of the product's beam containers."""

import json
import os

import numpy as np

import fftvis_amd
from fftvis_amd.core.beams import spline_order
from oracle import fftvis_oracle as orc


def rel_l2(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / (nb if nb else 1.0)


def oracle_beam(beam, polarized, freqs, order=1, use_feed="x"):
    """The oracle's twin of a product beam.  Unpolarized runs go through the ORACLE's own restatement of
    ``prepare_beam_unpolarized`` (E-field -> power of one feed), never through the product's reduction; objects
    that are neither of this package's containers (third-party analytic beams) are handed over as they are: the
    oracle calls their ``compute_response`` at every source, as the reference does (cpu/beams.py:69-81)."""
    if isinstance(beam, fftvis_amd.AiryBeam):
        # this package's dish is DEFINED with both types (E-field e in every slot, power e^2): no reduction involved
        return orc.AiryBeam(beam.diameter, "efield" if polarized else "power")
    elif isinstance(beam, fftvis_amd.TabulatedBeam):
        ob = orc.TabulatedBeam(beam.data, freqs, beam.za_max, "efield" if beam.is_efield else "power", order)
    else:
        ob = beam
    return ob if polarized else orc.prepare_beam_unpolarized(ob, use_feed)


def oracle_simulate(cfg, fp32_inputs=False, mode="exact", coord_mgr=None):
    """Run the oracle on simulate_vis-style keyword arguments.  ``fp32_inputs=True``: on the inputs as the reference
    rounds them at the configuration's precision (``orc.simulate(precision=...)``); ``mode="scale"``: the per-element
    error scale instead of the visibilities (``oracle_scale``)."""
    beams = cfg["beam"] if isinstance(cfg["beam"], list) else [cfg["beam"]]
    order = spline_order(cfg.get("beam_spline_opts"))
    ob = [oracle_beam(b, cfg["polarized"], cfg["freqs"], order, cfg.get("use_feed", "x")) for b in beams]
    return orc.simulate(
        cfg["ants"], cfg["freqs"], cfg["fluxes"], ob, cfg["ra"], cfg["dec"], cfg["times"],
        cfg["telescope_loc"], baselines=cfg.get("baselines"), beam_idx=cfg.get("beam_idx"),
        polarized=cfg["polarized"], beam_coefs=cfg.get("beam_coefs"),
        force_use_type3=cfg.get("force_use_type3", True),
        reference_compat=cfg.get("reference_compat", True), coord_mgr=coord_mgr, mode=mode,
        precision=cfg.get("precision", 2) if fp32_inputs else 2,
    )


def oracle_scale(cfg, coord_mgr=None):
    """Per output element, the l2 norm over sources of the strength row that feeds it (``orc.simulate(mode="scale")``):
    cheap, no sums over sources times targets."""
    return oracle_simulate(cfg, mode="scale", coord_mgr=coord_mgr)


# ---------------------------------------------------------------------------------------------------------------------
# Element-wise comparison of a forward run with the oracle
# ---------------------------------------------------------------------------------------------------------------------
def floored_rel(err, exact, floor):
    """rel l2 of one part of a result; a part whose exact norm is below ``floor`` is measured against ``floor``."""
    return float(np.linalg.norm(err) / max(np.linalg.norm(exact), floor, 1e-300))


def worst_part(err, exact, axis, floor):
    """The worst ``floored_rel`` over the slices of ``axis``."""
    return max(floored_rel(np.take(err, i, axis), np.take(exact, i, axis), floor) for i in range(exact.shape[axis]))


def group_scale(scale):
    """The error scale per group of products: diagonal outputs (00, 11) take sqrt(S00^2 + S11^2), off-diagonal ones
    (01, 10) sqrt(S01^2 + S10^2).  No packing the engine does mixes the two groups."""
    if scale.ndim != 5:
        return scale
    out = np.empty_like(scale)
    out[:, :, 0, 0] = out[:, :, 1, 1] = np.hypot(scale[:, :, 0, 0], scale[:, :, 1, 1])
    out[:, :, 0, 1] = out[:, :, 1, 0] = np.hypot(scale[:, :, 0, 1], scale[:, :, 1, 0])
    return out


def max_phase(cfg):
    """Phi, the largest phase of a run: 2 pi nu_max |b|_max / c over its baselines."""
    ants = cfg["ants"]
    bls = cfg.get("baselines") or [red[0] for red in orc.get_pos_reds(ants, include_autos=True)]
    b = max(float(np.linalg.norm(np.asarray(ants[j], float) - np.asarray(ants[i], float))) for i, j in bls)
    return 2 * np.pi * float(np.max(np.abs(cfg["freqs"]))) * b / orc.speed_of_light


def error_base(cfg):
    """The unit the element-wise metrics are measured in: the run's eps in fp64; max(eps, 2^-24 Phi) in fp32, where
    the rounding of coordinates and phases to float32 moves a phase by about 2^-24 of the largest one."""
    precision = cfg.get("precision", 2)
    eps = cfg.get("eps") or orc.default_accuracy_dict[precision]
    return eps if precision == 2 else max(eps, 2.0**-24 * max_phase(cfg))


def error_family(cfg):
    """Which bound of ``FORWARD_BOUNDS`` a configuration is held to."""
    if cfg.get("precision", 2) == 1:
        return "fp32 sigma 1.25" if cfg.get("upsample_factor") == 1.25 else "fp32"
    if cfg.get("upsample_factor") == 1.25:
        return "sigma 1.25"
    if cfg.get("beam_coefs") is not None:
        return "eigenbeams"
    ants = cfg["ants"]
    z = np.array([ants[a] for a in ants], float)
    z = (z @ orc.get_plane_to_xy_rotation_matrix(z).T)[:, 2]
    if np.ptp(z) > 1e-6:
        return "3-D"
    if not cfg.get("force_use_type3", False) and orc.check_antpos_griddability(ants)[0]:
        return "lattice"
    return "2-D"


def forward_errors(got, exact, scale, base, autos=None):
    """A forward result against the oracle's exact output, in units of ``base``: rel l2 of the whole array; the worst rel l2
    of a channel, of a time step and (polarized) of a product group, each part floored at 1e-3 of the whole as in the
    adjoint's check; the largest element ratio |err| / (base scale) with the scale per product group (``group_scale``),
    over the baselines (``element``) and over the autos (``element_auto``; ``autos``: a mask over the last axis)."""
    got = np.asarray(got).astype(np.complex128)
    err = got - exact
    floor = 1e-3 * np.linalg.norm(exact)
    m = {"rel_l2": floored_rel(err, exact, floor) / base, "channel": worst_part(err, exact, 0, floor) / base,
         "time": worst_part(err, exact, 1, floor) / base}
    if exact.ndim == 5:
        d, o = (0, 1), (1, 0)
        m["product"] = max(floored_rel(err[:, :, d, d], exact[:, :, d, d], floor),
                           floored_rel(err[:, :, d, o], exact[:, :, d, o], floor)) / base
    s = group_scale(scale)
    ratio = np.abs(err) / (base * np.maximum(s, 1e-6 * s.max() + 1e-300))
    autos = np.zeros(exact.shape[-1], bool) if autos is None else np.asarray(autos, bool)
    m["element"] = float(ratio[..., ~autos].max()) if (~autos).any() else 0.0
    m["element_auto"] = float(ratio[..., autos].max()) if autos.any() else 0.0
    return m


# Element-wise bounds of ``check_forward``, in units of ``error_base`` (eps; fp32: max(eps, 2^-24 Phi)), per family:
# rel l2 of the whole array, worst rel l2 of a channel / time step / product group ("part"), largest element ratio
# |err| / (base scale) ("element"; autos included: in every family they measured at or below the other baselines).
# Measured on an MI355X over the 523 forward-vs-oracle comparisons of the three GPU forward modules (run them with
# FFTVIS_TEST_METRICS=<file> to log every comparison's metrics, one JSON line each); worst whole / part / element and
# the number of comparisons:
#   2-D                           2.88 / 7.05 / 12.8   (135)
#   2-D, gridded matrix type 3    2.53 / 8.59 / 23.1    (32)  the type-3 runs of test_simulate_gridded_type1_vs_type3 at
#       eps 1e-10: unit hex-7 and 10 m square lattices, 1 - 30 m baselines, the smallest arrays and grids of any 2-D run.
#       They run about 2x higher than every other 2-D run in part and element (the same arrays on the type-1 path
#       measure below 0.6); the cause was not isolated, so they keep a bound of their own.
#   3-D and height terms          5.94 / 5.94 / 9.98  (117)
#   lattice                       0.46 / 0.53 / 1.52   (74)
#   lattice at eps 1e-13          0.39 / 0.61 / 1.46    (2)  the default fp64 eps (C1 fixture, all-up sky)
#   sigma 1.25                    2.40 / 3.72 / 10.3   (43)
#   eigenbeams                    1.24 / 2.01 / 8.05   (19)
#   fp32                          1.48 / 2.74 / 7.92   (93)
#   fp32 at sigma 1.25            0.40 / 0.44 / 1.10    (4)
#   fp32 at sigma 1.25 below its floor  0.44 / 5.19 / 24.3  (4)  eps 6e-8 and 1e-9 asked of sigma = 1.25 in fp32, which
#       delivers about 1e-4 at best (the engine warns): the error follows that floor, not eps or Phi.
# The fp32 base: in 69 of the 93 fp32 comparisons the Phi term was the larger (2^-24 Phi / eps from 1.2 to 150: the
# gridded matrix at eps 6e-8, HERA-350's Hermitian, dedup and C5 runs at eps 1e-4); their worst whole / part / element,
# 1.48 / 1.94 / 6.74, match the eps-dominated runs' 1.02 / 2.74 / 7.92: the errors follow max(eps, 2^-24 Phi).
# Against the rounded-input oracle C1 in fp32 measures a whole-array rel l2 of 8.8e-5 at eps 1e-4 and of 0.9 - 1.0 eps at
# eps 1e-5 (the 2e-3 check of test_sim_fp32 against unrounded inputs stays as it was).  Every bound keeps a margin of at
# least 2 over its measured worst.
FORWARD_BOUNDS = {
    "2-D": {"rel_l2": 6.0, "part": 14.5, "element": 26.0},
    "2-D, gridded matrix type 3": {"rel_l2": 5.1, "part": 17.5, "element": 47.0},
    "3-D": {"rel_l2": 12.0, "part": 12.0, "element": 20.0},
    "lattice": {"rel_l2": 1.0, "part": 1.2, "element": 3.2},
    "lattice, eps 1e-13": {"rel_l2": 0.8, "part": 1.3, "element": 3.0},
    "sigma 1.25": {"rel_l2": 5.0, "part": 7.5, "element": 21.0},
    "eigenbeams": {"rel_l2": 2.5, "part": 4.1, "element": 17.0},
    "fp32": {"rel_l2": 3.0, "part": 5.5, "element": 16.0},
    "fp32 sigma 1.25": {"rel_l2": 0.8, "part": 0.9, "element": 2.2},
    "fp32 sigma 1.25, eps below its floor": {"rel_l2": 0.9, "part": 10.5, "element": 49.0},
}


def check_forward(got, cfg, exact, scale=None, sub=None, label="", family=None):
    """A forward result (``got``: the whole run of ``cfg``) element by element against the oracle: ``exact`` is the oracle's
    output on the baselines ``sub`` (indices into cfg's baselines; all by default) -- in fp32 the rounded-input oracle
    (``oracle_simulate(cfg, fp32_inputs=True)``) --, ``scale`` its ``oracle_scale`` (computed when not given).  Asserts
    every metric of ``forward_errors`` against ``FORWARD_BOUNDS`` (``family``: that bound instead of the configuration's
    ``error_family``) and returns them."""
    scfg = cfg if sub is None else dict(cfg, baselines=[cfg["baselines"][i] for i in sub])
    if scale is None:
        scale = oracle_scale(scfg)
    got = np.asarray(got) if sub is None else np.asarray(got)[..., sub]
    assert got.shape == exact.shape == scale.shape, (got.shape, exact.shape, scale.shape)
    fam, base = family or error_family(cfg), error_base(cfg)
    ants = scfg["ants"]
    bls = scfg.get("baselines") or [red[0] for red in orc.get_pos_reds(ants, include_autos=True)]
    autos = [not np.any(np.asarray(ants[i], float) != np.asarray(ants[j], float)) for i, j in bls]
    m = forward_errors(got, exact, scale, base, autos)
    if os.environ.get("FFTVIS_TEST_METRICS"):  # the calibration log ``FORWARD_BOUNDS`` was measured with
        with open(os.environ["FFTVIS_TEST_METRICS"], "a") as f:
            f.write(json.dumps(dict(m, test=os.environ.get("PYTEST_CURRENT_TEST", ""), label=str(label), family=fam,
                                    base=base, eps=cfg.get("eps"), phi_term=2.0**-24 * max_phase(cfg))) + "\n")
    b = FORWARD_BOUNDS[fam]
    info = (label, fam, base, m)
    assert m["rel_l2"] <= b["rel_l2"], info
    assert max(m["channel"], m["time"], m.get("product", 0.0)) <= b["part"], info
    assert m["element"] <= b["element"], info
    assert m["element_auto"] <= b["element"], info
    return m


def install_reference_dependency_stubs(monkeypatch):
    """Minimal stand-ins for the pieces of astropy / matvis the reference's engine touches when it builds its
    coordinate manager (cpu_simulate.py:686-709), put into ``sys.modules`` for one test: ``astropy.units``
    (``rad``, ``s``), ``astropy.time.Time(jd, format="jd")`` (indexing, differences with ``.to``),
    ``astropy.coordinates.SkyCoord`` and ``matvis.core.coords.CoordinateRotation`` with its ``_methods`` registry
    and one subclass, ``CoordinateRotationERFA``, whose vectors come from the oracle's sidereal stand-in.
    Returns the list that records every manager constructed (kwargs, ``_set_bcrs`` calls, rotations)."""
    import sys
    import types

    made = []

    class Unit:
        __array_ufunc__ = None  # ndarray * unit defers to __rmul__, as astropy's units do

        def __init__(self, name):
            self.name = name

        def __rmul__(self, other):
            return Quantity(np.asarray(other, dtype=float), self)

    class Quantity:
        def __init__(self, value, unit):
            self.value, self.unit = value, unit

        def to(self, unit):
            scale = {("d", "s"): 86400.0, ("s", "s"): 1.0, ("rad", "rad"): 1.0}[(self.unit.name, unit.name)]
            return Quantity(self.value * scale, unit)

        def __lt__(self, other):
            return self.value < (other.value if isinstance(other, Quantity) else other)

        def __gt__(self, other):
            return self.value > (other.value if isinstance(other, Quantity) else other)

    un = types.ModuleType("astropy.units")
    un.rad, un.s, un.d = Unit("rad"), Unit("s"), Unit("d")

    class Time:
        def __init__(self, val, format="jd"):
            assert format == "jd"
            self.jd = np.asarray(val, dtype=float)

        def __len__(self):
            return self.jd.size

        def __getitem__(self, i):
            return Time(self.jd[i])

        def __sub__(self, other):
            return Quantity(self.jd - other.jd, un.d)

    class SkyCoord:
        def __init__(self, ra, dec, frame):
            assert frame == "icrs" and ra.unit.name == "rad" and dec.unit.name == "rad"
            self.ra, self.dec = ra, dec

    class CoordinateRotation:
        _methods = {}

        def __init_subclass__(cls):
            CoordinateRotation._methods[cls.__name__] = cls

    class CoordinateRotationERFA(CoordinateRotation):
        def __init__(self, flux, times, telescope_loc, skycoords, chunk_size=None, source_buffer=1.0, precision=1,
                     update_bcrs_every=0.0):
            self.kw = dict(flux=flux, times=times, telescope_loc=telescope_loc, skycoords=skycoords,
                           chunk_size=chunk_size, source_buffer=source_buffer, precision=precision)
            self.update_bcrs_every = update_bcrs_every
            self.times = times
            self.bcrs_set, self.rotated, self.setup_calls = [], [], 0
            self.o = orc.SimpleCoordinateRotation(flux, times.jd, telescope_loc, skycoords.ra.value,
                                                  skycoords.dec.value)
            made.append(self)

        def _set_bcrs(self, t):
            self.bcrs_set.append(t)

        def setup(self):
            self.setup_calls += 1

        def rotate(self, ti):
            self.rotated.append(ti)
            self.o.rotate(ti)
            self.all_coords_topo = self.o._topo

    mods = {
        "astropy": types.ModuleType("astropy"), "astropy.units": un,
        "astropy.time": types.ModuleType("astropy.time"),
        "astropy.coordinates": types.ModuleType("astropy.coordinates"),
        "matvis": types.ModuleType("matvis"), "matvis.core": types.ModuleType("matvis.core"),
        "matvis.core.coords": types.ModuleType("matvis.core.coords"),
    }
    mods["astropy"].units = un
    mods["astropy.time"].Time = Time
    mods["astropy.coordinates"].SkyCoord = SkyCoord
    mods["matvis.core.coords"].CoordinateRotation = CoordinateRotation
    mods["matvis"].core = mods["matvis.core"]
    mods["matvis.core"].coords = mods["matvis.core.coords"]
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    return made, Time


def oracle_adjoint(cfg, G, full_stokes=False, sources=None, coord_mgr=None):
    """The oracle's exact A^T G (``orc.simulate_adjoint``) for simulate_vis-style keyword arguments, with the same beam
    twins as ``oracle_simulate``: (n, nfreqs) or (n, nfreqs, 4), n = nsrc or len(sources)."""
    beams = cfg["beam"] if isinstance(cfg["beam"], list) else [cfg["beam"]]
    order = spline_order(cfg.get("beam_spline_opts"))
    ob = [oracle_beam(b, cfg["polarized"], cfg["freqs"], order, cfg.get("use_feed", "x")) for b in beams]
    return orc.simulate_adjoint(
        G, cfg["ants"], cfg["freqs"], ob, cfg["ra"], cfg["dec"], cfg["times"], cfg["telescope_loc"],
        baselines=cfg.get("baselines"), beam_idx=cfg.get("beam_idx"), polarized=cfg["polarized"],
        full_stokes=full_stokes, coord_mgr=coord_mgr, force_use_type3=cfg.get("force_use_type3", True),
        reference_compat=cfg.get("reference_compat", True), nchunks=cfg.get("min_chunks", 1), sources=sources,
    )
