"""Pins the oracle's per-element error scale (``orc.simulate(mode="scale")``), which the GPU forward tests divide their
element-wise errors by, and its fp32 inputs (``orc.simulate(precision=1)``) against what the engine's host code makes
of the same inputs.  CPU only."""

import numpy as np
import pytest

from fftvis_amd import synth
from oracle import fftvis_oracle as orc
from tests.test_oracle_adjoint import _case


def _one_source(kw, s):
    f = kw["fluxes"]
    return dict(kw, ra=kw["ra"][s:s + 1], dec=kw["dec"][s:s + 1], fluxes=f[s:s + 1])


def _up_everywhere(kw):
    """A catalog row above the horizon at every time step."""
    rot = orc.SimpleCoordinateRotation(None, kw["times"], kw["telescope_loc"], kw["ra"], kw["dec"])
    up = []
    for ti in range(len(kw["times"])):
        rot.rotate(ti)
        up.append(rot._topo[2])
    return int(np.flatnonzero(np.all(np.array(up) > 0, axis=0))[0])


VARIANTS = [("I", "airy", "coplanar", True), ("polarized_I", "table3", "coplanar", True),
            ("full", "table3", "coplanar", True), ("full", "two", "subset", True), ("full", "two", "subset", False),
            ("polarized_I", "two", "coplanar", False), ("full", "airy", "non_coplanar", True),
            ("I", "airy", "lattice", True), ("full", "two", "lattice", False)]


@pytest.mark.parametrize("sky,beams,array,compat", VARIANTS)
def test_one_source_scale_is_the_visibility_modulus(sky, beams, array, compat):
    """With one source the strength row that feeds an element has one entry, so the scale is |V| element by element:
    unpolarized, polarized with a Stokes-I sky, a full-Stokes sky, two beams with flipped baselines in both forms,
    3-D, the type-1 lattice path."""
    kw = _case(sky, beams, array, compat)
    one = _one_source(kw, _up_everywhere(kw))
    vis = orc.simulate(**one)
    sc = orc.simulate(**one, mode="scale")
    assert sc.shape == vis.shape and sc.dtype == np.float64
    np.testing.assert_allclose(sc, np.abs(vis), rtol=1e-12, atol=1e-14 * np.abs(vis).max())
    assert np.abs(vis).max() > 0


@pytest.mark.parametrize("compat", [True, False])
def test_one_source_eigenbeam_scale_bounds_the_visibility(compat):
    """Eigenbeam terms add with weights |a1 a2|: the scale is at least |V| (the triangle inequality), and above it
    where the terms do not line up."""
    kw = _case("full", "two", "coplanar", compat)
    kw.pop("beam_idx")
    rng = np.random.default_rng(3)
    coefs = rng.normal(size=(7, 2, 2)) + 1j * rng.normal(size=(7, 2, 2))
    one = dict(_one_source(kw, _up_everywhere(kw)), beam_coefs=coefs)
    vis = orc.simulate(**one)
    sc = orc.simulate(**one, mode="scale")
    assert np.all(sc >= np.abs(vis) * (1 - 1e-12) - 1e-14 * np.abs(vis).max())
    assert np.any(sc > 1.01 * np.abs(vis))


@pytest.mark.parametrize("sky,beams,array,compat", [("full", "two", "subset", False), ("I", "airy", "lattice", True),
                                                    ("polarized_I", "table3", "non_coplanar", True)])
def test_scale_squares_add_over_disjoint_sources(sky, beams, array, compat):
    """The squared scales of two disjoint parts of a catalog add up to the whole's, and so do source chunks."""
    kw = _case(sky, beams, array, compat, nsrc=20)
    whole = orc.simulate(**kw, mode="scale")
    a, b = np.arange(0, 20, 3), np.setdiff1d(np.arange(20), np.arange(0, 20, 3))
    parts = [orc.simulate(**dict(kw, ra=kw["ra"][p], dec=kw["dec"][p], fluxes=kw["fluxes"][p]), mode="scale")
             for p in (a, b)]
    np.testing.assert_allclose(parts[0] ** 2 + parts[1] ** 2, whole**2, rtol=1e-12, atol=1e-14 * whole.max() ** 2)
    np.testing.assert_allclose(orc.simulate(**kw, mode="scale", nchunks=3), whole, rtol=1e-12)


def test_fp32_inputs_are_what_the_engine_derives():
    """``precision=1`` feeds the oracle ra, dec, freqs, antenna positions and the coherency rounded as the reference
    rounds them.  The engine's host code derives its fp32 baselines from the same rounded positions (``prepare_array``
    gives the same bits from the oracle's rounded positions as from the unrounded ones), and they agree with the
    oracle's fp64 baselines of those positions to float32 rounding; its fp32 coherency is the oracle's bit for bit.  The
    rounding moves a run: the rounded-input oracle is a different answer."""
    from fftvis_amd.core import utils
    from fftvis_amd.gpu.gpu_simulate import prepare_array

    cfg = synth.make_config("C2", nsrc=50, nfreq=3, ntimes=1, z_scatter=0.05)
    ants, bls = cfg["ants"], cfg["baselines"]
    rounded = {k: orc.fp32_rounded(v) for k, v in ants.items()}
    R32, b32, cop32 = prepare_array(ants, bls, 1e-6, np.float32)
    Rr, br, copr = prepare_array(rounded, bls, 1e-6, np.float32)
    assert b32.dtype == np.float32 and np.array_equal(b32, br) and np.array_equal(R32, Rr) and cop32 == copr
    antvecs = orc.fp32_rounded(np.array([ants[a] for a in ants]))
    R = orc.get_plane_to_xy_rotation_matrix(antvecs).T
    key = {a: i for i, a in enumerate(ants)}
    rot = R @ antvecs.T
    bo = np.array([rot[:, key[j]] - rot[:, key[i]] for i, j in bls]).T / orc.speed_of_light
    assert np.abs(b32 - bo).max() <= 4 * 2.0**-24 * np.abs(bo).max()
    # the coherency of the oracle's precision = 1 path equals what the engine's host code hands the device in fp32
    # (SimHandle.set_sources: complex64 for a polarized sky, float32 otherwise)
    _, _, fl4 = synth.catalog(50, cfg["freqs"], 1, polarized_sky=True)
    for fl, pol in ((fl4, True), (cfg["fluxes"], False)):
        coh, pol_sky = utils.prepare_source_catalog(fl, pol)
        dev = np.ascontiguousarray(coh, dtype=np.complex64 if pol_sky else np.float32)
        ours = orc.fp32_coherency(orc.prepare_source_catalog(fl, pol)[0])
        assert np.array_equal(ours, dev.astype(complex)), pol
    c1 = synth.make_config("C1", nsrc=30, nfreq=2, ntimes=1)
    kw = dict(ants=c1["ants"], freqs=c1["freqs"], fluxes=c1["fluxes"], beam_list=[orc.AiryBeam(14.0, "power")],
              ra=c1["ra"], dec=c1["dec"], times=c1["times"], telescope_loc=c1["telescope_loc"],
              baselines=c1["baselines"])
    v64, v32 = orc.simulate(**kw), orc.simulate(**kw, precision=1)
    d = np.linalg.norm(v32 - v64) / np.linalg.norm(v64)
    assert 1e-9 < d < 1e-5, d
    np.testing.assert_array_equal(orc.simulate(**kw, precision=1, mode="scale") > 0, orc.simulate(**kw, mode="scale") > 0)
