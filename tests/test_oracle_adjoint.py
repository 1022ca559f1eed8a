"""Pins the oracle's exact adjoint (``orc.simulate_adjoint``), which the GPU adjoint tests compare with element by
element.  Against the oracle's own forward ``orc.simulate``: the dot identity Re <A F, G> = <F, A^T G> between two
exact sums, column by column from one-source runs, and its source subsets.  CPU only."""

import numpy as np
import pytest

from fftvis_amd import synth
from oracle import fftvis_oracle as orc

BIDX = np.array([0, 1, 0, 1, 1, 0, 1])


def _case(sky, beams, array, compat, nsrc=12, nfreq=2, seed=0):
    """HERA-7 keyword arguments of ``orc.simulate`` (oracle beams), fluxes included."""
    c = synth.make_config("C1", seed=seed, nsrc=nsrc, nfreq=nfreq, ntimes=2)
    freqs = c["freqs"]
    polarized = sky != "I"
    kw = dict(ants=c["ants"], freqs=freqs, fluxes=c["fluxes"], ra=c["ra"], dec=c["dec"], times=c["times"],
              telescope_loc=c["telescope_loc"], baselines=c["baselines"], polarized=polarized,
              reference_compat=compat, force_use_type3=True)
    if sky == "full":
        kw["fluxes"] = synth.catalog(nsrc, freqs, seed, polarized_sky=True)[2]

    def beam(obj):
        return obj if polarized else orc.prepare_beam_unpolarized(obj)

    if beams == "airy":
        kw["beam_list"] = [beam(orc.AiryBeam(14.0))]
    elif beams == "two":
        kw["beam_list"] = [beam(orc.AiryBeam(14.0)), beam(orc.AiryBeam(10.0))]
        kw["beam_idx"] = BIDX
    else:  # cubic-spline table with a complex leakage term
        tab = synth.synthetic_efield_table(freqs, nza=91, naz=180)
        kw["beam_list"] = [beam(orc.TabulatedBeam(tab, freqs, order=3))]
    if array == "non_coplanar":
        h = np.random.default_rng(5).normal(size=7)
        kw["ants"] = {k: np.array([v[0], v[1], 1.5 * h[k]]) for k, v in c["ants"].items()}
        kw["baselines"] = c["baselines"] + [(3, 0), (6, 1)]
    elif array == "subset":  # every other baseline, a quarter of them reversed, and an auto
        bl = c["baselines"]
        kw["baselines"] = [bl[i] for i in range(0, len(bl), 2)] + [(b, a) for a, b in bl[1::4]] + [(0, 0)]
    elif array == "lattice":  # the forward takes the type-1 transform, the adjoint the type-3 sum
        kw["force_use_type3"] = False
        kw["baselines"] = c["baselines"] + [(3, 0), (6, 1), (2, 2)]
    else:
        kw["baselines"] = c["baselines"] + [(3, 0), (6, 1), (2, 2)]
    return kw


def _forward(kw, F):
    return orc.simulate(**dict(kw, fluxes=F))


def _adjoint(kw, G, **extra):
    a = {k: v for k, v in kw.items() if k != "fluxes"}
    return orc.simulate_adjoint(G, **a, full_stokes=np.ndim(kw["fluxes"]) == 3, **extra)


def _random_g(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("array", ["coplanar", "non_coplanar", "subset", "lattice"])
@pytest.mark.parametrize("beams", ["airy", "two", "table3"])
@pytest.mark.parametrize("sky", ["I", "polarized_I", "full"])
def test_oracle_adjoint_dot_identity(sky, beams, array, compat):
    """|Re <A F, G> - <F, A^T G>| <= 1e-12 |F| |A^T G|, both sides exact fp64 sums (the GPU test's bound,
    10 eps |A F| |G|, is far looser).  Measured worst over the matrix: 5.4e-16."""
    kw = _case(sky, beams, array, compat)
    rng = np.random.default_rng(1)
    F = rng.normal(size=np.shape(kw["fluxes"]))
    AF = _forward(kw, F)
    G = _random_g(AF.shape, 2)
    AtG = _adjoint(kw, G)
    assert AtG.shape == F.shape and AtG.dtype == np.float64
    lhs = np.vdot(G, AF).real
    rhs = float(np.sum(F * AtG))
    assert np.count_nonzero(AtG) > 0
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(F) * np.linalg.norm(AtG), (lhs, rhs)


def test_lattice_type1_forward_is_the_type3_map():
    """On a lattice the type-1 forward and the type-3 forward are one map to rounding: the adjoint's type-3 sum is the
    transpose of both."""
    kw = _case("full", "two", "lattice", False)
    t1 = _forward(kw, kw["fluxes"])
    t3 = _forward(dict(kw, force_use_type3=True), kw["fluxes"])
    assert np.linalg.norm(t1 - t3) <= 1e-13 * np.linalg.norm(t3)


def test_oracle_adjoint_columns_from_one_source_runs():
    """A^T G [s, f, k] = Re <A e_sk, G> with A e_sk the oracle's forward of source s alone at unit Stokes k: full Stokes,
    two complex-Jones table beams, the exact flipped forms, flipped and exactly duplicated baselines."""
    c = synth.make_config("C1", nsrc=6, nfreq=2, ntimes=2)
    freqs = c["freqs"]
    tabs = [orc.TabulatedBeam(synth.synthetic_efield_table(freqs, d, nza=91, naz=180), freqs) for d in (14.0, 10.0)]
    bl = c["baselines"] + [(1, 0), (3, 0), (0, 1), (0, 1), (4, 4), (2, 5)]
    kw = dict(ants=c["ants"], freqs=freqs, beam_list=tabs, times=c["times"], telescope_loc=c["telescope_loc"],
              baselines=bl, beam_idx=BIDX, polarized=True, reference_compat=False)
    nsrc, nf = 6, 2
    G = _random_g((nf, 2, 2, 2, len(bl)), 3)
    got = orc.simulate_adjoint(G, ra=c["ra"], dec=c["dec"], full_stokes=True, **kw)
    exp = np.zeros((nsrc, nf, 4))
    for s in range(nsrc):
        for k in range(4):
            unit = np.zeros((1, nf, 4))
            unit[..., k] = 1.0
            col = orc.simulate(fluxes=unit, ra=c["ra"][s:s + 1], dec=c["dec"][s:s + 1], **kw)
            exp[s, :, k] = [np.vdot(G[f], col[f]).real for f in range(nf)]  # block-diagonal in frequency
    assert np.count_nonzero(exp) > 0
    assert np.abs(got - exp).max() <= 1e-12 * np.abs(exp).max()


def test_oracle_adjoint_source_subset_and_chunks():
    """``sources=`` rows are the same rows of the full result (to the rounding of a narrower product), in the order asked
    for; source chunks change nothing."""
    kw = _case("full", "two", "coplanar", True, nsrc=15)
    G = _random_g((2, 2, 2, 2, len(kw["baselines"])), 4)
    full = _adjoint(kw, G)
    rows = np.array([13, 2, 7, 0, 14])
    assert np.abs(_adjoint(kw, G, sources=rows) - full[rows]).max() <= 1e-14 * np.abs(full).max()
    assert np.abs(_adjoint(kw, G, nchunks=4) - full).max() <= 1e-14 * np.abs(full).max()
