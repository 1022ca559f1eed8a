"""GPU tests of the adjoint (``simulate_vis_adjoint``, ``torch_simulate_vis``, ``fv_sim_run_adjoint``).

The adjoint is defined by the real inner products: Re <A F, G> = <F, A^T G> for real F and complex G, with A the map
``simulate_vis`` computes from ``fluxes``.  Checked through that identity against the forward over the configuration
matrix, column by column against the oracle's forward, at HERA-350 scale, through torch's gradcheck, and for
reproducibility and its edge cases."""

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from oracle import fftvis_oracle as orc
from tests.helpers import oracle_beam, oracle_simulate, rel_l2

pytestmark = pytest.mark.gpu


def _random_g(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)


def _adj_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k != "fluxes"}


def _base(nsrc=60, nfreq=3, ntimes=2, seed=0):
    return synth.make_config("C1", seed=seed, nsrc=nsrc, nfreq=nfreq, ntimes=ntimes)


def _config(polarized, sky, beams, array, precision, compat):
    c1 = _base()
    freqs = c1["freqs"]
    cfg = dict(c1, polarized=polarized, precision=precision, reference_compat=compat,
               eps=6e-8 if precision == 2 else 1e-5)
    if sky == "full":
        _, _, cfg["fluxes"] = synth.catalog(60, freqs, 0, polarized_sky=True)
    bidx = np.array([0, 1, 0, 1, 1, 0, 1])
    if beams == "airy":
        cfg["beam"] = fftvis_amd.AiryBeam(14.0)
    elif beams == "two":
        cfg["beam"] = [fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(10.0)]
        cfg["beam_idx"] = bidx
    else:  # tabulated, cubic spline
        cfg["beam"] = fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, nza=91, naz=180), freqs)
        cfg["beam_spline_opts"] = {"order": 3}
    if array == "coplanar":
        cfg["force_use_type3"] = False  # a lattice: the forward takes the type-1 path, the adjoint type 3
        cfg["baselines"] = c1["baselines"] + [(3, 0), (6, 1), (2, 2)]  # flipped pairs and an auto
    elif array == "coplanar_type3":  # the same array with the forward on the 2-D type-3 path (the production path)
        cfg["force_use_type3"] = True
        cfg["baselines"] = c1["baselines"] + [(3, 0), (6, 1), (2, 2)]
    elif array == "non_coplanar":
        hrng = np.random.default_rng(5)
        cfg["ants"] = {k: np.array([v[0], v[1], 1.5 * hrng.normal()]) for k, v in c1["ants"].items()}
        cfg["baselines"] = c1["baselines"] + [(3, 0), (6, 1)]
    else:  # a subset, partly reversed
        bl = c1["baselines"]
        cfg["baselines"] = [bl[i] for i in range(0, len(bl), 2)] + [(b, a) for a, b in bl[1::4]] + [(0, 0)]
    return cfg


def _dot_check(cfg, seed=3, tol_eps=None):
    """|Re <A F, G> - <F, A^T G>| <= 10 eps |A F| |G| with seeded random real F and complex G."""
    rng = np.random.default_rng(seed)
    F = rng.normal(size=np.shape(cfg["fluxes"]))
    AF = fftvis_amd.simulate_vis(**dict(cfg, fluxes=F))
    G = _random_g(AF.shape, AF.dtype, seed + 1)
    full = F.ndim == 3
    AtG = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg), full_stokes=full)
    assert AtG.shape == F.shape
    assert AtG.dtype == (np.float32 if cfg["precision"] == 1 else np.float64)
    lhs = np.vdot(G.astype(np.complex128), AF.astype(np.complex128)).real
    rhs = float(np.sum(F * AtG.astype(np.float64)))
    eps = tol_eps or cfg["eps"]
    bound = 10 * eps * np.linalg.norm(AF) * np.linalg.norm(G)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    return F, G, AtG


SKIES = [(False, "I"), (True, "I"), (True, "full")]


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("array", ["coplanar", "coplanar_type3", "non_coplanar", "subset"])
@pytest.mark.parametrize("beams", ["airy", "two", "table3"])
@pytest.mark.parametrize("polarized,sky", SKIES)
def test_adjoint_dot_identity(gpu, polarized, sky, beams, array, precision, compat):
    _dot_check(_config(polarized, sky, beams, array, precision, compat))


@pytest.mark.parametrize("polarized", [False, True])
def test_adjoint_matches_oracle_columns(gpu, polarized):
    """HERA-7, 30 sources, 4 channels, 2 times: A^T G against the transpose built column by column from the oracle's
    forward (one unit source at a time; the map is block-diagonal in frequency)."""
    cfg = dict(synth.make_config("C1", nsrc=30, nfreq=4, ntimes=2), polarized=polarized)
    nsrc, nf = cfg["fluxes"].shape
    shape = (nf, 2, 2, 2, len(cfg["baselines"])) if polarized else (nf, 2, len(cfg["baselines"]))
    G = _random_g(shape, np.complex128, 11)
    got = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
    exp = np.zeros((nsrc, nf))
    for s in range(nsrc):
        col = oracle_simulate(dict(cfg, fluxes=np.ones((1, nf)), ra=cfg["ra"][s:s + 1], dec=cfg["dec"][s:s + 1]))
        for f in range(nf):
            exp[s, f] = np.vdot(col[f], G[f]).real  # Re sum conj(A e_sf) G
    assert rel_l2(got, exp) <= 10 * cfg["eps"]


def test_adjoint_at_scale_hera350(gpu):
    """HERA-350, 1e5 sources, polarized, 2 channels, 2 times: the dot identity, and the gradient at 20 seeded sources
    against Re sum conj(A e_s) G with A e_s the oracle's direct sum."""
    cfg = synth.make_config("C3", nsrc=100_000, nfreq=2, ntimes=2)
    F, G, AtG = _dot_check(cfg, seed=21)
    rng = np.random.default_rng(4)
    # sources above the horizon at some time are the informative ones: pick among those with a nonzero gradient
    live = np.flatnonzero(np.any(AtG != 0, axis=1))
    pick = rng.choice(live, 20, replace=False)
    beams = [oracle_beam(cfg["beam"], True, cfg["freqs"])]
    exp = np.zeros((len(pick), 2))
    for n, s in enumerate(pick):
        col = orc.simulate(cfg["ants"], cfg["freqs"], np.ones((1, 2)), beams, cfg["ra"][s:s + 1], cfg["dec"][s:s + 1],
                           cfg["times"], cfg["telescope_loc"], baselines=cfg["baselines"], polarized=True)
        exp[n] = [np.vdot(col[f], G[f]).real for f in range(2)]
    assert rel_l2(AtG[pick], exp) <= 10 * cfg["eps"]


HERA350_CASES = {
    # two beams (flipped pairs; the forward packs the real-Jones pair), full Stokes, the exact flipped forms
    "two_beams_full_stokes_exact": dict(beams="two", full=True, compat=False, precision=2),
    "table_stokes_i_fp32": dict(beams="table", full=False, compat=True, precision=1),
}


@pytest.mark.parametrize("name", list(HERA350_CASES))
def test_adjoint_dot_identity_hera350(gpu, name):
    """The dot identity on HERA-350 (the 2-D type-3 forward with its Hermitian / real packings and column plans) for
    the flips, skies, reference_compat forms and precisions the single full-scale case above does not take."""
    c = HERA350_CASES[name]
    cfg = synth.make_config("C3", nsrc=20_000, nfreq=2, ntimes=2)
    cfg.update(reference_compat=c["compat"], precision=c["precision"], eps=6e-8 if c["precision"] == 2 else 1e-5)
    if c["beams"] == "two":
        cfg["beam"] = [fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(12.0)]
        cfg["beam_idx"] = np.arange(len(cfg["ants"])) % 2
    if c["full"]:
        _, _, cfg["fluxes"] = synth.catalog(20_000, cfg["freqs"], 0, polarized_sky=True)
    _dot_check(cfg, seed=31)


def test_channel_blocks_match_one_block(gpu, monkeypatch):
    """Accumulators bounded by FFTVIS_HIP_ADJ_ACC_BYTES: a run in one-channel blocks agrees with the run in one block
    (to the transforms' accuracy: a block groups its channels on grids of its own)."""
    cfg = dict(_base(nsrc=200, nfreq=5, ntimes=3), polarized=True)
    _, _, cfg["fluxes"] = synth.catalog(200, cfg["freqs"], 0, polarized_sky=True)
    G = _random_g((5, 3, 2, 2, len(cfg["baselines"])), np.complex128, 9)
    one = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg), full_stokes=True)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(8 * 8 * 200))  # one channel of a coherency sky per block
    blocks = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg), full_stokes=True)
    assert rel_l2(blocks, one) <= 10 * cfg["eps"]


def test_adjoint_gives_its_device_memory_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after an adjoint call what it held before, but
    for the adjoint plans' tables and per-baseline arrays: no grid, accumulator or staged buffer stays."""
    import ctypes

    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = dict(_base(), polarized=True)
    AF = fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    fftvis_amd.simulate_vis_adjoint(_random_g(AF.shape, AF.dtype, 1), **_adj_kwargs(cfg))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


@pytest.mark.parametrize("full", [False, True])
def test_torch_gradcheck(gpu, full):
    import torch

    cfg = _base(nsrc=5, nfreq=2, ntimes=1)
    cfg.update(eps=1e-12, polarized=full)
    kw = _adj_kwargs(cfg)
    rng = np.random.default_rng(8)
    F = torch.tensor(rng.uniform(0.5, 1.5, (5, 2, 4) if full else (5, 2)), dtype=torch.float64, device="cuda",
                     requires_grad=True)
    assert torch.autograd.gradcheck(lambda f: fftvis_amd.torch_simulate_vis(f, **kw), (F,), eps=1e-3, atol=1e-7,
                                    rtol=1e-6)
    out = fftvis_amd.torch_simulate_vis(F, **kw)
    assert out.device == F.device and out.is_complex()


def test_device_tensor_input_matches_host(gpu):
    import torch

    cfg = dict(_base(), polarized=True)
    AF = fftvis_amd.simulate_vis(**cfg)
    G = _random_g(AF.shape, AF.dtype, 2)
    host = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg), full_stokes=False)
    dev = fftvis_amd.simulate_vis_adjoint(torch.from_numpy(G).cuda(), **_adj_kwargs(cfg))
    assert dev.device.type == "cuda"
    assert np.array_equal(dev.cpu().numpy(), host)
    cpu = fftvis_amd.simulate_vis_adjoint(torch.from_numpy(G), **_adj_kwargs(cfg))  # a host tensor gives a host tensor
    assert isinstance(cpu, torch.Tensor) and cpu.device.type == "cpu"
    assert np.array_equal(cpu.numpy(), host)
    # a non-contiguous device tensor (its contiguous copy is made on torch's stream) gives the same result
    Gt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(G, 1, 0))).cuda().movedim(0, 1)
    assert not Gt.is_contiguous()
    assert np.array_equal(fftvis_amd.simulate_vis_adjoint(Gt, **_adj_kwargs(cfg)).cpu().numpy(), host)


def test_lanes_reproducible(gpu, monkeypatch):
    cfg = dict(_base(nsrc=200, ntimes=4), polarized=True)
    G = _random_g((3, 4, 2, 2, len(cfg["baselines"])), np.complex128, 5)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
        b = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
        assert np.array_equal(a, b), lanes
        res[lanes] = a
    assert rel_l2(res["1"], res["2"]) < 1e-14


def test_sources_that_never_rise_are_zero(gpu):
    cfg = _base()
    dec = cfg["dec"].copy()
    dec[:10] = np.deg2rad(75.0)  # circumpolar below the horizon at HERA's latitude (-30.7 deg)
    cfg["dec"] = dec
    G = _random_g((3, 2, len(cfg["baselines"])), np.complex128, 6)
    got = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
    assert np.all(got[:10] == 0.0)
    assert np.count_nonzero(got[10:]) > 0


def test_nan_input_fails(gpu):
    cfg = _base()
    G = _random_g((3, 2, len(cfg["baselines"])), np.complex128, 7)
    G[1, 0, 3] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="NaN"):
        fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
    # the handle stays usable
    G[1, 0, 3] = 0
    assert np.all(np.isfinite(fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))))
