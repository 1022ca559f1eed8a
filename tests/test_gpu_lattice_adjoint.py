"""GPU tests of the lattice path's type-2 adjoint: ``simulate_vis_adjoint(..., adjoint_path="type2")``.

On a flat, griddable array the forward is a type-1 transform; its transpose is a type-2 transform: mode fill, the pruned
FFT the other way round, a periodic gather at the (source, channel) entries (``k_t2_fill``, ``k_t2_gather``).  Every
result here is compared element by element with the oracle's exact transpose through the metrics and bounds of
``tests/test_gpu_adjoint.py`` (``_adjoint_errors``: whole, worst channel, worst Stokes component, largest element; fp64
10 eps, fp32 ``K32`` / ``K32_CHANNEL`` / ``C_MAX`` times the type-1 forward's own error on the same configuration), and
with the type-1 forward through the dot identity.  Every comparison prints its figures, as ratio / base, before it
asserts.

Measured on an MI355X over every comparison of this file, as ratio / base (the worst of each metric):
  fp64 (base = eps; bound 10, sigma 1.25: 20): whole 0.09, channel 0.72, Stokes 0.17, largest element 0.11; HERA-350:
    0.07, 0.07, -, 0.06; sigma 1.25: 0.003; the torch backward: 0.08, 0.11, 0.12, 0.10;
  fp32 (base = the type-1 forward's own error or eps, whichever is larger: 1.0e-5 on HERA-7, 2.2e-5 on HERA-350): whole
    1.27 (HERA-350 0.97), channel 1.37 (1.76), Stokes 0.88, largest element 1.39 (1.45), against K32 = 8,
    K32_CHANNEL = 30, C_MAX = 6: the existing constants hold with a margin of more than 4, none was widened;
  type 2 against type 3 on the same inputs, fp64: at most 0.33 eps (bound 20 eps);
  the dot identity: below 5e-4 of its bound (10 eps |A F| |G|, loose for random F and G);
  periodic wrap (HERA-7: planes of n2 = 48 = 3 x 16, w = 9): of 60 sources, 8 / 13 have a footprint across the low x / y
    edge at some (time, channel) and 12 / 15 across the high one.
"""

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from fftvis_amd.core.antenna_gridding import check_antpos_griddability
from fftvis_amd.core import utils
from oracle import fftvis_oracle as orc
from tests.helpers import oracle_adjoint, oracle_simulate, rel_l2
from tests.test_gpu_adjoint import (C_MAX, K32, K32_CHANNEL, SKIES, _adj_kwargs, _adjoint_errors, _assert_metrics, _base,
                                    _config, _edge_cfg, _forward_error, _random_g, _sources_to_check, _up)

pytestmark = pytest.mark.gpu


def _adjoint(G, cfg, path="type2", **kw):
    return fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg), adjoint_path=path, **kw)


def _handle():
    """The handle the last call used (the only idle one: acquiring a handle closes the others)."""
    from fftvis_amd.gpu import gpu_simulate

    (h,) = gpu_simulate._IDLE_HANDLES.values()
    return h


def _close(label, cfg, G, AtG, F=None, AF=None, sources=None, k64=10.0, coord_mgr=None):
    """A^T G (rows ``sources``) against the oracle's exact transpose: ``test_gpu_adjoint._assert_close_to_oracle`` with
    the figures printed first."""
    exact = oracle_adjoint(cfg, np.asarray(G).astype(np.complex128), full_stokes=np.ndim(AtG) == 3, sources=sources,
                           coord_mgr=coord_mgr)
    assert np.count_nonzero(exact) > 0
    got = AtG if sources is None else AtG[sources]
    if cfg.get("precision", 2) == 2:
        base, k, kc = cfg["eps"], k64, k64
    else:
        base, k, kc = max(_forward_error(cfg, F, AF), cfg["eps"]), K32, K32_CHANNEL
    m = _adjoint_errors(got, exact)
    print("type-2 adjoint", label, "base %.3e" % base, {key: round(v / base, 3) for key, v in m.items()})
    _assert_metrics(m, base, k, kc)
    return m


def _dot(label, cfg, seed=3, sources=None, against_type3=False):
    """|Re <A F, G> - <F, A^T G>| <= 10 eps |A F| |G| with the type-1 forward (``_dot_check``'s tolerance), then A^T G
    element-wise against the oracle."""
    assert cfg["force_use_type3"] is False
    rng = np.random.default_rng(seed)
    F = rng.normal(size=np.shape(cfg["fluxes"]))
    AF = fftvis_amd.simulate_vis(**dict(cfg, fluxes=F))
    G = _random_g(AF.shape, AF.dtype, seed + 1)
    full = F.ndim == 3
    AtG = _adjoint(G, cfg, full_stokes=full)
    assert _handle().last_adjoint_path() == 2
    assert AtG.shape == F.shape and AtG.dtype == (np.float32 if cfg["precision"] == 1 else np.float64)
    lhs = np.vdot(G.astype(np.complex128), AF.astype(np.complex128)).real
    rhs = float(np.sum(F * AtG.astype(np.float64)))
    bound = 10 * cfg["eps"] * np.linalg.norm(AF) * np.linalg.norm(G)
    print("type-2 adjoint", label, "dot identity / bound %.2e" % (abs(lhs - rhs) / bound))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    if sources is None and len(F) > 2000:
        sources = _sources_to_check(cfg)
    _close(label, cfg, G, AtG, F, AF, sources=sources)
    if against_type3:  # each is within 10 eps of the exact transpose
        t3 = _adjoint(G, cfg, "type3", full_stokes=full)
        assert _handle().last_adjoint_path() == 3
        d = rel_l2(AtG if sources is None else AtG[sources], t3 if sources is None else t3[sources])
        print("type-2 adjoint", label, "against type 3 / eps %.3f" % (d / cfg["eps"]))
        assert d <= 20 * cfg["eps"]
    return F, G, AtG


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("beams", ["airy", "two", "table3"])
@pytest.mark.parametrize("polarized,sky", SKIES)
def test_matrix_dot_identity_and_oracle(gpu, polarized, sky, beams, precision, compat):
    """The lattice with flipped pairs and an auto: per-pair mode planes, the conjugated and (compat off) transposed
    flips; in fp64 also type 2 against type 3 on the same inputs."""
    cfg = _config(polarized, sky, beams, "coplanar", precision, compat)
    _dot(f"matrix {sky} pol={polarized} {beams} fp{32 * precision} compat={compat}", cfg, against_type3=precision == 2)


def test_the_path_is_the_one_asked_for(gpu):
    cfg = _config(True, "I", "two", "coplanar", 2, True)
    G = _random_g((3, 2, 2, 2, len(cfg["baselines"])), np.complex128, 4)
    default = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
    assert _handle().last_adjoint_path() == 3
    t3 = _adjoint(G, cfg, "type3")
    assert _handle().last_adjoint_path() == 3 and np.array_equal(default, t3)
    auto = _adjoint(G, cfg, "auto")
    assert _handle().last_adjoint_path() == 2
    t2 = _adjoint(G, cfg, "type2")
    assert _handle().last_adjoint_path() == 2 and np.array_equal(auto, t2)
    assert not np.array_equal(t2, t3) and rel_l2(t2, t3) <= 20 * cfg["eps"]
    # a default call on the handle that last ran type 2 is the type-3 transform again, bit for bit
    assert np.array_equal(fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg)), default)
    assert _handle().last_adjoint_path() == 3


def _not_lattice_cases():
    forced = _config(True, "I", "two", "coplanar", 2, True)
    forced["force_use_type3"] = True
    non = dict(_config(True, "I", "two", "non_coplanar", 2, True), force_use_type3=False)  # not flat
    sc = dict(synth.make_config("C3", nsrc=300, nfreq=2, ntimes=2, array="scattered350"), force_use_type3=False)  # no lattice
    rng = np.random.default_rng(2)
    sc["baselines"] = [sc["baselines"][i] for i in sorted(rng.choice(len(sc["baselines"]), 200, replace=False))]
    return {"force_use_type3": forced, "non_coplanar": non, "scattered350": sc}


@pytest.mark.parametrize("name", ["force_use_type3", "non_coplanar", "scattered350"])
def test_auto_is_type3_off_the_lattice_and_type2_refuses(gpu, name):
    cfg = _not_lattice_cases()[name]
    nbl = len(cfg["baselines"])
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    G = _random_g((nf, nt, 2, 2, nbl) if cfg["polarized"] else (nf, nt, nbl), np.complex128, 5)
    default = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg))
    auto = _adjoint(G, cfg, "auto")
    assert _handle().last_adjoint_path() == 3
    assert np.array_equal(auto, default)
    with pytest.raises(ValueError, match="type2"):
        _adjoint(G, cfg, "type2")


@pytest.mark.parametrize("precision", [2, 1])
def test_hera350(gpu, precision):
    """HERA-350, all 61 075 baselines (7 957 modes, n_modes = 241: planes of n2 = 512, the register-resident FFT passes
    with every output kept), polarized, 20 000 sources, 2 channels, 2 times: the dot identity, and ~64 chosen sources
    against the oracle."""
    cfg = synth.make_config("C3", nsrc=20_000, nfreq=2, ntimes=2)
    assert len(cfg["baselines"]) == 61075
    cfg.update(force_use_type3=False, precision=precision, eps=6e-8 if precision == 2 else 1e-5)
    _dot(f"HERA-350 fp{32 * precision}", cfg, seed=21, against_type3=precision == 2)
    st = _handle().stats()
    assert st["n2x"] == 512 and st["n2z"] == 248 * 65536 + 248, st


def _edge(nsrc=61, nfreq=3, ntimes=2, **kw):
    """``test_gpu_adjoint._edge_cfg`` on the lattice path: HERA-7, full-Stokes sky, two complex-Jones table beams with
    flipped pairs and an auto, the exact flipped forms, fp64."""
    return dict(_edge_cfg(nsrc=nsrc, nfreq=nfreq, ntimes=ntimes), force_use_type3=False, **kw)


def _adjoint_of_random(cfg, seed=12, path="type2", **kw):
    shape = (len(cfg["freqs"]), len(cfg["times"]), 2, 2, len(cfg["baselines"]))
    G = _random_g(shape, np.complex128, seed)
    return G, _adjoint(G, cfg, path, full_stokes=True, **kw)


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_source_chunks(gpu, monkeypatch, lanes):
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    cfg = _edge(nsrc=61, ntimes=4, min_chunks=3)
    G, AtG = _adjoint_of_random(cfg)
    _close(f"chunks lanes {lanes}", cfg, G, AtG)


def test_several_frequency_batches(gpu, monkeypatch):
    """FFTVIS_HIP_GRID_BYTES small enough for one channel per batch: five batches per (time, pair) instead of one."""
    from fftvis_amd.gpu import gpu_simulate

    cfg = _edge(nsrc=40, nfreq=5)
    gpu_simulate.release_handles()
    G, one = _adjoint_of_random(cfg)
    h = _handle()
    n2 = int(h.stats()["n2x"])
    launches_one = h.stats()["spread_launches"]
    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_GRID_BYTES", str(2 * n2 * n2 * 4 * 16))  # two buffers of four planes: one channel
    _, many = _adjoint_of_random(cfg)
    launches_many = _handle().stats()["spread_launches"]
    gpu_simulate.release_handles()
    nt = 2  # one launch per (time, batch, beam pair)
    assert launches_one >= 2 * nt and launches_many == 5 * launches_one, (launches_one, launches_many)
    _close("frequency batches", cfg, G, many)
    assert rel_l2(many, one) <= 1e-12  # a channel's transform does not depend on its batch


@pytest.mark.parametrize("block_ch", [5, 1, 2])
def test_channel_blocks(gpu, monkeypatch, block_ch):
    cfg = _edge(nsrc=40, nfreq=5)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * 8 * 8 * 40))  # doubles x coherency reals x sources
    G, AtG = _adjoint_of_random(cfg)
    _close(f"channel blocks of {block_ch}", cfg, G, AtG)


def test_upsample_125(gpu):
    """upsample_factor = 1.25 (run_type1 takes an explicit sigma), at the forward's sigma = 1.25 tolerance of 20 eps."""
    cfg = _edge(upsample_factor=1.25)
    G, AtG = _adjoint_of_random(cfg)
    assert _handle().stats()["upsample_used"] == 1.25
    _close("sigma 1.25", cfg, G, AtG, k64=20.0)


def test_empty_time_step_and_sources_that_never_rise(gpu):
    cfg = _edge()
    t0 = cfg["times"][0]
    lst = orc.gmst_rad(t0) + synth.HERA_LON
    rng = np.random.default_rng(1)
    # around the meridian at the first time: half a sidereal day later all are below the horizon
    set_ = dict(cfg, ra=lst + rng.uniform(-0.3, 0.3, 61), dec=synth.HERA_LAT + rng.uniform(-0.3, 0.3, 61),
                times=t0 + np.array([0.0, 0.25, 0.5]))
    up = _up(set_)
    assert np.any(up[0] > 0) and not np.any(up[-1] > 0)
    G, AtG = _adjoint_of_random(set_)
    _close("empty time step", set_, G, AtG)
    never = _base()
    dec = never["dec"].copy()
    dec[:10] = np.deg2rad(75.0)  # circumpolar below the horizon at HERA's latitude
    never = dict(never, dec=dec, force_use_type3=False)
    G = _random_g((3, 2, len(never["baselines"])), np.complex128, 6)
    got = _adjoint(G, never)
    assert np.all(got[:10] == 0.0) and np.count_nonzero(got[10:]) > 0
    _close("never rise", never, G, got)


def test_coord_mgr_and_device_astrometry(gpu):
    from oracle import astrometry as oa

    cfg = _edge(ntimes=3)
    eq = orc.eq_unit_vectors(cfg["ra"], cfg["dec"])
    ctxs = np.stack([oa.plausible_context(20 + t, synth.HERA_LAT) for t in range(3)])

    class Mgr:  # the slice of matvis' manager the engine consumes
        def setup(self):
            pass

        def rotate(self, ti):
            self.all_coords_topo = oa.icrs_to_enu(eq, ctxs[ti])

    kw = dict(cfg, coord_method="CoordinateRotationERFA")
    G, host = _adjoint_of_random(kw, coord_mgr=Mgr())
    assert _handle().last_adjoint_path() == 2
    _, dev = _adjoint_of_random(kw, astrom=ctxs, device_astrometry=True)
    _close("coord_mgr", cfg, G, host, coord_mgr=Mgr())
    _close("device astrometry", cfg, G, dev, coord_mgr=Mgr())
    assert rel_l2(host, _adjoint_of_random(cfg)[1]) > 1e-3  # and it is not the sidereal answer


def test_periodic_wrap(gpu):
    """Footprints that cross either edge of the periodic planes in both dimensions: origins recomputed on the host with
    t1_origin's formula from what the engine is given (lattice basis in seconds, topocentric vectors, channels) and the
    plane size and kernel width the run reports."""
    cfg = dict(_base(), force_use_type3=False)
    G = _random_g((3, 2, len(cfg["baselines"])), np.complex128, 8)
    AtG = _adjoint(G, cfg)
    st = _handle().stats()
    n2, w = int(st["n2x"]), int(st["w"])
    ok, _, basis = check_antpos_griddability({k: np.asarray(v) for k, v in cfg["ants"].items()})
    assert ok
    B = (basis / utils.speed_of_light).astype(np.float64)
    rot = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    low = np.zeros((2, len(cfg["ra"])), bool)
    high = np.zeros((2, len(cfg["ra"])), bool)
    for ti in range(len(cfg["times"])):
        rot.rotate(ti)
        topo = np.asarray(rot._topo)
        live = topo[2] > 0
        x = B.T @ topo  # (3, nsrc): theta / 2 pi per Hz
        for f in cfg["freqs"]:
            u = x[:2] * f
            u -= np.floor(u + 0.5)
            i0 = np.ceil((u + 0.5) * n2 - 0.5 * w).astype(int)
            low |= (i0 < 0) & live
            high |= (i0 + w > n2) & live
    print("type-2 adjoint periodic wrap: n2 %d w %d, sources crossing low x / y %d / %d, high x / y %d / %d"
          % (n2, w, low[0].sum(), low[1].sum(), high[0].sum(), high[1].sum()))
    assert low[0].any() and low[1].any() and high[0].any() and high[1].any()
    m = _close("periodic wrap", cfg, G, AtG)
    # the sources whose footprints wrap are as accurate as the rest
    wrap = np.flatnonzero(low.any(axis=0) | high.any(axis=0))
    exact = oracle_adjoint(cfg, G, sources=wrap)
    assert rel_l2(AtG[wrap], exact) <= 10 * cfg["eps"], m


def test_reproducible_and_lanes_agree(gpu, monkeypatch):
    cfg = dict(_base(nsrc=200, ntimes=4), polarized=True, force_use_type3=False)
    G = _random_g((3, 4, 2, 2, len(cfg["baselines"])), np.complex128, 5)
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a = _adjoint(G, cfg)
        b = _adjoint(G, cfg)
        assert np.array_equal(a, b), lanes
        res[lanes] = a
    assert rel_l2(res["1"], res["2"]) <= 1e-12


def test_nan_input_fails(gpu):
    cfg = dict(_base(), force_use_type3=False)
    G = _random_g((3, 2, len(cfg["baselines"])), np.complex128, 7)
    G[1, 0, 3] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="NaN"):
        _adjoint(G, cfg)
    G[1, 0, 3] = 0  # the handle stays usable
    assert np.all(np.isfinite(_adjoint(G, cfg)))


def test_device_tensor_input_matches_host(gpu):
    import torch

    cfg = dict(_base(), polarized=True, force_use_type3=False)
    G = _random_g((3, 2, 2, 2, len(cfg["baselines"])), np.complex128, 2)
    host = _adjoint(G, cfg)
    dev = _adjoint(torch.from_numpy(G).cuda(), cfg)
    assert dev.device.type == "cuda" and np.array_equal(dev.cpu().numpy(), host)


def test_gives_its_device_memory_back(gpu, monkeypatch):
    """``test_adjoint_gives_its_device_memory_back`` on the type-2 path: planes, entry records, accumulators and staged
    buffers go; the mode tables and twiddles stay."""
    import ctypes

    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = dict(_base(), polarized=True, force_use_type3=False)
    AF = fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _adjoint(_random_g(AF.shape, AF.dtype, 1), cfg)
    assert _handle().last_adjoint_path() == 2
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


def test_torch_backward_and_gradcheck(gpu):
    import torch

    cfg = _edge()
    kw = dict(_adj_kwargs(cfg), adjoint_path="type2")
    rng = np.random.default_rng(14)
    F0 = rng.normal(size=cfg["fluxes"].shape)
    D = _random_g((3, 2, 2, 2, len(cfg["baselines"])), np.complex128, 15)
    F = torch.tensor(F0, dtype=torch.float64, device="cuda", requires_grad=True)
    V = fftvis_amd.torch_simulate_vis(F, **kw)
    (V - torch.from_numpy(D).cuda()).abs().pow(2).sum().backward()
    assert _handle().last_adjoint_path() == 2
    resid = oracle_simulate(dict(cfg, fluxes=F0)) - D
    exact = 2 * oracle_adjoint(cfg, resid, full_stokes=True)
    m = _adjoint_errors(F.grad.cpu().numpy(), exact)
    print("type-2 adjoint torch backward", {key: round(v / cfg["eps"], 3) for key, v in m.items()})
    _assert_metrics(m, cfg["eps"], 10.0)
    for full in (False, True):
        small = dict(_base(nsrc=5, nfreq=2, ntimes=1), eps=1e-12, polarized=full, force_use_type3=False)
        kws = dict(_adj_kwargs(small), adjoint_path="type2")
        Fs = torch.tensor(rng.uniform(0.5, 1.5, (5, 2, 4) if full else (5, 2)), dtype=torch.float64, device="cuda",
                          requires_grad=True)
        assert torch.autograd.gradcheck(lambda f: fftvis_amd.torch_simulate_vis(f, **kws), (Fs,), eps=1e-3, atol=1e-7,
                                        rtol=1e-6)
        assert _handle().last_adjoint_path() == 2
