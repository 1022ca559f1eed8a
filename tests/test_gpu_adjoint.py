"""GPU tests of the adjoint (``simulate_vis_adjoint``, ``torch_simulate_vis``, ``fv_sim_run_adjoint``).

The adjoint is defined by the real inner products: Re <A F, G> = <F, A^T G> for real F and complex G, with A the map
``simulate_vis`` computes from ``fluxes``.  Checked through that identity against the forward over the configuration
matrix, element by element against the oracle's exact transpose (``oracle_adjoint``) in every configuration the identity
is checked in and at the edges of the device's slicing (source chunks, channel blocks, frequency groups, upsampling,
empty steps, coordinate managers), column by column against the oracle's forward, at HERA-350 scale, through torch's
gradcheck and backward, and for reproducibility."""

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from oracle import fftvis_oracle as orc
from tests.helpers import floored_rel, oracle_adjoint, oracle_beam, oracle_simulate, rel_l2, worst_part

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


# Element-wise tolerances against the oracle's exact A^T G (``_assert_close_to_oracle``).  base = eps in fp64; in fp32
# base = max(the forward's own rel l2 error against the oracle on the same configuration, eps).
#   rel l2 of the whole result and (full Stokes) of every Stokes component <= K * base: K = 10 in fp64 (the forward's
#   10 eps), K32 in fp32;
#   rel l2 of every channel <= K * base in fp64, K32_CHANNEL * base in fp32;
#   max |err| <= C_MAX * base * max |exact| over all elements.
# Measured on an MI355X over every configuration below (the 144 of test_adjoint_dot_identity, the HERA-350 cases, the
# edges), as ratio / base: fp64 whole, channel, Stokes <= 0.37, 2.33, 0.70 (HERA-350 <= 0.12, 0.24, 0.10); fp32 whole,
# Stokes <= 2.37, 2.90, channel <= 13.4; max |err| / (base max |exact|) <= 0.46 in fp64, 2.77 in fp32.  A channel is
# looser than the whole in fp32 because channel norms differ by 30x on HERA-7 (most sources sit in the sidelobes above
# 100 MHz) and the fp32 rounding of the catalog alone (ra, dec, as the engine rounds them) moves such a weak channel by
# about 1e-5 of its own norm.  The bounds keep a margin of at least 2 over these.
K32 = 8.0
K32_CHANNEL = 30.0
C_MAX = 6.0


def _adjoint_errors(got, exact):
    """rel l2 of the whole result, worst rel l2 of a channel and of a Stokes component, and max |err| / max |exact|.  A
    part whose exact norm is below 1e-3 of the whole (Q and V under beams whose four Jones terms are equal, where the
    exact gradient is 0) is measured against 1e-3 of the whole."""
    got = np.asarray(got, dtype=np.float64)
    err = got - exact
    floor = 1e-3 * np.linalg.norm(exact)
    m = {"rel_l2": floored_rel(err, exact, floor), "channel": worst_part(err, exact, 1, floor),
         "max_abs": float(np.abs(err).max() / max(np.abs(exact).max(), 1e-300))}
    if exact.ndim == 3:
        m["stokes"] = worst_part(err, exact, 2, floor)
    return m


def _forward_error(cfg, F, AF, max_bls=600):
    """The forward's rel l2 error against the oracle for fluxes F (on an even subset of at most max_bls baselines)."""
    bls = cfg["baselines"]
    pick = np.arange(0, len(bls), max(1, len(bls) // max_bls))
    exp = oracle_simulate(dict(cfg, fluxes=F, baselines=[bls[i] for i in pick]))
    return rel_l2(AF[..., pick].astype(np.complex128), exp)


def _assert_metrics(m, base, k, k_channel=None):
    for key, kk in (("rel_l2", k), ("channel", k_channel or k), ("stokes", k)):
        if key in m:
            assert m[key] <= kk * base, (key, m, base)
    assert m["max_abs"] <= C_MAX * base, (m, base)


def _assert_close_to_oracle(cfg, G, AtG, F=None, AF=None, sources=None, k64=10.0, coord_mgr=None):
    """A^T G (rows ``sources``, all by default) element-wise against ``oracle_adjoint``; fp32 is measured against the
    forward's own error on the same configuration (F, AF: a forward run of it)."""
    exact = oracle_adjoint(cfg, np.asarray(G).astype(np.complex128), full_stokes=np.ndim(AtG) == 3, sources=sources,
                           coord_mgr=coord_mgr)
    assert np.count_nonzero(exact) > 0
    got = AtG if sources is None else AtG[sources]
    if cfg.get("precision", 2) == 2:
        base, k, kc = cfg["eps"], k64, k64
    else:
        base, k, kc = max(_forward_error(cfg, F, AF), cfg["eps"]), K32, K32_CHANNEL
    m = _adjoint_errors(got, exact)
    _assert_metrics(m, base, k, kc)
    return m


def _sources_to_check(cfg, n=64, seed=0):
    """About n catalog rows that exercise a large catalog's adjoint: near zenith at every time, in the beam's sidelobes
    (za 20 - 70 deg), rising or setting between the time steps, the lowest of those above the horizon at some time, and
    random live ones to fill up.  Sorted catalog indices."""
    rot = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    up = []
    for ti in range(len(cfg["times"])):
        rot.rotate(ti)
        up.append(rot._topo[2])
    up = np.array(up)
    rng = np.random.default_rng(seed)
    live = np.flatnonzero(np.any(up > 0, axis=0))
    always = np.flatnonzero(np.all(up > 0, axis=0))
    za = np.degrees(np.arccos(np.clip(up[0], -1, 1)))
    q = n // 4
    zenith = always[np.argsort(-up[:, always].min(axis=0))[:q]]
    side = np.flatnonzero((za > 20) & (za < 70))
    side = rng.choice(side, min(q, side.size), replace=False)
    moving = np.flatnonzero(np.any(up > 0, axis=0) & np.any(up <= 0, axis=0))
    moving = rng.choice(moving, min(q // 2, moving.size), replace=False)
    low = live[np.argsort(up[:, live].max(axis=0))[:q - q // 2]]
    pick = np.unique(np.concatenate([zenith, side, moving, low]))
    rest = np.setdiff1d(live, pick)
    return np.sort(np.concatenate([pick, rng.choice(rest, max(0, n - pick.size), replace=False)]))


def _dot_check(cfg, seed=3, tol_eps=None, sources=None):
    """|Re <A F, G> - <F, A^T G>| <= 10 eps |A F| |G| with seeded random real F and complex G; then A^T G element-wise
    against the oracle's exact transpose (catalogs beyond 2000 sources on ``_sources_to_check``'s rows)."""
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
    if sources is None and len(F) > 2000:
        sources = _sources_to_check(cfg)
    _assert_close_to_oracle(cfg, G, AtG, F, AF, sources=sources)
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
    # 8 channels over 100 - 200 MHz: one channel block holds several frequency groups (f_first != f_base)
    "band_8ch_two_beams_full_stokes": dict(beams="two", full=True, compat=True, precision=2, nfreq=8),
    # 3 cm of height scatter: the 3-D adjoint at scale (the forward adds height terms)
    "z_scatter_table_stokes_i": dict(beams="table", full=False, compat=True, precision=2, z_scatter=0.03),
}


@pytest.mark.parametrize("name", list(HERA350_CASES))
def test_adjoint_dot_identity_hera350(gpu, name):
    """The dot identity on HERA-350 (the 2-D type-3 forward with its Hermitian / real packings and column plans) for
    the flips, skies, reference_compat forms and precisions the single full-scale case above does not take, and A^T G
    against the oracle on ~64 chosen sources (``_sources_to_check``) with all 61 075 baselines: runs of hundreds of
    members through k_adj_strengths' 16-lane fold, with flips in both forms."""
    c = HERA350_CASES[name]
    cfg = synth.make_config("C3", nsrc=20_000, nfreq=c.get("nfreq", 2), ntimes=2, z_scatter=c.get("z_scatter", 0.0))
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


def _edge_cfg(nsrc=61, nfreq=3, ntimes=2, seed=0):
    """HERA-7, polarized full-Stokes sky, two complex-Jones table beams with flipped pairs and an auto, the exact
    flipped forms (the feed transposition), fp64."""
    cfg = _base(nsrc=nsrc, nfreq=nfreq, ntimes=ntimes, seed=seed)
    freqs = cfg["freqs"]
    _, _, cfg["fluxes"] = synth.catalog(nsrc, freqs, seed, polarized_sky=True)
    tabs = [fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, d, nza=91, naz=180), freqs)
            for d in (14.0, 10.0)]
    cfg.update(polarized=True, beam=tabs, beam_idx=np.array([0, 1, 0, 1, 1, 0, 1]), reference_compat=False,
               baselines=cfg["baselines"] + [(3, 0), (6, 1), (2, 2)])
    return cfg


def _adjoint_of_random(cfg, seed=12, **kw):
    shape = (len(cfg["freqs"]), len(cfg["times"]), 2, 2, len(cfg["baselines"]))
    G = _random_g(shape, np.complex128, seed)
    return G, fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(cfg), full_stokes=True, **kw)


def _up(cfg):
    """Topocentric up component (ntimes, nsrc) of the catalog under the sidereal rotation."""
    rot = orc.SimpleCoordinateRotation(None, cfg["times"], cfg["telescope_loc"], cfg["ra"], cfg["dec"])
    out = []
    for ti in range(len(cfg["times"])):
        rot.rotate(ti)
        out.append(rot._topo[2])
    return np.array(out)


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_adjoint_source_chunks_match_oracle(gpu, monkeypatch, lanes):
    """min_chunks = 3 with 61 sources (chunks of 21, 21, 19) over 4 time steps, on one lane and on two."""
    monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
    cfg = dict(_edge_cfg(nsrc=61, ntimes=4), min_chunks=3)
    G, AtG = _adjoint_of_random(cfg)
    _assert_close_to_oracle(cfg, G, AtG)


@pytest.mark.parametrize("block_ch,ratio", [(5, 0.99), (1, 0.99), (2, 0.99), (2, 0.85), (2, 0.5)])
def test_adjoint_channel_blocks_and_groups_match_oracle(gpu, monkeypatch, block_ch, ratio):
    """nf = 5 (100 - 200 MHz) in channel blocks of block_ch (FFTVIS_HIP_ADJ_ACC_BYTES) with frequency groups cut by
    FFTVIS_HIP_GROUP_RATIO: several groups in one block (0.99: a group per channel; 0.85 splits 100 | 125 MHz), one
    group per block (0.5), the last block short."""
    cfg = _edge_cfg(nsrc=40, nfreq=5)
    monkeypatch.setenv("FFTVIS_HIP_ADJ_ACC_BYTES", str(block_ch * 8 * 8 * 40))  # doubles x coherency reals x sources
    monkeypatch.setenv("FFTVIS_HIP_GROUP_RATIO", str(ratio))
    G, AtG = _adjoint_of_random(cfg)
    _assert_close_to_oracle(cfg, G, AtG)


def test_adjoint_upsample_125_matches_oracle(gpu):
    """upsample_factor = 1.25, and "auto" where the adjoint picks 1.25 (a wide array with few sources and baselines),
    at the forward's sigma = 1.25 tolerance (20 eps: test_sim_variants_match_oracle's upsample_1p25)."""
    cfg = dict(_edge_cfg(), upsample_factor=1.25)
    G, AtG = _adjoint_of_random(cfg)
    _assert_close_to_oracle(cfg, G, AtG, k64=20.0)
    wide = synth.make_config("C3", nsrc=3000, nfreq=2, ntimes=2)
    rng = np.random.default_rng(2)
    wide["baselines"] = [wide["baselines"][i] for i in sorted(rng.choice(61075, 300, replace=False))]
    G = _random_g((2, 2, 2, 2, 300), np.complex128, 13)
    auto = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(dict(wide, upsample_factor="auto")))
    same = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(dict(wide, upsample_factor=1.25)))
    two = fftvis_amd.simulate_vis_adjoint(G, **_adj_kwargs(dict(wide, upsample_factor=2)))
    assert np.array_equal(auto, same) and not np.array_equal(auto, two)  # "auto" took 1.25
    _assert_close_to_oracle(wide, G, auto, k64=20.0)


def _edge_variants():
    cfg = _edge_cfg()
    up = _up(cfg)
    one = int(np.flatnonzero(np.all(up > 0, axis=0))[0])
    # sources around the meridian at the first time: half a sidereal day later all are below the horizon
    t0 = cfg["times"][0]
    lst = orc.gmst_rad(t0) + synth.HERA_LON
    rng = np.random.default_rng(1)
    set_ = dict(cfg, ra=lst + rng.uniform(-0.3, 0.3, 61), dec=synth.HERA_LAT + rng.uniform(-0.3, 0.3, 61),
                times=t0 + np.array([0.0, 0.25, 0.5]))
    return {
        "empty_time_step": set_,
        "one_source": dict(cfg, ra=cfg["ra"][one:one + 1], dec=cfg["dec"][one:one + 1], fluxes=cfg["fluxes"][one:one + 1]),
        "single_baseline": dict(cfg, baselines=[(0, 3)]),
        "autos_only": dict(cfg, baselines=[(0, 0), (1, 1), (3, 3)]),
        "exact_duplicates": dict(cfg, baselines=cfg["baselines"] + [(0, 1), (0, 1), (1, 0), (2, 5), (2, 5)]),
        # beams 0 on antennas 0-2, 1 on 3-6, and no listed baseline between them: the cross pair has n == 0
        "unused_cross_pair": dict(cfg, beam_idx=np.array([0, 0, 0, 1, 1, 1, 1]),
                                  baselines=[(0, 1), (0, 2), (2, 1), (3, 4), (5, 3), (6, 5), (4, 4)]),
    }


@pytest.mark.parametrize("name", list(_edge_variants()))
def test_adjoint_edges_match_oracle(gpu, name):
    cfg = _edge_variants()[name]
    if name == "empty_time_step":
        up = _up(cfg)
        assert np.any(up[0] > 0) and not np.any(up[-1] > 0)
    G, AtG = _adjoint_of_random(cfg)
    _assert_close_to_oracle(cfg, G, AtG)


def test_adjoint_coord_mgr_and_device_astrometry_match_oracle(gpu):
    """Per-time astrometry contexts with every term switched on: applied on the host and streamed (``coord_mgr=``), and
    applied on the device (``astrom=``, ``device_astrometry=True``), both against the oracle driven by the same manager."""
    from oracle import astrometry as oa

    cfg = _edge_cfg(ntimes=3)
    eq = orc.eq_unit_vectors(cfg["ra"], cfg["dec"])
    ctxs = np.stack([oa.plausible_context(20 + t, synth.HERA_LAT) for t in range(3)])

    class Mgr:  # the slice of matvis' manager the engine consumes
        def setup(self):
            pass

        def rotate(self, ti):
            self.all_coords_topo = oa.icrs_to_enu(eq, ctxs[ti])

    kw = dict(cfg, coord_method="CoordinateRotationERFA")
    G, host = _adjoint_of_random(kw, coord_mgr=Mgr())
    _, dev = _adjoint_of_random(kw, astrom=ctxs, device_astrometry=True)
    exact_kw = dict(coord_mgr=Mgr())
    _assert_close_to_oracle(cfg, G, host, **exact_kw)
    _assert_close_to_oracle(cfg, G, dev, **exact_kw)
    assert rel_l2(host, _adjoint_of_random(cfg)[1]) > 1e-3  # and it is not the sidereal answer


def test_torch_backward_matches_oracle(gpu):
    """d/dF sum |V(F) - D|^2 through torch_simulate_vis equals 2 A^T (A F - D), A and A^T both the oracle's: fp64,
    polarized, full Stokes, two beams, element-wise."""
    import torch

    cfg = _edge_cfg()
    kw = _adj_kwargs(cfg)
    rng = np.random.default_rng(14)
    F0 = rng.normal(size=cfg["fluxes"].shape)
    shape = (3, 2, 2, 2, len(cfg["baselines"]))
    D = _random_g(shape, np.complex128, 15)
    F = torch.tensor(F0, dtype=torch.float64, device="cuda", requires_grad=True)
    V = fftvis_amd.torch_simulate_vis(F, **kw)
    loss = (V - torch.from_numpy(D).cuda()).abs().pow(2).sum()
    loss.backward()
    resid = oracle_simulate(dict(cfg, fluxes=F0)) - D
    exact = 2 * oracle_adjoint(cfg, resid, full_stokes=True)
    m = _adjoint_errors(F.grad.cpu().numpy(), exact)
    _assert_metrics(m, cfg["eps"], 10.0)


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
