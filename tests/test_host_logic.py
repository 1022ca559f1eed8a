"""CPU-only tests of the product's host logic and of the C-ABI library's surface."""

import ctypes
import os
import re

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from fftvis_amd.core import coords, utils
from fftvis_amd.core.beams import TabulatedBeam, describe_beam
from oracle import fftvis_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    """Every function include/fftvis_hip.h declares must be exported (no compute calls here)."""
    hdr = open(os.path.join(ROOT, "include", "fftvis_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(fv_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 25
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.SYMBOLS), "ctypes table out of sync with the header"
    assert _lib.lib().fv_version() >= 100


def test_library_reports_errors_not_crashes():
    L = _lib.lib()
    assert L.fv_nufft3(0, 7, 2, 0, None, None, None, None, 1, 0, None, None, None, 1e-6, 2.0, None) == 1
    assert b"precision" in L.fv_last_error()
    h = ctypes.c_void_p()
    assert L.fv_sim_create(ctypes.byref(h), 0, 2, 1e-6, 3.0, 0) == 1  # bad upsample factor
    assert b"upsample" in L.fv_last_error()
    assert L.fv_sim_sync(None) == 1


def test_host_helpers_match_oracle():
    rng = np.random.default_rng(3)
    for _ in range(10):
        ants = {i: np.r_[rng.integers(-3, 4, 2) * 14.6, 0.0] for i in range(8)}
        assert utils.get_pos_reds(ants) == orc.get_pos_reds(ants)
        assert utils.get_pos_reds(ants, include_autos=False) == orc.get_pos_reds(ants, include_autos=False)
    for args in [(3, 30, 1), (10, 5, 1), (8, 128, 20), (8, 256, 60), (2, 8, 2), (6, 20, 30), (5, 7, 11)]:
        assert utils.get_task_chunks(*args) == orc.get_task_chunks(*args)
    av = rng.normal(size=(12, 3)) * [100, 100, 1]
    np.testing.assert_allclose(utils.get_plane_to_xy_rotation_matrix(av),
                               orc.get_plane_to_xy_rotation_matrix(av), atol=1e-14)
    sm = rng.normal(size=(5, 3, 4))
    np.testing.assert_allclose(utils.prepare_source_catalog(sm, True)[0],
                               orc.prepare_source_catalog(sm, True)[0])
    a = utils.prepare_beam_evaluation([0, 1, 2, 3], [(0, 1), (1, 0), (2, 3), (3, 1), (0, 0)], [0, 2, 2, 1])
    b = orc.prepare_beam_evaluation([0, 1, 2, 3], [(0, 1), (1, 0), (2, 3), (3, 1), (0, 0)], [0, 2, 2, 1])
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]


def test_task_chunks_reference_values():
    """reference tests/test_core_utils.py:26-45."""
    n, fc, tc, nf, nt = utils.get_task_chunks(3, 30, 1)
    assert (n, nf, nt) == (3, 10, 1)
    assert utils.get_task_chunks(10, 5, 1)[0] == 1
    # every (t, f) cell is covered exactly once for the multi-GPU shard shapes we use
    for nproc, nfreq, ntime in [(8, 256, 60), (8, 128, 20), (4, 64, 10), (2, 64, 10)]:
        n, fc, tc, _, _ = utils.get_task_chunks(nproc, nfreq, ntime)
        cover = np.zeros((ntime, nfreq), int)
        for f, t in zip(fc, tc):
            cover[t, f] += 1
        assert (cover == 1).all()


def test_validate_beam_idx_errors():
    """error texts of reference core/utils.py:358-429."""
    with pytest.raises(ValueError, match="beam_idx must be provided"):
        utils.validate_beam_idx(None, None, 2, 5)
    with pytest.raises(ValueError, match="length nant"):
        utils.validate_beam_idx(np.array([0, 1]), None, 2, 5)
    with pytest.raises(ValueError, match="greater than the number of beams"):
        utils.validate_beam_idx(np.array([0, 1, 2]), None, 2, 3)
    with pytest.raises(ValueError, match="should not be provided when beam_coefs"):
        utils.validate_beam_idx(np.array([0]), np.ones((1, 1, 1)), 1, 1)
    assert utils.validate_beam_idx(None, None, 1, 4) is None
    np.testing.assert_array_equal(utils.validate_beam_idx(None, None, 3, 3), np.arange(3))


def test_sidereal_rotation_matches_oracle_and_is_orthonormal():
    times = np.linspace(2459845.0, 2459845.05, 4)
    R = coords.SiderealRotation(times, (synth.HERA_LAT, synth.HERA_LON)).matrices()
    for i, t in enumerate(times):
        Ro = orc.eq_to_enu_matrix(orc.gmst_rad(t) + synth.HERA_LON, synth.HERA_LAT)
        np.testing.assert_allclose(R[i], Ro, atol=1e-14)
        np.testing.assert_allclose(R[i] @ R[i].T, np.eye(3), atol=1e-14)
    # a source at the local zenith maps to 'up'
    lst = coords.gmst_rad(times[0]) + synth.HERA_LON
    z = coords.eq_unit_vectors(np.array([lst]), np.array([synth.HERA_LAT]))
    np.testing.assert_allclose(R[0] @ z[:, 0], [0, 0, 1], atol=1e-12)


def test_describe_beam_rules():
    freqs = np.linspace(100e6, 120e6, 3)
    assert describe_beam(fftvis_amd.AiryBeam(14.0), False, freqs) == ("airy", 14.0)
    tab = TabulatedBeam(synth.synthetic_efield_table(freqs, nza=19, naz=36), freqs)
    kind, data, za_max = describe_beam(tab, True, freqs)
    assert kind == "table" and data.shape == (3, 2, 2, 19, 36) and data.dtype == np.complex128
    kind, data, _ = describe_beam(tab, False, freqs)  # power of feed 0
    assert data.shape == (3, 19, 36) and data.dtype == np.float64
    np.testing.assert_allclose(data, (np.abs(tab.data[:, :, 0]) ** 2).sum(1))
    with pytest.raises(ValueError, match="E-field"):
        describe_beam(TabulatedBeam(data, freqs), True, freqs)
    with pytest.raises(NotImplementedError):
        describe_beam(object(), False, freqs)

    class FakeUVBeam:  # pyuvdata future-array-shape layout
        data_array = np.transpose(tab.data, (1, 2, 0, 3, 4))
        axis1_array = 2 * np.pi * np.arange(36) / 36
        axis2_array = np.linspace(0, np.pi, 19)
        freq_array = freqs

    kind, d2, zm = describe_beam(FakeUVBeam(), True, freqs)
    np.testing.assert_allclose(d2, tab.data)
    assert np.isclose(zm, np.pi)


def test_engine_argument_errors_need_no_gpu():
    cfg = synth.make_config("C1", nsrc=5, nfreq=2, ntimes=1)
    with pytest.raises(ValueError, match="not compatible with unpolarized"):
        fftvis_amd.simulate_vis(**cfg, beam_coefs=np.ones((7, 1, 2)))
    with pytest.raises(ValueError, match="Unsupported backend"):
        fftvis_amd.create_simulation_engine("tpu")
    assert fftvis_amd.default_accuracy_dict == {1: 6e-8, 2: 1e-13}


def test_no_cpu_fallback_without_gpu():
    """On a box without a GPU the product refuses to compute (it never routes to the oracle)."""
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    cfg = synth.make_config("C1", nsrc=5, nfreq=2, ntimes=1)
    with pytest.raises(_lib.FftvisHipError):
        fftvis_amd.simulate_vis(**cfg)
    with pytest.raises(_lib.FftvisHipError):
        fftvis_amd.gpu.gpu_nufft2d(np.zeros(3), np.zeros(3), np.ones(3, complex), np.zeros(2), np.zeros(2), 1e-6)
    src = ""
    for dp, _, fs in os.walk(os.path.join(ROOT, "fftvis_amd")):
        for f in fs:
            if f.endswith(".py"):
                src += open(os.path.join(dp, f)).read()
    assert "import oracle" not in src and "from oracle" not in src


def _lattice_cases():
    def lin(n=10, sp=1.5):
        return {i: np.array([i * sp, 0.0, 0.0]) for i in range(n)}

    def sq(n=5):
        return {i * n + j: np.array([i, j, 0.0]) for i in range(n) for j in range(n)}

    holes = sq()
    holes.pop(3)
    holes.pop(16)
    r = np.random.default_rng(42)
    scat = {i: np.array([r.uniform(0, 10), r.uniform(0, 10), 0.0]) for i in range(15)}
    h = np.sqrt(3) / 2
    hexg = {0: np.array([-0.5, h, 0]), 1: np.array([0.5, h, 0]), 2: np.array([-1.0, 0, 0]),
            3: np.array([0.0, 0, 0]), 4: np.array([1.0, 0, 0]), 5: np.array([-0.5, -h, 0]),
            6: np.array([0.5, -h, 0])}
    return [("linear", lin(), True), ("square-full", sq(), True), ("square-holey", holes, True),
            ("hex-grid", hexg, True), ("non-griddable", scat, False),
            ("autos-only", {0: np.zeros(3)}, False), ("autos-only-2", {0: np.zeros(3), 1: np.zeros(3)}, False)]


@pytest.mark.parametrize("name,antpos,expected", _lattice_cases())
def test_check_antpos_griddability(name, antpos, expected):
    """Verdicts of reference tests/test_antenna_gridding.py:60-82, for the product's lattice
    detection and the oracle's restatement; griddable layouts must map onto integers and the
    returned basis must reproduce the antenna offsets."""
    from fftvis_amd.core.antenna_gridding import check_antpos_griddability

    for fn in (check_antpos_griddability, orc.check_antpos_griddability):
        ok, grid, B = fn(antpos)
        assert ok is expected
        if expected:
            k0 = list(antpos)[0]
            for k, pos in grid.items():
                assert np.allclose(pos, np.round(pos).astype(int))
                np.testing.assert_allclose(B @ pos, antpos[k] - antpos[k0], atol=1e-9)


def test_benchmark_arrays_are_lattices():
    from fftvis_amd.core.antenna_gridding import check_antpos_griddability

    for kind, nant in (("hera7", 7), ("hera37", 37), ("hera350", 350)):
        ants = synth.hera_like_array(kind)
        ok, grid, _ = check_antpos_griddability(ants)
        assert len(ants) == nant and ok


def test_bench_dumped_outputs_are_whole_or_a_fixed_sample(tmp_path):
    """`bench.py --dump-outputs`: a block within the budget is written whole (complex -> trailing (re, im) axis, the
    engine's real type); a larger one as a seeded sample whose flat indices are written beside it, the same on every
    run, and the files stay within the budget.  CPU tensors stand in for the device's."""
    import torch

    import bench

    small = torch.randn(8, 2, 21, dtype=torch.complex128)
    big = torch.randn(16, 4, 2, 2, 1021, dtype=torch.complex128)
    f32 = torch.randn(3, 5, dtype=torch.complex64)
    budget = 1 << 20
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), [("vis", small), ("big", big), ("f32", f32)], budget)
    assert sorted(os.listdir(tmp_path / "a")) == ["big_sample.npy", "big_sample_index.npy", "f32.npy", "vis.npy"]
    v = np.load(tmp_path / "a" / "vis.npy")
    assert v.dtype == np.float64 and np.array_equal(v[..., 0] + 1j * v[..., 1], small.numpy())
    f = np.load(tmp_path / "a" / "f32.npy")
    assert f.dtype == np.float32 and f.shape == (3, 5, 2)
    s, i = np.load(tmp_path / "a" / "big_sample.npy"), np.load(tmp_path / "a" / "big_sample_index.npy")
    assert i.dtype == np.float64 and np.all(np.diff(i) > 0) and len(i) > 0.9 * budget // 24
    assert np.array_equal(torch.view_as_real(big).reshape(-1, 2).numpy()[i.astype(np.int64)], s)
    assert (s.nbytes + i.nbytes) <= budget
    assert np.array_equal(i, np.load(tmp_path / "b" / "big_sample_index.npy"))


def test_round4_bench_arrays_are_what_their_names_say():
    """`bench.py --array scattered` / `--workload C3z`: the scattered array has 350 antennas inside HERA-350's
    footprint, is flat, is NOT a lattice and repeats no baseline vector; the height-scattered HERA-350 exceeds the
    reference's flat_array_tol (cpu_simulate.py:655) after the plane fit, i.e. takes the 3-D transform."""
    from fftvis_amd.core.antenna_gridding import check_antpos_griddability
    from fftvis_amd.gpu.gpu_simulate import prepare_array

    ref = np.array(list(synth.hera_like_array("hera350").values()))
    sc = synth.hera_like_array("scattered350")
    a = np.array(list(sc.values()))
    assert a.shape == (350, 3) and np.all(a[:, 2] == 0)
    assert np.all(a[:, :2].min(0) >= ref[:, :2].min(0)) and np.all(a[:, :2].max(0) <= ref[:, :2].max(0))
    assert not check_antpos_griddability(sc)[0]
    bl = synth.all_cross_baselines(sc)
    _, b, coplanar = prepare_array(sc, bl, 1e-6, np.float64)
    assert coplanar and len(np.unique(np.round(b[:2].T * 299792458.0, 6), axis=0)) == len(bl) == 61075
    assert np.array_equal(a, np.array(list(synth.hera_like_array("scattered350").values())))  # seeded
    cz = synth.make_config("C3", nsrc=4, nfreq=2, ntimes=1, z_scatter=0.03)
    _, bz, coplanar_z = prepare_array(cz["ants"], cz["baselines"], 1e-6, np.float64)
    assert not coplanar_z and 0.05 < np.abs(bz[2]).max() * 299792458.0 < 0.5


def test_spline_opts_orders():
    """The reference passes {"order": 1} (map_coordinates) or {"kx": 1, "ky": 1} (az_za_simple) in its
    own tests (tests/test_cpu_beams.py:72,82,411,428) and its CLI defaults to order 3 (cli.py:50,146):
    the device implements 1 and 3; anything else is refused loudly, never silently downgraded."""
    from fftvis_amd.core.beams import checked_spline_order, spline_order
    from fftvis_amd.gpu.gpu_simulate import GPUSimulationEngine

    assert spline_order(None) == 1 and spline_order({}) == 1
    assert spline_order({"order": 1}) == 1 and spline_order({"kx": 1, "ky": 1}) == 1
    assert spline_order({"order": 3}) == 3 and spline_order({"kx": 3, "ky": 3}) == 3
    assert checked_spline_order(None) == 1 and checked_spline_order({"order": 3}) == 3
    cfg = synth.make_config("C1", nsrc=5, nfreq=2, ntimes=1)
    eng = GPUSimulationEngine()
    assert [checked_spline_order({"order": n}) for n in range(6)] == list(range(6))
    assert checked_spline_order({"kx": 2, "ky": 2}) == 2
    for opts in ({"kx": 6, "ky": 6}, {"order": 7}, {"order": -1}):
        with pytest.raises(ValueError, match="spline order not supported"):
            eng.simulate(ants=cfg["ants"], freqs=cfg["freqs"], fluxes=cfg["fluxes"], beam_list=[cfg["beam"]],
                         ra=cfg["ra"], dec=cfg["dec"], times=cfg["times"], telescope_loc=cfg["telescope_loc"],
                         beam_spline_opts=opts, coord_method="SiderealRotation")


def test_upsample_1p25_below_its_floor_warns():
    """upsample_factor=1.25 cannot deliver better than ~1e-8 in fp64 (1e-4 in fp32): asking for less
    is answered with a RuntimeWarning before anything touches the GPU."""
    from fftvis_amd.gpu.gpu_simulate import GPUSimulationEngine

    cfg = synth.make_config("C1", nsrc=5, nfreq=2, ntimes=1)
    kw = dict(ants=cfg["ants"], freqs=cfg["freqs"], fluxes=cfg["fluxes"], beam_list=[cfg["beam"]], ra=cfg["ra"],
              dec=cfg["dec"], times=cfg["times"], telescope_loc=cfg["telescope_loc"], upsample_factor=1.25,
              coord_method="SiderealRotation")
    for prec, eps in ((2, 1e-10), (1, 1e-6)):
        with pytest.warns(RuntimeWarning, match="upsample_factor=1.25 delivers about"):
            try:
                GPUSimulationEngine().simulate(precision=prec, eps=eps, **kw)
            except Exception:  # no GPU here: the warning comes first
                pass


class _StubAnalyticBeam:
    """Shaped like a pyuvdata analytic beam: compute_response(az_array=, za_array=, freq_array=) ->
    (Naxes_vec, Nfeeds, Nfreqs, Npts).  E-field = Airy / sqrt(2) in every slot, feed 'y' 30 % weaker."""

    beam_type = "efield"
    feed_array = np.array(["x", "y"])

    def __init__(self, diameter=14.0):
        self.diameter = diameter  # has .diameter and "Airy"-free name: must NOT be mapped onto a formula
        self.calls = 0

    def compute_response(self, *, az_array, za_array, freq_array, **kw):
        from scipy.special import j1

        self.calls += 1
        x = np.pi * self.diameter * freq_array[0] * np.sin(za_array) / 299792458.0
        e = np.where(x == 0, 1.0, 2 * j1(x) / np.where(x == 0, 1, x)) / np.sqrt(2.0)
        out = np.zeros((2, 2, 1, az_array.size), dtype=complex)
        out[0, 0, 0], out[1, 0, 0] = e, 0.5 * e
        out[0, 1, 0], out[1, 1, 0] = 0.7 * e, 0.35 * e
        return out


class AiryBeamLookalike(_StubAnalyticBeam):
    """A third-party class that merely LOOKS like an Airy dish (name + .diameter): its response is a Gaussian
    with a dipole-like azimuth term, nothing the closed form can follow."""

    def compute_response(self, *, az_array, za_array, freq_array, **kw):
        self.calls += 1
        g = np.exp(-0.5 * (za_array * self.diameter * freq_array[0] / 299792458.0) ** 2)
        out = np.zeros((2, 2, 1, az_array.size), dtype=complex)
        out[0, 0, 0], out[1, 0, 0] = g * np.cos(az_array), -g * np.sin(az_array) * np.cos(za_array)
        out[0, 1, 0], out[1, 1, 0] = g * np.sin(az_array), g * np.cos(az_array) * np.cos(za_array)
        return out


def test_third_party_analytic_beams_are_probed_never_guessed(monkeypatch):
    """VERDICT r1 #3 / r2 next #8 / ADVICE r2 (medium): an object with compute_response is followed through that
    method.  It runs in closed form only when its OWN response at the probes equals this package's Airy form
    times one constant per Jones slot (to 1e-12) -- then with exactly those constants; anything else is sampled
    onto a table whose node spacing is refined until the device interpolant meets the tolerance against
    compute_response between the nodes.  A class name or a .diameter attribute decides nothing."""
    from fftvis_amd.core import beams as cb
    from fftvis_amd.core.beams import is_sampled_analytic, response_at

    freqs = np.array([120e6, 180e6, 250e6])
    b = _StubAnalyticBeam()
    assert is_sampled_analytic(b) and not is_sampled_analytic(fftvis_amd.AiryBeam(14.0))
    kind, D, js, ps = describe_beam(b, True, freqs, order=3)
    assert kind == "airy" and D == 14.0 and ps == 1.0
    np.testing.assert_allclose(js, np.array([[1, 0.7], [0.5, 0.35]]) / np.sqrt(2), rtol=0, atol=1e-14)
    kind, D, js, px = describe_beam(b, False, freqs, use_feed="x")
    _, _, _, py = describe_beam(b, False, freqs, use_feed="y")
    assert kind == "airy" and np.isclose(px, 0.5 * (1 + 0.25)) and np.isclose(py, 0.49 * px)
    np.testing.assert_array_equal(cb.airy_factors(("airy", 14.0)), [1, 0, 1, 0, 1, 0, 1, 0, 1])
    # the lookalike is NOT that form: sampled, refined, and the table reproduces ITS response to the tolerance
    look = AiryBeamLookalike()
    assert cb.fit_airy_closed_form(look, True, freqs) is None
    kind, tab, za_max = describe_beam(look, True, freqs, order=3, tol=1e-7)
    nzp, naz = tab.shape[-2:]
    nza = nzp - cb.SAMPLED_PAD
    assert kind == "table" and tab.shape[:3] == (3, 2, 2) and naz >= 720 and nza >= 181
    assert np.isclose(za_max, 0.5 * np.pi * (nzp - 1) / (nza - 1))  # SAMPLED_PAD nodes past the horizon
    rng = np.random.default_rng(3)
    za, az = rng.uniform(0, np.pi / 2, 400), rng.uniform(0, 2 * np.pi, 400)
    for fi in (0, 2):
        want = response_at(look, True, freqs[fi], az, za)
        got = np.stack([cb._interp_table(pl, za_max, az, za, 3) for pl in tab[fi].reshape(4, nzp, naz)]).reshape(2, 2, -1)
        assert np.abs(got - want).max() < 2e-7
    # azimuth-independent but not Airy (frequency-dependent gain): 8 azimuth nodes, finer za nodes than 0.5 deg
    class Gain(_StubAnalyticBeam):
        def compute_response(self, *, az_array, za_array, freq_array, **kw):
            return super().compute_response(az_array=az_array, za_array=za_array, freq_array=freq_array) * freq_array[0] / 1e8

    kind, tab, za_max = describe_beam(Gain(), True, freqs, order=3, tol=1e-7)
    assert kind == "table" and tab.shape[-1] == cb.SAMPLED_AZ_SYMMETRIC_NODES and tab.shape[-2] > 181 + cb.SAMPLED_PAD
    # a 25 m dish at 1.4 GHz (pattern scale ~0.5 deg: under-resolved by a fixed 0.5-degree grid) is refined further
    kind, tab25, _ = describe_beam(Gain(25.0), True, np.array([1.3e9, 1.4e9]), order=3, tol=1e-7)
    assert tab25.shape[-2] > tab.shape[-2]
    # an order-1 table of a pattern with azimuth structure cannot reach 1e-7 within the byte limit: refused, loudly
    monkeypatch.setenv("FFTVIS_HIP_BEAM_TABLE_BYTES", str(2**28))
    with pytest.raises(ValueError, match="no .za, az. table within"):
        describe_beam(look, True, freqs[:1], order=1, tol=1e-7)
    monkeypatch.delenv("FFTVIS_HIP_BEAM_TABLE_BYTES")
    # a pattern that is not finite below the horizon is padded by reflection instead
    class Hard(AiryBeamLookalike):
        def compute_response(self, *, az_array, za_array, freq_array, **kw):
            out = super().compute_response(az_array=az_array, za_array=za_array, freq_array=freq_array)
            out[..., za_array > np.pi / 2 + 1e-12] = np.nan
            return out

    kind, tabh, _ = describe_beam(Hard(), True, freqs[:1], order=3, tol=1e-7)
    assert kind == "table" and np.all(np.isfinite(tabh))
    # the memory estimate counts a table for such beams
    from fftvis_amd.core.utils import get_desired_chunks

    small = int(0.9 * 205 * 720 * 4 * 16 * 8)  # less than one 8-channel table: chunks cannot help, the count saturates
    assert get_desired_chunks(small, 1, [look], 2, 2, 7, 1000, 2, nfreq=8)[0] > get_desired_chunks(
        small, 1, [fftvis_amd.AiryBeam(14.0)], 2, 2, 7, 1000, 2, nfreq=8)[0]

    # a wrapper object (BeamInterface-like) around the analytic beam is followed too
    class Wrapper:
        def __init__(self, beam):
            self.beam = beam

    assert describe_beam(Wrapper(_StubAnalyticBeam()), True, freqs, order=3)[0] == "airy"
    assert describe_beam(Wrapper(look), True, freqs[:1], order=3)[0] == "table"
    assert describe_beam(Wrapper(fftvis_amd.AiryBeam(12.0)), True, freqs) == ("airy", 12.0)


def test_use_feed_selects_the_feed():
    """use_feed='y' must not silently return the x-feed power beam (reference wrapper.py:278-279)."""
    from fftvis_amd.core.beams import feed_index

    freqs = np.array([150e6])
    data = synth.synthetic_efield_table(freqs, nza=19, naz=36)
    data[:, :, 1] *= 0.5  # feed y: half the E-field
    tab = TabulatedBeam(data, freqs)
    _, px, _ = describe_beam(tab, False, freqs, use_feed="x")
    _, py, _ = describe_beam(tab, False, freqs, use_feed="y")
    np.testing.assert_allclose(px, (np.abs(data[:, :, 0]) ** 2).sum(1))
    np.testing.assert_allclose(py, (np.abs(data[:, :, 1]) ** 2).sum(1))
    assert not np.allclose(px, py)

    class FakeUVBeam:  # feeds stored in the order (y, x): the name decides, not the position
        data_array = np.transpose(data, (1, 2, 0, 3, 4))[:, ::-1]
        axis1_array = 2 * np.pi * np.arange(36) / 36
        axis2_array = np.linspace(0, np.pi, 19)
        freq_array = freqs
        feed_array = np.array(["y", "x"])
        beam_type = "efield"

    _, qx, _ = describe_beam(FakeUVBeam(), False, freqs, use_feed="x")
    _, qy, _ = describe_beam(FakeUVBeam(), False, freqs, use_feed="y")
    np.testing.assert_allclose(qx, px)
    np.testing.assert_allclose(qy, py)
    assert feed_index("X") == 0 and feed_index("y") == 1 and feed_index("x", ["n", "e"]) == 1
    for bad in ("z", "", "xy"):
        with pytest.raises(ValueError, match="use_feed"):
            feed_index(bad)
    cfg = synth.make_config("C1", nsrc=5, nfreq=2, ntimes=1)
    with pytest.raises(ValueError, match="use_feed"):
        fftvis_amd.simulate_vis(**cfg, use_feed="q")


def test_memory_and_coordinate_knobs_are_honoured_or_refused():
    """VERDICT r1 #6/#9, ADVICE (medium): no silent knobs.  max_memory -> chunks (device estimate),
    ERFA / Astropy coordinate methods without a coord_mgr raise, unknown methods raise."""
    from fftvis_amd.core.utils import get_desired_chunks, get_required_chunks
    from fftvis_amd.gpu.gpu_simulate import GPUSimulationEngine

    # plenty of memory: one chunk; shrinking the budget raises the count monotonically, capped at 100 / nsrc
    args = dict(nax=2, nfeed=2, nant=350, nsrc=1_000_000, nbeam=1, nbeampix=181 * 360, precision=2, nfreq=256)
    big = get_required_chunks(280 * 2**30, **args)
    mid = get_required_chunks(30 * 2**30, **args)
    tiny = get_required_chunks(2**20, **args)
    assert big == 1 and 1 < mid < tiny == 100
    n, per = get_desired_chunks(280 * 2**30, 3, [], 2, 2, 350, 1_000_000, 2, nfreq=256)
    assert (n, per) == (3, 333_334)  # min_chunks wins when memory does not bind
    assert get_desired_chunks(1000, 1, [], 1, 1, 7, 40, 2)[0] == 40  # never more chunks than sources
    cfg = synth.make_config("C1", nsrc=5, nfreq=2, ntimes=1)
    kw = dict(ants=cfg["ants"], freqs=cfg["freqs"], fluxes=cfg["fluxes"], beam_list=[cfg["beam"]], ra=cfg["ra"],
              dec=cfg["dec"], times=cfg["times"], telescope_loc=cfg["telescope_loc"])
    eng = GPUSimulationEngine()
    # matvis / astropy are absent here: the reference's methods are refused, never approximated
    for method in ("CoordinateRotationERFA", "CoordinateRotationAstropy"):
        with pytest.raises(ValueError, match="needs matvis / astropy"):
            eng.simulate(coord_method=method, **kw)
    with pytest.raises(ValueError, match="needs matvis / astropy"):
        eng.simulate(**kw)  # the default IS the reference's ERFA method
    with pytest.raises(ValueError, match="needs matvis / astropy|unknown coord_method"):
        eng.simulate(coord_method="Sidereal", **kw)
    with pytest.raises(ValueError, match="nchunks"):
        eng.simulate(coord_method="SiderealRotation", nchunks=0, **kw)
    with pytest.raises(ValueError, match="source_buffer"):
        eng.simulate(coord_method="SiderealRotation", source_buffer=0.0, **kw)
    with pytest.raises(ValueError, match="interpolation_function"):
        eng.simulate(coord_method="SiderealRotation", interpolation_function="healpix", **kw)


def test_reference_default_call_builds_the_matvis_manager(monkeypatch):
    """``engine.simulate(**kw)`` with precisely the keywords wrapper.py:308-336 passes (no
    coord_mgr, coord_method="CoordinateRotationERFA") builds matvis' manager the way cpu_simulate.py:686-709 does.
    matvis / astropy are stubs in sys.modules; the device part is cut off at the handle (no GPU here)."""
    from tests.helpers import install_reference_dependency_stubs
    from fftvis_amd.gpu import gpu_simulate

    made, Time = install_reference_dependency_stubs(monkeypatch)
    cfg = synth.make_config("C1", nsrc=11, nfreq=2, ntimes=3)

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached

    monkeypatch.setattr(gpu_simulate, "_acquire_handle", stop)
    ants = {k: np.array(v) for k, v in cfg["ants"].items()}
    kw = dict(  # wrapper.py:308-336, keyword for keyword
        ants=ants, freqs=cfg["freqs"], fluxes=cfg["fluxes"], beam_list=[cfg["beam"]], beam_idx=None,
        ra=cfg["ra"], dec=cfg["dec"], times=cfg["times"], telescope_loc=cfg["telescope_loc"], baselines=None,
        precision=2, polarized=False, eps=1e-13, upsample_factor=2, beam_spline_opts=None, flat_array_tol=1e-6,
        interpolation_function="az_za_map_coordinates", nprocesses=1, nthreads=None,
        coord_method="CoordinateRotationERFA", coord_method_params={"update_bcrs_every": 1e9},
        force_use_type3=False, force_use_ray=False, trace_mem=False, nchunks=3, source_buffer=0.75,
        beam_coefs=None)
    with pytest.raises(Reached):
        gpu_simulate.GPUSimulationEngine().simulate(**kw)
    (m,) = made
    assert type(m).__name__ == "CoordinateRotationERFA"
    assert isinstance(m.kw["times"], Time) and np.array_equal(m.kw["times"].jd, cfg["times"])  # :686-687
    assert m.kw["chunk_size"] == 4 and m.kw["source_buffer"] == 0.75 and m.kw["precision"] == 2  # ceil(11 / 3)
    assert m.kw["flux"].shape == (11, 2) and m.kw["flux"].dtype == np.complex128
    assert np.allclose(m.kw["flux"], 0.5 * cfg["fluxes"])  # the prepared coherency (cpu/utils.py:70)
    assert np.array_equal(m.kw["skycoords"].ra.value, cfg["ra"]) and m.kw["telescope_loc"] is cfg["telescope_loc"]
    assert m.bcrs_set == [0]  # update_bcrs_every (1e9 s) exceeds the span: BCRS fixed once (:706-709)
    made.clear()
    with pytest.raises(Reached):
        gpu_simulate.GPUSimulationEngine().simulate(**dict(kw, coord_method_params=None, precision=1))
    assert made[0].bcrs_set == [] and made[0].kw["flux"].dtype == np.complex64
    with pytest.raises(ValueError, match="unknown coord_method"):
        gpu_simulate.GPUSimulationEngine().simulate(**dict(kw, coord_method="CoordinateRotationNope"))
    # a caller's own manager still wins, and the named approximation builds nothing
    made.clear()
    with pytest.raises(Reached):
        gpu_simulate.GPUSimulationEngine().simulate(**dict(kw, coord_method="SiderealRotation"))
    assert made == []


def test_engine_registers_with_the_reference_abc(monkeypatch):
    """where ``fftvis`` is importable the GPU engine is an instance of ITS ABC."""
    import abc
    import sys
    import types
    from fftvis_amd.gpu import gpu_simulate

    assert gpu_simulate.register_with_reference() is False  # the reference is not installed here

    class SimulationEngine(abc.ABC):
        pass

    mod = types.ModuleType("fftvis.core.simulate")
    mod.SimulationEngine = SimulationEngine
    monkeypatch.setitem(sys.modules, "fftvis.core.simulate", mod)
    assert gpu_simulate.register_with_reference() is True
    assert isinstance(gpu_simulate.GPUSimulationEngine(), SimulationEngine)


def test_sanitizer_builds_of_the_cpu_code_are_clean():
    """SURVEY section 5 / VERDICT r1 #8: AddressSanitizer + UBSan on the CPU builds -- the oracle's C files and
    the HOST side of libfftvis_hip (argument checking and error reporting of every C-ABI entry point, driven by
    tools/abi_sanitize_check.cpp; device code is not instrumented).  `make -C oracle sanitize` builds and runs
    both and fails on any sanitizer report; neither needs a GPU."""
    import subprocess

    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "sanitize"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "sanitize_check: ok" in r.stdout and "abi_sanitize_check: ok" in r.stdout
