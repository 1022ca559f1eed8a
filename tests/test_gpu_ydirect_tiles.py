"""Direct y sums (fv_ydirect.h): what the launch shape and the workgroup's layout can get wrong.  The cut of the rows
into slices (FFTVIS_HIP_YD_SLICES; the default follows the device's size), every point slot of a workgroup, a u-group
too large for one, and four transforms per frequency.  Forced on with FFTVIS_HIP_YDIRECT=1; that a run took the path
shows in `fft_cells`, as in test_gpu_ydirect.py, whose bounds these are: 10 eps + 1e-12 against the oracle's exact sums
at eps = 1e-10."""

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import synth
from tests.helpers import oracle_simulate, rel_l2
from tests.test_gpu_ydirect import _hex_outrigger, _run

pytestmark = pytest.mark.gpu
EPS = 1e-10
BOUND = 10 * EPS + 1e-12
SLICES = "FFTVIS_HIP_YD_SLICES"
TILE, RESEED = 32, 128  # YD_RT, YD_RESEED
POINT_CAP = 1024        # YD_THREADS * YD_PTM: the points of a work range, so of one u-group


def _run_sliced(cfg, monkeypatch, n):
    if n is None:
        monkeypatch.delenv(SLICES, raising=False)
    else:
        monkeypatch.setenv(SLICES, str(n))
    out = _run(cfg, monkeypatch, "1")
    monkeypatch.delenv(SLICES, raising=False)
    return out


def test_row_slices_forced_and_default(gpu, monkeypatch):
    """HERA-37 plus outrigger, 2 channels x 2 times, on a band whose na_y is a multiple of neither the tile height nor
    the seed distance: 1, 2 and 3 slices and the default cut.  Every block against the oracle; the blocks agree with
    one another to 1e-13 (they differ in where the partial sums are cut: rounding only); the 3-slice cut ends in a
    shorter slice."""
    f_top, na_y = None, 0
    for f in 158e6 + 0.9e6 * np.arange(8):
        cfg, sub = _hex_outrigger(False, EPS, freqs=(150e6, f), nsrc=40)
        _, st = _run(cfg, monkeypatch, "1")
        na_y = int(st["n2z"]) % 65536
        if na_y % TILE != 0 and na_y % RESEED != 0:
            f_top = f
            break
    assert f_top is not None, na_y
    tiles = -(-na_y // TILE)
    rps = -(-tiles // 3) * TILE
    assert -(-na_y // rps) == 3 and 0 < na_y - 2 * rps < rps, (na_y, rps)  # three slices, the last one shorter
    cfg, sub = _hex_outrigger(False, EPS, freqs=(150e6, f_top), nsrc=300)
    exact = oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub]))
    _, st_off = _run(cfg, monkeypatch, "0")
    blocks = {}
    for n in (1, 2, 3, None):
        v, st = _run_sliced(cfg, monkeypatch, n)
        assert int(st["n2z"]) % 65536 == na_y
        assert st["fft_cells"] < st_off["fft_cells"]
        e = rel_l2(v[..., sub], exact)
        print(f"ydirect slices={n} na_y={na_y}: oracle {e:.3e}")
        assert e < BOUND, (n, e)
        blocks[n] = v
    for n in (2, 3, None):
        d = rel_l2(blocks[n], blocks[1])
        print(f"ydirect slices={n} against one slice: {d:.3e}")
        assert d < 1e-13, (n, d)


def _line(nant, polarized, nsrc=200):
    """A north-south line of nant antennas at pairwise-distinct separations (a seeded increasing sequence, every new
    separation at least 1 cm from all earlier ones): every baseline has u = 0, so all evaluation points -- nant (nant - 1) / 2
    plain, both signs of them packed -- fall into ONE u-group.  1 channel x 1 time."""
    rng = np.random.default_rng(11)
    pos, seps = [0.0], []
    while len(pos) < nant:
        c = pos[-1] + rng.uniform(3.0, 8.0)
        new = [c - p for p in pos]
        if all(abs(a - b) > 0.01 for a in new for b in seps):
            pos.append(c)
            seps += new
    seps = np.sort(seps)
    assert len(seps) == nant * (nant - 1) // 2 and np.diff(seps).min() > 0.01
    ants = {i: np.array([0.0, y, 0.0]) for i, y in enumerate(pos)}
    freqs = np.array([150e6])
    ra, dec, flux = synth.catalog(nsrc, freqs, 5)
    beam = (fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, nza=91, naz=180), freqs) if polarized
            else fftvis_amd.AiryBeam(14.0))
    return dict(ants=ants, fluxes=flux, ra=ra, dec=dec, freqs=freqs, times=np.array([2459845.0]), beam=beam,
                telescope_loc=(synth.HERA_LAT, synth.HERA_LON), baselines=synth.all_cross_baselines(ants), polarized=polarized,
                precision=2, eps=EPS, force_use_type3=True, coord_method="SiderealRotation")


@pytest.mark.parametrize("polarized", [False, True], ids=["plain", "packed"])
def test_every_point_slot_of_a_workgroup(gpu, monkeypatch, polarized):
    """HERA-37's ranges hold few points: the higher point slot of a thread, and waves whose slot is empty, never run
    there.  42 antennas on a line: 861 baselines, 861 points in one u-group and one work range -- every thread's first
    slot, the second slot on five waves and a part of the sixth, none on the last two.  (The issue behind this test
    counted on both signs of 435 baselines, 870 points, from 30 antennas; these grids are too small for the packed
    gather at s and -s, so a baseline is one point whether polarized or not -- FFTVIS_HIP_DEBUG_YDIRECT=1 prints
    "435 points" for 30 -- and 42 antennas is the line with about that many points.)  One transform unpolarized, four
    polarized; against the oracle on every 20th baseline."""
    cfg = _line(42, polarized)
    npts = len(cfg["baselines"])
    assert POINT_CAP // 2 + 5 * 64 < npts == 861 < POINT_CAP - 2 * 64
    v, st = _run(cfg, monkeypatch, "1")
    _, st_off = _run(cfg, monkeypatch, "0")
    assert st["fft_cells"] < st_off["fft_cells"], (st["fft_cells"], st_off["fft_cells"])  # the forced run took the path
    sub = list(range(0, npts, 20))
    exact = oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub]))
    e = rel_l2(v[..., sub], exact)
    print(f"ydirect line of 42, polarized={polarized}: oracle {e:.3e}")
    assert np.isfinite(v).all() and e < BOUND, e


def test_a_group_too_large_for_a_workgroup_falls_back(gpu, monkeypatch):
    """The same line with the fewest antennas whose one u-group exceeds a work range's points (a baseline is one point
    here, see above: n (n - 1) / 2 > 1 024 at 46 antennas, 1 035 points): no tables can be built, the forced run keeps
    the FFT y-pass -- the switched-off run's `fft_cells` -- and stays within the bound."""
    nant = next(n for n in range(2, 100) if n * (n - 1) // 2 > POINT_CAP)
    cfg = _line(nant, True)
    assert len(cfg["baselines"]) > POINT_CAP
    v, st = _run(cfg, monkeypatch, "1")
    _, st_off = _run(cfg, monkeypatch, "0")
    assert st["fft_cells"] == st_off["fft_cells"], (st["fft_cells"], st_off["fft_cells"])
    sub = list(range(0, len(cfg["baselines"]), 20))
    exact = oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub]))
    e = rel_l2(v[..., sub], exact)
    print(f"ydirect line of {nant} (fallen back): oracle {e:.3e}")
    assert e < BOUND, e


def test_four_transforms(gpu, monkeypatch):
    """Two beams: a packed list per beam and the cross list with four plain transforms per frequency, at eps = 1e-10
    against the oracle and against the switched-off run to 10 eps."""
    cfg, sub = _hex_outrigger(True, EPS, nsrc=300)
    freqs = cfg["freqs"]
    other = fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, 12.0, nza=91, naz=180), freqs)
    two = dict(cfg, beam=[cfg["beam"], other], beam_idx=np.arange(len(cfg["ants"])) % 2)
    v, st = _run(two, monkeypatch, "1")
    off, st_off = _run(two, monkeypatch, "0")
    assert st["fft_cells"] < st_off["fft_cells"]
    exact = oracle_simulate(dict(two, baselines=[two["baselines"][i] for i in sub]))
    e, d = rel_l2(v[..., sub], exact), rel_l2(v, off)
    print(f"ydirect four transforms: oracle {e:.3e}, on vs off {d:.3e}")
    assert e < BOUND, e
    assert d < 10 * EPS, d
