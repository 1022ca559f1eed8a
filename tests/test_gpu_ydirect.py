"""Direct y sums of the type-3 forward on lattice arrays (fv_ydirect.h): the x-pass output is
contracted per distinct u and every target sums its column with exact phases -- no y-pass, no grid C, no interpolation
along y.  Small shapes with the path forced on (FFTVIS_HIP_YDIRECT=1) against the oracle's exact sums, against the FFT
y-pass (FFTVIS_HIP_YDIRECT=0) and against itself under the switches that change what is stored or gathered; then the
default rule of geometry on a lattice and on a scattered array.  That a run took the path shows in its statistics:
`fft_cells` then holds the x-pass and the cells of B the sums read, not a y-pass."""

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import synth
from tests.helpers import check_forward, oracle_simulate, rel_l2

pytestmark = pytest.mark.gpu
SWITCH = "FFTVIS_HIP_YDIRECT"


def _run(cfg, monkeypatch, mode, env=()):
    """One run on a fresh handle with the switch at `mode` (None: the default rule); returns (block, statistics)."""
    from fftvis_amd.gpu import gpu_simulate

    gpu_simulate.release_handles()
    monkeypatch.setenv("FFTVIS_HIP_HANDLE_CACHE_BYTES", str(2**40))
    if mode is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, mode)
    for k in env:
        monkeypatch.setenv(k, "1")
    v = fftvis_amd.simulate_vis(**cfg)
    (h,) = gpu_simulate._IDLE_HANDLES.values()
    st = h.stats()
    for k in env:
        monkeypatch.delenv(k)
    monkeypatch.delenv(SWITCH, raising=False)
    gpu_simulate.release_handles()
    return v, st


def _hex_outrigger(polarized, eps, freqs=(150e6, 158e6), nsrc=2000):
    """HERA-37 plus one outrigger (its baselines have a u of their own: groups of a single target, and a grid large
    enough for the packed transforms), 2 channels x 2 times; a tenth of the baselines given backwards, two autos, one
    exact duplicate.  Returns the configuration and a baseline subset with the outrigger, an auto, flipped members and
    the duplicate."""
    ants = dict(synth.hera_like_array("hera37"))
    out = len(ants)
    ants[out] = np.array([391.3, 247.9, 0.0])
    freqs = np.asarray(freqs, float)
    ra, dec, flux = synth.catalog(nsrc, freqs, 3)
    bl = synth.all_cross_baselines(ants)
    flipped = list(range(4, len(bl), 10))
    for i in flipped:
        bl[i] = (bl[i][1], bl[i][0])
    with_out = [i for i, b in enumerate(bl) if out in b]
    bl += [(3, 3), (9, 9), bl[11]]
    n = len(bl)
    beam = (fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, nza=91, naz=180), freqs) if polarized
            else fftvis_amd.AiryBeam(14.0))
    cfg = dict(ants=ants, fluxes=flux, ra=ra, dec=dec, freqs=freqs, times=np.linspace(2459845.0, 2459845.01, 2), beam=beam,
               telescope_loc=(synth.HERA_LAT, synth.HERA_LON), baselines=bl, polarized=polarized, precision=2, eps=eps,
               force_use_type3=True, coord_method="SiderealRotation")
    sub = sorted({0, 11, 57, 300, flipped[0], flipped[7], flipped[-1], with_out[0], with_out[5], with_out[-1], n - 3, n - 2, n - 1})
    return cfg, sub


_EXACT = {}


def _exact(polarized):
    """The oracle's exact sums on the subset: they do not depend on eps, so one evaluation per beam serves every case."""
    if polarized not in _EXACT:
        cfg, sub = _hex_outrigger(polarized, 6e-8)
        _EXACT[polarized] = oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub]))
    return _EXACT[polarized]


@pytest.mark.parametrize("polarized", [True, False], ids=["packed", "plain"])
@pytest.mark.parametrize("eps", [1e-4, 6e-8, 1e-10])
def test_direct_y_sums_match_the_oracle_and_the_fft_y_pass(gpu, monkeypatch, polarized, eps):
    """A polarized table beam (packed values: two transforms, gathered at s and -s) and an unpolarized beam (plain
    values), forced on: against the oracle on a subset with the outrigger, an auto and flipped members to
    10 eps + 1e-12, and against the forced-off run to 10 eps; the exact duplicate comes back bit-equal."""
    cfg, sub = _hex_outrigger(polarized, eps)
    on, st_on = _run(cfg, monkeypatch, "1")
    off, st_off = _run(cfg, monkeypatch, "0")
    assert np.isfinite(on).all()
    assert st_on["fft_cells"] < st_off["fft_cells"], (st_on["fft_cells"], st_off["fft_cells"])  # no y-pass, no C
    exact = _exact(polarized)
    e_on, e_off, d = rel_l2(on[..., sub], exact), rel_l2(off[..., sub], exact), rel_l2(on, off)
    print(f"ydirect base case polarized={polarized} eps={eps:g}: oracle on {e_on:.3e} off {e_off:.3e}, on vs off {d:.3e}")
    assert e_on < 10 * eps + 1e-12, e_on
    assert d < 10 * eps, d
    n = len(cfg["baselines"])
    assert np.array_equal(on[..., n - 1], on[..., 11])
    check_forward(on, cfg, exact, sub=sub, label=f"ydirect {polarized} {eps:g}")


def test_direct_y_sums_with_source_chunks_and_two_beams(gpu, monkeypatch):
    """Source chunks add into the block through the values variant's `accumulate`; two beams run several pair lists
    (a packed list per beam and the cross list with four plain transforms).  Forced on: chunked against unchunked
    to 1e-12 (the sum over sources is linear; the two runs differ in rounding only), the two-beam run against the oracle."""
    cfg, sub = _hex_outrigger(True, 6e-8)
    one, st = _run(cfg, monkeypatch, "1")
    off, st_off = _run(cfg, monkeypatch, "0")
    assert st["fft_cells"] < st_off["fft_cells"]
    chunked, _ = _run(dict(cfg, min_chunks=3), monkeypatch, "1")
    assert rel_l2(chunked, one) < 1e-12, rel_l2(chunked, one)
    freqs = cfg["freqs"]
    other = fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs, 12.0, nza=91, naz=180), freqs)
    two = dict(cfg, beam=[cfg["beam"], other], beam_idx=np.arange(len(cfg["ants"])) % 2)
    v2, st2 = _run(two, monkeypatch, "1")
    v2_off, st2_off = _run(two, monkeypatch, "0")
    assert st2["fft_cells"] < st2_off["fft_cells"]
    v2c, _ = _run(dict(two, min_chunks=3), monkeypatch, "1")
    assert rel_l2(v2c, v2) < 1e-12, rel_l2(v2c, v2)
    exact = oracle_simulate(dict(two, baselines=[two["baselines"][i] for i in sub]))
    assert rel_l2(v2[..., sub], exact) < 10 * 6e-8 + 1e-12
    assert rel_l2(v2, v2_off) < 10 * 6e-8
    check_forward(v2, two, exact, sub=sub, label="ydirect two beams")


def test_direct_y_sums_row_slices_and_phase_seeds(gpu, monkeypatch):
    """The rows are cut into tiles of 32, slices of whole tiles, and the running phase is re-seeded every 128 rows: a
    band whose na_y is a multiple of neither (found by probing a few top frequencies; the grid's size is in the
    statistics), and C3's top channel (about 4 000 rows) with every 20th baseline -- both at eps = 1e-10, where an
    accumulated phase error would show, against the oracle."""
    f_top, na_y = None, 0
    for f in 158e6 + 0.9e6 * np.arange(8):
        cfg, sub = _hex_outrigger(False, 1e-10, freqs=(150e6, f), nsrc=40)
        _, st = _run(cfg, monkeypatch, "1")
        na_y = int(st["n2z"]) % 65536
        if na_y % 32 != 0:
            f_top = f
            break
    assert f_top is not None, na_y
    cfg, sub = _hex_outrigger(False, 1e-10, freqs=(150e6, f_top))
    v, st = _run(cfg, monkeypatch, "1")
    assert int(st["n2z"]) % 65536 == na_y and na_y % 32 != 0 and na_y % 128 != 0
    exact = oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub]))
    e = rel_l2(v[..., sub], exact)
    print(f"ydirect na_y={na_y}: oracle {e:.3e}")
    assert e < 10 * 1e-10 + 1e-12, (na_y, e)

    c3 = synth.make_config("C3", nsrc=5000, nfreq=2, ntimes=1)
    freqs = np.array([200e6])
    ra, dec, flux = synth.catalog(5000, freqs, 0)
    c3.update(freqs=freqs, fluxes=flux, ra=ra, dec=dec, eps=1e-10, baselines=c3["baselines"][::20],
              beam=fftvis_amd.TabulatedBeam(synth.synthetic_efield_table(freqs), freqs))
    v, st = _run(c3, monkeypatch, "1")
    off, st_off = _run(c3, monkeypatch, "0")
    # (so few baselines that the masked y-pass stores next to nothing: the cells of B the sums read are not fewer than
    # the y-pass moved, only counted differently)
    assert st["fft_cells"] != st_off["fft_cells"]
    rows = int(st["n2z"]) % 65536
    assert rows > 3500, rows
    n = len(c3["baselines"])
    s3 = sorted(set(np.random.default_rng(2).choice(n, 16, replace=False)) | {0, n - 1})
    exact = oracle_simulate(dict(c3, baselines=[c3["baselines"][i] for i in s3]))
    e, e_off = rel_l2(v[..., s3], exact), rel_l2(off[..., s3], exact)
    print(f"ydirect C3 top channel, {rows} rows: oracle on {e:.3e} off {e_off:.3e}")
    assert e < 10 * 1e-10 + 1e-12, e
    check_forward(v, c3, exact, sub=s3, label="ydirect C3 top channel")


def test_direct_y_sums_do_not_depend_on_plan_or_dedup_switches(gpu, monkeypatch):
    """The points, their u-groups and the arithmetic follow the geometry alone.  Forced on: with and without the column
    plan (B then holds every column; one geometry for both runs) the block agrees to 1e-13, and gathering every baseline
    by itself (FFTVIS_HIP_NO_TARGET_DEDUP=1) agrees to 6e-11 -- the members' vectors differ by rounding."""
    c3 = synth.make_config("C3", nsrc=3000, nfreq=2, ntimes=1)
    c3["baselines"] = c3["baselines"][::3] + [(5, 5), (349, 17)]
    monkeypatch.setenv("FFTVIS_HIP_GRID_SLACK", "0")  # one geometry for both runs (a plan's geometry takes no grid slack)
    some, st_some = _run(c3, monkeypatch, "1")
    every, st_every = _run(c3, monkeypatch, "1", env=("FFTVIS_HIP_NO_COLUMN_PLAN",))
    off, st_off = _run(c3, monkeypatch, "0")
    monkeypatch.delenv("FFTVIS_HIP_GRID_SLACK")
    print("ydirect switches: fft_cells plan", st_some["fft_cells"], "no plan", st_every["fft_cells"], "off", st_off["fft_cells"])
    # (the run without a plan stores and reads every column's blocks; the switched-off run keeps its plan and a y-pass)
    assert st_some["fft_cells"] < 0.8 * st_every["fft_cells"] and st_some["fft_cells"] < st_off["fft_cells"]
    assert rel_l2(some, every) < 1e-13, rel_l2(some, every)
    once, st_once = _run(c3, monkeypatch, "1")
    each, st_each = _run(c3, monkeypatch, "1", env=("FFTVIS_HIP_NO_TARGET_DEDUP",))
    assert st_once["interp_items"] < 0.5 * st_each["interp_items"]
    assert rel_l2(once, each) < 6e-11, rel_l2(once, each)


def test_direct_y_sums_are_taken_by_geometry_only(gpu, monkeypatch):
    """By default a lattice array on large grids (C3's shape) takes the direct sums and a scattered array -- no repeated
    u, two orders of magnitude more points per column -- keeps the FFT y-pass: its `fft_cells` are those of the run
    with the path switched off."""
    c3 = synth.make_config("C3", nsrc=3000, nfreq=2, ntimes=1)
    _, st_def = _run(c3, monkeypatch, None)
    _, st_on = _run(c3, monkeypatch, "1")
    _, st_off = _run(c3, monkeypatch, "0")
    assert st_def["fft_cells"] == st_on["fft_cells"] < st_off["fft_cells"]
    sc = synth.make_config("C3", nsrc=3000, nfreq=2, ntimes=1, array="scattered350")
    _, st_def = _run(sc, monkeypatch, None)
    _, st_off = _run(sc, monkeypatch, "0")
    assert st_def["fft_cells"] == st_off["fft_cells"]
