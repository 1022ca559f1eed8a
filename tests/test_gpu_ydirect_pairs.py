"""Direct y sums (fv_ydirect.h): walk slots.  A point (u, v) and its mirror image (u, -v) in the same u-group are
walked as one slot -- four real sums give both values -- and FFTVIS_HIP_YD_PAIRS=0 gives every point a slot of its own.
Forced on with FFTVIS_HIP_YDIRECT=1 at eps = 1e-10, against the oracle's exact sums with the bound of
test_gpu_ydirect.py (10 eps + 1e-12), and pairs on against pairs off.  What the plan paired is read from the line
FFTVIS_HIP_DEBUG_YDIRECT=1 prints ("ydirect slots ...: P pairs, S singles, ...") and compared with a count made here
from the baseline vectors."""

import re

import numpy as np
import pytest

from fftvis_amd import synth
from tests.helpers import oracle_simulate, rel_l2
from tests.test_gpu_ydirect import _hex_outrigger, _run
from tests.test_gpu_ydirect_tiles import _run_sliced

pytestmark = pytest.mark.gpu
EPS = 1e-10
BOUND = 10 * EPS + 1e-12
# Pairs on against off: the sums are regrouped (rounding: some 1e-15), and the -v member's phase follows its partner's
# v, which differs from its own by at most the clustering tolerance -- 1e-3 eps of phase at the top frequency.
PAIR_BOUND = 1e-2 * EPS + 1e-13
PAIRS, DEBUG = "FFTVIS_HIP_YD_PAIRS", "FFTVIS_HIP_DEBUG_YDIRECT"
PLAN_LINE = re.compile(r"ydirect plan pair (\d+) channels \[(\d+), (\d+)\): (\d+) items, (\d+) points on (\d+) u-groups")
SLOT_LINE = re.compile(r"ydirect slots pair (\d+) channels \[(\d+), (\d+)\): (\d+) pairs, (\d+) singles, (\d+) walk slots for (\d+) points")


def _vectors(cfg):
    pos = {k: np.asarray(v, float) for k, v in cfg["ants"].items()}
    return np.array([pos[j][:2] - pos[i][:2] for i, j in cfg["baselines"]])


def _host_count(vec, sides):
    """(points, pairs) of a list of baseline vectors: distinct (u, v) to the micrometre -- and their negatives when the
    run gathers at s and -s (sides = 2) -- and the (u, v), (u, -v) couples among them, v != 0."""
    q = np.rint(vec * 1e6).astype(np.int64)
    pts = {(int(u), int(v)) for u, v in q}
    if sides == 2:
        pts |= {(-u, -v) for u, v in pts}
    return len(pts), sum(1 for u, v in pts if v > 0 and (u, -v) in pts)


def _run_pairs(cfg, monkeypatch, capfd, on, slices=None):
    """One forced-on run with the debug lines; returns (block, statistics, [(points, pairs, singles, slots)] per plan)."""
    if on:
        monkeypatch.delenv(PAIRS, raising=False)
    else:
        monkeypatch.setenv(PAIRS, "0")
    monkeypatch.setenv(DEBUG, "1")
    capfd.readouterr()
    v, st = _run_sliced(cfg, monkeypatch, slices)
    err = capfd.readouterr().err
    monkeypatch.delenv(DEBUG)
    monkeypatch.delenv(PAIRS, raising=False)
    plans = {m.group(1, 2, 3): int(m.group(5)) for m in PLAN_LINE.finditer(err)}
    slots = {m.group(1, 2, 3): tuple(int(x) for x in m.group(7, 4, 5, 6)) for m in SLOT_LINE.finditer(err)}
    assert slots and set(slots) == set(plans), err[-2000:]
    for key, (npts, pairs, singles, nslots) in slots.items():
        assert npts == plans[key] and 2 * pairs + singles == npts and pairs + singles == nslots, (key, slots[key], plans[key])
    return v, st, sorted(slots.values())


def _members(cfg):
    """Baselines of the hexagon that the subset must hold: both members of a mirror pair (u and v both non-zero; the
    second one was given backwards where the list has such a couple) and an east-west baseline (v = 0)."""
    vec = _vectors(cfg)
    flipped = set(range(4, len(vec), 10))
    ew = next(i for i, b in enumerate(vec) if abs(b[1]) < 1e-9 and abs(b[0]) > 1.0)
    best = None
    for i, b in enumerate(vec):
        if abs(b[0]) < 1.0 or abs(b[1]) < 1.0:
            continue
        for j in np.flatnonzero((np.abs(vec[:, 0] - b[0]) < 1e-9) & (np.abs(vec[:, 1] + b[1]) < 1e-9)):
            if best is None or (int(j) in flipped and best[1] not in flipped):
                best = (i, int(j))
        if best is not None and best[1] in flipped:
            break
    assert best is not None
    return best, ew


_EXACT = {}


def _case(polarized):
    cfg, sub = _hex_outrigger(polarized, EPS, nsrc=300)
    pair, ew = _members(cfg)
    sub = sorted(set(sub) | set(pair) | {ew})
    if polarized not in _EXACT:
        _EXACT[polarized] = oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub]))
    return cfg, sub, pair, ew, _EXACT[polarized]


@pytest.mark.parametrize("polarized", [True, False], ids=["packed", "plain"])
def test_pairs_on_and_off_match_the_oracle_and_each_other(gpu, monkeypatch, capfd, polarized):
    """HERA-37 plus the outrigger, 2 channels x 2 times, a polarized table beam (packed: every baseline's two signs are
    points) and an unpolarized one (plain: the box of the targets is off centre, so the contraction carries the centre's
    phase).  The subset holds both members of a mirror pair, an east-west baseline (v = 0: a single), outrigger baselines
    (singles), flipped members, autos and the exact duplicate, which stays bit-equal to its twin.  The plan's count of
    pairs is the host's, and zero with the switch off."""
    cfg, sub, pair, ew, exact = _case(polarized)
    n = len(cfg["baselines"])
    vec = _vectors(cfg)
    assert abs(vec[pair[0]][0] - vec[pair[1]][0]) < 1e-9 and abs(vec[pair[0]][1] + vec[pair[1]][1]) < 1e-9 and vec[ew][1] == 0.0
    on, st_on, slots_on = _run_pairs(cfg, monkeypatch, capfd, True)
    off, st_off, slots_off = _run_pairs(cfg, monkeypatch, capfd, False)
    _, st_fft = _run(cfg, monkeypatch, "0")
    assert st_on["fft_cells"] == st_off["fft_cells"] < st_fft["fft_cells"]  # both took the path
    assert st_on["interp_items"] == st_off["interp_items"]
    counts = {_host_count(vec, s) for s in (1, 2)}
    for npts, pairs, singles, nslots in slots_on:
        assert (npts, pairs) in counts and pairs > 0, (npts, pairs, counts)
    for npts, pairs, singles, nslots in slots_off:
        assert pairs == 0 and singles == nslots == npts
    e_on, e_off, d = rel_l2(on[..., sub], exact), rel_l2(off[..., sub], exact), rel_l2(on, off)
    worst = max(rel_l2(on[..., [i]], off[..., [i]]) for i in (pair[0], pair[1], ew, n - 3))
    print(f"ydirect pairs polarized={polarized}: slots on {slots_on} off {slots_off}; oracle on {e_on:.3e} off {e_off:.3e}; "
          f"on vs off {d:.3e} (pair members, east-west, auto: at most {worst:.3e})")
    assert np.isfinite(on).all() and np.isfinite(off).all()
    assert e_on < BOUND, e_on
    assert e_off < BOUND, e_off
    assert d < PAIR_BOUND, d
    assert worst < PAIR_BOUND, worst
    for v in (on, off):
        assert np.array_equal(v[..., n - 1], v[..., 11])


def test_a_sheared_array_has_no_pairs(gpu, monkeypatch, capfd):
    """The same antennas with y -> y + 0.37 x: every baseline keeps its u, so the u-groups are those of the hexagon, but
    (u, -v) is a point only where u = 0.  Plain, every cross baseline given once in antenna order: a north-south
    baseline and its reverse are never both listed, no point has a partner and the plan reports zero pairs.  Packed with
    the list of the base case (flipped members, autos, the duplicate), a u = 0 baseline's own two signs are each other's
    mirror image: those pair, nothing else does, and the count is the host's.  Both against the oracle."""
    base, _ = _hex_outrigger(False, EPS, nsrc=300)
    ants = {k: np.array([p[0], p[1] + 0.37 * p[0], p[2]]) for k, p in base["ants"].items()}
    plain = dict(base, ants=ants, baselines=synth.all_cross_baselines(ants))
    u_base = {int(x) for x in np.rint(_vectors(dict(base, baselines=plain["baselines"]))[:, 0] * 1e6)}
    vec = _vectors(plain)
    assert {int(x) for x in np.rint(vec[:, 0] * 1e6)} == u_base
    npts, pairs = _host_count(vec, 1)
    assert pairs == 0
    v, st, slots = _run_pairs(plain, monkeypatch, capfd, True)
    assert slots == [(npts, 0, npts, npts)], (slots, npts)
    sub = list(range(0, len(plain["baselines"]), 45)) + [len(plain["baselines"]) - 1]
    e = rel_l2(v[..., sub], oracle_simulate(dict(plain, baselines=[plain["baselines"][i] for i in sub])))
    said = f"ydirect sheared, plain: slots {slots}, oracle {e:.3e}"  # (printed below: the next run's capture would swallow it)
    assert e < BOUND, e

    cfg, sub = _hex_outrigger(True, EPS, nsrc=300)
    packed = dict(cfg, ants=ants)
    vec = _vectors(packed)
    counts = {_host_count(vec, s) for s in (1, 2)}
    north_south = len({abs(int(y)) for x, y in np.rint(vec * 1e6) if x == 0 and y != 0})
    assert _host_count(vec, 2)[1] == north_south > 0
    v, st, slots = _run_pairs(packed, monkeypatch, capfd, True)
    for npts, pairs, singles, nslots in slots:
        assert (npts, pairs) in counts, (npts, pairs, counts)
    e = rel_l2(v[..., sub], oracle_simulate(dict(packed, baselines=[packed["baselines"][i] for i in sub])))
    print(f"{said}\nydirect sheared, packed list: slots {slots}, oracle {e:.3e}")
    assert e < BOUND, e


def test_c3_shape_slot_count_and_statistics(gpu, monkeypatch, capfd):
    """C3's array (HERA-350, packed) with few sources and every third baseline: the plan's pairs + singles are the
    host's count from the baseline vectors, and pairing changes neither `fft_cells` nor `interp_items`."""
    c3 = synth.make_config("C3", nsrc=3000, nfreq=2, ntimes=1)
    c3["baselines"] = c3["baselines"][::3]
    vec = _vectors(c3)
    counts = {s: _host_count(vec, s) for s in (1, 2)}
    on, st_on, slots_on = _run_pairs(c3, monkeypatch, capfd, True)
    off, st_off, slots_off = _run_pairs(c3, monkeypatch, capfd, False)
    print(f"ydirect C3 shape: host (points, pairs) {counts}, slots on {slots_on} off {slots_off}, on vs off {rel_l2(on, off):.3e}")
    for npts, pairs, singles, nslots in slots_on:
        assert (npts, pairs) in counts.values(), (npts, pairs, counts)
        assert pairs > 0 and nslots == npts - pairs
    for npts, pairs, singles, nslots in slots_off:
        assert pairs == 0 and nslots == npts
    assert st_on["fft_cells"] == st_off["fft_cells"] and st_on["interp_items"] == st_off["interp_items"]
    assert rel_l2(on, off) < 1e-2 * c3["eps"] + 1e-13


def test_row_slices_with_pairs(gpu, monkeypatch, capfd):
    """The band of test_gpu_ydirect_tiles.py whose na_y is a multiple of neither the tile height nor the seed distance,
    pairs on: 1, 2 and 3 slices agree to 1e-13 (they differ in where the four sums are cut: rounding only) and the
    one-slice block is within the bound of the oracle."""
    f_top, na_y = None, 0
    for f in 158e6 + 0.9e6 * np.arange(8):
        cfg, sub = _hex_outrigger(False, EPS, freqs=(150e6, f), nsrc=40)
        _, st = _run(cfg, monkeypatch, "1")
        na_y = int(st["n2z"]) % 65536
        if na_y % 32 != 0 and na_y % 128 != 0:
            f_top = f
            break
    assert f_top is not None, na_y
    cfg, sub = _hex_outrigger(False, EPS, freqs=(150e6, f_top), nsrc=300)
    blocks = {}
    for n in (1, 2, 3):
        blocks[n], st, slots = _run_pairs(cfg, monkeypatch, capfd, True, slices=n)
        assert int(st["n2z"]) % 65536 == na_y and all(s[1] > 0 for s in slots), (na_y, slots)
    e = rel_l2(blocks[1][..., sub], oracle_simulate(dict(cfg, baselines=[cfg["baselines"][i] for i in sub])))
    print(f"ydirect pairs, slices, na_y={na_y}: oracle {e:.3e}")
    assert e < BOUND, e
    for n in (2, 3):
        d = rel_l2(blocks[n], blocks[1])
        print(f"ydirect pairs, slices={n} against one slice: {d:.3e}")
        assert d < 1e-13, (n, d)
