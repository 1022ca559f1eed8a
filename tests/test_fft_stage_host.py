"""CPU checks of what holds the pruned FFT stage (tests/fft_stage_refs.py): the ladder's modelled plans are the table's,
every input slot and every output index of the long dimension lies under a footprint, no combination brings a lax bound
or a yardstick that is none, and -- the argument of the whole module as a test -- three faults injected into the CPU
port's FFT stage pass the eps check of the older, sparse op tests and are caught here."""

import numpy as np
import pytest

from tests import fft_stage_refs as F
from tests import nufft_op_refs as R


def _id(combo):
    return f"{combo[0]}-{combo[1]:g}-{combo[2]:g}"


def test_model_gives_every_plan_of_the_table():
    seen = set()
    for name, eps, sigma in F.COMBOS:
        cs = R.case(name)
        passes = F.plan(name, eps, sigma)
        g = passes[cs["long_dim"]]
        want = F.table_entry(name, eps, sigma)
        if want is not None:
            assert (g["P"], g["Q"], g["folded"]) == want, (name, eps, sigma, g)
        if name in F.CASES_FP64:
            seen |= {F.plan_key(p)[:4] for p in passes}
        short = passes[1 - cs["long_dim"]]
        if F.family(name) == "blk":  # both passes on the register-resident kernels: B in column blocks
            assert g["st"] and short["st"] and (short["P"], short["Q"]) == (1, 512), (name, eps, sigma, passes)
        else:  # a tiny short dimension: the port's grid stays small, the long pass has 16 to 24 lines of input
            assert short["n2"] <= 80 and 8 <= short["n_in"] <= 24, (name, eps, sigma, short)
    assert F.expected_table() <= seen, sorted(F.expected_table() - seen)
    # every line of the table is a rung, and the rungs in between are there
    for (eps, sigma), fams in F.TABLE.items():
        for fam, rungs in fams.items():
            for S in rungs:
                assert (f"fft_{fam}_{S}", eps, sigma) in F.COMBOS
    between = [c for c in F.COMBOS if F.family(c[0]) in ("row", "col") and F.table_entry(*c) is None and c[1] == 1e-6]
    assert {c[0] for c in between} == {"fft_row_800", "fft_row_1040"} and {c[2] for c in between} == {1.25}
    assert set(F.FP32_TABLE) == set(F.ROW32_RUNGS)


@pytest.mark.parametrize("combo", F.COMBOS, ids=_id)
def test_every_slot_and_every_output_of_the_long_dimension_is_under_a_footprint(combo):
    """From the geometry alone.  A point of the box can touch the slots [first, last) that the box's two ends reach; the
    slots outside round n_in up to whole bins of 8 (and n1 up to the next even number), the outputs outside are the
    guard cells of n_out -- at most 10 and 8 of them.  Inside, nothing is left out: sources sit at most two cells of
    the device's grid apart before their jitter of 0.4 spacings (three after it), targets at most three output cells."""
    name, eps, sigma = combo
    cs = R.case(name)
    d = cs["long_dim"]
    g, cov = F.plan(name, eps, sigma)[d], F.coverage(name, eps, sigma)[d]
    for key, n, pad, gap in (("in", g["n_in"], 10, 3.0), ("out", g["n_out"], 8, 3.0)):
        first, last = cov[key + "_reach"]
        assert 0 <= first and last <= n and last - first >= n - pad, (combo, key, first, last, n)
        assert cov[key][first:last].all(), (combo, key, np.flatnonzero(~cov[key][first:last])[:5])
        assert cov[key + "_gap"] <= gap < g["w"], (combo, key, cov[key + "_gap"])
    M, N = F._counts(cs["S"], R._RECIPES[name]["combos"])
    assert 2.0 * F.X_LONG / (M - 1) / g["h"] <= 2.0 and 2.0 * cs["S"] / (N - 1) * g["h"] * g["n2"] / (2 * np.pi) <= 3.0
    # so every residue of the pruned FFT is read, and a folded row has numbers in every one of its folds
    assert {int(i) % g["P"] for i in np.flatnonzero(cov["out"])} == set(range(g["P"]))
    for k in range(-(-g["n_in"] // g["Q"])):
        assert cov["in"][k * g["Q"]:(k + 1) * g["Q"]].any(), (combo, k)


@pytest.mark.parametrize("combo", F.COMBOS, ids=_id)
def test_combination_brings_no_lax_bound_and_a_real_yardstick(combo):
    """Conditions on the inputs, not measurements of the device (the rule of tests/test_nufft_op_host.py): where a run is
    anchored to the exact sum the derived floor is at most 5 units, the port's worst element at most 32 and the port meets
    the op's contract row by row; Z_case, one fp64 FFT against a long-double one in units of the FFT term, is at most 4
    -- a case beyond that is changed, never the cap.  The fp32 rungs that are NOT anchored are the ones whose floor
    forbids it."""
    name, eps, sigma = combo
    if combo in F.ANCHORED:
        b = R.bound(name, eps, sigma)
        assert np.isfinite(b["Y_case"]) and b["Y_case"] <= 32.0 and b["Y_plain"] <= 32.0, (b["Y_case"], b["Y_plain"])
        assert np.isfinite(b["floor"]).all() and b["floor"].max() <= 5.0, float(b["floor"].max())
        assert np.all(b["port_rows"] <= 5 * eps), (b["port_rows"] / eps).max()
        m = R.judge(np.array(R.port_result(name, eps, sigma)), name, eps, sigma, label="port")
        assert m["ok_element"] and m["ok_rows"], m
    else:
        assert R.floor(R.case(name), eps, sigma).max() > 5.0
    z = F.z_case(name, eps, sigma)
    assert 0.0 < z <= 4.0, z
    assert 4.0 <= F.k_factor(name, eps, sigma) <= 16.0


def test_fft_argument_of_the_port_and_the_fft_term():
    name, eps, sigma = "fft_row_62", 1e-9, 2.0
    cs = R.case(name)
    a, b = R.port_result(name, eps, sigma), F.port(name, eps, sigma, F.fft_fp64)
    assert np.abs(a - b).max() <= 0.01 * F.fft_term(name, eps, sigma).min()  # the default IS scipy's fp64 ifftn
    l2 = R.row_norms(cs["c"])[1]
    t2 = R.floor(cs, eps, sigma) * (eps * l2[:, None]) - R.phase_term(cs)[:, None] * (1 if R.EXTENDED else 2)
    assert np.allclose(t2, F.fft_term(name, eps, sigma), rtol=1e-9)
    assert np.allclose(R.fft_term(cs, eps, sigma, precision=1), 2.0**29 * F.fft_term(name, eps, sigma))


# ---------------------------------------------------------------------------------------------------------------------
# Teeth
# ---------------------------------------------------------------------------------------------------------------------
def _long_axis(name):
    return 2 - R.case(name)["long_dim"]  # the port's grid is [t][y][x]


def _port_grid_slots(name, eps, sigma):
    """Which slots of the port's fine grid, along the long dimension, the case's sources write (the port's own rule)."""
    from oracle import cpu_nufft

    cs = R.case(name)
    x = np.asarray(cs["coords"][cs["long_dim"]], float)
    w, _ = cpu_nufft.es_params(eps, sigma)
    xc = 0.5 * (x.min() + x.max())
    s = np.asarray(cs["targets"][cs["long_dim"]], float)
    _, n2, h = cpu_nufft._geom(np.abs(x - xc).max(), np.abs(s - 0.5 * (s.min() + s.max())).max(), sigma, w)
    a = np.ceil((x - xc) / h + n2 // 2 - w / 2).astype(int)
    hit = np.zeros(n2, bool)
    for k in range(w):
        hit[a + k] = True
    return hit


def _faults(name, eps, sigma):
    """(a) one output bin of the long dimension times 1 + 1e-10; (b) one residue class of outputs, every P-th bin,
    rotated by 1e-11 rad; (c) the contribution of one input slot dropped -- a slot no source of the sparse twin writes
    and one of the dense case does."""
    ax = _long_axis(name)
    P = F.plan(name, eps, sigma)[R.case(name)["long_dim"]]["P"]
    dense, sparse = _port_grid_slots(name, eps, sigma), _port_grid_slots(name + "_sparse", eps, sigma)
    assert dense.size == sparse.size  # the same boxes: the same grid
    n2 = dense.size
    free = np.flatnonzero(dense & ~sparse)
    slot = int(free[np.argmin(np.abs(free - (n2 // 2 + n2 // 7)))])

    def index(i):
        return tuple(i if d == ax else slice(None) for d in range(3))

    def bin_scaled(grid, axes):
        out = F.fft_fp64(grid, axes)
        out[index(n2 // 2 + n2 // 5)] *= 1.0 + 1e-10
        return out

    def residue_rotated(grid, axes):
        out = F.fft_fp64(grid, axes)
        out[index(slice(1, None, P))] *= np.exp(1e-11j)
        return out

    def slot_dropped(grid, axes):
        grid = grid.copy()
        grid[index(slot)] = 0.0
        return F.fft_fp64(grid, axes)

    return {"bin scaled": bin_scaled, "residue rotated": residue_rotated, "slot dropped": slot_dropped}


@pytest.mark.parametrize("name", F.TEETH)
def test_faults_the_sparse_eps_check_passes_are_caught(name):
    """Each fault, put into the port through ``fft=``, passes the element and row bound on the twin of the case with 400
    random sources and 300 random targets -- the density of the older op tests -- and fails the differential bound
    against the unfaulted port on the dense case; a dropped input slot also fails the dense case's anchor."""
    eps, sigma = 1e-6, 2.0
    twin = name + "_sparse"
    assert R.case(twin)["c"].shape[1] == 400 and R.case(twin)["targets"][0].size == 300
    good = F.port(name, eps, sigma, F.fft_fp64)
    assert F.diff_ok(good, F.port(name, eps, sigma, F.fft_longdouble), name, eps, sigma)[0]
    for label, fft in _faults(name, eps, sigma).items():
        m = R.judge(F.port(twin, eps, sigma, fft), twin, eps, sigma, label=label)
        assert m["ok_element"] and m["ok_rows"], (label, m)
        ok, worst, K = F.diff_ok(F.port(name, eps, sigma, fft), good, name, eps, sigma)
        assert not ok and worst > 10 * K, (label, worst, K)
        m = R.judge(F.port(name, eps, sigma, fft), name, eps, sigma, label=label)
        assert (m["ok_element"] and m["ok_rows"]) == (label != "slot dropped"), (label, m)
