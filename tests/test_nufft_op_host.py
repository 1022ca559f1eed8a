"""CPU checks of the references that hold the type-3 transform op (tests/nufft_op_refs.py): the extended-precision exact
sum against 50-digit arithmetic and against the fp64 oracle, the caps every seeded case must respect so that none
brings a lax bound with it, and the metric itself -- it must see a wrong corner target, a leak between rows of different
scale and a transform that is 100 times too coarse, all of which the whole-array rel l2 lets through."""

import mpmath
import numpy as np
import pytest

from oracle import nudft
from tests import nufft_op_refs as R



def test_registry_is_what_the_tests_assume():
    for name in R.CASES:
        cs = R.case(name)
        M, N, ntr = cs["coords"][0].size, cs["targets"][0].size, cs["c"].shape[0]
        assert M <= 400 and N <= 300 and ntr <= 24 and len(cs["coords"]) == len(cs["targets"]) == cs["dim"]
        corner = cs["kind"] == 1
        for x, s in zip(cs["coords"], cs["targets"]):  # a corner target sits on the box's extremes in EVERY dimension
            assert np.all((s[corner] == s.min()) | (s[corner] == s.max()))
        if corner.any():
            assert corner.sum() == 2 ** cs["dim"]
            hit = np.ones(M, bool)
            for x in cs["coords"]:
                hit &= (x == x.min()) | (x == x.max())
            assert hit.sum() >= 2 ** cs["dim"]  # and the source box has its corners too
        if cs["precision"] == 1:
            assert cs["c"].dtype == np.complex64 and all(a.dtype == np.float32 for a in cs["coords"] + cs["targets"])
            assert R.max_phase(cs) <= 60.0 and M <= 200
    sc = R.case("2d_rowscales_24")["c"]
    assert np.isclose(R.row_norms(sc)[1][-1] / R.row_norms(sc)[1][0], 1e12, rtol=0.5)


@pytest.mark.parametrize("name", ["2d_corners", "2d_tiny_8x8", "3d_cubic"])
def test_exact_sum_against_50_digits(name):
    """Six elements of three cases, corner targets among them, to 2^-60 of ||c_t||_1 (where long double is no wider than
    double ``exact_type3`` is the fp64 oracle and is held to that sum's own rounding instead)."""
    cs = R.case(name)
    re, im = R.exact(name)
    ntr, N = re.shape
    l1, l2 = R.row_norms(cs["c"])
    tol = 2.0**-60 * l1 if R.EXTENDED else R.phase_term(cs, precision=2) + cs["c"].shape[1] * 2.0**-53 * l2
    mpmath.mp.dps = 50
    picks = [(0, 0), (ntr - 1, 1), (1, int(np.flatnonzero(cs["kind"] == 1)[-1])), (0, N - 1), (ntr - 1, N // 2), (1, N // 3)]
    assert sum(cs["kind"][k] == 1 for _, k in picks) >= 3
    for t, k in picks:
        tot = mpmath.mpc(0)
        for j in range(cs["c"].shape[1]):
            ph = sum(mpmath.mpf(float(s[k])) * mpmath.mpf(float(x[j])) for x, s in zip(cs["coords"], cs["targets"]))
            cj = cs["c"][t, j]
            tot += mpmath.mpc(float(cj.real), float(cj.imag)) * mpmath.expj(ph)
        # longdouble -> mpf exactly: through its two double halves
        hi_r, hi_i = float(re[t, k]), float(im[t, k])
        got = mpmath.mpc(mpmath.mpf(hi_r) + mpmath.mpf(float(re[t, k] - hi_r)),
                         mpmath.mpf(hi_i) + mpmath.mpf(float(im[t, k] - hi_i)))
        assert abs(got - tot) <= float(tol[t]), (name, t, k, float(abs(got - tot) / l1[t]))


@pytest.mark.parametrize("name", R.CASES)
def test_exact_sum_against_fp64_oracle(name):
    """The fp64 oracle forms its phases in fp64 (term 1 of ``floor`` at u = 2^-53) and adds M rounded terms
    (M u ||c_t||_2, the same allowance ``gpu_nudft_direct`` gets); the extended sum agrees with it to exactly that."""
    cs = R.case(name)
    got = nudft.nudft_type3([np.asarray(a, float) for a in cs["coords"]], cs["c"].astype(complex),
                            [np.asarray(a, float) for a in cs["targets"]])
    err = R._err(got, R.exact(name))
    M = cs["c"].shape[1]
    lim = R.phase_term(cs, precision=2) + M * 2.0**-53 * R.row_norms(cs["c"])[1]
    assert np.all(err <= lim[:, None]), (name, float((err / lim[:, None]).max()))


@pytest.mark.parametrize("name,eps,sigma", R.combos(R.CASES))
def test_cases_bring_no_lax_bound(name, eps, sigma):
    """Conditions on the INPUTS of the op tests, not measurements of the device: the port's own worst element is finite
    and at most 32 units of eps ||c_t||_2 (measured: 25 in 2-D, 30 in 3-D), the derived floor at most 5 at every element.
    A case that breaks either is changed (geometry, seed, the tolerances it runs at) -- never the cap."""
    b = R.bound(name, eps, sigma)
    assert np.isfinite(b["Y_case"]) and b["Y_case"] <= 32.0, b["Y_case"]
    assert np.isfinite(b["Y_plain"]) and b["Y_plain"] <= 32.0
    assert np.isfinite(b["floor"]).all() and b["floor"].max() <= 5.0, float(b["floor"].max())
    assert np.all(b["port_rows"] <= 5 * eps), (b["port_rows"] / eps).max()  # the port meets the op's own contract, row by row
    # and the port passes its own bound, as it must by construction
    m = R.judge(np.array(R.port_result(name, eps, sigma)), name, eps, sigma, label="port")
    assert m["ok_element"] and m["ok_rows"], m


def test_every_family_and_tolerance_is_covered():
    """The tolerance lists the op tests promise, per family -- a recipe that narrows its own list must leave another case
    of the family at that tolerance."""
    def covered(names, sigma):
        return {eps for n in names for eps in R.eps_list(n, sigma)}
    assert covered(R.CASES_FP64_2D, 2.0) == set(R.EPS_SIGMA2) and covered(R.CASES_FP64_2D, 1.25) == set(R.EPS_SIGMA125)
    assert covered(R.CASES_FP64_3D, 2.0) == set(R.EPS_SIGMA2) and covered(R.CASES_FP64_3D, 1.25) == set(R.EPS_SIGMA125)
    assert covered(["2d_plain32", "2d_corners32"], 2.0) == {1e-3, 1e-4} and covered(["2d_plain32"], 1.25) == {1e-4}
    assert covered(["3d_plain32", "3d_corners32"], 2.0) == {1e-3, 1e-4}
    assert covered(["3d_corners32"], 1.25) == {1e-3}
    for n in ("2d_corners", "2d_rowscales_5", "2d_rowscales_19", "2d_rowscales_24", "2d_tiny_16x5", "2d_tiny_8x8"):
        assert R.eps_list(n, 2.0) == R.EPS_SIGMA2 and R.eps_list(n, 1.25) == R.EPS_SIGMA125


def test_metric_sees_what_whole_array_rel_l2_does_not():
    name, eps, sigma = "2d_rowscales_5", 1e-9, 2.0
    cs, b, ex = R.case(name), R.bound(name, eps, sigma), R.exact(name)
    l2 = R.row_norms(cs["c"])[1]
    small, big = int(np.argmin(l2)), int(np.argmax(l2))
    corner = int(np.flatnonzero(cs["kind"] == 1)[0])
    good = np.array(R.port_result(name, eps, sigma))
    assert R.whole_rel_l2(good, ex) < 5 * eps
    m = R.judge(good, name, eps, sigma)
    assert m["ok_element"] and m["ok_rows"]

    bad = good.copy()  # one corner target of the smallest row, wrong by 3 x its bound
    bad[small, corner] = (complex(float(ex[0][small, corner]), float(ex[1][small, corner]))
                          + 3.0 * b["element"][small, corner] * eps * l2[small])
    assert R.whole_rel_l2(bad, ex) < 5 * eps  # the old check passes
    m = R.judge(bad, name, eps, sigma)
    assert not m["ok_element"] and m["worst_margin_at"] == [small, corner] and m["worst_kind"] == "corner"

    leak = good.copy()  # 1e-9 of the largest row added into the smallest
    leak[small] += 1e-9 * good[big]
    assert R.whole_rel_l2(leak, ex) < 5 * eps
    m = R.judge(leak, name, eps, sigma)
    assert not m["ok_element"] and not m["ok_rows"] and m["worst_row"] == small


@pytest.mark.parametrize("name,sigma,eps", R.SENSITIVITY)
def test_port_at_100_eps_is_rejected(name, sigma, eps):
    cs = R.case(name)
    coarse = R.port(cs["coords"], cs["c"], cs["targets"], 100 * eps, sigma)
    m = R.judge(coarse, name, eps, sigma, label="port at 100 eps")
    assert not m["ok_element"] and not m["ok_rows"], m


def test_row_permutation_is_judged_row_by_row():
    name, eps = "2d_rowscales_5", 1e-9
    perm = np.array([3, 0, 4, 2, 1])
    good = np.array(R.port_result(name, eps, 2.0))
    assert R.judge(good[perm], name, eps, 2.0, rows=perm)["ok_element"]
    assert not R.judge(good, name, eps, 2.0, rows=perm)["ok_element"]  # rows that did not follow the permutation
