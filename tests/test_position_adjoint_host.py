"""CPU tests of the position gradient's host side: the exports, the C entry point's argument checking, the Python argument
errors that are raised before a device is needed, the baseline-to-antenna scatter, and the exact reference the GPU tests
compare with (``position_adjoint_refs.exact_gbls``), pinned here against finite differences of the oracle."""

import ctypes
import functools

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib, synth
from tests.helpers import oracle_simulate
from tests.position_adjoint_refs import exact_gants, exact_gbls, position_config, random_complex, vis_shape


def test_position_adjoint_is_exported():
    assert callable(fftvis_amd.simulate_vis_position_adjoint) and callable(fftvis_amd.torch_simulate_vis_array)
    assert callable(fftvis_amd.baseline_to_antenna_gradient)
    assert "fv_sim_run_position_adjoint" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "fv_sim_run_position_adjoint")


def test_run_position_adjoint_argument_checks():
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    assert L.fv_sim_run_position_adjoint(None, 0, 1, 0, 1, buf, 0, buf, 0, 0) == 1
    assert b"handle" in L.fv_last_error()
    for g, out in [(None, buf), (buf, None)]:
        assert L.fv_sim_run_position_adjoint(None, 0, 1, 0, 1, g, 0, out, 0, 0) == 1
        assert b"null adjoint" in L.fv_last_error()
    for flags in [(2, 0), (0, -1), (3, 3)]:
        assert L.fv_sim_run_position_adjoint(None, 0, 1, 0, 1, buf, flags[0], buf, flags[1], 0) == 1
        assert b"on_device" in L.fv_last_error()
    for acc in (2, -1):
        assert L.fv_sim_run_position_adjoint(None, 0, 1, 0, 1, buf, 0, buf, 0, acc) == 1
        assert b"accumulate" in L.fv_last_error()


def test_argument_errors_come_before_device_work():
    cfg = position_config(sky="I")
    good = np.zeros(vis_shape(cfg), complex)
    nbls = len(cfg["baselines"])
    for wrt in ("positions", (), ("ants", "ants"), ("ants", "fluxes")):
        with pytest.raises(ValueError, match="wrt"):
            fftvis_amd.simulate_vis_position_adjoint(good, **cfg, wrt=wrt)
    for shape in [(3, 2, nbls), (3, 2, 2, 2, nbls - 1), (2, 3, 2, 2, nbls)]:
        with pytest.raises(ValueError, match="output shape"):
            fftvis_amd.simulate_vis_position_adjoint(np.zeros(shape, complex), **cfg)
    with pytest.raises(NotImplementedError, match="beam_coefs"):
        fftvis_amd.simulate_vis_position_adjoint(good, **cfg, beam_coefs=np.ones((7, 1, 3), complex))
    with pytest.raises(ValueError, match="backend"):
        fftvis_amd.simulate_vis_position_adjoint(good, **cfg, backend="cpu")
    with pytest.raises(ValueError, match="fluxes must have shape"):
        fftvis_amd.simulate_vis_position_adjoint(good, **dict(cfg, fluxes=np.ones((5, 3))))
    with pytest.raises(TypeError, match="adjoint_path"):
        fftvis_amd.simulate_vis_position_adjoint(good, **cfg, adjoint_path="type3")
    with pytest.raises(TypeError, match="antpos"):
        import torch

        fftvis_amd.torch_simulate_vis_array(torch.ones(24, 3), torch.zeros(7, 3), **{k: v for k, v in cfg.items() if k != "fluxes"})


def test_scatter_helper():
    """Worked by hand: ants 10, 20, 30; baselines (10, 20), (30, 20), (20, 20), (10, 30)."""
    ants = {10: np.zeros(3), 20: np.ones(3), 30: 2 * np.ones(3)}
    bls = [(10, 20), (30, 20), (20, 20), (10, 30)]
    g = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0], [100.0, 200.0, 300.0], [0.5, 0.25, 0.125]])
    got = fftvis_amd.baseline_to_antenna_gradient(g, ants, bls)
    want = np.array([[-1.5, -2.25, -3.125],      # 10: first antenna of baselines 0 and 3
                     [11.0, 22.0, 33.0],         # 20: second of 0 and 1; the auto cancels
                     [-9.5, -19.75, -29.875]])   # 30: first of 1, second of 3
    assert got.shape == (3, 3) and got.dtype == np.float64 and np.array_equal(got, want)
    assert np.all(got.sum(axis=0) == 0)
    only_auto = fftvis_amd.baseline_to_antenna_gradient(g[2:3], ants, [(20, 20)])
    assert np.all(only_auto == 0)
    with pytest.raises(ValueError, match="shape"):
        fftvis_amd.baseline_to_antenna_gradient(g[:3], ants, bls)
    import torch

    tg = fftvis_amd.baseline_to_antenna_gradient(torch.from_numpy(g), ants, bls)
    assert isinstance(tg, torch.Tensor) and np.array_equal(tg.numpy(), want)


def _fd_config(heights, polarized, compat):
    """5 antennas in +-40 m, 40 sources, 120 and 170 MHz, 2 times, two Airy beams through beam_idx, all pairs with autos
    plus the flipped baselines (3, 1) and (4, 0)."""
    c1 = synth.make_config("C1", nsrc=40, nfreq=2, ntimes=2)
    rng = np.random.default_rng(17)
    xy = rng.uniform(-40.0, 40.0, size=(5, 2))
    z = {"flat": np.zeros(5), "cm": 0.03 * rng.normal(size=5), "m": np.array([3.0, -3.0, 3.0, -3.0, 3.0])}[heights]
    return dict(c1, ants={i: np.array([xy[i, 0], xy[i, 1], z[i]]) for i in range(5)}, freqs=np.array([120e6, 170e6]),
                beam=[fftvis_amd.AiryBeam(14.0), fftvis_amd.AiryBeam(9.0)], beam_idx=np.array([0, 1, 1, 0, 1]),
                baselines=[(i, j) for i in range(5) for j in range(i, 5)] + [(3, 1), (4, 0)],
                polarized=polarized, reference_compat=compat)


@functools.lru_cache(maxsize=None)
def _fd_gradient(heights, polarized, compat):
    """dL/d ants, L = Re <G, V(ants)>, by central differences of the oracle at h = 2 mm and 1 mm, Richardson-extrapolated."""
    cfg = _fd_config(heights, polarized, compat)
    G = random_complex(vis_shape(cfg), 31)

    def loss(a, d, h):
        ants = {k: v.copy() for k, v in cfg["ants"].items()}
        ants[a][d] += h
        return np.vdot(G, oracle_simulate(dict(cfg, ants=ants))).real

    def central(a, d, h):
        return (loss(a, d, h) - loss(a, d, -h)) / (2 * h)

    fd = np.array([[(4 * central(a, d, 1e-3) - central(a, d, 2e-3)) / 3 for d in range(3)] for a in range(5)])
    return cfg, G, fd


@pytest.mark.parametrize("heights", ["flat", "cm", "m"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("polarized", [False, True])
def test_reference_equals_finite_differences_of_the_oracle(polarized, compat, heights):
    """The yardstick of the GPU tests against Richardson-extrapolated central differences of the oracle: the whole
    (nant, 3) gradient and every component (east, north, up) to 1e-9 -- 16 x the worst measured (6.1e-11, east on the
    +-3 m array; the whole gradient agreed to <= 1.1e-11), and far below any error the sign, the factor 2 pi / c or a flip
    rule could make.  On the flat array the forward drops the heights; the up component of the exact map is still what
    the differences see (a perturbed height takes the 3-D sum)."""
    cfg, G, fd = _fd_gradient(heights, polarized, compat)
    got = exact_gants(cfg, G)
    assert got.shape == (5, 3) and np.count_nonzero(fd) == 15
    whole = np.linalg.norm(got - fd) / np.linalg.norm(fd)
    comps = [np.linalg.norm(got[:, d] - fd[:, d]) / np.linalg.norm(fd[:, d]) for d in range(3)]
    print("position reference vs finite differences", heights, polarized, compat, whole, comps)
    assert whole <= 1e-9 and max(comps) <= 1e-9, (whole, comps)
    assert np.abs(got.sum(axis=0)).max() <= 1e-12 * np.abs(exact_gbls(cfg, G)).sum()
