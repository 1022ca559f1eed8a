"""The two surfaces of the fit layer's row passes give the same bits: for every operation (objective, Gauss-Newton
weighting), calibration (none, per-antenna gains, 2 x 2 Jones matrices) and precision, the call on a handle
(``fv_sim_run_residual*``, ``fv_sim_*weight_block``) and the stand-alone call on host arrays (``fv_*residual_chi2``,
``fv_*weight_rows``) launch the same kernels on the same values, so G, the rows' sums and the gradient (or H) block are
equal byte for byte -- no tolerance.

A handle of five antennas with their ten cross pairs, 2 frequencies x 2 times and 20 sources is run forward into a device
block V; the stand-alone call gets a host copy of that V, and of the same data, weights, gains or matrices and direction.
The objective's handle call runs the forward again into ``gvis``: the forward of a handle returns the same bits on every
run, which the test asserts first.  The weighting passes take two parts, a direction, and ask for the H block."""

import ctypes

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.position_adjoint_refs import position_config

pytestmark = pytest.mark.gpu

NANT, NF, NT, NSRC = 5, 2, 2, 20
PAIRS = [(i, j) for i in range(NANT) for j in range(i + 1, NANT)]
CDT = {1: np.complex64, 2: np.complex128}
RDT = {1: np.float32, 2: np.float64}


def _config(kind, precision):
    cfg = position_config("flat", "I" if kind == "jones" else "unpol", "airy", True, precision, nsrc=NSRC, nfreq=NF, ntimes=NT)
    nums = sorted(cfg["ants"])[:NANT]
    cfg["ants"] = {a: cfg["ants"][a] for a in nums}
    cfg["baselines"] = [(nums[i], nums[j]) for i, j in PAIRS]
    return cfg


def _inputs(kind, precision, shape):
    """data, weights, two parts, the gains or matrices and their direction (None without a calibration)."""
    rng = np.random.default_rng(11 + precision)
    cdt = CDT[precision]

    def c(s, scale=1.0):
        return (scale * (rng.normal(size=s) + 1j * rng.normal(size=s))).astype(cdt)

    data, parts = c(shape), [c(shape), c(shape)]
    w = rng.uniform(0.5, 2.0, size=shape).astype(RDT[precision])
    w[rng.random(shape) < 0.2] = 0  # flagged samples
    x = dx = None
    if kind != "none":
        xs = (NF, NT, 2, 2, NANT) if kind == "jones" else (NF, NT, 2 if len(shape) == 5 else 1, NANT)
        x = c(xs, 0.1)
        x += np.eye(2, dtype=cdt)[:, :, None] if kind == "jones" else 1
        dx = c(xs, 0.3)
    return data, w, parts, x, dx


def _standalone(op, kind, precision, V, data, w, parts, x, dx, tpol):
    """The stand-alone call on copies of the host arrays: (G, rows, gradient or H block)."""
    L, p = _lib.lib(), _lib.ptr
    nrows, nbls = NF * NT, len(PAIRS)
    a1 = np.array([i for i, _ in PAIRS], np.int32)
    a2 = np.array([j for _, j in PAIRS], np.int32)
    vis, own = V.copy(), [q.copy() for q in parts]
    rows = np.full(nrows, -1.0)
    grad = None if kind == "none" else np.full(x.shape, 7.0, np.complex128)
    ptrs = (ctypes.c_void_p * len(own))(*[q.ctypes.data for q in own])
    pairs = (nrows, nbls) + ((tpol,) if kind == "gains" else ()) + (NANT, p(a1), p(a2))
    if op == "objective":
        if kind == "none":
            _lib.check(L.fv_residual_chi2(0, precision, nrows, tpol * nbls, p(vis), p(data), p(w), p(rows)))
        else:
            fn = L.fv_gain_residual_chi2 if kind == "gains" else L.fv_jones_residual_chi2
            _lib.check(fn(0, precision, *pairs, p(x), p(vis), p(data), p(w), p(rows), p(grad)))
        return vis, rows, grad
    if kind == "none":
        _lib.check(L.fv_weight_rows(0, precision, nrows, tpol * nbls, len(own), ptrs, p(w), p(rows)))
    else:
        fn = L.fv_gain_weight_rows if kind == "gains" else L.fv_jones_weight_rows
        _lib.check(fn(0, precision, *pairs, p(x), p(dx), len(own), ptrs, p(vis), p(w), p(rows), p(grad)))
        assert np.array_equal(vis, V)  # read only
    return own[0], rows, grad


def _on_the_handle(op, kind, h, V_dev, data, w, parts, x, dx):
    """The handle's call, the block and the parts on the device, everything else on the host: (G, rows, gradient or H)."""
    import torch

    grad = None if kind == "none" else np.full(x.shape, 7.0, np.complex128)
    if op == "objective":
        call = {"none": h.run_residual, "gains": h.run_gain_residual, "jones": h.run_jones_residual}[kind]
        rows = call(0, NT, 0, NF, data, w, *(() if kind == "none" else (x,)), V_dev, *(() if kind == "none" else (grad,)))
        G = V_dev
    else:
        dev = [torch.from_numpy(q).cuda() for q in parts]
        torch.cuda.synchronize()
        if kind == "none":
            rows = h.weight_block(0, NT, 0, NF, dev, w)
        else:
            call = h.gain_weight_block if kind == "gains" else h.jones_weight_block
            rows = call(0, NT, 0, NF, dev, V_dev, w, x, dx, grad)
        G = dev[0]
    return G.cpu().numpy(), rows.reshape(-1), grad


@pytest.mark.parametrize("precision", [2, 1])
@pytest.mark.parametrize("kind", ["none", "gains", "jones"])
@pytest.mark.parametrize("op", ["objective", "weighting"])
def test_handle_and_standalone_calls_give_the_same_bytes(gpu, op, kind, precision):
    import torch

    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _config(kind, precision)
    polarized = kind == "jones"
    gs.release_handles()
    fftvis_amd.simulate_vis(**cfg)
    key, h = gs._acquire_handle(0, precision, cfg["eps"], 2, polarized)  # configured for exactly this run
    try:
        assert h.nbls == len(PAIRS)
        shape = h.out_shape(NT, NF)
        V_dev = torch.empty(shape, dtype=torch.complex64 if precision == 1 else torch.complex128, device="cuda")
        torch.cuda.synchronize()

        def forward():
            _lib.check(h._L.fv_sim_run(h._h, 0, NT, 0, NF, ctypes.c_void_p(V_dev.data_ptr()), 1))
            h.sync()  # (a run into a device block is only queued)
            return V_dev.cpu().numpy()

        V = forward()
        assert np.isfinite(V).all() and np.array_equal(forward(), V)
        if kind != "none":
            h.set_gain_pairs(NANT, [i for i, _ in PAIRS], [j for _, j in PAIRS])
        data, w, parts, x, dx = _inputs(kind, precision, shape)
        ref = _standalone(op, kind, precision, V.reshape(NF * NT, -1), data, w, parts, x, dx, 4 if polarized else 1)
        got = _on_the_handle(op, kind, h, V_dev, data, w, parts, x, dx)
    finally:
        gs._return_handle(key, h)
        gs.release_handles()
    assert got[0].tobytes() == ref[0].tobytes(), "G"
    assert got[1].tobytes() == ref[1].tobytes() and np.all(ref[1] > 0), "rows"
    if kind != "none":
        assert got[2].tobytes() == ref[2].tobytes() and np.count_nonzero(ref[2]) == ref[2].size, "gradient block"
