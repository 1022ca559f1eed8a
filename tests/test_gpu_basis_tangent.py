"""GPU tests of the basis-beam tangent (``simulate_vis_basis_jvp``, ``fv_sim_run_basis_tangent``, the ``jvp`` of
``torch_simulate_vis_basis``).

dV[C; D] = sum_kl (conj(D1k) C2l + conj(C1k) D2l) M_kl, the derivative of V = simulate_vis(fluxes, beam_coefs=C) along a
direction D of the coefficients (plus the forward of d_fluxes).  Checked element by element against the exact reference
``basis_adjoint_refs.exact_dv`` (two oracle forwards; the map is sesquilinear) over the basis adjoint's configuration
matrix, through Re <dV, G> = Re <D, gcoefs> + <d_fluxes, gflux> against the independently written device adjoint, against
the device's own forward, on directions whose two halves cancel, for the bits of stacks of directions and of lane counts,
at the edges of the device's slicing, through the bare C ABI and through torch's forward-mode AD.

Element-wise tolerances against the exact reference, as multiples of base.  base = eps in fp64; in fp32
base = max(the forward's own rel l2 error against the oracle on the same configuration, eps)
(``test_gpu_basis_adjoint._forward_base``).
  rel l2 of the whole result <= 10 base in fp64 (20 at upsample_factor = 1.25): the project's bound for the forward -- the
  pass IS a forward run with other weights in the gather;
  every other bound (a channel, a feed product, the largest single error, and every fp32 factor) is set at no less than
  2 x the worst ratio measured on an MI355X over the comparisons of this module (FFTVIS_TEST_METRICS=<file> logs each
  comparison's ratios, one JSON line each).  Channel norms of dV differ by up to 25 x on HERA-7, so a part whose exact
  norm is below 1e-3 of the whole is measured against 1e-3 of the whole (``worst_part``).  Measured, as ratio / base:
  fp64 (base 6e-8), the 36 matrix cells: whole <= 0.081, a channel <= 0.50, a feed product <= 0.17, max |err| / max |exact|
  <= 0.098; the edges: 0.12, 2.75, 0.22, 0.13, all four at upsample_factor = 1.25 (at 2: below the matrix's figures).
  fp32 (base 1e-5: the forward's own error stayed below eps in every cell), the 36 matrix cells: whole <= 0.82,
  a channel <= 1.81, a feed product <= 1.18, max |err| <= 1.00.
  The identities, as fractions of their bounds: the dot identity with the device adjoint 7e-5 (fp64) and 3e-4 (fp32), the
  device's own forward 1.2e-10 and 3.5e-4.
Cancelling directions, relative to |V|: dV[C; i C] and dV[C; C] - 2 simulate_vis.  The weights are summed in fp64 before
the product with M_kl, where conj(i C1) C2 = -(conj(C1) i C2) and conj(C1) C2 + conj(C1) C2 = 2 conj(C1) C2 hold exactly, so
both are expected at 0 and are held to CANCEL units of the precision's rounding (2^-53, 2^-24): rounding level, three
orders and more under eps.  Measured, in those units: dV[C; i C] 0.78 in fp64 (the two complex products round
differently under fused multiply-adds) and exactly 0 in fp32; dV[C; C] - 2 simulate_vis <= 2.07 in fp64 and <= 2.47 in
fp32 (two runs of the same transforms; the spread's sums are not ordered).  CANCEL = 8 is 3.2 x the worst.
"""

import ctypes
import functools
import json
import os

import numpy as np
import pytest

import fftvis_amd
from fftvis_amd import _lib
from tests.basis_adjoint_refs import basis_config, exact_dv, random_complex
from tests.helpers import floored_rel, rel_l2, worst_part
from tests.test_gpu_basis_adjoint import _forward_base

pytestmark = pytest.mark.gpu

K64_PART = 10.0   # fp64: a channel, a feed product (20 at upsample_factor = 1.25, like the whole): 3.6 x the worst measured
K32 = 5.0         # fp32: the whole (6 x)
K32_PART = 10.0   # fp32: a channel, a feed product (5.5 x)
C_MAX = 2.0       # fp64: max |err| / (base max |exact|) (4 at upsample_factor = 1.25; 20 x and 31 x)
C_MAX32 = 5.0     # fp32 (5 x)
CANCEL = 8.0      # cancelling directions: units of the precision's rounding, relative to |V|
D_SEED = 5


def _errors(got, exact):
    """rel l2 of the whole result, the worst rel l2 of a channel and of a feed product, and max |err| / max |exact|; a
    part whose exact norm is below 1e-3 of the whole is measured against 1e-3 of the whole."""
    err = np.asarray(got).astype(np.complex128) - exact
    floor = 1e-3 * np.linalg.norm(exact)
    feeds = lambda a: a.reshape(a.shape[:2] + (4,) + a.shape[4:])
    return {"rel_l2": floored_rel(err, exact, floor), "channel": worst_part(err, exact, 0, floor),
            "feed": worst_part(feeds(err), feeds(exact), 2, floor),
            "max_abs": float(np.abs(err).max() / max(np.abs(exact).max(), 1e-300))}


def _log(label, cfg, m, base):
    rec = {"label": label, "precision": cfg.get("precision", 2), "base": base, **{k: v / base for k, v in m.items()}}
    print("basis-tangent metrics", json.dumps(rec))
    path = os.environ.get("FFTVIS_TEST_METRICS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _assert_close(label, cfg, got, exact, base, k64=10.0):
    assert np.count_nonzero(exact) > 0 and np.isfinite(exact).all()
    assert got.shape == exact.shape
    m = _errors(got, exact)
    _log(label, cfg, m, base)
    fp64 = cfg.get("precision", 2) == 2
    whole, part = (k64, K64_PART * k64 / 10.0) if fp64 else (K32, K32_PART)
    assert m["rel_l2"] <= whole * base, (label, m, base)
    assert m["channel"] <= part * base and m["feed"] <= part * base, (label, m, base)
    assert m["max_abs"] <= (C_MAX * k64 / 10.0 if fp64 else C_MAX32) * base, (label, m, base)
    return m


def _jvp(cfg, **kw):
    return fftvis_amd.simulate_vis_basis_jvp(**cfg, **kw)


def _vis_shape(cfg):
    return (len(cfg["freqs"]), len(cfg["times"]), 2, 2, len(cfg["baselines"]))


def _direction(cfg, seed=D_SEED):
    return random_complex(np.shape(cfg["beam_coefs"]), seed)


@functools.lru_cache(maxsize=None)
def _matrix_reference(tables, sky, compat, array):
    """The exact tangent of a matrix cell (it does not depend on the run's precision)."""
    cfg = basis_config(tables, sky, compat, array)
    return exact_dv(cfg, _direction(cfg))


@pytest.mark.parametrize("array", ["coplanar", "non_coplanar", "height_terms"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("tables", ["airy", "real", "complex"])
@pytest.mark.parametrize("sky", ["I", "full"])
@pytest.mark.parametrize("precision", [2, 1])
def test_basis_tangent_matrix(gpu, precision, sky, tables, compat, array):
    cfg = basis_config(tables, sky, compat, array, precision)
    dv = _jvp(cfg, d_beam_coefs=_direction(cfg))
    assert dv.shape == _vis_shape(cfg) and dv.dtype == (np.complex64 if precision == 1 else np.complex128)
    _assert_close(f"matrix {precision} {sky} {tables} {compat} {array}", cfg, dv, _matrix_reference(tables, sky, compat, array),
                  _forward_base(cfg))


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("precision", [2, 1])
def test_dot_identity_with_the_device_adjoint(gpu, precision, compat):
    """Re <dV, G> = Re <D, gcoefs> + <d_fluxes, gflux> between independently written passes, to 10 eps |dV| |G|
    (test_gpu_adjoint's bound)."""
    cfg = basis_config("complex", "full", compat, "height_terms", precision)
    cdt = np.complex64 if precision == 1 else np.complex128
    G = random_complex(_vis_shape(cfg), 4).astype(cdt)
    D = _direction(cfg)
    dF = np.random.default_rng(3).normal(size=cfg["fluxes"].shape)
    dv = _jvp(cfg, d_beam_coefs=D, d_fluxes=dF).astype(np.complex128)
    gf, gc = fftvis_amd.simulate_vis_basis_adjoint(G, **cfg)
    lhs = np.vdot(G.astype(np.complex128), dv).real
    rhs = np.vdot(gc.astype(np.complex128), D).real + float(np.sum(dF * gf.astype(np.float64)))
    bound = 10 * cfg["eps"] * np.linalg.norm(dv) * np.linalg.norm(G)
    print("basis-tangent dot", precision, compat, abs(lhs - rhs) / bound)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("precision", [2, 1])
def test_against_the_devices_own_forward(gpu, precision, compat):
    """dV against (V(C + D) - V(C - D)) / 2 from two forward runs on the device.  Each of the three runs is within the
    forward's 10 eps of its own norm: |dV - difference| <= 10 eps (|dV| + max(|V(C + D)|, |V(C - D)|))."""
    cfg = basis_config("complex", "full", compat, "coplanar", precision)
    C, D = cfg["beam_coefs"], _direction(cfg)
    dv = _jvp(cfg, d_beam_coefs=D).astype(np.complex128)
    Vp = fftvis_amd.simulate_vis(**dict(cfg, beam_coefs=C + D)).astype(np.complex128)
    Vm = fftvis_amd.simulate_vis(**dict(cfg, beam_coefs=C - D)).astype(np.complex128)
    d = np.linalg.norm(dv - 0.5 * (Vp - Vm))
    bound = 10 * cfg["eps"] * (np.linalg.norm(dv) + max(np.linalg.norm(Vp), np.linalg.norm(Vm)))
    print("basis-tangent vs forward", precision, compat, d / bound)
    assert d <= bound, (d, bound)


@pytest.mark.parametrize("array", ["coplanar", "height_terms"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("precision", [2, 1])
def test_cancelling_directions(gpu, precision, compat, array):
    """dV[C; i C] = 0 and dV[C; C] = 2 V, at the precision's rounding level relative to |V|."""
    cfg = basis_config("complex", "full", compat, array, precision)
    cdt = np.complex64 if precision == 1 else np.complex128
    C = cfg["beam_coefs"].astype(cdt)  # (the coefficients the device holds)
    V = fftvis_amd.simulate_vis(**cfg).astype(np.complex128)
    nV = np.linalg.norm(V)
    both = _jvp(cfg, d_beam_coefs=np.stack([1j * C, C])).astype(np.complex128)
    u = 2.0**-24 if precision == 1 else 2.0**-53
    quarter, same = np.linalg.norm(both[0]) / nV, np.linalg.norm(both[1] - 2 * V) / nV
    print("basis-tangent cancelling", json.dumps({"precision": precision, "compat": compat, "array": array,
                                                  "iC": quarter / u, "C": same / u}))
    assert np.linalg.norm(both[1]) > nV
    assert quarter <= CANCEL * u and same <= CANCEL * u, (quarter / u, same / u)


def _edge_cfg(**kw):
    """HERA-7, complex tables, full-Stokes sky, the exact form of the off-diagonal terms, fp64."""
    return basis_config("complex", "full", False, "coplanar", 2, **kw)


def test_a_stack_of_directions_equals_single_calls_bit_for_bit(gpu, monkeypatch):
    from fftvis_amd.gpu import gpu_simulate

    cfg = _edge_cfg()
    Ds = np.stack([_direction(cfg, s) for s in (11, 12, 13)])
    stack = _jvp(cfg, d_beam_coefs=Ds)
    assert stack.shape == (3,) + _vis_shape(cfg)
    for q in range(3):
        assert np.array_equal(stack[q], _jvp(cfg, d_beam_coefs=Ds[q])), q
    assert np.array_equal(_jvp(cfg, d_beam_coefs=Ds[:1])[0], stack[0])  # a stack of one keeps its axis
    # a byte budget of two directions' output: the stack is cut 2 + 1
    calls = []
    real = gpu_simulate.SimHandle.run_basis_tangent
    monkeypatch.setattr(gpu_simulate.SimHandle, "run_basis_tangent",
                        lambda self, *a: calls.append(int(a[4].shape[0])) or real(self, *a))
    monkeypatch.setenv("FFTVIS_BASIS_TANGENT_BYTES", str(2 * stack[0].nbytes))
    cut = _jvp(cfg, d_beam_coefs=Ds)
    assert calls == [2, 1] and np.array_equal(cut, stack)


def test_one_basis_beam(gpu):
    """K = 1: no off-diagonal term."""
    cfg = _edge_cfg()
    cfg.update(beam=cfg["beam"][:1], beam_coefs=cfg["beam_coefs"][:, :1])
    D = _direction(cfg)
    _assert_close("K = 1", cfg, _jvp(cfg, d_beam_coefs=D), exact_dv(cfg, D), cfg["eps"])


def test_source_chunks_add(gpu):
    cfg = dict(_edge_cfg(nsrc=25), min_chunks=2)
    D = _direction(cfg)
    _assert_close("min_chunks 2", cfg, _jvp(cfg, d_beam_coefs=D), exact_dv(cfg, D), cfg["eps"])


def test_upsample_125(gpu):
    cfg = dict(_edge_cfg(), upsample_factor=1.25)
    D = _direction(cfg)
    _assert_close("sigma 1.25", cfg, _jvp(cfg, d_beam_coefs=D), exact_dv(cfg, D), cfg["eps"], k64=20.0)


def test_reproducible_for_a_lane_count(gpu, monkeypatch):
    cfg = _edge_cfg(nsrc=40, ntimes=4)
    Ds = np.stack([_direction(cfg, s) for s in (1, 2)])
    res = {}
    for lanes in ("1", "2"):
        monkeypatch.setenv("FFTVIS_HIP_LANES", lanes)
        a, b = _jvp(cfg, d_beam_coefs=Ds), _jvp(cfg, d_beam_coefs=Ds)
        assert np.array_equal(a, b), lanes
        res[lanes] = a
    assert rel_l2(res["1"], res["2"]) <= 1e-12


def test_a_forward_call_after_the_pass_returns_the_same_bits(gpu):
    cfg = _edge_cfg()
    before = fftvis_amd.simulate_vis(**cfg)
    _jvp(cfg, d_beam_coefs=_direction(cfg))
    assert np.array_equal(fftvis_amd.simulate_vis(**cfg), before)


def test_bulk_device_memory_is_given_back(gpu, monkeypatch):
    """Beyond FFTVIS_HIP_ADJ_KEEP_BYTES (here 0) a cached handle holds after a call no more than it held after the
    forward: neither the staged directions nor the (ndir, ...) output stays."""
    monkeypatch.setenv("FFTVIS_HIP_ADJ_KEEP_BYTES", "0")
    cfg = _edge_cfg()
    fftvis_amd.simulate_vis(**cfg)
    held = ctypes.c_int64(0)
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    before = held.value
    _jvp(cfg, d_beam_coefs=np.stack([_direction(cfg, s) for s in range(8)]))
    _lib.check(_lib.lib().fv_device_bytes_on(0, ctypes.byref(held)))
    assert held.value - before < 1 << 20, (before, held.value)


def test_raw_c_abi(gpu):
    """fv_sim_run_basis_tangent through a bare ctypes handle configured by the engine's own setters: device and host
    pointers, a (time, frequency) sub-block, a value that is not finite refused with the handle left usable, and a handle
    without basis beams refused."""
    import torch

    from fftvis_amd import synth
    from fftvis_amd.gpu import gpu_simulate as gs

    cfg = _edge_cfg()
    Ds = np.stack([_direction(cfg, s) for s in (21, 22)])
    want = _jvp(cfg, d_beam_coefs=Ds)
    nf, nt = len(cfg["freqs"]), len(cfg["times"])
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    key, h = gs._acquire_handle(0, 2, cfg["eps"], 2, True)  # configured for exactly this run
    try:
        dD = torch.from_numpy(Ds).cuda()
        dV = torch.full(want.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        assert L.fv_sim_run_basis_tangent(h._h, 0, nt, 0, nf, p(dD), 1, 2, p(dV), 1) == 0, L.fv_last_error()
        assert np.array_equal(dV.cpu().numpy(), want)  # always overwritten
        hV = np.full(want.shape, 7.0, dtype=np.complex128)  # host pointers
        assert L.fv_sim_run_basis_tangent(h._h, 0, nt, 0, nf, hp(Ds), 0, 2, hp(hV), 0) == 0, L.fv_last_error()
        assert np.array_equal(hV, want)
        # one time step, the upper channels: host pointers, then device pointers
        blk = np.full((2, nf - 1, 1) + want.shape[3:], 7.0, dtype=np.complex128)
        assert L.fv_sim_run_basis_tangent(h._h, 1, 2, 1, nf, hp(Ds), 0, 2, hp(blk), 0) == 0, L.fv_last_error()
        assert rel_l2(blk, want[:, 1:, 1:2]) <= 10 * cfg["eps"] and blk.any()
        dblk = torch.full(blk.shape, 7.0, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        assert L.fv_sim_run_basis_tangent(h._h, 1, 2, 1, nf, p(dD), 1, 2, p(dblk), 1) == 0, L.fv_last_error()
        assert np.array_equal(dblk.cpu().numpy(), blk)
        for bad in (np.nan, complex(0.0, np.inf)):
            B = Ds.copy()
            B[1, 3, 2, 1] = bad
            assert L.fv_sim_run_basis_tangent(h._h, 0, nt, 0, nf, hp(B), 0, 2, hp(hV), 0) == 1
            assert b"not finite" in L.fv_last_error()
            dB = torch.from_numpy(B).cuda()
            torch.cuda.synchronize()
            assert L.fv_sim_run_basis_tangent(h._h, 0, nt, 0, nf, p(dB), 1, 2, p(dV), 1) == 1
            assert b"not finite" in L.fv_last_error()
            hV[...] = 7.0
            assert L.fv_sim_run_basis_tangent(h._h, 0, nt, 0, nf, hp(Ds), 0, 2, hp(hV), 0) == 0, L.fv_last_error()
            assert np.array_equal(hV, want)
    finally:
        gs._return_handle(key, h)
    plain = synth.make_config("C1", nsrc=20, nfreq=3, ntimes=2)
    fftvis_amd.simulate_vis(**dict(plain, polarized=True))
    key, h = gs._acquire_handle(0, 2, plain["eps"], 2, True)
    try:
        buf = torch.zeros(8192, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        assert L.fv_sim_run_basis_tangent(h._h, 0, 1, 0, 1, p(buf), 1, 1, p(buf), 1) == 1
        assert b"fv_sim_set_basis" in L.fv_last_error()
    finally:
        gs._return_handle(key, h)


def test_a_value_that_is_not_finite_fails_through_python(gpu):
    cfg = _edge_cfg()
    D = _direction(cfg)
    good = _jvp(cfg, d_beam_coefs=D)
    B = D.copy()
    B[2, 1, 0] = np.nan
    with pytest.raises(_lib.FftvisHipError, match="finite"):
        _jvp(cfg, d_beam_coefs=B)
    assert np.array_equal(_jvp(cfg, d_beam_coefs=D), good)


def test_tensors_in_give_tensors_out(gpu):
    import torch

    cfg = _edge_cfg()
    D = _direction(cfg)
    dF = np.random.default_rng(2).normal(size=cfg["fluxes"].shape)
    want = _jvp(cfg, d_beam_coefs=D, d_fluxes=dF)
    got = _jvp(cfg, d_beam_coefs=torch.from_numpy(D).cuda(), d_fluxes=torch.from_numpy(dF).cuda())
    assert got.device.type == "cuda" and got.dtype == torch.complex128 and np.array_equal(got.cpu().numpy(), want)
    host = _jvp(cfg, d_beam_coefs=torch.from_numpy(D))
    assert isinstance(host, torch.Tensor) and host.device.type == "cpu"
    only_f = _jvp(cfg, d_fluxes=dF)  # the flux part alone is the forward on d_fluxes
    assert np.array_equal(only_f, fftvis_amd.simulate_vis(**dict(cfg, fluxes=dF)))


def test_forward_ad_equals_the_direct_calls(gpu):
    import torch
    import torch.autograd.forward_ad as fwAD

    cfg = _edge_cfg()
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "beam_coefs")}
    D = _direction(cfg)
    dF = np.random.default_rng(6).normal(size=cfg["fluxes"].shape)
    F = torch.tensor(cfg["fluxes"], dtype=torch.float64, device="cuda")
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda")
    tF = torch.tensor(dF, dtype=torch.float64, device="cuda")
    tC = torch.tensor(D, dtype=torch.complex128, device="cuda")
    V = fftvis_amd.simulate_vis(**cfg)

    def check(out, want):
        primal, tangent = fwAD.unpack_dual(out)
        assert tangent is not None and tangent.device == F.device and tangent.dtype == torch.complex128
        assert rel_l2(primal.cpu().numpy(), V) <= 1e-12
        assert rel_l2(tangent.cpu().numpy(), want) <= 1e-12

    with fwAD.dual_level():
        check(fftvis_amd.torch_simulate_vis_basis(fwAD.make_dual(F, tF), fwAD.make_dual(C, tC), **kw),
              _jvp(cfg, d_beam_coefs=D, d_fluxes=dF))
        check(fftvis_amd.torch_simulate_vis_basis(F, fwAD.make_dual(C, tC), **kw), _jvp(cfg, d_beam_coefs=D))
        check(fftvis_amd.torch_simulate_vis_basis(fwAD.make_dual(F, tF), C, **kw), _jvp(cfg, d_fluxes=dF))


def test_torch_gradcheck_forward_ad(gpu):
    """fp64, 6 sources, one channel, one time, eps 1e-12; the basis adjoint's gradcheck steps, with forward-mode AD."""
    import torch

    cfg = basis_config("complex", "full", False, nsrc=6, nfreq=1, ntimes=1)
    cfg.update(eps=1e-12, baselines=cfg["baselines"][:5] + [(3, 0), (2, 2)])
    kw = {k: v for k, v in cfg.items() if k not in ("fluxes", "beam_coefs")}
    rng = np.random.default_rng(8)
    F = torch.tensor(rng.uniform(0.5, 1.5, (6, 1, 4)), dtype=torch.float64, device="cuda", requires_grad=True)
    C = torch.tensor(cfg["beam_coefs"], dtype=torch.complex128, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda f, c: fftvis_amd.torch_simulate_vis_basis(f, c, **kw), (F, C), eps=1e-3,
                                    atol=1e-7, rtol=1e-6, check_forward_ad=True)
